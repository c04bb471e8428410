// CPU-only sanitizer harness of the call-state record's rules (tests/test_call_state_host.py builds it with
// g++ -DPN_NO_HIP -fsanitize=address,undefined, like lim_sanitize.cpp): pn_call_rules.h over heap buffers of EXACTLY the bytes handed
// in — a whole record, every shorter length from 0 to 10639 in steps that hit 15, 16, 17 and 10639, one byte too many — and over
// hostile records: every header word wrong, every invariant at its edge and one step outside, every word of an absent section
// set in turn, random bytes behind a good header.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_call_rules.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "call_state_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

typedef std::vector<unsigned char> R;
static uint32_t as_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static void put(R &r, int word, uint32_t v) { for (int i = 0; i < 4; i++) r[4 * (size_t)word + i] = (unsigned char)(v >> (8 * i)); }   // little-endian, header included
static void body(R &r, int word, uint32_t v) { put(r, PN_CALL_HEADER_WORDS + word, v); }
// the check over a heap copy of exactly `n` bytes, so that a read past the end is the sanitizer's
static int check(const R &r, size_t n) {
  unsigned char *p = (unsigned char *)malloc(n ? n : 1);
  if (n) memcpy(p, r.data(), n);
  const int v = pn_call_record_check(n ? p : p, n);
  free(p);
  return v;
}
static R good(uint32_t mask) {
  R r(PN_RATE_CALL_STATE_BYTES, 0);
  put(r, 0, PN_RATE_CALL_MAGIC); put(r, 1, PN_RATE_CALL_VERSION); put(r, 2, PN_RATE_CALL_STATE_BYTES); put(r, 3, mask);
  if (mask & PN_CALL_PLC) {
    for (int i = 0; i < PN_PLC_HIST + PN_PLC_P_MAX; i++) body(r, i, as_bits(0.001f * (float)(i % 97) - 0.04f));
    body(r, PN_CALL_W_META, 480u); body(r, PN_CALL_W_META + 1, 2u); body(r, PN_CALL_W_META + 2, 7u);
  }
  if (mask & PN_CALL_AGC) { body(r, PN_CALL_W_AGC, as_bits(3.5f)); body(r, PN_CALL_W_AGC + 1, as_bits(8.0f)); body(r, PN_CALL_W_AGC + 2, 99u); }
  if (mask & PN_CALL_LIM) { body(r, PN_CALL_W_LIM, as_bits(0.25f)); body(r, PN_CALL_W_LIM + 1, 2u); body(r, PN_CALL_W_LIM + 2, 5u); }
  if (mask & PN_CALL_MIX) body(r, PN_CALL_W_MIX, as_bits(12.0f));
  return r;
}

int main() {
  static_assert(PN_RATE_CALL_STATE_BYTES == 10640 && PN_CALL_BODY_WORDS == 2656 && PN_CALL_ALL == 15 && PN_SS_BAD_STATE == -7, "the header's constants");
  const size_t N = PN_RATE_CALL_STATE_BYTES;
  // ---- every mask gives a good record; NULL; every length but the right one is a size verdict, and nothing past the buffer is read
  for (uint32_t m = 0; m <= PN_CALL_ALL; m++) CHECK(check(good(m), N) == PN_SS_OK);
  CHECK(pn_call_record_check(NULL, N) == PN_SS_BAD_ARG);
  { R r = good(PN_CALL_ALL), big = r;
    big.push_back(0);
    for (size_t n = 0; n < N; n += (n < 40 ? 1 : 997)) CHECK(check(r, n) == PN_SS_BAD_SIZE);
    CHECK(check(r, N - 1) == PN_SS_BAD_SIZE && check(big, N + 1) == PN_SS_BAD_SIZE && strstr(pn_last_error(), "10640"));
    R bad = r; put(bad, 0, 0x12345678u);
    CHECK(check(bad, 16) == PN_SS_BAD_MAGIC && check(bad, N) == PN_SS_BAD_MAGIC);        // the header's verdicts come first
    bad = r; put(bad, 1, 2u); CHECK(check(bad, N) == PN_SS_BAD_VERSION && check(bad, 20) == PN_SS_BAD_VERSION);
    bad = r; put(bad, 2, (uint32_t)N + 16u); CHECK(check(bad, N) == PN_SS_BAD_SIZE);
    bad = r; put(bad, 3, 16u | PN_CALL_ALL); CHECK(check(bad, N) == PN_SS_BAD_STATE && strstr(pn_last_error(), "mask"));
    bad = r; put(bad, 3, 0x80000000u); CHECK(check(bad, N) == PN_SS_BAD_STATE); }
  // ---- PLC: P at 239 / 240 / 720 / 721 and 0; r > 0 with P == 0; word 3
  { const struct { uint32_t P, r; int want; } k[] = {{239u, 0u, PN_SS_BAD_STATE}, {240u, 0u, PN_SS_OK}, {720u, 5u, PN_SS_OK}, {721u, 0u, PN_SS_BAD_STATE}, {0u, 0u, PN_SS_OK},
                                                     {0u, 1u, PN_SS_BAD_STATE}, {1u, 0u, PN_SS_BAD_STATE}, {0xffffffffu, 1u, PN_SS_BAD_STATE}, {480u, 0x7fffffffu, PN_SS_OK}};
    for (auto &c : k) { R r = good(PN_CALL_ALL); body(r, PN_CALL_W_META, c.P); body(r, PN_CALL_W_META + 1, c.r); CHECK(check(r, N) == c.want); }
    R r = good(PN_CALL_ALL); body(r, PN_CALL_W_META + 3, 1u); CHECK(check(r, N) == PN_SS_BAD_STATE); }
  // ---- AGC: the level, the gain at both ends and one step outside, the spare word
  { const struct { int word; uint32_t v; int want; } k[] = {
        {0, as_bits(0.0f), PN_SS_OK}, {0, as_bits(-0.0f), PN_SS_OK}, {0, as_bits(INFINITY), PN_SS_OK}, {0, as_bits(NAN), PN_SS_BAD_STATE}, {0, as_bits(-1e-30f), PN_SS_BAD_STATE},
        {1, 0u, PN_SS_OK}, {1, as_bits(1.0f / 1024.0f), PN_SS_OK}, {1, as_bits(nextafterf(1.0f / 1024.0f, 0.0f)), PN_SS_BAD_STATE}, {1, as_bits(1024.0f), PN_SS_OK},
        {1, as_bits(nextafterf(1024.0f, INFINITY)), PN_SS_BAD_STATE}, {1, as_bits(NAN), PN_SS_BAD_STATE}, {1, as_bits(INFINITY), PN_SS_BAD_STATE}, {1, as_bits(-1.0f), PN_SS_BAD_STATE},
        {1, as_bits(-0.0f), PN_SS_BAD_STATE}, {2, 0xffffffffu, PN_SS_OK}, {3, 1u, PN_SS_BAD_STATE}};
    for (auto &c : k) { R r = good(PN_CALL_ALL); body(r, PN_CALL_W_AGC + c.word, c.v); CHECK(check(r, N) == c.want); } }
  // ---- limiter: gain bits 0, the smallest subnormal, 1.0, one step above, NaN; the spare word
  { const struct { int word; uint32_t v; int want; } k[] = {
        {0, 0u, PN_SS_OK}, {0, 1u, PN_SS_OK}, {0, as_bits(1.0f), PN_SS_OK}, {0, as_bits(nextafterf(1.0f, 2.0f)), PN_SS_BAD_STATE}, {0, as_bits(NAN), PN_SS_BAD_STATE},
        {0, as_bits(-0.0f), PN_SS_BAD_STATE}, {0, as_bits(2.0f), PN_SS_BAD_STATE}, {0, as_bits(-0.5f), PN_SS_BAD_STATE}, {1, 1000u, PN_SS_OK}, {2, 0xffffffffu, PN_SS_OK},
        {3, 0x80000000u, PN_SS_BAD_STATE}};
    for (auto &c : k) { R r = good(PN_CALL_ALL); body(r, PN_CALL_W_LIM + c.word, c.v); CHECK(check(r, N) == c.want); } }
  // ---- MIX: the level finite and >= 0, the padding
  { const struct { int word; uint32_t v; int want; } k[] = {{0, 0u, PN_SS_OK}, {0, as_bits(FLT_MAX), PN_SS_OK}, {0, as_bits(INFINITY), PN_SS_BAD_STATE}, {0, as_bits(NAN), PN_SS_BAD_STATE},
                                                            {0, as_bits(-1.0f), PN_SS_BAD_STATE}, {1, 1u, PN_SS_BAD_STATE}, {2, 1u, PN_SS_BAD_STATE}, {3, 1u, PN_SS_BAD_STATE}};
    for (auto &c : k) { R r = good(PN_CALL_ALL); body(r, PN_CALL_W_MIX + c.word, c.v); CHECK(check(r, N) == c.want); } }
  // ---- an absent section with one non-zero word: every word of every section in turn, under every mask that lacks it; a present
  // section's invariants are not asked of an absent one's neighbours
  { const struct { uint32_t bit; int lo, hi; } sec[] = {{PN_CALL_PLC, PN_CALL_W_HIST, PN_CALL_W_AGC}, {PN_CALL_AGC, PN_CALL_W_AGC, PN_CALL_W_LIM},
                                                        {PN_CALL_LIM, PN_CALL_W_LIM, PN_CALL_W_MIX}, {PN_CALL_MIX, PN_CALL_W_MIX, PN_CALL_BODY_WORDS}};
    for (auto &s : sec)
      for (int w = s.lo; w < s.hi; w += (s.hi - s.lo > 4 ? 7 : 1)) {
        R r = good(PN_CALL_ALL & ~s.bit);
        body(r, w, 0x00000100u); CHECK(check(r, N) == PN_SS_BAD_STATE);
        body(r, w, 0u); CHECK(check(r, N) == PN_SS_OK);
      }
    R r = good(PN_CALL_ALL & ~PN_CALL_PLC); body(r, PN_CALL_W_META - 1, 0x80000000u); CHECK(check(r, N) == PN_SS_BAD_STATE);     // (-0.0f in the last word of q is not zero)
    r = good(0); r[N - 1] = 1; CHECK(check(r, N) == PN_SS_BAD_STATE); }
  // ---- random bytes behind a good header, and wholly random records: any verdict, no bad access
  { uint32_t x = 12345u;
    int seen_ok = 0;
    for (int it = 0; it < 200; it++) {
      R r = good(PN_CALL_ALL);
      for (size_t i = (it & 1) ? 0 : 12; i < N; i++) { x = x * 1664525u + 1013904223u; r[i] = (unsigned char)(x >> 24); }
      if (it % 4 == 0) for (int w = PN_CALL_W_META; w < PN_CALL_BODY_WORDS; w++) body(r, w, 0u);
      const int v = check(r, N);
      CHECK(v == PN_SS_OK || v == PN_SS_BAD_MAGIC || v == PN_SS_BAD_VERSION || v == PN_SS_BAD_SIZE || v == PN_SS_BAD_STATE);
      seen_ok += v == PN_SS_OK;
    }
    (void)seen_ok; }
  // ---- the verdict function itself, as the kernel calls it
  { uint32_t h[4] = {PN_RATE_CALL_MAGIC, PN_RATE_CALL_VERSION, PN_RATE_CALL_STATE_BYTES, 0u}, t[PN_CALL_TAIL_WORDS] = {0};
    CHECK(pn_call_verdict(h, t, false) == PN_SS_OK && pn_call_verdict(h, t, true) == PN_SS_BAD_STATE);
    h[3] = PN_CALL_PLC; CHECK(pn_call_verdict(h, t, true) == PN_SS_OK); }
  printf("ok\n");
  return 0;
}
