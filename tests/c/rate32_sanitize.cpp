// CPU-only sanitizer harness of the rate converter's HIP-free pieces at 32000 Hz, the rational 3:2 rate (tests/test_rate32_host.py
// builds it with g++ -DPN_NO_HIP -fsanitize=address,undefined, like rate_sanitize.cpp): the design into exactly-sized destinations
// and one too small, the state-record check over truncated and hostile records in exactly-sized heap copies, and the mixed
// converter's list rules on lists holding 32000.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_rate_mixed.h"
#include <stdio.h>
#include <string.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "rate32_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)
static bool says(const char *what) { return strstr(pn_last_error(), what) != NULL; }

int main() {
  const int rate = 32000, f = pn_rate_factor(rate), D = 48, n = 2 * D + 1;
  const size_t bytes = 336;
  CHECK(f == PN_RATE_F_3_2 && pn_rate_factor_L(f) == 3 && pn_rate_factor_M(f) == 2 && pn_rate_factor_hz(f) == rate);
  CHECK(pn_rate_factor_frame(f) == 320 && pn_rate_factor_delay(f) == 1952 && pn_rate_down_tail(f) == 48 && 4 * pn_rate_record_words(f) == bytes);
  CHECK(pn_rate_mixed_factor(rate) == f && pn_rate_mixed_frame(rate) == 320 && pn_rate_mixed_delay(rate) == 1952);
  CHECK(320 <= PN_RATE_MIXED_ROW && 320 % 16 == 0 && bytes <= PN_RATE_STATE_MAX_BYTES && n <= PN_RATE_MAX_TAPS);
  for (int bad : {32001, 31999, 64000, 16001, 3200, 320000}) CHECK(pn_rate_factor(bad) == 0 && pn_rate_mixed_factor(bad) == 0);
  // ---- the design: h is the table of 3, g = (float)(h * 2 / 3); a destination one float short is refused before anything is written
  {
    std::vector<float> h3(n), h(n), g(n), g3(n);
    CHECK(pn_rate_design(3, 0, h3.data(), n) == n && pn_rate_design(f, 0, h.data(), n) == n);
    CHECK(pn_rate_design(3, 1, g3.data(), n) == n && pn_rate_design(f, 1, g.data(), n) == n);
    CHECK(memcmp(h.data(), h3.data(), n * sizeof(float)) == 0);
    CHECK(h[D] == 1.0f && g[D] == (float)(2.0 / 3.0));
    for (int k = 1; k <= D; k++) {
      CHECK(g[D + k] == g[D - k]);
      if (k % 3 == 0) CHECK(g[D + k] == 0.0f); else CHECK(g[D + k] != 0.0f);
      CHECK(fabsf(g[D + k] - 2.0f * g3[D + k]) <= 1.2e-7f * fabsf(g[D + k]) + 1e-30f);     // twice the 16 kHz down tap, up to one rounding each
    }
    for (int down = 0; down < 2; down++) {
      std::vector<float> small(n - 1, 7.0f);
      CHECK(pn_rate_design(f, down, small.data(), n - 1) == -1 && says("need room"));
      for (float v : small) CHECK(v == 7.0f);
      CHECK(pn_rate_design(f, down, NULL, n) == -1);
      std::vector<float> none(1);
      CHECK(pn_rate_design(f, down, none.data(), 0) == -1);
    }
    for (int badf : {31, 33, 23, 320, -32}) { float x[4]; CHECK(pn_rate_design(badf, 0, x, 4) == -1); }
  }
  // ---- records at 32000
  {
    std::vector<unsigned char> rec(bytes, 0);
    uint32_t hd[4];
    pn_rate_record_header(hd, rate);
    memcpy(rec.data(), hd, 16);
    CHECK(hd[0] == PN_RATE_STATE_MAGIC && hd[1] == PN_RATE_STATE_VERSION && hd[2] == bytes && hd[3] == (uint32_t)rate);
    CHECK(pn_rate_record_check(rec.data(), bytes, rate) == PN_SS_OK);
    CHECK(pn_rate_record_check(NULL, bytes, rate) == PN_SS_BAD_ARG);
    for (int other : {8000, 16000, 24000, 48000, 44100}) CHECK(pn_rate_record_check(rec.data(), bytes, other) == PN_SS_BAD_RATE);
    for (size_t c = 0; c < bytes; c++) {                  // every truncation, in an exact-size copy
      std::vector<unsigned char> t(rec.begin(), rec.begin() + c);
      CHECK(pn_rate_record_check(c ? t.data() : (const void *)"", c, rate) == PN_SS_BAD_SIZE);
    }
    { std::vector<unsigned char> t(rec); t.push_back(0); CHECK(pn_rate_record_check(t.data(), t.size(), rate) == PN_SS_BAD_SIZE); }
    for (int b = 0; b < 16; b++)
      for (int bit = 0; bit < 8; bit++) {
        std::vector<unsigned char> t(rec);
        t[b] ^= (unsigned char)(1 << bit);
        const int want = b < 4 ? PN_SS_BAD_MAGIC : b < 8 ? PN_SS_BAD_VERSION : b < 12 ? PN_SS_BAD_SIZE : PN_SS_BAD_RATE;
        CHECK(pn_rate_record_check(t.data(), bytes, rate) == want);
      }
    // the records of the other rates in a 32000 slot, and a 32000 header that claims their sizes (in copies of exactly that many bytes)
    for (int other : {8000, 16000, 24000}) {
      const size_t ob = 4 * pn_rate_record_words(pn_rate_factor(other));
      std::vector<unsigned char> t(ob, 0);
      uint32_t oh[4];
      pn_rate_record_header(oh, other);
      memcpy(t.data(), oh, 16);
      CHECK(pn_rate_record_check(t.data(), ob, other) == PN_SS_OK && pn_rate_record_check(t.data(), ob, rate) == PN_SS_BAD_RATE);
      oh[3] = (uint32_t)rate;
      memcpy(t.data(), oh, 16);
      CHECK(pn_rate_record_check(t.data(), ob, rate) == PN_SS_BAD_SIZE && pn_rate_record_check(t.data(), ob, other) == PN_SS_BAD_RATE);
      // the device import's verdict for the same header words is the host check's
      CHECK(pn_rate_header_verdict(oh[0], oh[1], oh[2], oh[3], rate) == PN_SS_BAD_SIZE);
    }
    uint32_t x = 2463534242u;
    for (int it = 0; it < 200; it++) {                     // the body is not looked at
      std::vector<unsigned char> t(rec);
      for (int k = 0; k < 3; k++) { x = x * 1664525u + 1013904223u; t[16 + (x >> 8) % (bytes - 16)] ^= (unsigned char)(x >> 24); }
      CHECK(pn_rate_record_check(t.data(), bytes, rate) == PN_SS_OK);
    }
  }
  // ---- lists holding 32000
  {
    const int five[5] = {8000, 16000, 24000, 32000, 48000};
    for (int nn = 1; nn <= 11; nn++) {
      std::vector<int32_t> r(nn);
      for (int i = 0; i < nn; i++) r[i] = five[(i + 3) % 5];
      CHECK(pn_rate_mixed_rates_list_check(r.data(), nn) == 0);
      for (int at = nn - 1; at >= 0; at--) {
        r[at] = at % 2 ? 44100 : 32001;
        CHECK(pn_rate_mixed_rates_list_check(r.data(), nn) == -1);
        char want[32];
        snprintf(want, sizeof(want), "index %d:", at);
        CHECK(says(want) && says(at % 2 ? "44100" : "32001") && says("32000 or 48000"));
      }
    }
    const int B = 5;
    std::vector<int32_t> ids = {4, 0, 2}, rs = {32000, 8000, 32000}, badr = {32000, 32000, 44100};
    CHECK(pn_rate_mixed_set_check(B, ids.data(), 3, rs.data()) == 0);
    CHECK(pn_rate_mixed_set_check(B, ids.data(), 3, badr.data()) == -1 && says("index 2:"));
    std::vector<int32_t> cur = {32000, 48000, 16000, 32000, 8000}, a = {0, 3}, b = {0, 2}, c = {3, 1};
    CHECK(pn_rate_mixed_record_rate(cur.data(), a.data(), 2) == 32000);
    CHECK(pn_rate_mixed_record_rate(cur.data(), b.data(), 2) == -1 && says("one rate"));
    CHECK(pn_rate_mixed_record_rate(cur.data(), c.data(), 2) == -1 && says("no converter state"));
    CHECK(pn_rate_records_list_check(B, cur.data(), a.data(), 2, true) == 0 && pn_rate_records_list_check(B, cur.data(), b.data(), 2, true) == 0);
    CHECK(pn_rate_records_list_check(B, cur.data(), c.data(), 2, true) == -1);
  }
  puts("ok");
  return 0;
}
