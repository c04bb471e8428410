// CPU-only sanitizer harness of the rate converter's HIP-free pieces (tests/test_rate_host.py builds it with
// g++ -DPN_NO_HIP -fsanitize=address,undefined, like host_sanitize.cpp): the filter design for each rate into exactly-sized
// destinations, and the state-record check over well-formed, truncated and corrupted records held in exactly-sized heap copies,
// so that a read past a table or past the bytes a caller handed in aborts.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_rate_design.h"
#include <stdio.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "rate_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

int main() {
  const int rates[3] = {8000, 16000, 24000}, factors[3] = {6, 3, 2};
  const size_t rec_bytes[3] = {912, 528, 400};
  for (int bad : {48000, 44100, 0, -1, 12000, 7999}) CHECK(pn_rate_factor(bad) == 0);
  for (int ri = 0; ri < 3; ri++) {
    const int rate = rates[ri], L = pn_rate_factor(rate), D = PN_RATE_TAPS * L, n = 2 * D + 1;
    CHECK(L == factors[ri] && n <= PN_RATE_MAX_TAPS && pn_rate_down_tail(L) == 2 * D);
    CHECK(4 * pn_rate_record_words(L) == rec_bytes[ri]);
    // the design, both tables, into destinations of exactly 2D + 1 floats; one float short is refused before anything is written
    for (int down = 0; down < 2; down++) {
      std::vector<float> t(n);
      CHECK(pn_rate_design(L, down, t.data(), n) == n);
      CHECK(t[D] == (down ? (float)(1.0 / L) : 1.0f));
      for (int k = 1; k <= D; k++) {
        CHECK(t[D + k] == t[D - k]);
        if (k % L == 0) CHECK(t[D + k] == 0.0f);
        CHECK(t[D + k] == t[D + k] && fabsf(t[D + k]) < 1.0f);
      }
      std::vector<float> small(n - 1);
      CHECK(pn_rate_design(L, down, small.data(), n - 1) == -1);
      CHECK(pn_rate_design(L, down, NULL, n) == -1);
    }
    for (int badL : {0, 1, 4, 5, 7, -2}) { float x[4]; CHECK(pn_rate_design(badL, 0, x, 4) == -1); }
    // records
    const size_t bytes = rec_bytes[ri];
    std::vector<unsigned char> rec(bytes, 0);
    { uint32_t h[4]; pn_rate_record_header(h, rate); memcpy(rec.data(), h, 16);
      CHECK(h[0] == PN_RATE_STATE_MAGIC && h[1] == PN_RATE_STATE_VERSION && h[2] == bytes && h[3] == (uint32_t)rate); }
    CHECK(rec[0] == 'P' && rec[1] == 'N' && rec[2] == 'R' && rec[3] == 'S');
    CHECK(pn_rate_record_check(rec.data(), bytes, rate) == PN_SS_OK);
    CHECK(pn_rate_record_check(NULL, bytes, rate) == PN_SS_BAD_ARG);
    for (int other = 0; other < 3; other++) if (other != ri) CHECK(pn_rate_record_check(rec.data(), bytes, rates[other]) == PN_SS_BAD_RATE);
    CHECK(pn_rate_record_check(rec.data(), bytes, 48000) == PN_SS_BAD_RATE);
    // every truncation, in an exact-size copy: never OK, never a read past the end
    for (size_t c = 0; c < bytes; c++) {
      std::vector<unsigned char> t(rec.begin(), rec.begin() + c);
      const int v = pn_rate_record_check(c ? t.data() : (const void *)"", c, rate);
      CHECK(v == PN_SS_BAD_SIZE);
    }
    { std::vector<unsigned char> t(rec); t.push_back(0); CHECK(pn_rate_record_check(t.data(), t.size(), rate) == PN_SS_BAD_SIZE); }
    // every single-byte corruption of the header is refused with the verdict of its field; the body is not looked at
    for (int b = 0; b < 16; b++)
      for (int bit = 0; bit < 8; bit++) {
        std::vector<unsigned char> t(rec);
        t[b] ^= (unsigned char)(1 << bit);
        const int want = b < 4 ? PN_SS_BAD_MAGIC : b < 8 ? PN_SS_BAD_VERSION : b < 12 ? PN_SS_BAD_SIZE : PN_SS_BAD_RATE;
        CHECK(pn_rate_record_check(t.data(), bytes, rate) == want);
      }
    { uint32_t x = 2463534242u;
      for (int it = 0; it < 200; it++) {
        std::vector<unsigned char> t(rec);
        for (int k = 0; k < 3; k++) { x = x * 1664525u + 1013904223u; t[16 + (x >> 8) % (bytes - 16)] ^= (unsigned char)(x >> 24); }
        CHECK(pn_rate_record_check(t.data(), bytes, rate) == PN_SS_OK);
      } }
  }
  puts("ok");
  return 0;
}
