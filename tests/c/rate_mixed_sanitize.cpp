// CPU-only sanitizer harness of the mixed rate converter's HIP-free rules (tests/test_rate_mixed_host.py builds it with
// g++ -DPN_NO_HIP -fsanitize=address,undefined, like rate_sanitize.cpp): the four-rate table, lists of rates, rate changes and the
// one-rate-per-call rule of the records, fed hostile lists held in exactly-sized heap copies, so that a read past a list aborts.
// Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_rate_mixed.h"
#include <stdio.h>
#include <string.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "rate_mixed_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)
static bool says(const char *what) { return strstr(pn_last_error(), what) != NULL; }

int main() {
  const int rates[4] = {8000, 16000, 24000, 48000}, factors[4] = {6, 3, 2, 1}, frames[4] = {80, 160, 240, 480}, delays[4] = {512, 992, 1472, 2880};
  for (int i = 0; i < 4; i++) {
    CHECK(pn_rate_mixed_factor(rates[i]) == factors[i] && pn_rate_mixed_frame(rates[i]) == frames[i] && pn_rate_mixed_delay(rates[i]) == delays[i]);
    CHECK(frames[i] <= PN_RATE_MIXED_ROW && frames[i] % 8 == 0);
  }
  CHECK(pn_rate_factor(48000) == 0);                        // the single-rate surface keeps refusing 48000
  for (int bad : {44100, 12000, 0, -1, 7999, 96000, 1}) {
    CHECK(pn_rate_mixed_factor(bad) == 0);
    CHECK(pn_rate_mixed_frame(bad) == -1 && says("48000"));
    CHECK(pn_rate_mixed_delay(bad) == -1);
  }
  // ---- lists of rates: the first bad index is named, and nothing past the list is read
  CHECK(pn_rate_mixed_rates_list_check(NULL, 0) == 0);
  CHECK(pn_rate_mixed_rates_list_check(NULL, 3) == -1);
  CHECK(pn_rate_mixed_rates_list_check(NULL, -1) == -1);
  for (int n = 1; n <= 9; n++) {
    std::vector<int32_t> r(n);
    for (int i = 0; i < n; i++) r[i] = rates[i % 4];
    CHECK(pn_rate_mixed_rates_list_check(r.data(), n) == 0);
    CHECK(pn_rate_mixed_rates_list_check(r.data(), -n) == -1);
    for (int at = n - 1; at >= 0; at--) {                    // bad entries at `at` and behind it: `at` is the one named
      r[at] = at % 2 ? 44100 : 12000;
      CHECK(pn_rate_mixed_rates_list_check(r.data(), n) == -1);
      char want[32];
      snprintf(want, sizeof(want), "index %d:", at);
      CHECK(says(want) && says(at % 2 ? "44100" : "12000"));
    }
  }
  // ---- a rate change: ids distinct and in range, rates out of the four
  {
    const int B = 5;
    std::vector<int32_t> ids = {4, 0, 2}, rs = {48000, 8000, 16000};
    CHECK(pn_rate_mixed_set_check(B, ids.data(), 3, rs.data()) == 0);
    CHECK(pn_rate_mixed_set_check(B, NULL, 0, NULL) == 0);
    CHECK(pn_rate_mixed_set_check(B, NULL, 2, rs.data()) == -1);
    CHECK(pn_rate_mixed_set_check(B, ids.data(), 3, NULL) == -1);
    CHECK(pn_rate_mixed_set_check(B, ids.data(), -3, rs.data()) == -1);
    std::vector<int32_t> dup = {1, 3, 1};
    CHECK(pn_rate_mixed_set_check(B, dup.data(), 3, rs.data()) == -1 && says("twice"));
    for (int32_t out : {5, -1, 1 << 30, -(1 << 30)}) {
      std::vector<int32_t> o = {0, out, 1};
      CHECK(pn_rate_mixed_set_check(B, o.data(), 3, rs.data()) == -1 && says("out of range"));
    }
    std::vector<int32_t> many = {0, 1, 2, 3, 4, 0}, mr(6, 8000);
    CHECK(pn_rate_mixed_set_check(B, many.data(), 6, mr.data()) == -1);
    std::vector<int32_t> badr = {48000, 8000, 44100};
    CHECK(pn_rate_mixed_set_check(B, ids.data(), 3, badr.data()) == -1 && says("index 2:"));
  }
  // ---- records: one rate per call, never a 48000 slot
  {
    std::vector<int32_t> cur = {8000, 48000, 16000, 24000, 8000};
    std::vector<int32_t> a = {0, 4}, b = {4}, c = {0, 2}, d = {1}, e = {0, 1}, f = {3, 3};
    CHECK(pn_rate_mixed_record_rate(cur.data(), a.data(), 2) == 8000);
    CHECK(pn_rate_mixed_record_rate(cur.data(), b.data(), 1) == 8000);
    CHECK(pn_rate_mixed_record_rate(cur.data(), f.data(), 2) == 24000);
    CHECK(pn_rate_mixed_record_rate(cur.data(), c.data(), 2) == -1 && says("one rate"));
    CHECK(pn_rate_mixed_record_rate(cur.data(), d.data(), 1) == -1 && says("no converter state"));
    CHECK(pn_rate_mixed_record_rate(cur.data(), e.data(), 2) == -1);
    CHECK(pn_rate_mixed_record_rate(cur.data(), a.data(), 0) == -1);
    CHECK(pn_rate_mixed_record_rate(cur.data(), NULL, 2) == -1);
    CHECK(pn_rate_mixed_record_rate(NULL, a.data(), 2) == -1);
    // the rate it gives is one whose record the single-rate check accepts
    for (int i = 0; i < 3; i++) {
      std::vector<int32_t> one(1, rates[i]), id(1, 0);
      const int R = pn_rate_mixed_record_rate(one.data(), id.data(), 1);
      CHECK(R == rates[i]);
      std::vector<unsigned char> rec(4 * pn_rate_record_words(pn_rate_factor(R)), 0);
      uint32_t h[4];
      pn_rate_record_header(h, R);
      memcpy(rec.data(), h, 16);
      CHECK(pn_rate_record_check(rec.data(), rec.size(), R) == PN_SS_OK);
      CHECK(pn_rate_record_check(rec.data(), rec.size(), rates[(i + 1) % 3]) == PN_SS_BAD_RATE);
    }
  }
  puts("ok");
  return 0;
}
