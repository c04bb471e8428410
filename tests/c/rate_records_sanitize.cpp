// CPU-only sanitizer harness of the rules behind the converter's device-side records (tests/test_rate_pipe_host.py builds it with
// g++ -DPN_NO_HIP -fsanitize=address,undefined, like rate_mixed_sanitize.cpp): the host-only list rule of a device record call
// (pn_rate_mixed.h pn_rate_records_list_check) over exactly-sized heap copies of hostile lists, and the header verdict the device
// import shares with the host check (pn_rate_design.h pn_rate_header_verdict) against pn_rate_record_check over exactly-sized
// records, so that a read past a list or a header aborts.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_rate_mixed.h"
#include <stdio.h>
#include <string.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "rate_records_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)
static bool says(const char *what) { return strstr(pn_last_error(), what) != NULL; }

int main() {
  static_assert(PN_RATE_STATE_MAX_BYTES == 912, "the fixed stride of a mixed converter's device records");
  const int rates[3] = {8000, 16000, 24000};
  size_t largest = 0;
  for (int R : rates) { const size_t b = 4 * pn_rate_record_words(pn_rate_factor(R)); CHECK(b % 16 == 0 && b <= PN_RATE_STATE_MAX_BYTES); if (b > largest) largest = b; }
  CHECK(largest == PN_RATE_STATE_MAX_BYTES);
  // ---- the list of a device record call: in range, distinct on import, never a 48000 slot; a mixed list of rates is legal
  {
    const int B = 6;
    std::vector<int32_t> cur = {8000, 48000, 16000, 24000, 8000, 16000};
    std::vector<int32_t> all = {0, 2, 3, 4, 5}, dup = {0, 2, 0}, with48 = {0, 1}, only48 = {1};
    for (bool distinct : {false, true}) {
      CHECK(pn_rate_records_list_check(B, cur.data(), all.data(), 5, distinct) == 0);            // three rates in one call
      CHECK(pn_rate_records_list_check(B, cur.data(), NULL, 0, distinct) == 0);
      CHECK(pn_rate_records_list_check(B, cur.data(), NULL, 2, distinct) == -1);
      CHECK(pn_rate_records_list_check(B, cur.data(), all.data(), -5, distinct) == -1);
      CHECK(pn_rate_records_list_check(B, cur.data(), with48.data(), 2, distinct) == -1 && says("no converter state") && says("stream 1"));
      CHECK(pn_rate_records_list_check(B, cur.data(), only48.data(), 1, distinct) == -1 && says("no converter state"));
      for (int32_t out : {6, -1, 1 << 30, -(1 << 30)}) {
        std::vector<int32_t> o = {0, out, 2};
        CHECK(pn_rate_records_list_check(B, cur.data(), o.data(), 3, distinct) == -1 && says("out of range"));
      }
      // a single-rate converter (no table of rates): only the id rule
      CHECK(pn_rate_records_list_check(B, NULL, with48.data(), 2, distinct) == 0);
    }
    CHECK(pn_rate_records_list_check(B, cur.data(), dup.data(), 3, false) == 0);                 // export: duplicates allowed
    CHECK(pn_rate_records_list_check(B, cur.data(), dup.data(), 3, true) == -1 && says("twice"));
    std::vector<int32_t> many = {0, 2, 3, 4, 5, 0, 2};
    CHECK(pn_rate_records_list_check(B, cur.data(), many.data(), 7, true) == -1);
    CHECK(pn_rate_records_list_check(B, cur.data(), many.data(), 7, false) == 0);
  }
  // ---- the header verdict, against the host check on exactly-sized records of every rate
  for (int R : rates) {
    const size_t want = 4 * pn_rate_record_words(pn_rate_factor(R));
    uint32_t good[4];
    pn_rate_record_header(good, R);
    CHECK(good[2] == want && (int32_t)good[3] == R);
    const int other = R == 8000 ? 16000 : 8000;
    struct Case { uint32_t h[4]; int verdict; } cases[] = {
        {{good[0], good[1], good[2], good[3]}, PN_SS_OK},
        {{good[0] ^ 0x01000000u, good[1], good[2], good[3]}, PN_SS_BAD_MAGIC},
        {{good[0], 2, good[2], good[3]}, PN_SS_BAD_VERSION},
        {{0, 0, good[2], good[3]}, PN_SS_BAD_MAGIC},
        {{good[0], good[1], (uint32_t)(4 * pn_rate_record_words(pn_rate_factor(other))), (uint32_t)other}, PN_SS_BAD_RATE},
        {{good[0], good[1], good[2], (uint32_t)other}, PN_SS_BAD_RATE},
        {{good[0], good[1], good[2], 44100u}, PN_SS_BAD_RATE},
        {{good[0], good[1], good[2], 48000u}, PN_SS_BAD_RATE},
        {{good[0], good[1], good[2] + 4, good[3]}, PN_SS_BAD_SIZE},
        {{good[0], good[1], 0, good[3]}, PN_SS_BAD_SIZE},
        {{good[0], good[1], (uint32_t)(4 * pn_rate_record_words(pn_rate_factor(other))), good[3]}, PN_SS_BAD_SIZE},
    };
    for (const Case &c : cases) {
      CHECK(pn_rate_header_verdict(c.h[0], c.h[1], c.h[2], c.h[3], R) == c.verdict);
      std::vector<unsigned char> rec(want, 0x5a);                  // exactly a record of R: the check reads its 16 header bytes only
      memcpy(rec.data(), c.h, 16);
      CHECK(pn_rate_record_check(rec.data(), rec.size(), R) == c.verdict);
      CHECK(c.verdict == PN_SS_OK || pn_last_error()[0]);
    }
    // a slot without a filter gives every header BAD_RATE, and the verdict reads nothing
    CHECK(pn_rate_header_verdict(good[0], good[1], good[2], good[3], 48000) == PN_SS_BAD_RATE);
    CHECK(pn_rate_header_verdict(good[0], good[1], good[2], good[3], 0) == PN_SS_BAD_RATE);
    // the buffer's own length stays the host check's business: a good header in a short or long buffer
    std::vector<unsigned char> shortrec(want - 4, 0), longrec(want + 4, 0), tiny(15, 0);
    memcpy(shortrec.data(), good, 16); memcpy(longrec.data(), good, 16);
    CHECK(pn_rate_record_check(shortrec.data(), shortrec.size(), R) == PN_SS_BAD_SIZE);
    CHECK(pn_rate_record_check(longrec.data(), longrec.size(), R) == PN_SS_BAD_SIZE);
    CHECK(pn_rate_record_check(tiny.data(), tiny.size(), R) == PN_SS_BAD_SIZE);
    CHECK(pn_rate_record_check(NULL, want, R) == PN_SS_BAD_ARG);
  }
  puts("ok");
  return 0;
}
