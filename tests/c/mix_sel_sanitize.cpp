// CPU-only sanitizer harness of the conference mix's loudest-N rules (tests/test_mix_sel_host.py builds it with
// g++ -DPN_NO_HIP -fsanitize=address,undefined, like conf_sanitize.cpp): pn_mix_rules.h over exactly-sized heap buffers — the level
// of rows of zeros, ones, subnormals, NaN, inf and FLT_MAX and of a row whose level depends on the order, the hold, the selection
// at k = 0, 1 and 32 with ties and a NaN, and the three value checks with the index they name.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_mix_rules.h"
#include <stdio.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "mix_sel_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

typedef std::vector<float> F;

int main() {
  static_assert(PN_MIX_REPORT_WORDS == 4 && PN_FRAME == 480, "the header's constants");
  // ---- the level
  { F z(480, 0.0f), nz(480, -0.0f), one(480, 1.0f), sub(480, 1e-30f), big(480, FLT_MAX);
    CHECK(pn_mix_level_host(z.data()) == 0.0f && !signbit(pn_mix_level_host(z.data())));
    CHECK(pn_mix_level_host(nz.data()) == 0.0f && !signbit(pn_mix_level_host(nz.data())));     // (-0)(-0) = +0
    CHECK(pn_mix_level_host(one.data()) == 480.0f);
    CHECK(pn_mix_level_host(sub.data()) == 0.0f);                                              // every product underflows
    CHECK(isinf(pn_mix_level_host(big.data())));
    F n(one); n[479] = NAN; CHECK(isnan(pn_mix_level_host(n.data())));
    F i(one); i[0] = -INFINITY; CHECK(isinf(pn_mix_level_host(i.data())) && pn_mix_level_host(i.data()) > 0);
    // the order: 4096 at sample 0 (its square 2^24), 1 everywhere else.  Group 0 is ((2^24 + 1) + 1) + 1 = 2^24 (each add rounds
    // back to even), the other 119 groups are 4; the butterfly adds 4s and 8s .. to 2^24 exactly: 2^24 + 476.  The sequential sum
    // never leaves 2^24
    F o(480, 1.0f); o[0] = 4096.0f;
    CHECK(pn_mix_level_host(o.data()) == 16777216.0f + 476.0f);
    float seq = 0.0f;
    for (int j = 0; j < 480; j++) { const float p = o[j] * o[j]; seq = seq + p; }
    CHECK(seq == 16777216.0f); }
  // ---- the hold
  { CHECK(pn_mix_hold_level(0.0f, 100.0f, 1.0f) == 1.0f);                  // d == 0: E
    CHECK(pn_mix_hold_level(0.5f, 100.0f, 1.0f) == 50.0f && pn_mix_hold_level(0.5f, 100.0f, 50.0f) == 50.0f && pn_mix_hold_level(0.5f, 100.0f, 51.0f) == 51.0f);
    CHECK(pn_mix_hold_level(0.5f, INFINITY, 1.0f) == 1.0f && pn_mix_hold_level(0.5f, NAN, 1.0f) == 1.0f);   // a non-finite level never sticks
    CHECK(isnan(pn_mix_hold_level(0.5f, 100.0f, NAN)) && isinf(pn_mix_hold_level(0.5f, 100.0f, INFINITY)));
    CHECK(pn_mix_hold_check(0.0f) == 0 && pn_mix_hold_check(-0.0f) == 0 && pn_mix_hold_check(0.99999994f) == 0);
    CHECK(pn_mix_hold_check(1.0f) == -1 && pn_mix_hold_check(-1e-30f) == -1 && pn_mix_hold_check(NAN) == -1 && pn_mix_hold_check(INFINITY) == -1); }
  // ---- the selection
  { std::vector<uint8_t> sel(32, 7);
    CHECK(pn_mix_select_host(NULL, 0, 3, NULL) == 0);
    F one = {5.0f};
    CHECK(pn_mix_select_host(one.data(), 1, 1, sel.data()) == 1 && sel[0] == 1 && sel[1] == 7);
    F lv = {1.0f, 9.0f, 3.0f, 9.0f, 0.0f, -9.0f};                          // ties 9, 9, |-9|: the lower slot wins
    CHECK(pn_mix_select_host(lv.data(), 6, 2, sel.data()) == 2 && sel[1] == 1 && sel[3] == 1 && sel[5] == 0 && sel[0] == 0 && sel[2] == 0);
    CHECK(pn_mix_select_host(lv.data(), 6, 1, sel.data()) == 1 && sel[1] == 1 && sel[3] == 0);
    CHECK(pn_mix_select_host(lv.data(), 6, 0, sel.data()) == 6 && pn_mix_select_host(lv.data(), 6, 6, sel.data()) == 6 && pn_mix_select_host(lv.data(), 6, 32, sel.data()) == 6);
    lv[4] = NAN; lv[0] = INFINITY;                                         // NaN ranks above +inf
    CHECK(pn_mix_select_host(lv.data(), 6, 1, sel.data()) == 1 && sel[4] == 1);
    CHECK(pn_mix_select_host(lv.data(), 6, 2, sel.data()) == 2 && sel[4] == 1 && sel[0] == 1);
    F z(32, 0.0f);                                                         // all equal: the first N slots
    std::vector<uint8_t> s32(32, 7);
    CHECK(pn_mix_select_host(z.data(), 32, 3, s32.data()) == 3 && s32[0] && s32[1] && s32[2] && !s32[3] && !s32[31]);
    CHECK(pn_mix_select_host(z.data(), 33, 3, s32.data()) == -1 && pn_mix_select_host(z.data(), 32, 33, s32.data()) == -1 && pn_mix_select_host(z.data(), -1, 0, s32.data()) == -1);
    CHECK(pn_mix_select_host(NULL, 2, 0, s32.data()) == -1 && pn_mix_select_host(z.data(), 2, 0, NULL) == -1); }
  // ---- the value checks name the first bad index
  { F g = {1.0f, 0.0f, -0.0f, 1e-20f, FLT_MAX, 0.5f};
    CHECK(pn_mix_gains_list_check(g.data(), 6) == 0 && pn_mix_gains_list_check(NULL, 0) == 0 && pn_mix_gains_list_check(NULL, 1) == -1 && pn_mix_gains_list_check(g.data(), -1) == -1);
    for (int at = 0; at < 6; at++)
      for (float bad : {NAN, INFINITY, -INFINITY, -1.0f, -1e-40f}) {
        F t(g);
        t[at] = bad;
        if (at < 5) t[5] = NAN;                                            // a later bad one is not the one named
        CHECK(pn_mix_gains_list_check(t.data(), 6) == -1);
        char want[32];
        snprintf(want, sizeof(want), "at index %d:", at);
        CHECK(strstr(pn_last_error(), want) != NULL);
      }
    std::vector<int32_t> ids = {3, 0, 2}, dup = {3, 0, 3}, far = {3, 4, 2};
    F w = {1.0f, 2.0f, 0.0f}, wb = {1.0f, 2.0f, -2.0f};
    CHECK(pn_mix_gains_set_check(4, ids.data(), 3, w.data()) == 0 && pn_mix_gains_set_check(4, ids.data(), 0, NULL) == 0);
    CHECK(pn_mix_gains_set_check(4, dup.data(), 3, w.data()) == -1 && strstr(pn_last_error(), "twice"));
    CHECK(pn_mix_gains_set_check(4, far.data(), 3, w.data()) == -1 && strstr(pn_last_error(), "out of range"));
    CHECK(pn_mix_gains_set_check(4, ids.data(), 3, wb.data()) == -1 && strstr(pn_last_error(), "at index 2:"));
    std::vector<int32_t> n = {0, 32, 5}, nb = {0, 33, -1}, nn = {-1, 2, 2};
    CHECK(pn_mix_speakers_set_check(4, ids.data(), 3, n.data()) == 0 && pn_mix_speakers_set_check(4, ids.data(), 0, NULL) == 0);
    CHECK(pn_mix_speakers_set_check(4, ids.data(), 3, nb.data()) == -1 && strstr(pn_last_error(), "at index 1:"));
    CHECK(pn_mix_speakers_set_check(4, ids.data(), 3, nn.data()) == -1 && strstr(pn_last_error(), "at index 0:"));
    CHECK(pn_mix_speakers_set_check(4, dup.data(), 3, n.data()) == -1 && pn_mix_speakers_set_check(4, far.data(), 3, n.data()) == -1 && pn_mix_speakers_set_check(4, ids.data(), 3, NULL) == -1); }
  puts("ok");
  return 0;
}
