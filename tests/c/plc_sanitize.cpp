// CPU-only sanitizer harness of the packet-loss concealment rules (tests/test_plc_host.py builds it with
// g++ -DPN_NO_HIP -ffp-contract=off -fsanitize=address,undefined, like mix_sel_sanitize.cpp): pn_plc_rules.h over exactly-sized heap
// buffers — a history of exactly 1920 floats under the search and under the period at every lag from 240 to 720 (P = 720 reads back
// to hist[1920 - 1440 + 540]), a q of exactly P floats, the gain at its edges, the synthetic sample at the last index of q, an
// exactly periodic history continued bit for bit, the score's refusals.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_plc_rules.h"
#include <stdio.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "plc_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

typedef std::vector<float> F;

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main() {
  static_assert(PN_PLC_HIST == 1920 && PN_PLC_P_MIN == 240 && PN_PLC_P_MAX == 720 && PN_PLC_REPORT_WORDS == 4 && PN_FRAME == 480 && PN_PLC_STATE_BYTES == 10576,
                "the header's constants");
  // ---- the gain
  CHECK(pn_plc_gain_host(0) == 1.0f && pn_plc_gain_host(479) == 1.0f && pn_plc_gain_host(480) == 1.0f);
  CHECK(pn_plc_gain_host(481) == 2399.0f / 2400.0f && pn_plc_gain_host(960) == 0.8f && pn_plc_gain_host(2879) == 1.0f / 2400.0f);
  CHECK(pn_plc_gain_host(2880) == 0.0f && !signbit(pn_plc_gain_host(2880)) && pn_plc_gain_host((int64_t)1 << 40) == 0.0f && pn_plc_gain_host(-5) == 1.0f);
  // ---- the score
  CHECK(pn_plc_score(0.0f, 1.0f) == 0.0f && pn_plc_score(-1.0f, 1.0f) == 0.0f && pn_plc_score(1.0f, 0.0f) == 0.0f && pn_plc_score(NAN, 1.0f) == 0.0f && pn_plc_score(1.0f, NAN) == 0.0f);
  CHECK(pn_plc_score(INFINITY, INFINITY) == 0.0f && pn_plc_score(3.0f, 2.0f) == 4.5f && isinf(pn_plc_score(1e30f, 1.0f)));
  { F sc = {0.0f, 2.0f, 2.0f, 1.0f}, z(5, 0.0f), n = {NAN, 0.0f, 1.0f};
    CHECK(pn_plc_best(sc.data(), 4) == 1 && pn_plc_best(z.data(), 5) == 0 && pn_plc_best(n.data(), 3) == 2); }
  // ---- the search and the period over exactly-sized buffers
  { F zero(PN_PLC_HIST, 0.0f);
    CHECK(pn_plc_coarse_host(zero.data()) == 40 && pn_plc_pitch_host(zero.data()) == 240);
    F bad(PN_PLC_HIST, NAN);
    CHECK(pn_plc_pitch_host(bad.data()) == 240);
    uint32_t seed = 1;
    F noise(PN_PLC_HIST);
    for (float &v : noise) v = (float)((int)(lcg(seed) & 0xffff) - 32768) / 32768.0f;
    const int P = pn_plc_pitch_host(noise.data());
    CHECK(P >= PN_PLC_P_MIN && P <= PN_PLC_P_MAX);
    for (int l = PN_PLC_LAG_LO; l <= PN_PLC_LAG_HI; l++) { const int L = pn_plc_fine_host(noise.data(), l); CHECK(L >= PN_PLC_P_MIN && L <= PN_PLC_P_MAX && L >= 6 * l - 5 && L <= 6 * l + 5); }
    for (int p = PN_PLC_P_MIN; p <= PN_PLC_P_MAX; p++) {
      F q(p, -1.0f);
      CHECK(pn_plc_period_host(noise.data(), p, q.data()) == 0);
      CHECK(q[0] == noise[PN_PLC_HIST - p] && q[p - p / 4 - 1] == noise[PN_PLC_HIST - p / 4 - 1]);
      CHECK(pn_plc_syn_host(q.data(), p, (uint32_t)((p - 1) / PN_FRAME), (p - 1) % PN_FRAME) == pn_plc_gain_host(p - 1) * q[p - 1] && pn_plc_syn_host(q.data(), p, 0, 479) == q[479 % p]);
      CHECK(pn_plc_syn_host(q.data(), p, 5, 479) == (1.0f / 2400.0f) * q[2879 % p]);
      CHECK(pn_plc_syn_host(q.data(), p, 6, 0) == 0.0f && pn_plc_syn_host(q.data(), p, PN_PLC_RUN_MAX, 479) == 0.0f);
    }
    F q(PN_PLC_P_MAX);
    CHECK(pn_plc_period_host(noise.data(), 239, q.data()) == -1 && pn_plc_period_host(noise.data(), 721, q.data()) == -1);
    CHECK(pn_plc_period_host(NULL, 240, q.data()) == -1 && pn_plc_period_host(noise.data(), 240, NULL) == -1); }
  // ---- an exactly periodic history is continued bit for bit, whichever multiple of the period the search takes
  for (int per : {240, 263, 359, 480, 719, 720}) {
    F base(per), hist(PN_PLC_HIST);
    for (int i = 0; i < per; i++) {
      double v = 0;
      for (int h = 1; h <= 6; h++) v += cos(2.0 * 3.14159265358979323846 * h * (i + 0.25 * h) / per) / h;
      base[i] = (float)(0.2 * v);
    }
    for (int i = 0; i < PN_PLC_HIST; i++) hist[i] = base[i % per];
    const int P = pn_plc_pitch_host(hist.data());
    CHECK(P % per == 0);
    F q(P);
    CHECK(pn_plc_period_host(hist.data(), P, q.data()) == 0);
    for (int n = 0; n < PN_FRAME; n++) CHECK(pn_plc_syn_host(q.data(), P, 0, n) == base[(PN_PLC_HIST + n) % per]);
  }
  // ---- the cross-fade: its ends, and equal inputs
  CHECK(pn_plc_xfade_host(1.0f, 3.0f, 0) == 1.0f + (1.0f / 480.0f) * 2.0f && pn_plc_xfade_host(0.5f, 0.5f, 100) == 0.5f);
  CHECK(pn_plc_xfade_host(0.0f, 1.0f, 239) == 479.0f / 480.0f);
  puts("ok");
  return 0;
}
