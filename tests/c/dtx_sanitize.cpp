// CPU-only sanitizer harness of the DTX send side's rules (tests/test_dtx_host.py builds it with
// g++ -DPN_NO_HIP -ffp-contract=off -fsanitize=address,undefined, like cng_sanitize.cpp): pn_dtx_rules.h over exactly-sized heap
// buffers — a row of exactly n_s floats at every row length, a state of exactly 24 words, a report of exactly 8, exactly 13 lags, a SID
// of exactly 14 bytes, a workspace of exactly PN_DTX_WS_WORDS floats — through every decision, the rows no finite arithmetic survives
// (NaN, inf, a square that overflows), subnormals, zeros, +-full scale, the counters at their ceilings, every order, the refusals.
// Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_dtx_rules.h"
#include <stdio.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "dtx_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

static uint32_t rnd(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float noise(uint32_t &s, float amp) { return amp * ((float)(rnd(s) & 0xffff) - 32767.5f) * (1.0f / 32768.0f); }

int main() {
  static_assert(PN_DTX_N_PARAMS == 9 && PN_DTX_REPORT_WORDS == 8 && PN_DTX_STATE_WORDS == 24 && PN_DTX_LAGS == 13 && PN_DTX_WS_WORDS >= 16 + 13, "the header's constants");
  // ---- the table
  CHECK(pn_dtx_level_hd(0.0f) == 127 && pn_dtx_level_hd(1.0f) == 0 && pn_dtx_level_hd(NAN) == 0 && pn_dtx_level_hd(INFINITY) == 0 && pn_dtx_level_hd(-1.0f) == 127);
  for (int L = 0; L < 128; L++) CHECK(pn_dtx_level_hd(pn_kCngLevel[L] * pn_kCngLevel[L]) == L);
  { const float e[127] = PN_DTX_EDGES; for (int i = 0; i + 1 < 127; i++) CHECK(e[i] > e[i + 1] && pn_dtx_level_hd(e[i]) == i); }
  { uint32_t c; const float cf = PN_DTX_KQ; memcpy(&c, &cf, 4); CHECK(c == 0x42fe03f8u); }
  // ---- parameters
  std::vector<float> p(PN_DTX_N_PARAMS);
  pn_dtx_default_params_host(p.data());
  CHECK(pn_dtx_params_check_host(p.data()) == 0 && pn_dtx_params_check_host(NULL) == -1);
  for (int i = 0; i < PN_DTX_N_PARAMS; i++) {
    std::vector<float> q(p);
    q[i] = NAN;
    CHECK(pn_dtx_params_check_host(q.data()) == -1 && strstr(pn_last_error(), "index"));
    q[i] = -3.0f;
    CHECK(pn_dtx_params_check_host(q.data()) == -1);
  }
  // ---- frames over exactly-sized buffers, at every row length and order
  static const int kRows[5] = {80, 160, 240, 320, 480};
  uint32_t seed = 12345u;
  long decisions[3] = {0, 0, 0};
  for (int ri = 0; ri < 5; ri++)
    for (int order = 0; order <= 12; order += 3) {
      const int ns = kRows[ri];
      p[PN_DTX_ORDER] = (float)order; p[PN_DTX_HANGOVER] = 2.0f; p[PN_DTX_MAX_INTERVAL] = 5.0f; p[PN_DTX_FLOOR_DRIFT] = 1.9f;
      std::vector<uint32_t> st(PN_DTX_STATE_WORDS, 0u), rep(PN_DTX_REPORT_WORDS);
      for (int t = 0; t < 60; t++) {
        std::vector<float> row(ns);
        float prev = 0.0f;
        for (int n = 0; n < ns; n++) { prev = 0.8f * prev + noise(seed, t % 20 < 4 ? 0.3f : 1e-3f); row[n] = prev; }
        if (t == 30) for (int n = 0; n < ns; n++) row[n] = 0.0f;
        if (t == 33) row[ns - 1] = NAN;
        if (t == 36) row[0] = INFINITY;
        if (t == 39) row[ns / 2] = 3e19f;
        if (t == 42) for (int n = 0; n < ns; n++) row[n] = n % 2 ? -1e-41f : 1e-41f;
        if (t == 45) for (int n = 0; n < ns; n++) row[n] = n % 2 ? -1.0f : 1.0f;
        const int d = pn_dtx_frame_host(p.data(), st.data(), row.data(), ns, t % 7 == 6 ? NULL : rep.data());
        CHECK(d >= PN_DTX_FRAME && d <= PN_DTX_NONE);
        decisions[d]++;
        if (t == 33 || t == 36 || t == 39) CHECK(d == PN_DTX_FRAME);
        if (t % 7 != 6) CHECK(rep[0] == (uint32_t)d && (rep[1] & PN_DTX_ON) && ((rep[1] & PN_DTX_NONFINITE) != 0) == (t == 33 || t == 36 || t == 39));
        std::vector<uint8_t> sid(PN_CNG_SID_BYTES);
        pn_dtx_sid_bytes(&st[PN_DTX_W_SID], sid.data());
        CHECK(pn_cng_sid_check(sid.data()) == 0 && sid[0] <= order && st[22] == 0u && st[23] == 0u);
        PnCngSid dec;
        CHECK(pn_cng_sid_decode_host(sid.data(), &dec) == 0);
      }
    }
  CHECK(decisions[0] > 0 && decisions[1] > 0 && decisions[2] > 0);
  // ---- the counters at their ceilings
  { pn_dtx_default_params_host(p.data());
    p[PN_DTX_HANGOVER] = 0.0f;
    std::vector<uint32_t> st(PN_DTX_STATE_WORDS, 0u), rep(PN_DTX_REPORT_WORDS);
    std::vector<float> row(80);
    for (int n = 0; n < 80; n++) row[n] = n % 2 ? -1e-3f : 1e-3f;
    CHECK(pn_dtx_frame_host(p.data(), st.data(), row.data(), 80, rep.data()) == PN_DTX_FRAME);
    CHECK(pn_dtx_frame_host(p.data(), st.data(), row.data(), 80, rep.data()) == PN_DTX_SID && (rep[7] >> 16) == 1u);
    st[PN_DTX_W_FRAMES] = PN_DTX_SAT; st[PN_DTX_W_SINCE] = PN_DTX_SINCE_MAX; st[PN_DTX_W_SID + 3] |= 0xffff0000u;
    CHECK(pn_dtx_frame_host(p.data(), st.data(), row.data(), 80, rep.data()) == PN_DTX_NONE && st[PN_DTX_W_FRAMES] == PN_DTX_SAT && st[PN_DTX_W_SINCE] == PN_DTX_SINCE_MAX);
    p[PN_DTX_MAX_INTERVAL] = 65535.0f;
    CHECK(pn_dtx_frame_host(p.data(), st.data(), row.data(), 80, rep.data()) == PN_DTX_SID && (rep[7] >> 16) == 0u && st[PN_DTX_W_SINCE] == 0u);
  }
  // ---- the Levinson step alone over exactly 13 lags and 14 bytes
  { std::vector<float> R(PN_DTX_LAGS);
    std::vector<uint8_t> sid(PN_CNG_SID_BYTES);
    for (int order = 0; order <= 12; order++) {
      for (int j = 0; j < PN_DTX_LAGS; j++) R[j] = powf(0.9f, (float)j) * 1e-4f;
      CHECK(pn_dtx_sid_from_acorr_host(R.data(), order, sid.data()) == order && sid[0] == order && sid[1] == 40 && pn_cng_sid_check(sid.data()) == 0);
      for (int j = 0; j < PN_DTX_LAGS; j++) R[j] = j % 2 ? -0.999f : 1.0f;
      CHECK(pn_dtx_sid_from_acorr_host(R.data(), order, sid.data()) >= 0 && pn_cng_sid_check(sid.data()) == 0);
      R[0] = NAN;
      CHECK(pn_dtx_sid_from_acorr_host(R.data(), order, sid.data()) == 0 && sid[0] == 0);
    }
    CHECK(pn_dtx_sid_from_acorr_host(R.data(), 13, sid.data()) == -1 && pn_dtx_sid_from_acorr_host(R.data(), -1, sid.data()) == -1);
    CHECK(pn_dtx_sid_from_acorr_host(NULL, 1, sid.data()) == -1 && pn_dtx_sid_from_acorr_host(R.data(), 1, NULL) == -1);
  }
  // ---- refusals of a frame
  { pn_dtx_default_params_host(p.data());
    std::vector<uint32_t> st(PN_DTX_STATE_WORDS, 0u);
    std::vector<float> row(80, 0.0f);
    CHECK(pn_dtx_frame_host(NULL, st.data(), row.data(), 80, NULL) == -1 && pn_dtx_frame_host(p.data(), NULL, row.data(), 80, NULL) == -1);
    CHECK(pn_dtx_frame_host(p.data(), st.data(), NULL, 80, NULL) == -1 && pn_dtx_frame_host(p.data(), st.data(), row.data(), 79, NULL) == -1);
    const std::vector<uint8_t> on(2, 1);
    const int32_t ids[2] = {0, 1}, twice[2] = {1, 1};
    CHECK(pn_dtx_on_set_check(2, ids, 2, on.data()) == 0 && pn_dtx_on_set_check(2, twice, 2, on.data()) == -1 && pn_dtx_on_set_check(2, ids, 2, NULL) == -1);
  }
  printf("ok\n");
  return 0;
}
