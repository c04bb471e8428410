// CPU-only sanitizer harness of the comfort-noise rules (tests/test_cng_host.py builds it with
// g++ -DPN_NO_HIP -ffp-contract=off -fsanitize=address,undefined, like plc_sanitize.cpp): pn_cng_rules.h over exactly-sized heap
// buffers — a SID of exactly 14 bytes (and of 2 + M where only those are read), a state of exactly 16 words, a row of exactly n_s
// floats at every row length, the table at both ends, the counter through its wrap, the counts at their ceiling, the refusals.
// Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_cng_rules.h"
#include <stdio.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "cng_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

int main() {
  static_assert(PN_CNG_MAX_ORDER == 12 && PN_CNG_SID_BYTES == 14 && PN_CNG_STATE_WORDS == 16 && PN_CNG_REPORT_WORDS == 4 && PN_CNG_DEFAULT_LEVEL == 60 && PN_CNG_TILE == 80,
                "the header's constants");
  // ---- the table and the constants
  CHECK(pn_kCngLevel[0] == 1.0f && pn_kCngLevel[20] == 0.1f && pn_kCngLevel[127] > 4.46e-7f && pn_kCngLevel[127] < 4.47e-7f);
  { uint32_t c; const float cf = PN_CNG_C; memcpy(&c, &cf, 4); CHECK(c == 0x381cc471u); }
  CHECK(pn_cng_mix(0u) == 0u && pn_cng_u(0u, 0u) == -65535 && pn_cng_key(7u, 0u) == 7u && pn_cng_key(0u, 1u) == 0x9e3779b1u);
  CHECK(pn_cng_count(0u) == 1u && pn_cng_count(PN_CNG_SAT - 1u) == PN_CNG_SAT && pn_cng_count(PN_CNG_SAT) == PN_CNG_SAT);
  // ---- decode over exactly-sized SIDs
  { std::vector<uint8_t> sid(PN_CNG_SID_BYTES);
    pn_cng_default_sid(sid.data());
    PnCngSid d;
    CHECK(pn_cng_sid_decode_host(sid.data(), &d) == 0 && d.M == 0 && d.g == pn_kCngLevel[60]);
    for (int M = 0; M <= 12; M++) {
      std::vector<uint8_t> s(2 + M);                 // only 2 + M bytes exist: nothing behind N_M is read
      s[0] = (uint8_t)M; s[1] = 127;
      for (int i = 0; i < M; i++) s[2 + i] = (uint8_t)(i % 2 ? 254 : 0);
      CHECK(pn_cng_sid_check(s.data()) == 0);
      std::vector<uint8_t> kept(PN_CNG_SID_BYTES, 0xAA);
      pn_cng_sid_store(s.data(), kept.data());
      CHECK(kept[0] == M && kept[1] == 127 && (M == 12 || kept[13] == 0));
      CHECK(pn_cng_sid_decode_host(kept.data(), &d) == 0 && d.M == M && d.g > 0.0f && d.g <= pn_kCngLevel[127]);
      for (int i = 0; i < 12; i++) CHECK(i < M ? d.k[i] == (i % 2 ? 32766.0f : -32766.0f) / 32768.0f : d.k[i] == 0.0f);
    }
    sid[0] = 13; CHECK(pn_cng_sid_check(sid.data()) == -1);
    sid[0] = 1; sid[1] = 128; CHECK(pn_cng_sid_check(sid.data()) == -1);
    sid[1] = 0; sid[2] = 255; CHECK(pn_cng_sid_decode_host(sid.data(), &d) == -1);
    sid[0] = 0; CHECK(pn_cng_sid_decode_host(sid.data(), &d) == 0 && d.g == 1.0f);      // (N_1 is not looked at with M = 0)
    CHECK(pn_cng_sid_check(NULL) == -1 && pn_cng_sid_decode_host(sid.data(), NULL) == -1);
    std::vector<int32_t> ids = {1, 0};
    std::vector<uint8_t> two(2 * PN_CNG_SID_BYTES, 0);
    CHECK(pn_cng_sids_set_check(2, ids.data(), 2, two.data(), PN_CNG_SID_BYTES) == 0 && pn_cng_sids_set_check(2, ids.data(), 2, two.data(), 13) == -1);
    CHECK(pn_cng_sids_set_check(2, ids.data(), 2, NULL, 14) == -1 && pn_cng_sids_set_check(1, ids.data(), 2, two.data(), 14) == -1);
    two[PN_CNG_SID_BYTES] = 13;
    CHECK(pn_cng_sids_set_check(2, ids.data(), 2, two.data(), PN_CNG_SID_BYTES) == -1); }
  // ---- rows of exactly n_s floats, a state of exactly 16 words, through the counter's wrap
  for (int ns : {80, 160, 240, 320, 480})
    for (int M : {0, 1, 2, 12})
      for (int ext = 0; ext < 3; ext++) {
        std::vector<uint8_t> sid(PN_CNG_SID_BYTES, 0);
        sid[0] = (uint8_t)M; sid[1] = 30;
        for (int i = 0; i < M; i++) sid[2 + i] = ext == 0 ? 0 : ext == 1 ? 254 : (uint8_t)(40 + 17 * i);
        PnCngSid d;
        CHECK(pn_cng_sid_decode_host(sid.data(), &d) == 0);
        std::vector<uint32_t> st(PN_CNG_STATE_WORDS, 0u), rep(4, 0u);
        st[PN_CNG_W_CTR] = 0xffffffffu - 100u; st[PN_CNG_W_TOTAL] = PN_CNG_SAT - 1u;
        for (int t = 0; t < 4; t++) {
          std::vector<float> row(ns, NAN);
          CHECK(pn_cng_frame_host(&d, st.data(), pn_cng_key(5u, 3u), t > 0, ns, row.data(), rep.data()) == 0);
          for (float v : row) CHECK(isfinite(v) && fabsf(v) < 1.0f);
          CHECK(rep[0] == (uint32_t)(t + 1) && rep[1] == PN_CNG_SAT && rep[3] == 0xffffffffu - 100u + (uint32_t)((t + 1) * ns));
          float g; memcpy(&g, &rep[2], 4); CHECK(g == d.g);
        }
        std::vector<float> row(ns);
        CHECK(pn_cng_frame_host(&d, st.data(), 0u, 0, ns - 1, row.data(), NULL) == -1 && pn_cng_frame_host(&d, st.data(), 0u, 0, 0, row.data(), NULL) == -1);
        CHECK(pn_cng_frame_host(NULL, st.data(), 0u, 0, ns, row.data(), NULL) == -1 && pn_cng_frame_host(&d, NULL, 0u, 0, ns, row.data(), NULL) == -1 &&
              pn_cng_frame_host(&d, st.data(), 0u, 0, ns, NULL, NULL) == -1);
        d.M = 13; CHECK(pn_cng_frame_host(&d, st.data(), 0u, 0, ns, row.data(), NULL) == -1);
      }
  // ---- M = 0 is the scaled excitation itself; a changed SID ramps from prev to g
  { PnCngSid d = {}; d.g = 0.5f;
    std::vector<uint32_t> st(PN_CNG_STATE_WORDS, 0u);
    std::vector<float> row(80);
    CHECK(pn_cng_frame_host(&d, st.data(), 9u, 0, 80, row.data(), NULL) == 0);
    for (int n = 0; n < 80; n++) CHECK(row[n] == 0.5f * ((float)pn_cng_u((uint32_t)n, 9u) * PN_CNG_C));
    d.g = 0.25f;
    CHECK(pn_cng_frame_host(&d, st.data(), 9u, 1, 80, row.data(), NULL) == 0);
    CHECK(row[79] == (0.5f + 1.0f * (0.25f - 0.5f)) * ((float)pn_cng_u(159u, 9u) * PN_CNG_C));
    CHECK(row[0] == (0.5f + (1.0f / 80.0f) * (0.25f - 0.5f)) * ((float)pn_cng_u(80u, 9u) * PN_CNG_C)); }
  puts("ok");
  return 0;
}
