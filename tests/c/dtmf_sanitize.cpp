// CPU-only sanitizer harness of the DTMF detector's rule (tests/test_dtmf_host.py builds it with
// g++ -DPN_NO_HIP -ffp-contract=off -fsanitize=address,undefined, like agc_sanitize.cpp): pn_dtmf_rules.h over exactly-sized heap
// buffers — a row of exactly 480 floats, a state of exactly 24 words, a report of exactly four, the parameters at exactly seven floats,
// the tables at exactly 8 x 480, 8 x 480 and 16 — through a keypad sequence, the hostile rows (NaN, inf, 3e38, zeros, -0.0,
// subnormals, a full-scale square), a concealed frame, every parameter's edges, the counters' saturation.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_dtmf_rules.h"
#include <stdio.h>
#include <string>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "dtmf_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

typedef std::vector<float> F;
typedef std::vector<uint32_t> U;

static const char kDigits[] = "123A456B789C*0#D";
// frame `frame` of the digit's dual tone, both at amplitude amp, phases running on from sample 0
static F tone(char digit, float amp, int frame) {
  const int i = (int)(strchr(kDigits, digit) - kDigits);
  F x(PN_FRAME);
  for (int j = 0; j < PN_FRAME; j++) {
    const double t = (frame * PN_FRAME + j) / 48000.0;
    x[j] = (float)(amp * (sin(6.283185307179586 * pn_dtmf_freq(i / 4) * t) + sin(6.283185307179586 * pn_dtmf_freq(4 + i % 4) * t)));
  }
  return x;
}

int main() {
  static_assert(PN_DTMF_N_PARAMS == 7 && PN_DTMF_REPORT_WORDS == 4 && PN_DTMF_STATE_BYTES == 96 && PN_DTMF_ON == 1 && PN_DTMF_HIT == 2 && PN_DTMF_BEGIN == 4 &&
                PN_DTMF_END == 8 && PN_DTMF_HELD_LOST == 16 && PN_DTMF_OFF_FRAMES == 6, "the header's constants");
  F P(PN_DTMF_N_PARAMS);
  pn_dtmf_default_params_host(P.data());
  CHECK(P[0] == 0.005f && P[1] == 0.5f && P[2] == 6.3f && P[3] == 6.3f && P[4] == 6.3f && P[5] == 3.0f && P[6] == 2.0f);
  CHECK(pn_dtmf_params_check_host(P.data()) == 0 && pn_dtmf_params_check_host(NULL) == -1);
  // ---- every parameter at both edges and one step outside; the frame counts are whole numbers
  { const float lo[7] = {0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f}, hi[7] = {1.0f, 1.0f, 100.0f, 100.0f, 100.0f, 100.0f, 100.0f};
    for (int i = 0; i < PN_DTMF_N_PARAMS; i++) {
      const bool open_lo = i == 1;
      F q = P;
      q[i] = hi[i]; CHECK(pn_dtmf_params_check_host(q.data()) == 0);
      q[i] = nextafterf(hi[i], INFINITY); CHECK(pn_dtmf_params_check_host(q.data()) == -1);
      char want[32];
      snprintf(want, sizeof(want), "index %d ", i);
      CHECK(strstr(pn_last_error(), want));
      q[i] = lo[i]; CHECK(pn_dtmf_params_check_host(q.data()) == (open_lo ? -1 : 0));
      q[i] = open_lo ? nextafterf(lo[i], INFINITY) : nextafterf(lo[i], -INFINITY); CHECK(pn_dtmf_params_check_host(q.data()) == (open_lo ? 0 : -1));
      q[i] = NAN; CHECK(pn_dtmf_params_check_host(q.data()) == -1);
      if (i >= 5) { q[i] = 2.5f; CHECK(pn_dtmf_params_check_host(q.data()) == -1 && strstr(pn_last_error(), want)); }
    } }
  // ---- the tables into buffers of their exact sizes
  { F ct(PN_DTMF_NF * PN_FRAME), st(PN_DTMF_NF * PN_FRAME), rot(2 * PN_DTMF_NF);
    CHECK(pn_dtmf_tables_host(ct.data(), st.data(), rot.data()) == 0 && pn_dtmf_tables_host(NULL, st.data(), rot.data()) == -1);
    for (int k = 0; k < PN_DTMF_NF; k++) CHECK(ct[k * PN_FRAME] == 1.0f && st[k * PN_FRAME] == 0.0f && fabsf(ct[k * PN_FRAME + 479]) <= 1.0f);
    CHECK(rot[1] == (float)cos(6.283185307179586 * ((770 * 480) % 48000) / 48000.0)); }
  // ---- the switch list
  { std::vector<int32_t> ids = {2, 0, 1}, dup = {2, 0, 2};
    std::vector<uint8_t> on = {1, 0, 7};
    CHECK(pn_dtmf_on_set_check(3, ids.data(), 3, on.data()) == 0 && pn_dtmf_on_set_check(3, dup.data(), 3, on.data()) == -1 &&
          pn_dtmf_on_set_check(2, ids.data(), 3, on.data()) == -1 && pn_dtmf_on_set_check(3, ids.data(), 3, NULL) == -1 && pn_dtmf_on_set_check(3, NULL, 0, NULL) == 0); }
  // ---- whole frames over exactly-sized buffers: 40 ms on, 40 ms off for every digit
  { U st(PN_DTMF_STATE_WORDS, 0u), rep(PN_DTMF_REPORT_WORDS, 0xdeadbeefu);
    std::string begun, ended;
    F zero(PN_FRAME, 0.0f);
    for (int n = 0; n < 16; n++)
      for (int t = 0; t < 8; t++) {
        F x = t < 4 ? tone(kDigits[n], 0.1f, t) : zero;
        const int fl = pn_dtmf_frame_host(P.data(), st.data(), x.data(), 0, rep.data());
        CHECK(fl > 0 && (fl & PN_DTMF_ON) && (uint32_t)fl == (rep[0] & 0xffu) && st[22] == 0u && st[23] == 0u && rep[2] == st[20] && rep[3] == st[21]);
        if (fl & PN_DTMF_BEGIN) begun += (char)((rep[0] >> 8) & 0xff);
        if (fl & PN_DTMF_END) ended += (char)((rep[0] >> 16) & 0xff);
      }
    CHECK(begun == kDigits && ended == kDigits && st[20] == 16u && st[21] == 0x2a302344u);      // last4: "*0#D", newest in the low byte
    // bad arguments change nothing; report4 is optional
    const U before = st;
    F x = tone('5', 0.1f, 0);
    CHECK(pn_dtmf_frame_host(NULL, st.data(), x.data(), 0) == -1 && pn_dtmf_frame_host(P.data(), NULL, x.data(), 0) == -1 && pn_dtmf_frame_host(P.data(), st.data(), NULL, 0) == -1);
    F bad = P;
    bad[5] = 0.0f;
    CHECK(pn_dtmf_frame_host(bad.data(), st.data(), x.data(), 0) == -1 && st == before);
    // a concealed frame: the state stays, word for word
    const int fl = pn_dtmf_frame_host(P.data(), st.data(), x.data(), 1, rep.data());
    CHECK(fl == (PN_DTMF_ON | PN_DTMF_HELD_LOST) && st == before && rep[2] == 16u && rep[3] == 0x2a302344u);
    CHECK(pn_dtmf_frame_host(P.data(), st.data(), x.data(), 0) > 0 && st != before); }
  { // hostile rows: never a hit, never a stuck state — a digit behind them is still found
    const float fills[] = {NAN, INFINITY, -INFINITY, 3e38f, 0.0f, -0.0f, 1e-41f, 1.0f};
    U st(PN_DTMF_STATE_WORDS, 0u), rep(PN_DTMF_REPORT_WORDS);
    for (float fill : fills) {
      F y(PN_FRAME, fill);
      if (fill == 1.0f) for (int j = 0; j < PN_FRAME; j++) y[j] = (j / 48) % 2 ? -1.0f : 1.0f;      // a full-scale square
      const int fl = pn_dtmf_frame_host(P.data(), st.data(), y.data(), 0, rep.data());
      CHECK(fl == PN_DTMF_ON && st[18] == 0u && st[20] == 0u);
    }
    int begins = 0;
    for (int t = 0; t < 6; t++) {
      F x = tone('7', 0.2f, t);
      const int fl = pn_dtmf_frame_host(P.data(), st.data(), x.data(), 0, rep.data());
      CHECK(fl > 0);
      begins += (fl & PN_DTMF_BEGIN) != 0;
    }
    CHECK(begins == 1 && (st[18] & 0xffu) == '7' && st[20] == 1u); }
  { // the counters saturate: run at 65535, dur and count at 2^32 - 1
    U st(PN_DTMF_STATE_WORDS, 0u), rep(PN_DTMF_REPORT_WORDS);
    { F x = tone('1', 0.1f, 0); CHECK(pn_dtmf_frame_host(P.data(), st.data(), x.data(), 0, rep.data()) >= 0); }      // the half sums of a first row
    st[17] = (uint32_t)'1' | (0xfffeu << 16); st[18] = (uint32_t)'1'; st[19] = 0xfffffffeu; st[20] = 0xffffffffu;
    for (int t = 1; t < 4; t++) { F x = tone('1', 0.1f, t); CHECK(pn_dtmf_frame_host(P.data(), st.data(), x.data(), 0, rep.data()) & PN_DTMF_HIT); }
    CHECK((st[17] >> 16) == 0xffffu && st[19] == 0xffffffffu && st[20] == 0xffffffffu);
    // the digit ends, another begins: count stays saturated
    F zero(PN_FRAME, 0.0f);
    int ends = 0;                                      // (the frame half tone, half silence sits ON the purity threshold: a hit or not, by rounding)
    for (int t = 0; t < 3; t++) {
      CHECK(pn_dtmf_frame_host(P.data(), st.data(), zero.data(), 0, rep.data()) >= 0);
      if (rep[0] & PN_DTMF_END) { ends++; CHECK(((rep[0] >> 16) & 0xff) == '1' && rep[1] == 0xffffffffu); }
    }
    CHECK(ends == 1 && st[18] == 0u);
    for (int t = 0; t < 4; t++) { F x = tone('9', 0.1f, t); CHECK(pn_dtmf_frame_host(P.data(), st.data(), x.data(), 0, rep.data()) >= 0); }
    CHECK((st[18] & 0xffu) == '9' && st[20] == 0xffffffffu && (st[21] & 0xffu) == '9'); }
  puts("ok");
  return 0;
}
