// CPU-only sanitizer harness of the DTMF removal rule (tests/test_dtmf_clamp_host.py builds it with
// g++ -DPN_NO_HIP -ffp-contract=off -fsanitize=address,undefined, like dtmf_sanitize.cpp): pn_dtmf_clamp_rules.h over exactly-sized heap
// buffers — a row of exactly 480 floats, a state of exactly four words, a detector report row and a report of exactly four, the
// parameters at exactly four int32 — driven by the detector's own rule (pn_dtmf_rules.h) over a keypad sequence through a delay line
// of six rows, then every row kind by hand, hostile rows, every parameter's edges, the shifts at their ends (dur >= 31, post = 8),
// the counter's and the duration's saturation.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_dtmf_rules.h"
#include "../../percepnet_amd/csrc/pn_dtmf_clamp_rules.h"
#include <stdio.h>
#include <deque>
#include <string>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "dtmf_clamp_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

typedef std::vector<float> F;
typedef std::vector<uint32_t> U;
typedef std::vector<int32_t> I;

static const char kDigits[] = "123A456B789C*0#D";
static F tone(char digit, float amp, int frame) {
  const int i = (int)(strchr(kDigits, digit) - kDigits);
  F x(PN_FRAME);
  for (int j = 0; j < PN_FRAME; j++) {
    const double t = (frame * PN_FRAME + j) / 48000.0;
    x[j] = (float)(amp * (sin(6.283185307179586 * pn_dtmf_freq(i / 4) * t) + sin(6.283185307179586 * pn_dtmf_freq(4 + i % 4) * t)));
  }
  return x;
}
static bool all_zero(const F &x) { for (float v : x) if (v != 0.0f || signbit(v)) return false; return true; }

int main() {
  static_assert(PN_DTMF_CLAMP_N_PARAMS == 4 && PN_DTMF_CLAMP_REPORT_WORDS == 4 && PN_DTMF_CLAMP_STATE_BYTES == 16 && PN_DTMF_CLAMP_ON == 1 && PN_DTMF_CLAMP_MUTED == 2 &&
                PN_DTMF_CLAMP_FADE_OUT == 4 && PN_DTMF_CLAMP_FADE_IN == 8 && PN_DTMF_CLAMP_LATE == 16 && PN_DTMF_CLAMP_EVENT == 32 && PN_DTMF_CLAMP_EVENT_END == 64 &&
                PN_DTMF_CLAMP_DELAY == 6, "the header's constants");
  I P(PN_DTMF_CLAMP_N_PARAMS);
  pn_dtmf_clamp_default_params_host(P.data());
  CHECK(P[0] == 1 && P[1] == 0 && P[2] == 10 && P[3] == 80);
  CHECK(pn_dtmf_clamp_params_check_host(P.data()) == 0 && pn_dtmf_clamp_params_check_host(NULL) == -1);
  // ---- every parameter at both edges and one step outside; the in-time condition
  { const int32_t lo[4] = {0, 0, 0, 1}, hi[4] = {4, 8, 63, 65535};
    for (int i = 0; i < PN_DTMF_CLAMP_N_PARAMS; i++) {
      I q = P;
      char want[32];
      snprintf(want, sizeof(want), "index %d ", i);
      q[i] = hi[i]; CHECK(pn_dtmf_clamp_params_check_host(q.data()) == 0);
      q[i] = hi[i] + 1; CHECK(pn_dtmf_clamp_params_check_host(q.data()) == -1 && strstr(pn_last_error(), want));
      q[i] = lo[i]; CHECK(pn_dtmf_clamp_params_check_host(q.data()) == 0);
      q[i] = lo[i] - 1; CHECK(pn_dtmf_clamp_params_check_host(q.data()) == -1 && strstr(pn_last_error(), want));
      q[i] = INT32_MIN; CHECK(pn_dtmf_clamp_params_check_host(q.data()) == -1);
      q[i] = INT32_MAX; CHECK(pn_dtmf_clamp_params_check_host(q.data()) == -1);
    }
    for (int on = 1; on <= 7; on++)
      for (int pre = 0; pre <= 4; pre++) {
        I q = P;
        q[PN_DTMF_CLAMP_PRE] = pre;
        CHECK((pn_dtmf_clamp_params_check_host(q.data(), on) == 0) == (on + pre <= 5) && pn_dtmf_clamp_in_time(on, pre) == (on + pre <= 5));
      }
    I q = P;
    q[PN_DTMF_CLAMP_PRE] = 1;
    CHECK(pn_dtmf_clamp_params_check_host(q.data(), 5) == -1 && strstr(pn_last_error(), "on_frames 5") && strstr(pn_last_error(), "pre 1")); }
  // ---- the switch list
  { std::vector<int32_t> ids = {2, 0, 1}, dup = {2, 0, 2};
    std::vector<uint8_t> on = {1, 0, 7};
    CHECK(pn_dtmf_clamp_on_set_check(3, ids.data(), 3, on.data()) == 0 && pn_dtmf_clamp_on_set_check(3, dup.data(), 3, on.data()) == -1 &&
          pn_dtmf_clamp_on_set_check(2, ids.data(), 3, on.data()) == -1 && pn_dtmf_clamp_on_set_check(3, ids.data(), 3, NULL) == -1 && pn_dtmf_clamp_on_set_check(3, NULL, 0, NULL) == 0); }
  // ---- payloads
  { const char ev[] = "0123456789*#ABCD";
    for (int i = 0; i < 16; i++) {
      CHECK(pn_dtmf_event_code((uint32_t)ev[i]) == i);
      CHECK(pn_dtmf_event_payload_hd((uint32_t)ev[i], false, 10u, 3u, 80u) == ((uint32_t)i << 24 | 10u << 16 | 240u));
      CHECK(pn_dtmf_event_payload_hd((uint32_t)ev[i], true, 63u, 0xffffffffu, 65535u) == ((uint32_t)i << 24 | 1u << 23 | 63u << 16 | 65535u));
    }
    CHECK(pn_dtmf_event_code(0u) == -1 && pn_dtmf_event_code('E') == -1 && pn_dtmf_event_code('a') == -1 && pn_dtmf_event_payload_hd(0u, false, 10u, 3u, 80u) == 0u);
    CHECK(pn_dtmf_event_payload_hd('0', false, 0u, 819u, 80u) == 65520u && pn_dtmf_event_payload_hd('0', false, 0u, 820u, 80u) == 65535u &&
          pn_dtmf_event_payload_hd('0', false, 0u, 65535u, 1u) == 65535u && pn_dtmf_event_payload_hd('0', false, 0u, 65536u, 1u) == 65535u); }
  // ---- the detector drives it: 60 ms on, 60 ms off for every digit, the audio through a delay line of six rows, everything exactly sized
  { F DP(PN_DTMF_N_PARAMS);
    pn_dtmf_default_params_host(DP.data());
    U dst(PN_DTMF_STATE_WORDS, 0u), drep(PN_DTMF_REPORT_WORDS, 0u), st(PN_DTMF_CLAMP_STATE_WORDS, 0u), rep(PN_DTMF_CLAMP_REPORT_WORDS, 0xdeadbeefu);
    std::deque<F> line(PN_DTMF_CLAMP_DELAY, F(PN_FRAME, 0.0f));
    std::deque<bool> line_tone(PN_DTMF_CLAMP_DELAY, false);
    F zero(PN_FRAME, 0.0f);
    std::string begun, ended;
    uint32_t muted = 0u;
    int kinds = 0;
    for (int n = 0; n < 16; n++)
      for (int t = 0; t < 12; t++) {
        F x = t < 6 ? tone(kDigits[n], 0.1f, t) : zero;
        CHECK(pn_dtmf_frame_host(DP.data(), dst.data(), x.data(), 0, drep.data()) > 0);
        line.push_back(x); line_tone.push_back(t < 6);
        F y = line.front();
        const bool was_tone = line_tone.front();
        line.pop_front(); line_tone.pop_front();
        const F before = y;
        const int fl = pn_dtmf_clamp_frame_host(P.data(), st.data(), drep.data(), y.data(), rep.data());
        CHECK(fl > 0 && (fl & PN_DTMF_CLAMP_ON) && (uint32_t)fl == rep[0] && rep[3] == st[2] && !(fl & PN_DTMF_CLAMP_LATE));
        if (was_tone) CHECK((fl & PN_DTMF_CLAMP_MUTED) && all_zero(y));               // no tone sample leaves
        if (!(fl & (PN_DTMF_CLAMP_MUTED | PN_DTMF_CLAMP_FADE_OUT | PN_DTMF_CLAMP_FADE_IN))) CHECK(y == before);
        if (fl & PN_DTMF_CLAMP_MUTED) muted++;
        kinds |= fl;
        if (drep[0] & PN_DTMF_BEGIN) { CHECK((fl & PN_DTMF_CLAMP_EVENT) && (rep[1] >> 24) == (uint32_t)pn_dtmf_event_code((uint32_t)kDigits[n]) && !(rep[1] & (1u << 23))); begun += kDigits[n]; }
        if (drep[0] & PN_DTMF_END) { CHECK((fl & PN_DTMF_CLAMP_EVENT_END) && (rep[2] >> 24) == (uint32_t)pn_dtmf_event_code((uint32_t)kDigits[n]) && (rep[2] & (1u << 23)) && (rep[2] & 0xffffu) == drep[1] * 80u);
                                     ended += kDigits[n]; }
        if (!(drep[0] & PN_DTMF_END)) CHECK(rep[2] == 0u);
        if (((drep[0] >> 8) & 0xffu) == 0u) CHECK(rep[1] == 0u);
      }
    CHECK(begun == kDigits && ended == kDigits && st[2] == muted && muted >= 16u * 6u && muted <= 16u * 10u);
    CHECK((kinds & (PN_DTMF_CLAMP_FADE_OUT | PN_DTMF_CLAMP_FADE_IN | PN_DTMF_CLAMP_MUTED | PN_DTMF_CLAMP_EVENT | PN_DTMF_CLAMP_EVENT_END)) ==
          (PN_DTMF_CLAMP_FADE_OUT | PN_DTMF_CLAMP_FADE_IN | PN_DTMF_CLAMP_MUTED | PN_DTMF_CLAMP_EVENT | PN_DTMF_CLAMP_EVENT_END));
    // bad arguments change nothing; the detector's row and the report are optional
    const U keep = st;
    F y(PN_FRAME, 0.5f);
    CHECK(pn_dtmf_clamp_frame_host(NULL, st.data(), drep.data(), y.data()) == -1 && pn_dtmf_clamp_frame_host(P.data(), NULL, drep.data(), y.data()) == -1 &&
          pn_dtmf_clamp_frame_host(P.data(), st.data(), drep.data(), NULL) == -1);
    I bad = P;
    bad[PN_DTMF_CLAMP_PRE] = 5;
    CHECK(pn_dtmf_clamp_frame_host(bad.data(), st.data(), drep.data(), y.data()) == -1 && st == keep && y == F(PN_FRAME, 0.5f));
    U st0(PN_DTMF_CLAMP_STATE_WORDS, 0u);
    CHECK(pn_dtmf_clamp_frame_host(P.data(), st0.data(), NULL, y.data()) == PN_DTMF_CLAMP_ON && y == F(PN_FRAME, 0.5f) && st0 == U(PN_DTMF_CLAMP_STATE_WORDS, 0u)); }
  // ---- every row kind by hand, hostile rows: a BEGIN of dur 3 on a fresh state with pre = 4 is LATE at once; NaN rows vanish when muted
  { I q = P;
    q[PN_DTMF_CLAMP_PRE] = 4;
    U st(PN_DTMF_CLAMP_STATE_WORDS, 0u), rep(PN_DTMF_CLAMP_REPORT_WORDS), det = {PN_DTMF_ON | PN_DTMF_HIT | PN_DTMF_BEGIN | (uint32_t)'5' << 8, 3u, 1u, (uint32_t)'5'};
    F y(PN_FRAME, NAN);
    int fl = pn_dtmf_clamp_frame_host(q.data(), st.data(), det.data(), y.data(), rep.data());      // marks 0..3, M(6) = bits 2..6
    CHECK(fl == (PN_DTMF_CLAMP_ON | PN_DTMF_CLAMP_MUTED | PN_DTMF_CLAMP_LATE | PN_DTMF_CLAMP_EVENT) && all_zero(y) && st[0] == 0xfu && st[1] == 1u && st[2] == 1u && st[3] == 3u);
    CHECK(rep[1] == (5u << 24 | 10u << 16 | 240u) && rep[2] == 0u);
    U none = {PN_DTMF_ON, 0u, 1u, (uint32_t)'5'}, end = {PN_DTMF_ON | PN_DTMF_END | (uint32_t)'5' << 16, 3u, 1u, (uint32_t)'5'};
    y.assign(PN_FRAME, INFINITY);
    fl = pn_dtmf_clamp_frame_host(q.data(), st.data(), end.data(), y.data(), rep.data());
    CHECK(fl == (PN_DTMF_CLAMP_ON | PN_DTMF_CLAMP_MUTED | PN_DTMF_CLAMP_EVENT_END) && all_zero(y) && rep[2] == (5u << 24 | 1u << 23 | 10u << 16 | 240u) && st[3] == 0u);
    int fades = 0;
    for (int t = 0; t < 12; t++) {
      y.assign(PN_FRAME, 1.0f);
      fl = pn_dtmf_clamp_frame_host(q.data(), st.data(), none.data(), y.data(), rep.data());
      if (fl & PN_DTMF_CLAMP_FADE_IN) { fades++; CHECK(y[0] == 1.0f / 480.0f && y[479] == 1.0f && y[239] == 0.5f && st[1] == 0u); }
      else if (!(fl & PN_DTMF_CLAMP_MUTED)) CHECK(y == F(PN_FRAME, 1.0f));
    }
    CHECK(fades == 1 && st[2] == 7u);                                                   // the four marks pass through bits 2..6 in seven frames, then the fade in
    // a fade out in front of a digit that is in time: pre = 1, marks of dur 3
    U st2(PN_DTMF_CLAMP_STATE_WORDS, 0u);
    int seen = 0;
    for (int t = 0; t < 10; t++) {
      y.assign(PN_FRAME, -2.0f);
      fl = pn_dtmf_clamp_frame_host(P.data(), st2.data(), t == 0 ? det.data() : none.data(), y.data(), rep.data());
      CHECK(!(fl & PN_DTMF_CLAMP_LATE));
      if (fl & PN_DTMF_CLAMP_FADE_OUT) { CHECK(t == 1 && y[0] == -2.0f * (479.0f / 480.0f) && y[479] == 0.0f && signbit(y[479]) && st2[1] == 1u); seen |= 1; }
      if (fl & PN_DTMF_CLAMP_MUTED) { CHECK(t >= 2 && t <= 6 && all_zero(y)); seen |= 2; }
      if (fl & PN_DTMF_CLAMP_FADE_IN) { CHECK(t == 7); seen |= 4; }
    }
    CHECK(seen == 7 && st2[2] == 5u);
    // one row between two removed stretches: zeros, both fades flagged.  marks 1 at bit 6 and bit 4 with pre = post = 0
    I z = P;
    z[PN_DTMF_CLAMP_PRE] = 0;
    U st3 = {0x28u >> 1, 1u, 0u, 0u};                                                     // after the shift: bits 5 and 3 -> m = 0, m_next = 1, cut = 1
    y.assign(PN_FRAME, NAN);
    fl = pn_dtmf_clamp_frame_host(z.data(), st3.data(), NULL, y.data(), rep.data());
    CHECK(fl == (PN_DTMF_CLAMP_ON | PN_DTMF_CLAMP_FADE_OUT | PN_DTMF_CLAMP_FADE_IN) && all_zero(y) && st3[2] == 0u && st3[1] == 1u); }
  { // the shifts at their ends: dur >= 31 sets every bit; post = 8 reads up to bit 14; the counter saturates
    I q = P;
    q[PN_DTMF_CLAMP_POST] = 8; q[PN_DTMF_CLAMP_PRE] = 4;
    for (uint32_t dur : {30u, 31u, 32u, 0xffffffffu}) {
      U st = {0x80000000u, 0u, PN_DTMF_CLAMP_SAT - 1u, 0u}, rep(PN_DTMF_CLAMP_REPORT_WORDS), det = {PN_DTMF_ON | PN_DTMF_BEGIN | (uint32_t)'#' << 8, dur, 1u, (uint32_t)'#'};
      F y(PN_FRAME, 1.0f);
      CHECK(pn_dtmf_clamp_frame_host(q.data(), st.data(), det.data(), y.data(), rep.data()) > 0 && st[0] == (dur >= 31u ? 0xffffffffu : 0x7fffffffu) && st[2] == PN_DTMF_CLAMP_SAT);
      CHECK((rep[1] & 0xffffu) == (dur > 819u ? 65535u : dur * 80u) && st[3] == dur);
      CHECK(pn_dtmf_clamp_frame_host(q.data(), st.data(), det.data(), y.data(), rep.data()) > 0 && st[2] == PN_DTMF_CLAMP_SAT && rep[3] == PN_DTMF_CLAMP_SAT);
    }
    for (int k = 0; k < 32; k++) CHECK(pn_dtmf_clamp_any(1u << k, 6, 4, 8) == (k >= 2 && k <= 14) && pn_dtmf_clamp_any(1u << k, 31, 4, 8) == (k >= 27) && pn_dtmf_clamp_any(1u << k, 0, 4, 0) == (k == 0)); }
  puts("ok");
  return 0;
}
