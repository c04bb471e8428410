// CPU-only check of the rate converter's state table (tests/test_rate_host.py builds it with g++ -DPN_NO_HIP
// -fsanitize=address,undefined, like rate_sanitize.cpp): pn_rate_layout.h walked entry by entry.  Which event clears which buffer is
// compared with the matrix WRITTEN OUT below, ten buffers by eight events — the behaviour the converter had before the table
// existed, asymmetries included; the call-state sections with the constants of pn_call_rules.h; every width with its stage's PN_*
// constant.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_rate_layout.h"
#include <stdio.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "rate_layout_sanitize: CHECK failed at line %d: %s\n", __LINE__, #c); return 1; } } while (0)

enum { N_EVENTS = 8 };
static const unsigned kEvent[N_EVENTS] = {PN_RE_RESET, PN_RE_RESET_STREAMS, PN_RE_RATE, PN_RE_CONF, PN_RE_HOLD, PN_RE_IMPORT, PN_RE_AGAIN, PN_RE_SWITCH_ON};
// rows: tail_up, tail_down, level, plc_hist, plc_q, plc_meta, agc, lim, dtmf, clamp
// columns: whole reset, per-stream reset, rate change, conference change, hold change, tails-record import, its stage on again, its stage switched on for a stream
static const int kMatrix[PN_RS_COUNT][N_EVENTS] = {
    {1, 1, 1, 0, 0, 0, 0, 0},   // tail_up
    {1, 1, 1, 0, 0, 0, 0, 0},   // tail_down
    {1, 1, 1, 1, 1, 0, 0, 0},   // level
    {1, 1, 1, 0, 0, 1, 1, 0},   // plc_hist
    {1, 1, 1, 0, 0, 1, 1, 0},   // plc_q
    {1, 1, 1, 0, 0, 1, 1, 0},   // plc_meta
    {1, 1, 1, 0, 0, 1, 1, 0},   // agc
    {1, 1, 1, 0, 0, 1, 0, 0},   // lim
    {1, 1, 1, 0, 0, 1, 0, 1},   // dtmf
    {1, 1, 1, 0, 0, 1, 0, 1},   // clamp
};
static const int kStage[PN_RS_COUNT] = {PN_RST_CORE, PN_RST_CORE, PN_RST_MIX, PN_RST_PLC, PN_RST_PLC, PN_RST_PLC, PN_RST_AGC, PN_RST_LIM, PN_RST_DTMF, PN_RST_CLAMP};
// words per row (-1: the converter's down tail), the call-state bit, the section's offset and words in the record
static const int kWords[PN_RS_COUNT] = {2 * PN_RATE_TAPS, -1, 1, PN_PLC_HIST, PN_PLC_P_MAX, 4, PN_AGC_STATE_BYTES / 4, PN_LIM_STATE_BYTES / 4, PN_DTMF_STATE_BYTES / 4,
                                        PN_DTMF_CLAMP_STATE_BYTES / 4};
static const unsigned kBit[PN_RS_COUNT] = {0, 0, PN_CALL_MIX, PN_CALL_PLC, PN_CALL_PLC, PN_CALL_PLC, PN_CALL_AGC, PN_CALL_LIM, 0, 0};
static const int kOff[PN_RS_COUNT] = {-1, -1, PN_CALL_W_MIX, PN_CALL_W_HIST, PN_CALL_W_Q, PN_CALL_W_META, PN_CALL_W_AGC, PN_CALL_W_LIM, -1, -1};
static const int kCallWords[PN_RS_COUNT] = {0, 0, 4, PN_PLC_HIST, PN_PLC_P_MAX, 4, PN_AGC_STATE_BYTES / 4, PN_LIM_STATE_BYTES / 4, 0, 0};

int main() {
  static_assert(PN_RS_COUNT == 10 && PN_RS_TAIL_UP == 0 && PN_RS_TAIL_DOWN == 1 && PN_RS_LEVEL == 2 && PN_RS_PLC_HIST == 3 && PN_RS_PLC_Q == 4 && PN_RS_PLC_META == 5 &&
                PN_RS_AGC == 6 && PN_RS_LIM == 7 && PN_RS_DTMF == 8 && PN_RS_CLAMP == 9, "the ten buffers, in the order of the rows above");
  // the table lives on the heap for the walk, exactly sized: an index past an end is the sanitizer's
  PnRateStateEntry *t = new PnRateStateEntry[PN_RS_COUNT];
  for (int e = 0; e < PN_RS_COUNT; e++) t[e] = pn_kRateState[e];
  unsigned seen = 0;
  int body = 0;
  for (int e = 0; e < PN_RS_COUNT; e++) {
    // the events: the entry's bits are the matrix's row, and nothing beside the eight events
    unsigned want = 0;
    for (int k = 0; k < N_EVENTS; k++) {
      if (kMatrix[e][k]) want |= kEvent[k];
      CHECK(pn_rate_state_cleared(e, kEvent[k]) == (kMatrix[e][k] != 0));
      // an event of a stage clears the entries of that stage alone
      for (int s = 0; s < PN_RST_COUNT; s++) CHECK(pn_rate_state_cleared(e, kEvent[k], s) == (kMatrix[e][k] != 0 && s == kStage[e]));
    }
    CHECK(t[e].clears == want);
    CHECK(t[e].stage == kStage[e]);
    // the widths
    CHECK(t[e].words == kWords[e] && (t[e].words == PN_RS_TD) == (e == PN_RS_TAIL_DOWN));
    for (int f : {6, 3, 2, PN_RATE_F_3_2})
      CHECK(pn_rate_state_words(e, pn_rate_down_tail(f)) == (e == PN_RS_TAIL_DOWN ? pn_rate_down_tail(f) : kWords[e]));
    // the call-state section
    CHECK(t[e].call_bit == kBit[e] && t[e].call_off == kOff[e] && t[e].call_words == kCallWords[e]);
    if (t[e].call_bit) { CHECK(t[e].call_off >= 0 && t[e].call_off + t[e].call_words <= PN_CALL_BODY_WORDS); body += t[e].call_words; seen |= t[e].call_bit; }
  }
  delete[] t;
  CHECK(body == PN_CALL_BODY_WORDS && seen == PN_CALL_ALL);
  CHECK(pn_rate_call_words(PN_CALL_PLC) * 4 == PN_PLC_STATE_BYTES && pn_rate_call_words(PN_CALL_AGC) * 4 == PN_AGC_STATE_BYTES &&
        pn_rate_call_words(PN_CALL_LIM) * 4 == PN_LIM_STATE_BYTES && pn_rate_call_words(PN_CALL_MIX) == 4 && pn_rate_call_words(0) == PN_CALL_BODY_WORDS);
  // the stage events by their stage: the concealer on again clears its three buffers, the level control its one; a switch-on the detector's or the removal's
  for (int e = 0; e < PN_RS_COUNT; e++) {
    CHECK(pn_rate_state_cleared(e, PN_RE_AGAIN, PN_RST_PLC) == (e == PN_RS_PLC_HIST || e == PN_RS_PLC_Q || e == PN_RS_PLC_META));
    CHECK(pn_rate_state_cleared(e, PN_RE_AGAIN, PN_RST_AGC) == (e == PN_RS_AGC));
    CHECK(!pn_rate_state_cleared(e, PN_RE_AGAIN, PN_RST_LIM) && !pn_rate_state_cleared(e, PN_RE_AGAIN, PN_RST_MIX));
    CHECK(pn_rate_state_cleared(e, PN_RE_SWITCH_ON, PN_RST_DTMF) == (e == PN_RS_DTMF));
    CHECK(pn_rate_state_cleared(e, PN_RE_SWITCH_ON, PN_RST_CLAMP) == (e == PN_RS_CLAMP));
  }
  printf("ok\n");
  return 0;
}
