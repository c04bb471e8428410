// The per-stream state of a rate converter, described once — HIP-free (builds with -DPN_NO_HIP), so that the table is checked without
// a GPU (tests/c/rate_layout_sanitize.cpp) and pinned on the device cell by cell (tests/test_gpu_rate_state_events.py).  Every
// per-stream STATE buffer of pn_rate (pn_rate.cpp) is one entry of pn_kRateState, held as pn_rate::st[entry]; the whole reset, the
// per-stream reset, a rate change, a conference change, a hold change, the tails-record import, a stage coming on again and a
// stream being switched on all clear what this table says, by two walks (pn_rate.cpp state_clear_all: a memset of every row;
// state_clear_rows: pn_launch_zero_rows over a staged list).  The call-state record (pn_call_rules.h) takes its sections from here
// too.  A new stage's state is one new entry.  Settings (laws, conferences, gains, targets, ceilings, switches) are not state: no
// event here touches them.
//
// An entry: the words of a row (PN_RS_TD: the converter's own down tail, 2 T L / M of its rate, or of 8000 Hz on a mixed one), the
// stage that owns the buffer — it exists from that stage's first use on, and a clear of a buffer that does not exist is nothing —
// the events that clear it, and the section of the call-state record it travels in: the bit, the body offset and the words there.
// PN_RE_AGAIN and PN_RE_SWITCH_ON are events OF A STAGE: they clear the entries of that stage alone.
//
// The matrix has asymmetries, and they are the behaviour: the tails-record import leaves the tails (the record writes them) and the
// level; the limiter has no "on again" (it has no switch of its own); the level is the only state a conference or hold change clears.
#pragma once
#include "pn_rate_design.h"        // the tails
#include "pn_call_rules.h"         // the call-state record, and through it the PLC, AGC, limiter and mix rules
#include "pn_dtmf_clamp_rules.h"   // DTMF removal
#include "pn_dtmf_rules.h"         // DTMF detection
#include "pn_cng_rules.h"          // comfort noise
#include "pn_dtx_rules.h"          // the DTX send side

enum { PN_RS_TAIL_UP, PN_RS_TAIL_DOWN, PN_RS_LEVEL, PN_RS_PLC_HIST, PN_RS_PLC_Q, PN_RS_PLC_META, PN_RS_AGC, PN_RS_LIM, PN_RS_DTMF, PN_RS_CLAMP, PN_RS_COUNT };
enum { PN_RST_CORE, PN_RST_MIX, PN_RST_PLC, PN_RST_AGC, PN_RST_LIM, PN_RST_DTMF, PN_RST_CLAMP, PN_RST_COUNT };      // the owning stage
enum { PN_RE_RESET = 1,            // pn_rate_reset: every stream
       PN_RE_RESET_STREAMS = 2,    // pn_rate_reset_streams: the listed streams
       PN_RE_RATE = 4,             // pn_rate_set_stream_rates: the listed streams
       PN_RE_CONF = 8,             // pn_rate_set_stream_confs: the listed streams
       PN_RE_HOLD = 16,            // pn_rate_set_mix_hold: every stream
       PN_RE_IMPORT = 32,          // pn_rate_import_streams[_host]: the listed streams
       PN_RE_AGAIN = 64,           // the owning stage on again after a pause (pn_rate_set_plc, pn_rate_set_agc): every stream
       PN_RE_SWITCH_ON = 128,      // the owning stage switched on for streams that were off (pn_rate_set_stream_dtmf[_clamp]): those streams
       PN_RE_ANY_RESET = PN_RE_RESET | PN_RE_RESET_STREAMS | PN_RE_RATE };
enum { PN_RS_TD = -1 };

struct PnRateStateEntry {
  int words;                       // per row, or PN_RS_TD
  int stage;                       // PN_RST_*
  unsigned clears;                 // PN_RE_* bits
  unsigned call_bit;               // PN_CALL_*, 0: not in the call-state record
  int call_off, call_words;        // the section's body word offset and its words in the record (the level travels in a 16-byte group)
};
static constexpr PnRateStateEntry pn_kRateState[PN_RS_COUNT] = {
    // words per row            stage         cleared by                                          call-state section
    {PN_RATE_UP_TAIL,           PN_RST_CORE,  PN_RE_ANY_RESET,                                    0,           -1,              0},                        // tail_up
    {PN_RS_TD,                  PN_RST_CORE,  PN_RE_ANY_RESET,                                    0,           -1,              0},                        // tail_down
    {1,                         PN_RST_MIX,   PN_RE_ANY_RESET | PN_RE_CONF | PN_RE_HOLD,          PN_CALL_MIX, PN_CALL_W_MIX,   4},                        // level
    {PN_PLC_HIST,               PN_RST_PLC,   PN_RE_ANY_RESET | PN_RE_IMPORT | PN_RE_AGAIN,       PN_CALL_PLC, PN_CALL_W_HIST,  PN_PLC_HIST},              // plc_hist
    {PN_PLC_P_MAX,              PN_RST_PLC,   PN_RE_ANY_RESET | PN_RE_IMPORT | PN_RE_AGAIN,       PN_CALL_PLC, PN_CALL_W_Q,     PN_PLC_P_MAX},             // plc_q
    {4,                         PN_RST_PLC,   PN_RE_ANY_RESET | PN_RE_IMPORT | PN_RE_AGAIN,       PN_CALL_PLC, PN_CALL_W_META,  4},                        // plc_meta
    {PN_AGC_STATE_BYTES / 4,    PN_RST_AGC,   PN_RE_ANY_RESET | PN_RE_IMPORT | PN_RE_AGAIN,       PN_CALL_AGC, PN_CALL_W_AGC,   PN_AGC_STATE_BYTES / 4},   // agc
    {PN_LIM_STATE_BYTES / 4,    PN_RST_LIM,   PN_RE_ANY_RESET | PN_RE_IMPORT,                     PN_CALL_LIM, PN_CALL_W_LIM,   PN_LIM_STATE_BYTES / 4},   // lim
    {PN_DTMF_STATE_WORDS,       PN_RST_DTMF,  PN_RE_ANY_RESET | PN_RE_IMPORT | PN_RE_SWITCH_ON,   0,           -1,              0},                        // dtmf
    {PN_DTMF_CLAMP_STATE_WORDS, PN_RST_CLAMP, PN_RE_ANY_RESET | PN_RE_IMPORT | PN_RE_SWITCH_ON,   0,           -1,              0},                        // clamp
};

// The SECOND table: state of the stages at the converter's EDGES, at the streams' own rates — in front of the up-conversion and behind
// the down-conversion —, entries of the same type, held as pn_rate::st2[entry] and walked by the same two walks behind the first.  It
// stands apart because the first is pinned at its ten entries and seven stages (tests/c/rate_layout_sanitize.cpp), so its stages count
// on from PN_RST_COUNT.  Comfort noise (pn_cng_rules.h): cleared by the whole reset, the per-stream reset, a rate change (the lattice
// ran at the old rate), the tails-record import (the slot is another stream's) and "on again"; a conference, hold or switch change
// leaves it.  The DTX send side (pn_dtx_rules.h): cleared by the same resets, the rate change (the statistics are of the old rate's
// rows), the import, and for a stream that is switched on from off; a conference or hold change leaves it.  Neither travels in a record.
enum { PN_RS2_CNG, PN_RS2_DTX, PN_RS2_COUNT };
enum { PN_RST_CNG = PN_RST_COUNT, PN_RST_DTX };
static constexpr PnRateStateEntry pn_kRateState2[PN_RS2_COUNT] = {
    {PN_CNG_STATE_WORDS,        PN_RST_CNG,   PN_RE_ANY_RESET | PN_RE_IMPORT | PN_RE_AGAIN,       0,           -1,              0},                        // cng
    {PN_DTX_STATE_WORDS,        PN_RST_DTX,   PN_RE_ANY_RESET | PN_RE_IMPORT | PN_RE_SWITCH_ON,   0,           -1,              0},                        // dtx
};
constexpr bool pn_rate_state2_cleared(int e, unsigned event, int stage = -1) {
  return (pn_kRateState2[e].clears & event) != 0 && (stage < 0 || pn_kRateState2[e].stage == stage);
}

// the words of a row of entry e on a converter whose down tail has td words
constexpr int pn_rate_state_words(int e, int td) { return pn_kRateState[e].words == PN_RS_TD ? td : pn_kRateState[e].words; }
// does `event` (one PN_RE_* bit) clear entry e?  stage: the stage the event is of (PN_RE_AGAIN, PN_RE_SWITCH_ON), -1 for the others
constexpr bool pn_rate_state_cleared(int e, unsigned event, int stage = -1) {
  return (pn_kRateState[e].clears & event) != 0 && (stage < 0 || pn_kRateState[e].stage == stage);
}
// the words the entries with call-state bit `bit` take in the record (bit 0: those of every section)
constexpr int pn_rate_call_words(unsigned bit) {
  int w = 0;
  for (const PnRateStateEntry &e : pn_kRateState) if (e.call_bit && (!bit || e.call_bit == bit)) w += e.call_words;
  return w;
}
// the table and the record layout of pn_call_rules.h agree: a section starts where the sections before it end, the state of a
// stage is as wide as its rules say, and only the level is padded (to the 16-byte group the record gives it)
constexpr bool pn_rate_layout_ok() {
  int at = 0;
  unsigned bits = 0;
  for (const PnRateStateEntry &e : pn_kRateState) {
    if (!e.call_bit) { if (e.call_off != -1 || e.call_words) return false; continue; }
    int before = 0;
    for (const PnRateStateEntry &f : pn_kRateState) if (f.call_bit && f.call_off < e.call_off) before += f.call_words;
    if (before != e.call_off || e.call_off % 4 || e.words == PN_RS_TD || (e.call_words != e.words && e.call_bit != PN_CALL_MIX)) return false;
    at += e.call_words; bits |= e.call_bit;
  }
  return at == PN_CALL_BODY_WORDS && bits == PN_CALL_ALL;
}
static_assert(pn_rate_layout_ok(), "the sections of the call-state record, one behind the other, make its body");
static_assert(pn_kRateState[PN_RS_PLC_HIST].call_off == PN_CALL_W_HIST && pn_kRateState[PN_RS_PLC_Q].call_off == PN_CALL_W_Q &&
              pn_kRateState[PN_RS_PLC_META].call_off == PN_CALL_W_META && pn_kRateState[PN_RS_AGC].call_off == PN_CALL_W_AGC &&
              pn_kRateState[PN_RS_LIM].call_off == PN_CALL_W_LIM && pn_kRateState[PN_RS_LEVEL].call_off == PN_CALL_W_MIX, "every section at its PN_CALL_W_*");
static_assert(pn_rate_call_words(PN_CALL_PLC) == PN_PLC_STATE_BYTES / 4 && pn_rate_call_words(PN_CALL_AGC) == PN_AGC_STATE_BYTES / 4 &&
              pn_rate_call_words(PN_CALL_LIM) == PN_LIM_STATE_BYTES / 4 && pn_rate_call_words(PN_CALL_MIX) == 4 && pn_rate_call_words(0) == PN_CALL_BODY_WORDS,
              "every section as wide as its state");
static_assert(pn_kRateState[PN_RS_DTMF].words * 4 == PN_DTMF_STATE_BYTES && pn_kRateState[PN_RS_CLAMP].words * 4 == PN_DTMF_CLAMP_STATE_BYTES &&
              pn_kRateState[PN_RS_TAIL_UP].words == 2 * PN_RATE_TAPS, "the states outside the record at their rules' sizes");
