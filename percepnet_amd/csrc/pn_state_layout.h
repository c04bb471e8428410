// The per-stream state of a batched context, described once — HIP-free (builds with -DPN_NO_HIP), so that the layout and the
// ring phases are checked without a GPU (tests/c/host_sanitize.cpp).  Every per-stream device buffer of pn_ctx is one entry of
// pn_kState; allocation, zeroing, per-stream reset, the active-set fix-up, the stream-state records, the host state copies and
// the debug taps all walk this table (pn_context.cpp resolves it once per context).  A new state buffer is one new entry.
// The DSP entries are also the buffers of a front-end side (pn_dsp_layout.h), which the training-feature generator
// (pn_featgen.cpp) allocates, zeroes and resets by the same walk with pn_state_size.
//
// All buffers are 4-byte words (float2 / int buffers are described in words).  An entry is `slots` slots of `cols` words per
// row, `live` of which hold state between two frames; the slots lie one batch apart ([slots][rows][row_words]) or, for the
// history, back to back inside the row.  Classes, in the sense of the active set (pn_active.hip): a frame writes
//   RING     the one dead slot of a ring indexed by the frames done (t) or the network steps done (tn),
//   INPLACE  the state itself (saved and restored around a skipped tick),
//   SCRATCH  what the next frame recomputes before it reads it.
#pragma once
#include "pn_common.h"
#include "../../include/percepnet_hip.h"

enum { PN_ST_HIST, PN_ST_SYNTH, PN_ST_LAST_GAIN, PN_ST_LAST_PERIOD, PN_ST_SILENCE, PN_ST_YRING, PN_ST_EYRING, PN_ST_PS, PN_ST_FEAT,
       PN_ST_C1RING, PN_ST_C2RING, PN_ST_C2OUT, PN_ST_GRU1, PN_ST_GRU2, PN_ST_GRU3, PN_ST_GRU_GB, PN_ST_RB, PN_ST_GR, PN_ST_COUNT };
enum { PN_SS_NSEC = 11 };      // entries with a record offset = sections of a stream-state record (ordered by that offset)
enum { PN_CLS_RING, PN_CLS_INPLACE, PN_CLS_SCRATCH };
enum { PN_CNT_NONE, PN_CNT_T, PN_CNT_TN };
// operand shadow (fragment-order twin the GEMMs read): none, in the shadow-operand modes (fp16 operands, split precision)
// only, or in those modes and in the direct-operand family of the fp32 mode
enum { PN_SH_NONE, PN_SH_MODES, PN_SH_MODES_DIRECT };

struct PnStateEntry {
  int padded;            // rows: 0 = B, 1 = Bp (every network buffer)
  int row_words;         // words per row that are allocated and zeroed (the history's includes the 8-sample mirror)
  int slots, live, cols; // ring geometry
  int in_row;            // 1: the slots lie inside the row
  int counter, cls, shadow;
  int rec_off;           // body word offset in a stream-state record (PN_SS_*), or -1
};
static constexpr PnStateEntry pn_kState[PN_ST_COUNT] = {
    // rows  row_words        slots live cols            in_row counter     class           shadow              record
    {0, PN_HIST_STRIDE,      12, 11, PN_FRAME,         1, PN_CNT_T,    PN_CLS_RING,    PN_SH_NONE,         PN_SS_HIST},    // hist
    {0, PN_FRAME,             1,  1, PN_FRAME,         0, PN_CNT_NONE, PN_CLS_INPLACE, PN_SH_NONE,         PN_SS_SYNTH},   // synth
    {0, 1,                    1,  1, 1,                0, PN_CNT_NONE, PN_CLS_INPLACE, PN_SH_NONE,         -1},            // last_gain   (a record carries both
    {0, 1,                    1,  1, 1,                0, PN_CNT_NONE, PN_CLS_INPLACE, PN_SH_NONE,         -1},            // last_period  in its tail)
    {0, 1,                    1,  1, 1,                0, PN_CNT_NONE, PN_CLS_SCRATCH, PN_SH_NONE,         -1},            // silence
    {0, 2 * PN_SPEC_BINS,     6,  5, 2 * PN_SPEC_BINS, 0, PN_CNT_T,    PN_CLS_RING,    PN_SH_NONE,         PN_SS_SPEC},    // yring (float2)
    {0, 36,                   6,  5, 36,               0, PN_CNT_T,    PN_CLS_RING,    PN_SH_NONE,         PN_SS_EY},      // eyring
    {0, 2 * PN_SPEC_BINS,     1,  1, 2 * PN_SPEC_BINS, 0, PN_CNT_NONE, PN_CLS_SCRATCH, PN_SH_NONE,         -1},            // Ps (float2)
    {1, PN_FEAT_STRIDE,       1,  1, PN_FEAT_STRIDE,   0, PN_CNT_NONE, PN_CLS_SCRATCH, PN_SH_NONE,         -1},            // feat
    {1, 128,                  5,  4, 128,              0, PN_CNT_TN,   PN_CLS_RING,    PN_SH_MODES,        PN_SS_CONV1},   // c1ring
    {1, 512,                  3,  2, 512,              0, PN_CNT_TN,   PN_CLS_RING,    PN_SH_MODES,        PN_SS_CONV2},   // c2ring
    {1, 512,                  1,  1, 512,              0, PN_CNT_NONE, PN_CLS_SCRATCH, PN_SH_MODES_DIRECT, -1},            // c2out
    {1, 512,                  2,  1, 512,              0, PN_CNT_TN,   PN_CLS_RING,    PN_SH_MODES_DIRECT, PN_SS_GRU},     // gru1
    {1, 512,                  2,  1, 512,              0, PN_CNT_TN,   PN_CLS_RING,    PN_SH_MODES_DIRECT, PN_SS_GRU + 512},   // gru2
    {1, 512,                  2,  1, 512,              0, PN_CNT_TN,   PN_CLS_RING,    PN_SH_MODES_DIRECT, PN_SS_GRU + 1024},  // gru3
    {1, 512,                  2,  1, 512,              0, PN_CNT_TN,   PN_CLS_RING,    PN_SH_MODES_DIRECT, PN_SS_GRU + 1536},  // gru_gb
    {1, 128,                  2,  1, 128,              0, PN_CNT_TN,   PN_CLS_RING,    PN_SH_MODES_DIRECT, PN_SS_GRU_RB},  // rb
    {0, 68,                   1,  1, 68,               0, PN_CNT_NONE, PN_CLS_SCRATCH, PN_SH_NONE,         -1},            // gr
};

// An entry sized for `rows` rows: its words, and the distance between two of its slots.  A context passes B or Bp as `padded`
// says; the feature generator, whose rows no GEMM reads, B for every entry.
struct PnStateSize { size_t words; long long slot_stride; };
constexpr PnStateSize pn_state_size(const PnStateEntry &e, size_t rows) {
  return PnStateSize{(e.in_row ? 1 : e.slots) * rows * e.row_words, e.in_row ? e.cols : (long long)(rows * e.row_words)};
}

// The ring phases — the only place that spells them.  Before the frame with counters (t, tn) runs, an entry's live slots are
// first, first + 1, ... first + live - 1 (mod slots), oldest first; the frame writes the one slot that is not live, which
// thereby becomes the newest live one, and `first` moves up by one.  A ring writes slot counter % slots; a two-slot ring is a
// ping-pong pair whose step reads half counter & 1 and writes the other one.
constexpr int pn_state_write(const PnStateEntry &e, int64_t t, int64_t tn) {
  const int64_t n = e.counter == PN_CNT_T ? t : tn;
  return e.slots == 1 ? 0 : (e.slots == 2 ? (int)(n & 1) ^ 1 : (int)(n % e.slots));
}
constexpr int pn_state_first(const PnStateEntry &e, int64_t t, int64_t tn) { return (pn_state_write(e, t, tn) + 1) % e.slots; }

// the k of entry e's section in a record (sections are ordered by their offset), or -1
constexpr int pn_state_section(int e) {
  int k = 0;
  for (const PnStateEntry &f : pn_kState) k += f.rec_off >= 0 && f.rec_off < pn_kState[e].rec_off;
  return pn_kState[e].rec_off < 0 ? -1 : k;
}
// the record layout of include/percepnet_hip.h and the ring geometry agree: every section starts where the sections before it
// end, the four tail words follow the last one; the kernels key the history's mirror on section 0 and the tail on the last
constexpr bool pn_state_records_ok() {
  int n = 0, words = 0;
  for (const PnStateEntry &e : pn_kState) {
    if (e.rec_off < 0) continue;
    int before = 0;
    for (const PnStateEntry &f : pn_kState) if (f.rec_off >= 0 && f.rec_off < e.rec_off) before += f.live * f.cols;
    if (before != e.rec_off || e.cols % 4) return false;
    n++; words += e.live * e.cols;
  }
  return n == PN_SS_NSEC && words == PN_SS_TAIL && PN_SS_BODY_WORDS == PN_SS_TAIL + 4 && pn_state_section(PN_ST_HIST) == 0 &&
         pn_state_section(PN_ST_SYNTH) == PN_SS_NSEC - 1;
}
static_assert(pn_state_records_ok(), "record layout (percepnet_hip.h) and ring geometry agree");
static_assert(PN_STREAM_STATE_BYTES % 16 == 0 && PN_STREAM_STATE_HEADER_BYTES % 16 == 0, "records stay float4-aligned");
