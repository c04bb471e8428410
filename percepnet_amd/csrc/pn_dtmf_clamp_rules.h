// DTMF removal on the rate converter (include/percepnet_hip.h "DTMF removal"), the rule stated once — HIP-free (builds with -DPN_NO_HIP):
// the host's pn_dtmf_clamp_frame is pn_dtmf_clamp_frame_host below, the kernel (pn_rate_dtmf_clamp.hip) runs the SAME scalar statements
// (pn_dtmf_clamp_decide, pn_dtmf_clamp_sample, compiled for both sides), tests/dtmf_clamp_model.py restates them in numpy,
// tests/c/dtmf_clamp_sanitize.cpp runs them under the sanitizers over exactly-sized buffers.
//
// Where it sits.  Output row t of the engine is input row t - 6 (PN_DTMF_CLAMP_DELAY frames).  The detector
// (pn_dtmf_rules.h) runs IN FRONT of the engine, so in frame t this stage holds the detector's verdict on input rows up to t while the
// row in its hands is input row t - 6: a digit is known before its first sample comes out.  The stage works on y48, behind the engine
// and in front of the level control, the mix, the limiter and the down-conversion.  It reads the detector's REPORT row of this frame
// and nothing else of the detector.
//
// Parameters, one set per converter (PN_DTMF_CLAMP_N_PARAMS = 4 int32):
//   0 PN_DTMF_CLAMP_PRE           rows removed in front of a marked row       [0, 4]      1
//   1 PN_DTMF_CLAMP_POST          rows removed behind a marked row            [0, 8]      0
//   2 PN_DTMF_CLAMP_VOLUME        the volume field of an event payload        [0, 63]     10
//   3 PN_DTMF_CLAMP_TS_PER_FRAME  RTP timestamp units per 10 ms frame         [1, 65535]  80 (an 8 kHz RTP clock)
// In time.  A mark of input row p is final by frame p + on_frames (the detector's PN_DTMF_ON_FRAMES), and the row `pre` in front of it
// comes out in frame p - pre + 6, whose fade belongs to the frame before: the knowledge is in time exactly when on_frames + pre <= 5
// (pn_dtmf_clamp_in_time).  The converter's setters refuse what breaks it; the host function below does not, and then reports LATE.
//
// State of one stream (PN_DTMF_CLAMP_STATE_BYTES = 16, four words; all zero is fresh):
//   w0 marks, a 32-bit shift register: bit i is the mark of input row t - i
//   w1 bit 0 cut: the previous output row ended at gain 0
//   w2 rows muted so far, saturating at 2^32 - 1
//   w3 the dur of the previous frame's ongoing event (0: none)
//
// One frame of an advancing stream with removal on; det = the detector's report row of this frame (flags | cur << 8 | ended << 16, dur,
// count, last4), x = the stream's 480-sample row of y48:
//   marks     1. marks <<= 1
//             2. det is four zero words (detection off for the stream): nothing is set
//             3. otherwise, BEGIN with duration dur (the run of hits): bits 0 .. min(dur, 31) are set — a hit window spans two rows, so
//                dur hits cover dur + 1 rows
//             4. otherwise, cur != 0: bit 0 is set — gap frames and concealed frames (HELD_LOST) of a digit included
//   decision  M(k) = any mark bit in [k - pre, k + post] clipped to 0..31; m = M(6), m_next = M(5);
//             the gain at the row's end e = (m || m_next) ? 0 : 1, at its start s = cut ? 0 : 1
//   the row   m:                 all 480 samples become +0.0f, written WITHOUT being read (a NaN in a removed row is gone); MUTED, the
//                                count of w2 moves on; with s == 1 the cut is hard: LATE
//             !m, s 1, e 0:      fade out, x[j] * wd[j], wd[j] = (float)(479 - j) / 480.0f; FADE_OUT
//             !m, s 0, e 1:      fade in,  x[j] * wu[j], wu[j] = (float)(j + 1) / 480.0f;  FADE_IN
//             !m, s 0, e 0:      zeros, written without being read; FADE_OUT | FADE_IN (one row between two removed stretches)
//             s 1, e 1:          the row is neither read nor written
//             then cut = (e == 0).  A ramp value is ONE correctly rounded fp32 quotient of two exact integers (which is also the double
//             quotient narrowed once), the product is rounded once.
//   events    RFC 4733 §2.3: payload = event << 24 | E << 23 | volume << 16 | duration, to be sent big-endian; event 0..9 for '0'..'9',
//             10 '*', 11 '#', 12..15 'A'..'D'; duration = min(dur * ts_per_frame, 65535)
//             cur != 0:  word 1 = the ongoing event, E = 0, dur of this frame (a concealed frame repeats it); EVENT
//             END:       word 2 = the ended digit, E = 1, with the dur of the PREVIOUS frame's ongoing event (w3) — the detector's
//                        ended_dur, kept here so that an END and a BEGIN in one frame still carry it; EVENT_END.  Where this state
//                        never saw the digit ongoing (w3 == 0: removal was switched on inside it) the duration is one frame's
//             then w3 = cur ? dur : 0.  0 means no event: a real payload is never 0 because its duration is at least 1
//   Events describe the INPUT: they run PN_DTMF_CLAMP_DELAY frames (60 ms) ahead of the audio they describe.
// Report (PN_DTMF_CLAMP_REPORT_WORDS = 4): word 0 flags ON | MUTED | FADE_OUT | FADE_IN | LATE | EVENT | EVENT_END; word 1 the ongoing
// payload; word 2 the ended payload; word 3 rows muted so far.  A stream that is not on: four zero words, state and row untouched.
// Known limit: concealed frames among a digit's first on_frames hits are not counted in dur, so up to that many rows of its head stay.
#pragma once
#include "pn_mix_rules.h"    // pn_ids_check, pn_set_error, the header's PN_DTMF_* and PN_DTMF_CLAMP_* constants
#include <string.h>

#define PN_DTMF_CLAMP_STATE_BYTES 16
#define PN_DTMF_CLAMP_STATE_WORDS 4
#define PN_DTMF_CLAMP_DELAY 6                          // output row t is input row t - 6
#define PN_DTMF_CLAMP_SAT 0xffffffffu
// what a row needs: nothing (unity), zeros, or one of the two ramps
#define PN_DTMF_CLAMP_KEEP 0
#define PN_DTMF_CLAMP_ZERO 1
#define PN_DTMF_CLAMP_DOWN 2
#define PN_DTMF_CLAMP_UP 3
static_assert(PN_DTMF_CLAMP_N_PARAMS == 4 && PN_DTMF_CLAMP_REPORT_WORDS == 4 && PN_DTMF_REPORT_WORDS == 4 && PN_FRAME == 480, "four parameters, four words of state, four of report");

#if defined(__HIPCC__) && !defined(PN_NO_HIP)
#define PN_DTMF_CLAMP_HD __host__ __device__ __forceinline__
#else
#define PN_DTMF_CLAMP_HD static inline
#endif
#if defined(__GNUC__) && !defined(__clang__)
#define PN_DTMF_CLAMP_STRICT __attribute__((optimize("fp-contract=off")))
#else
#define PN_DTMF_CLAMP_STRICT
#endif

struct PnDtmfClampParams { int32_t v[PN_DTMF_CLAMP_N_PARAMS]; };   // (by value into the kernel: a parameter change is ordered like a launch)

static inline void pn_dtmf_clamp_default_params_host(int32_t *p) {
  p[PN_DTMF_CLAMP_PRE] = 1; p[PN_DTMF_CLAMP_POST] = 0; p[PN_DTMF_CLAMP_VOLUME] = 10; p[PN_DTMF_CLAMP_TS_PER_FRAME] = 80;
}
static inline bool pn_dtmf_clamp_in_time(int on_frames, int pre) { return on_frames + pre <= PN_DTMF_CLAMP_DELAY - 1; }
// -1 with pn_last_error naming the FIRST bad index.  on_frames > 0: the detector's PN_DTMF_ON_FRAMES, against which the guard in front
// must be in time; refused naming both values
static inline int pn_dtmf_clamp_params_check_host(const int32_t *p, int on_frames = 0) {
  if (!p) { pn_set_error("NULL argument"); return -1; }
  static const struct { const char *name; int32_t lo, hi; } k[PN_DTMF_CLAMP_N_PARAMS] = {{"pre", 0, 4}, {"post", 0, 8}, {"volume", 0, 63}, {"ts_per_frame", 1, 65535}};
  for (int i = 0; i < PN_DTMF_CLAMP_N_PARAMS; i++)
    if (p[i] < k[i].lo || p[i] > k[i].hi) {
      pn_set_error("DTMF removal parameter %d at index %d (%s): a whole number in [%d, %d]", (int)p[i], i, k[i].name, (int)k[i].lo, (int)k[i].hi);
      return -1;
    }
  if (on_frames > 0 && !pn_dtmf_clamp_in_time(on_frames, p[PN_DTMF_CLAMP_PRE])) {
    pn_set_error("DTMF removal: on_frames %d + pre %d > %d: a digit would be known after the row in front of it has left", on_frames, (int)p[PN_DTMF_CLAMP_PRE],
                 PN_DTMF_CLAMP_DELAY - 1);
    return -1;
  }
  return 0;
}
static inline int pn_dtmf_clamp_on_set_check(int B, const int32_t *ids, int n, const uint8_t *on) {
  if (n > 0 && !on) { pn_set_error("bad argument"); return -1; }
  return pn_ids_check(B, ids, n, true);
}

// the event code of a digit's ASCII, -1 for anything else
PN_DTMF_CLAMP_HD int pn_dtmf_event_code(uint32_t digit) {
  if (digit >= '0' && digit <= '9') return (int)(digit - '0');
  if (digit == '*') return 10;
  if (digit == '#') return 11;
  if (digit >= 'A' && digit <= 'D') return (int)(digit - 'A') + 12;
  return -1;
}
// the payload of `digit` after dur frames; 0 for no digit
PN_DTMF_CLAMP_HD uint32_t pn_dtmf_event_payload_hd(uint32_t digit, bool end, uint32_t volume, uint32_t dur, uint32_t ts_per_frame) {
  const int ev = pn_dtmf_event_code(digit);
  if (ev < 0) return 0u;
  // (dur * ts without overflow: anything beyond 65535 / ts saturates)
  const uint32_t d = dur > 65535u / ts_per_frame ? 65535u : dur * ts_per_frame;
  return ((uint32_t)ev << 24) | (end ? 1u << 23 : 0u) | ((volume & 63u) << 16) | d;
}
// any mark in [k - pre, k + post], clipped to 0..31
PN_DTMF_CLAMP_HD bool pn_dtmf_clamp_any(uint32_t marks, int k, int pre, int post) {
  int lo = k - pre, hi = k + post;
  lo = lo < 0 ? 0 : lo; hi = hi > 31 ? 31 : hi;
  const uint32_t upto_hi = hi == 31 ? 0xffffffffu : (1u << (hi + 1)) - 1u, below_lo = (1u << lo) - 1u;
  return (marks & upto_hi & ~below_lo) != 0u;
}
// The scalar half of a frame: st = the four state words, read and written; det = the detector's report row (NULL: four zero words);
// rep = this stage's report row.  Returns what the row needs (PN_DTMF_CLAMP_KEEP | ZERO | DOWN | UP)
PN_DTMF_CLAMP_HD int pn_dtmf_clamp_decide(const int32_t *prm, uint32_t *st, const uint32_t *det, uint32_t *rep) {
  const uint32_t d0 = det ? det[0] : 0u, d1 = det ? det[1] : 0u, d2 = det ? det[2] : 0u, d3 = det ? det[3] : 0u;
  const bool det_on = (d0 | d1 | d2 | d3) != 0u;
  const uint32_t cur = (d0 >> 8) & 0xffu, ended = (d0 >> 16) & 0xffu, dur = d1;
  uint32_t marks = st[0] << 1;
  if (det_on) {
    if (d0 & PN_DTMF_BEGIN) marks |= dur >= 31u ? 0xffffffffu : (1u << (dur + 1u)) - 1u;
    else if (cur != 0u) marks |= 1u;
  }
  const int pre = prm[PN_DTMF_CLAMP_PRE], post = prm[PN_DTMF_CLAMP_POST];
  const bool m = pn_dtmf_clamp_any(marks, PN_DTMF_CLAMP_DELAY, pre, post), m_next = pn_dtmf_clamp_any(marks, PN_DTMF_CLAMP_DELAY - 1, pre, post);
  const bool e0 = m || m_next, s0 = (st[1] & 1u) != 0u;          // the gain is 0 at the row's end, at its start
  uint32_t flags = PN_DTMF_CLAMP_ON, muted = st[2];
  int kind;
  if (m) { kind = PN_DTMF_CLAMP_ZERO; flags |= PN_DTMF_CLAMP_MUTED | (s0 ? 0u : PN_DTMF_CLAMP_LATE); muted = muted == PN_DTMF_CLAMP_SAT ? muted : muted + 1u; }
  else if (!s0 && e0) { kind = PN_DTMF_CLAMP_DOWN; flags |= PN_DTMF_CLAMP_FADE_OUT; }
  else if (s0 && !e0) { kind = PN_DTMF_CLAMP_UP; flags |= PN_DTMF_CLAMP_FADE_IN; }
  else if (s0 && e0) { kind = PN_DTMF_CLAMP_ZERO; flags |= PN_DTMF_CLAMP_FADE_OUT | PN_DTMF_CLAMP_FADE_IN; }
  else kind = PN_DTMF_CLAMP_KEEP;
  const uint32_t vol = (uint32_t)prm[PN_DTMF_CLAMP_VOLUME], ts = (uint32_t)prm[PN_DTMF_CLAMP_TS_PER_FRAME];
  uint32_t ongoing = 0u, done = 0u;
  if (det_on && cur != 0u) { ongoing = pn_dtmf_event_payload_hd(cur, false, vol, dur, ts); if (ongoing) flags |= PN_DTMF_CLAMP_EVENT; }
  if (det_on && (d0 & PN_DTMF_END)) { done = pn_dtmf_event_payload_hd(ended, true, vol, st[3] ? st[3] : 1u, ts); if (done) flags |= PN_DTMF_CLAMP_EVENT_END; }
  st[0] = marks; st[1] = e0 ? 1u : 0u; st[2] = muted; st[3] = det_on && cur != 0u ? dur : 0u;
  rep[0] = flags; rep[1] = ongoing; rep[2] = done; rep[3] = muted;
  return kind;
}
// sample j of a row that needs a ramp (kind DOWN or UP)
PN_DTMF_CLAMP_STRICT PN_DTMF_CLAMP_HD float pn_dtmf_clamp_sample(int kind, float x, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float num = kind == PN_DTMF_CLAMP_DOWN ? (float)(PN_FRAME - 1 - j) : (float)(j + 1);
  const float w = num / 480.0f;
  return x * w;
}

// One frame of one stream with removal on: state4 is read and written, det_report4 is the detector's report row of this frame (NULL:
// detection is off), row480 is changed in place as the rule says (not touched at unity gain).  Returns the flags, -1 for a bad
// argument.  report4, optional: the report row.  The in-time condition is NOT checked here: a guard that is too long reports LATE
static inline int pn_dtmf_clamp_frame_host(const int32_t *params, uint32_t *state4, const uint32_t *det_report4, float *row480, uint32_t *report4 = NULL) {
  if (!params || !state4 || !row480) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_clamp_params_check_host(params)) return -1;
  uint32_t rep[PN_DTMF_CLAMP_REPORT_WORDS];
  const int kind = pn_dtmf_clamp_decide(params, state4, det_report4, rep);
  if (kind == PN_DTMF_CLAMP_ZERO) for (int j = 0; j < PN_FRAME; j++) row480[j] = 0.0f;
  else if (kind != PN_DTMF_CLAMP_KEEP) for (int j = 0; j < PN_FRAME; j++) row480[j] = pn_dtmf_clamp_sample(kind, row480[j], j);
  if (report4) memcpy(report4, rep, sizeof(rep));
  return (int)rep[0];
}
