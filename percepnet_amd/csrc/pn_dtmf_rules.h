// In-band DTMF detection on the rate converter (include/percepnet_hip.h "DTMF detection"), the rule stated once — HIP-free (builds with
// -DPN_NO_HIP): the host's pn_dtmf_frame is pn_dtmf_frame_host below, the kernel (pn_rate_dtmf.hip pn_rate_dtmf_kernel) forms the same sums
// in the same order and runs the SAME scalar statements (pn_dtmf_power, pn_dtmf_decide and pn_dtmf_held, compiled for both sides), tests/dtmf_model.py restates them in numpy
// float32, tests/c/dtmf_sanitize.cpp runs them under the sanitizers over exactly-sized buffers.
// Every fp32 operation is singly rounded (no product is contracted into an add) and every sum runs in the ONE order written here.
// Samples are in the float convention (int16 / 32768).
//
// Frequencies f[0..3] = 697, 770, 852, 941 Hz (rows), f[4..7] = 1209, 1336, 1477, 1633 Hz (columns); the digit code of row r and column c
// is the ASCII of "123A456B789C*0#D"[4 r + c].
// Tables, computed in double and narrowed to float once: for k = 0..7, j = 0..479: m = (f[k] * j) % 48000 in integers,
// a = 6.283185307179586 * m / 48000.0, ct[k][j] = (float)cos(a), st[k][j] = (float)sin(a).  The rotation of one frame: m = (f[k] * 480) %
// 48000, cr[k] = (float)cos(a), ci[k] = (float)sin(a); rot16 = cr[0..7], ci[0..7].
//
// Parameters, one set per converter (PN_DTMF_N_PARAMS = 7 floats; pn_dtmf_params_check refuses NaN and anything outside a range):
//   0 PN_DTMF_MIN_RMS    the window's least RMS                          [0, 1]    0.005
//   1 PN_DTMF_PURITY     the two peaks' share of the window's energy     (0, 1]    0.5
//   2 PN_DTMF_TWIST_FWD  largest column power over row power             [1, 100]  6.3
//   3 PN_DTMF_TWIST_REV  largest row power over column power             [1, 100]  6.3
//   4 PN_DTMF_REL        a group's peak over its other three             [1, 100]  6.3
//   5 PN_DTMF_ON_FRAMES  hits in a row that begin a digit      a whole number in [1, 100]  3
//   6 PN_DTMF_OFF_FRAMES frames without it that end a digit    a whole number in [1, 100]  2
// State of one stream (PN_DTMF_STATE_BYTES = 96, 24 words; all zero is fresh): 0..7 Cp, 8..15 Sp, 16 Ep (f32, the previous row's half
// sums), 17 cand | run << 16, 18 cur | gap << 16, 19 dur, 20 count, 21 last4, 22 and 23 always 0.
//
// One frame of an advancing stream with detection on, x = its 480-sample row of x48; concealed: PLC filled this frame for it.
//   half sums  C[k] = sum x[j] * ct[k][j], S[k] = sum x[j] * st[k][j], Ec = sum x[j] * x[j] (pn_mix_rules.h pn_mix_level_host), all 17 in
//              the mix level's layout and order: products rounded separately, 120 groups of four from +0.0f in index order, padded to
//              128, two halves of 64 folded by the xor butterfly 32..1, the sum = half0[0] + half1[0]
//   window     the 20 ms of the previous row and this one, coherently and without a second pass over samples:
//              A = Cp + (C * cr - S * ci), B = Sp + (S * cr + C * ci), each product and each sum rounded separately in that bracketing;
//              P[k] = A * A + B * B; E = Ep + Ec.  Then Cp, Sp, Ep = C, S, Ec
//   peaks      Pr = -1.0f, r = 0; for k = 0..3 in order: P[k] > Pr -> Pr = P[k], r = k.  Pc, c likewise over k = 4..7 (c counts from 0).
//              Ties go to the lower index and a NaN never wins; Pr is P[r] unless all four are NaN
//   hit        E <= FLT_MAX && E >= (min_rms * min_rms) * 960.0f && Pr + Pc >= (purity * 480.0f) * E && Pc <= Pr * twist_fwd &&
//              Pr <= Pc * twist_rev && for every other k of either group P[k] * rel <= that group's peak: any NaN makes it false.
//              (A pure dual tone has P[r] + P[c] = 480 E.)
//   d          the digit code on a hit, else 0
//   debounce   in this order, cur0 being cur as the frame found it:
//              1. d != 0 && d == cand: run += 1, saturating at 65535.  Otherwise cand = d, run = d ? 1 : 0
//              2. cur0 != 0 && d == cur0: gap = 0, dur += 1 (saturating)
//              3. cur0 != 0 && d != cur0: gap += 1; gap >= off_frames: END, ended = cur0, its dur goes to the report, cur = 0, gap = 0,
//                 dur = 0; otherwise dur += 1 (saturating)
//              4. cur == 0 && d != 0 && run >= on_frames: cur = d, gap = 0, dur = run, count += 1 (saturating), BEGIN,
//                 last4 = (last4 << 8) | d
//   concealed  the whole state is left untouched and the row is not read; the report repeats cur, dur, count, last4 with HELD_LOST
//   not on     neither the row nor the state is read; the report row is four zero words
// Report (PN_DTMF_REPORT_WORDS = 4): word 0 flags | cur << 8 | ended << 16 (PN_DTMF_ON | HIT | BEGIN | END | HELD_LOST); word 1 the dur of
// cur or, with cur == 0 in a frame that ENDs, of the digit that ended, else 0; word 2 count; word 3 last4.
#pragma once
#include "pn_mix_rules.h"    // pn_mix_level_host: Ec in the one order; pn_ids_check, pn_set_error, the header's PN_DTMF_* constants
#include <float.h>
#include <math.h>
#include <string.h>

#define PN_DTMF_STATE_BYTES 96
#define PN_DTMF_STATE_WORDS 24
#define PN_DTMF_NF 8                                   // frequencies
#define PN_DTMF_NSUM 17                                // C[8], S[8], Ec
#define PN_DTMF_RUN_MAX 0xffffu
#define PN_DTMF_SAT 0xffffffffu
static_assert(PN_DTMF_N_PARAMS == 7 && PN_DTMF_REPORT_WORDS == 4 && PN_DTMF_STATE_BYTES == 4 * PN_DTMF_STATE_WORDS && PN_FRAME == 480, "seven parameters, 24 words of state, four of report");

#if defined(__HIPCC__) && !defined(PN_NO_HIP)
#define PN_DTMF_HD __host__ __device__ __forceinline__
#else
#define PN_DTMF_HD static inline
#endif
#if defined(__GNUC__) && !defined(__clang__)
#define PN_DTMF_STRICT __attribute__((optimize("fp-contract=off")))
#define PN_DTMF_UNROLL
#else
#define PN_DTMF_STRICT
#define PN_DTMF_UNROLL _Pragma("unroll")
#endif

struct PnDtmfParams { float v[PN_DTMF_N_PARAMS]; float rot[2 * PN_DTMF_NF]; };   // (by value into the kernel: a parameter change is ordered like a launch)
struct PnDtmfTables { float ct[PN_DTMF_NF][PN_FRAME], st[PN_DTMF_NF][PN_FRAME], rot[2 * PN_DTMF_NF]; };

static inline int pn_dtmf_freq(int k) { static const int f[PN_DTMF_NF] = {697, 770, 852, 941, 1209, 1336, 1477, 1633}; return f[k]; }
static inline const PnDtmfTables &pn_dtmf_tables_ref() {
  static const PnDtmfTables T = [] {
    PnDtmfTables t;
    for (int k = 0; k < PN_DTMF_NF; k++) {
      for (int j = 0; j <= PN_FRAME; j++) {
        const int m = (pn_dtmf_freq(k) * j) % 48000;
        const double a = 6.283185307179586 * m / 48000.0;
        if (j < PN_FRAME) { t.ct[k][j] = (float)cos(a); t.st[k][j] = (float)sin(a); }
        else { t.rot[k] = (float)cos(a); t.rot[PN_DTMF_NF + k] = (float)sin(a); }
      }
    }
    return t;
  }();
  return T;
}
// ct, st: [8][480] each; rot16: cr[0..7], ci[0..7]
static inline int pn_dtmf_tables_host(float *ct, float *st, float *rot16) {
  if (!ct || !st || !rot16) { pn_set_error("NULL argument"); return -1; }
  const PnDtmfTables &T = pn_dtmf_tables_ref();
  memcpy(ct, T.ct, sizeof(T.ct)); memcpy(st, T.st, sizeof(T.st)); memcpy(rot16, T.rot, sizeof(T.rot));
  return 0;
}

static inline void pn_dtmf_default_params_host(float *p) {
  p[PN_DTMF_MIN_RMS] = 0.005f; p[PN_DTMF_PURITY] = 0.5f; p[PN_DTMF_TWIST_FWD] = 6.3f; p[PN_DTMF_TWIST_REV] = 6.3f; p[PN_DTMF_REL] = 6.3f;
  p[PN_DTMF_ON_FRAMES] = 3.0f; p[PN_DTMF_OFF_FRAMES] = 2.0f;
}
// -1 with pn_last_error naming the FIRST bad index: NaN, a value outside its range, or a frame count that is no whole number
static inline int pn_dtmf_params_check_host(const float *p) {
  if (!p) { pn_set_error("NULL argument"); return -1; }
  static const struct { const char *name, *range; float lo, hi; bool open_lo, whole; } k[PN_DTMF_N_PARAMS] = {
      {"min_rms", "[0, 1]", 0.0f, 1.0f, false, false},      {"purity", "(0, 1]", 0.0f, 1.0f, true, false},
      {"twist_fwd", "[1, 100]", 1.0f, 100.0f, false, false}, {"twist_rev", "[1, 100]", 1.0f, 100.0f, false, false},
      {"rel", "[1, 100]", 1.0f, 100.0f, false, false},       {"on_frames", "a whole number in [1, 100]", 1.0f, 100.0f, false, true},
      {"off_frames", "a whole number in [1, 100]", 1.0f, 100.0f, false, true}};
  for (int i = 0; i < PN_DTMF_N_PARAMS; i++)
    if (!((k[i].open_lo ? p[i] > k[i].lo : p[i] >= k[i].lo) && p[i] <= k[i].hi && (!k[i].whole || p[i] == floorf(p[i])))) {     // (false for NaN)
      pn_set_error("DTMF parameter %g at index %d (%s): a value in %s", (double)p[i], i, k[i].name, k[i].range);
      return -1;
    }
  return 0;
}
static inline int pn_dtmf_on_set_check(int B, const int32_t *ids, int n, const uint8_t *on) {
  if (n > 0 && !on) { pn_set_error("bad argument"); return -1; }
  return pn_ids_check(B, ids, n, true);
}

// sum x[j] * w[j] in the layout and order of pn_mix_level_host (which is this with w = x)
PN_DTMF_STRICT static inline float pn_dtmf_dot_host(const float *x, const float *w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float v[128], t[64];
  for (int q = 0; q < 128; q++) {
    float e = 0.0f;
    if (q < PN_FRAME / 4)
      for (int i = 0; i < 4; i++) { const float p = x[4 * q + i] * w[4 * q + i]; e = e + p; }
    v[q] = e;
  }
  for (int half = 0; half < 2; half++) {
    float *h = v + 64 * half;
    for (int stride = 32; stride >= 1; stride >>= 1) {
      for (int i = 0; i < 64; i++) t[i] = h[i] + h[i ^ stride];
      memcpy(h, t, sizeof(t));
    }
  }
  return v[0] + v[64];
}

// The scalar half of a frame, in three pieces that the host runs one after the other (pn_dtmf_step) and every lane of the kernel's
// deciding wave runs with the state streaming through in between.  One text for both sides; no array is indexed by a value computed at
// run time, so the kernel keeps all of it in registers.
PN_DTMF_HD float pn_dtmf_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
PN_DTMF_HD uint32_t pn_dtmf_u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
PN_DTMF_HD uint32_t pn_dtmf_inc(uint32_t v) { return v == PN_DTMF_SAT ? v : v + 1u; }
// the window's powers: prev = state words 0..15 (Cp, Sp), sums = C[0..7], S[0..7]
PN_DTMF_STRICT PN_DTMF_HD void pn_dtmf_power(const float *rot, const uint32_t *prev, const float *sums, float *P) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
PN_DTMF_UNROLL
  for (int k = 0; k < PN_DTMF_NF; k++) {
    const float C = sums[k], S = sums[PN_DTMF_NF + k], cr = rot[k], ci = rot[PN_DTMF_NF + k];
    const float a0 = C * cr, a1 = S * ci, a2 = a0 - a1, A = pn_dtmf_f(prev[k]) + a2;
    const float b0 = S * cr, b1 = C * ci, b2 = b0 + b1, B = pn_dtmf_f(prev[PN_DTMF_NF + k]) + b2;
    const float aa = A * A, bb = B * B;
    P[k] = aa + bb;
  }
}
// a concealed frame's report row: tail = state words 16..23, which stay
PN_DTMF_HD void pn_dtmf_held(const uint32_t *tail, uint32_t *rep) {
  const uint32_t cur = tail[2] & 0xffu;
  rep[0] = PN_DTMF_ON | PN_DTMF_HELD_LOST | (cur << 8); rep[1] = cur ? tail[3] : 0u; rep[2] = tail[4]; rep[3] = tail[5];
}
// peaks, hit and debounce: tail = state words 16..23 (Ep, cand | run << 16, cur | gap << 16, dur, count, last4, 0, 0), read and written
PN_DTMF_STRICT PN_DTMF_HD void pn_dtmf_decide(const float *prm, const float *P, float Ec, uint32_t *tail, uint32_t *rep) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float E = pn_dtmf_f(tail[0]) + Ec;
  float Pr = -1.0f, Pc = -1.0f;
  int r = 0, c = 0;
PN_DTMF_UNROLL
  for (int k = 0; k < 4; k++) {
    if (P[k] > Pr) { Pr = P[k]; r = k; }
    if (P[4 + k] > Pc) { Pc = P[4 + k]; c = k; }
  }
  const float mr = prm[PN_DTMF_MIN_RMS], m2 = mr * mr, Emin = m2 * 960.0f, pu = prm[PN_DTMF_PURITY] * 480.0f, need = pu * E;
  const float both = Pr + Pc, cmax = Pr * prm[PN_DTMF_TWIST_FWD], rmax = Pc * prm[PN_DTMF_TWIST_REV], rel = prm[PN_DTMF_REL];
  bool hit = E <= FLT_MAX && E >= Emin && both >= need && Pc <= cmax && Pr <= rmax;
PN_DTMF_UNROLL
  for (int k = 0; k < 4; k++) {
    const float qr = P[k] * rel, qc = P[4 + k] * rel;
    hit = hit && (k == r || qr <= Pr) && (k == c || qc <= Pc);
  }
  // "123A456B789C*0#D"[4 r + c], four codes a word, low byte first
  const uint32_t row_codes = r == 0 ? 0x41333231u : r == 1 ? 0x42363534u : r == 2 ? 0x43393837u : 0x4423302au;
  const uint32_t d = hit ? (row_codes >> (8 * c)) & 0xffu : 0u;
  const uint32_t on_frames = (uint32_t)prm[PN_DTMF_ON_FRAMES], off_frames = (uint32_t)prm[PN_DTMF_OFF_FRAMES];
  uint32_t cand = tail[1] & 0xffu, run = tail[1] >> 16, cur = tail[2] & 0xffu, gap = tail[2] >> 16, dur = tail[3], count = tail[4], last4 = tail[5];
  uint32_t flags = PN_DTMF_ON | (hit ? PN_DTMF_HIT : 0u), ended = 0u, ended_dur = 0u;
  if (d != 0u && d == cand) run = run == PN_DTMF_RUN_MAX ? run : run + 1u;
  else { cand = d; run = d ? 1u : 0u; }
  if (cur != 0u) {
    if (d == cur) { gap = 0u; dur = pn_dtmf_inc(dur); }
    else {
      gap += 1u;
      if (gap >= off_frames) { flags |= PN_DTMF_END; ended = cur; ended_dur = dur; cur = 0u; gap = 0u; dur = 0u; }
      else dur = pn_dtmf_inc(dur);
    }
  }
  if (cur == 0u && d != 0u && run >= on_frames) {
    cur = d; gap = 0u; dur = run; count = pn_dtmf_inc(count); flags |= PN_DTMF_BEGIN;
    last4 = (last4 << 8) | d;
  }
  tail[0] = pn_dtmf_u(Ec); tail[1] = cand | (run << 16); tail[2] = cur | (gap << 16); tail[3] = dur; tail[4] = count; tail[5] = last4; tail[6] = 0u; tail[7] = 0u;
  rep[0] = flags | (cur << 8) | (ended << 16); rep[1] = cur ? dur : ended_dur; rep[2] = count; rep[3] = last4;
}
// st: the 24 state words, read and written unless concealed.  sums: C[0..7], S[0..7], Ec (not read when concealed)
static inline void pn_dtmf_step(const float *prm, const float *rot, uint32_t *st, const float *sums, bool concealed, uint32_t *rep) {
  if (concealed) { pn_dtmf_held(st + 16, rep); return; }
  float P[PN_DTMF_NF];
  pn_dtmf_power(rot, st, sums, P);
  memcpy(st, sums, 16 * sizeof(float));
  pn_dtmf_decide(prm, P, sums[2 * PN_DTMF_NF], st + 16, rep);
}

// One frame of one stream with detection on: state24 is read and written, row480 is read unless concealed.  Returns the flags, -1 for a
// bad argument.  report4, optional: the report row
static inline int pn_dtmf_frame_host(const float *params, uint32_t *state24, const float *row480, int concealed, uint32_t *report4 = NULL) {
  if (!params || !state24 || !row480) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_params_check_host(params)) return -1;
  const PnDtmfTables &T = pn_dtmf_tables_ref();
  float sums[PN_DTMF_NSUM] = {};
  if (!concealed) {
    for (int k = 0; k < PN_DTMF_NF; k++) { sums[k] = pn_dtmf_dot_host(row480, T.ct[k]); sums[PN_DTMF_NF + k] = pn_dtmf_dot_host(row480, T.st[k]); }
    sums[2 * PN_DTMF_NF] = pn_mix_level_host(row480);
  }
  uint32_t rep[PN_DTMF_REPORT_WORDS];
  pn_dtmf_step(params, T.rot, state24, sums, concealed != 0, rep);
  if (report4) memcpy(report4, rep, sizeof(rep));
  return (int)rep[0] & 0xff;
}
