// Packet-loss concealment on the rate converter (include/percepnet_hip.h "packet-loss concealment"), the signal rule stated once —
// HIP-free (builds with -DPN_NO_HIP): the host's pn_plc_pitch / pn_plc_period / pn_plc_gain are these functions, the kernel
// (pn_rate_plc.hip pn_rate_plc_kernel) computes the same values in the same order, tests/plc_model.py restates them in numpy
// float32, tests/c/plc_sanitize.cpp runs them under the sanitizers over exactly-sized buffers.
// Every fp32 operation is singly rounded (no product is contracted into an add; divisions are the correctly rounded ones) and every
// sum runs in the ONE order written here.
//
// State of one stream (PN_PLC_STATE_BYTES = 10576, in three arrays on the device):
//   hist  [4][480] float  7680 B  a ring of the last four rows the engine was given, real or synthetic; row `head` is the OLDEST and
//                                 the one the next row replaces.  hist[i] below is the linear view, oldest first: ring row
//                                 (head + i / 480) & 3, column i % 480; hist[1919] is the newest sample
//   q     [720] float     2880 B  the period buffer; q[0..P) is live
//   meta  [4] uint32        16 B  P (0 until the first loss), r = consecutive lost frames so far, lost frames since reset, head
//
// One frame of an advancing stream, x = its 48 kHz row:
//   received, r == 0   x is not altered; it replaces the oldest history row
//   lost, r == 0       P = pitch(hist), q = period(hist, P); then as "lost"
//   lost               x[n] = syn(480 r + n); x replaces the oldest history row; r += 1 (it stays at PN_PLC_RUN_MAX); lost += 1
//   received, r > 0    n < 240: s = syn(480 r + n), x[n] = s + w * (x[n] - s) with w = (float)(2 n + 1) / 480.0f — the difference, the
//                      product and the sum each rounded; n >= 240: the real bits.  x replaces the oldest history row; r = 0
//   syn(m) = m < 2880 ? gain(m) * q[m % P] : +0.0f   (one product; r >= 6 is silence without a look at q)
#pragma once
#include "pn_host_rules.h"   // pn_set_error, PN_FRAME, the header's PN_PLC_* constants
#include <math.h>
#include <string.h>

#define PN_PLC_COARSE_N 320                    // d[k] = hist[6 k + 5]: every sixth sample, the newest included
#define PN_PLC_COARSE_K0 160                   // the coarse sums run over k = 160 .. 319
#define PN_PLC_LAG_LO 40                       // coarse lags 40 .. 120 (8 kHz samples): 66.7 .. 200 Hz
#define PN_PLC_LAG_HI 120
#define PN_PLC_FINE_K0 960                     // the fine sums run over k = 960 .. 1919 (20 ms), in PN_PLC_FINE_PARTS interleaved parts
#define PN_PLC_FINE_PARTS 8
#define PN_PLC_FINE_MAX 11                     // at most 11 fine lags: 6 l - 5 .. 6 l + 5 clipped to [PN_PLC_P_MIN, PN_PLC_P_MAX]
#define PN_PLC_FADE_START 480                  // gain 1 over the first 10 ms of a loss
#define PN_PLC_FADE_END 2880                   // silence from 60 ms on
#define PN_PLC_XFADE 240                       // the cross-fade into the first received frame: 5 ms
#define PN_PLC_RUN_MAX 0x7fffffffu
#define PN_PLC_STATE_BYTES (4 * (PN_PLC_HIST + PN_PLC_P_MAX + 4))
static_assert(PN_PLC_HIST == 4 * PN_FRAME && PN_PLC_HIST == 6 * PN_PLC_COARSE_N && 2 * PN_PLC_P_MAX <= PN_PLC_HIST &&
              6 * PN_PLC_LAG_LO == PN_PLC_P_MIN && 6 * PN_PLC_LAG_HI == PN_PLC_P_MAX && PN_PLC_COARSE_K0 >= PN_PLC_LAG_HI &&
              PN_PLC_FINE_K0 >= PN_PLC_P_MAX && (PN_PLC_HIST - PN_PLC_FINE_K0) % PN_PLC_FINE_PARTS == 0 && PN_PLC_STATE_BYTES == 10576,
              "four rows of history hold two periods of the longest lag and both search windows");

#if defined(__GNUC__) && !defined(__clang__)
#define PN_PLC_STRICT __attribute__((optimize("fp-contract=off")))
#else
#define PN_PLC_STRICT
#endif

// The score of a lag from its cross term c and its energy e: c * c / e (a product, then a division) where c > 0, e > 0 and the
// quotient is not NaN (inf / inf); +0.0f otherwise.
PN_PLC_STRICT static inline float pn_plc_score(float c, float e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(c > 0.0f && e > 0.0f)) return 0.0f;
  const float cc = c * c, s = cc / e;
  return s == s ? s : 0.0f;
}
// The best of n scores: best = +0.0f at index 0; index i in ascending order wins when score[i] > best, strictly — ties and a row
// of zeros go to the smallest lag.
static inline int pn_plc_best(const float *score, int n) {
  float best = 0.0f;
  int at = 0;
  for (int i = 0; i < n; i++)
    if (score[i] > best) { best = score[i]; at = i; }
  return at;
}

// The coarse lag in [40, 120]: for every lag l, c = the sum over k = 160 .. 319 ASCENDING of d[k] * d[k - l] and e = the sum of
// d[k - l] * d[k - l], each from +0.0f as acc = acc + product.
PN_PLC_STRICT static inline int pn_plc_coarse_host(const float *hist) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float d[PN_PLC_COARSE_N], score[PN_PLC_LAG_HI - PN_PLC_LAG_LO + 1];
  for (int k = 0; k < PN_PLC_COARSE_N; k++) d[k] = hist[6 * k + 5];
  for (int l = PN_PLC_LAG_LO; l <= PN_PLC_LAG_HI; l++) {
    float c = 0.0f, e = 0.0f;
    for (int k = PN_PLC_COARSE_K0; k < PN_PLC_COARSE_N; k++) {
      const float pc = d[k] * d[k - l], pe = d[k - l] * d[k - l];
      c = c + pc; e = e + pe;
    }
    score[l - PN_PLC_LAG_LO] = pn_plc_score(c, e);
  }
  return PN_PLC_LAG_LO + pn_plc_best(score, PN_PLC_LAG_HI - PN_PLC_LAG_LO + 1);
}
// The lag P in [240, 720] around the coarse lag l: L runs over [max(240, 6 l - 5), min(720, 6 l + 5)].  For every L the 960 terms
// k = 960 .. 1919 are summed in 8 interleaved parts: part j = the sum over i = 0 .. 119 ASCENDING of the terms k = 960 + 8 i + j, from
// +0.0f; then c = ((((((p0 + p1) + p2) + p3) + p4) + p5) + p6) + p7, and e the same over hist[k - L]^2.
PN_PLC_STRICT static inline int pn_plc_fine_host(const float *hist, int l) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lo = 6 * l - 5 < PN_PLC_P_MIN ? PN_PLC_P_MIN : 6 * l - 5, hi = 6 * l + 5 > PN_PLC_P_MAX ? PN_PLC_P_MAX : 6 * l + 5;
  float score[PN_PLC_FINE_MAX];
  for (int L = lo; L <= hi; L++) {
    float pc[PN_PLC_FINE_PARTS], pe[PN_PLC_FINE_PARTS];
    for (int j = 0; j < PN_PLC_FINE_PARTS; j++) {
      float c = 0.0f, e = 0.0f;
      for (int k = PN_PLC_FINE_K0 + j; k < PN_PLC_HIST; k += PN_PLC_FINE_PARTS) {
        const float tc = hist[k] * hist[k - L], te = hist[k - L] * hist[k - L];
        c = c + tc; e = e + te;
      }
      pc[j] = c; pe[j] = e;
    }
    float c = pc[0], e = pe[0];
    for (int j = 1; j < PN_PLC_FINE_PARTS; j++) { c = c + pc[j]; e = e + pe[j]; }
    score[L - lo] = pn_plc_score(c, e);
  }
  return lo + pn_plc_best(score, hi - lo + 1);
}
static inline int pn_plc_pitch_host(const float *hist) { return pn_plc_fine_host(hist, pn_plc_coarse_host(hist)); }

// The period: the last P samples of the history, its last O = P / 4 cross-faded into the period before, so that the buffer's end
// meets its start.  i < P - O: q[i] = hist[1920 - P + i].  Otherwise a = hist[1920 - P + i], b = hist[1920 - 2 P + i],
// w = ((float)(i - (P - O)) + 0.5f) / (float)O, q[i] = a + w * (b - a): a == b gives a exactly.  Reads hist[1920 - 2 P + P - O ..].
PN_PLC_STRICT static inline int pn_plc_period_host(const float *hist, int P, float *q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!hist || !q || P < PN_PLC_P_MIN || P > PN_PLC_P_MAX) { pn_set_error("PLC period: a lag in [%d, %d] and two buffers", PN_PLC_P_MIN, PN_PLC_P_MAX); return -1; }
  const int O = P / 4;
  for (int i = 0; i < P; i++) {
    const float a = hist[PN_PLC_HIST - P + i];
    if (i < P - O) { q[i] = a; continue; }
    const float b = hist[PN_PLC_HIST - 2 * P + i], w = ((float)(i - (P - O)) + 0.5f) / (float)O, dba = b - a, t = w * dba;
    q[i] = a + t;
  }
  return 0;
}
// g(m), m = samples since the loss began: 1 for the first 10 ms, then (float)(2880 - m) / 2400.0f down to silence at 60 ms
static inline float pn_plc_gain_host(int64_t m) {
  if (m < PN_PLC_FADE_START) return 1.0f;
  if (m >= PN_PLC_FADE_END) return 0.0f;
  return (float)(PN_PLC_FADE_END - (int)m) / (float)(PN_PLC_FADE_END - PN_PLC_FADE_START);
}
// one synthetic sample, and the cross-fade of the first received row
PN_PLC_STRICT static inline float pn_plc_syn_host(const float *q, int P, uint32_t r, int n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (r >= (uint32_t)(PN_PLC_FADE_END / PN_FRAME) || P < PN_PLC_P_MIN) return 0.0f;   // (a run without a lag: no state a frame leaves)
  const int m = PN_FRAME * (int)r + n;
  return pn_plc_gain_host(m) * q[m % P];
}
PN_PLC_STRICT static inline float pn_plc_xfade_host(float syn, float real, int n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float w = (float)(2 * n + 1) / (float)(2 * PN_PLC_XFADE), d = real - syn, t = w * d;
  return syn + t;
}
