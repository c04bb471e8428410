// Automatic level control on the rate converter (include/percepnet_hip.h "automatic level control"), the rule stated once — HIP-free
// (builds with -DPN_NO_HIP): the host's pn_agc_frame is pn_agc_frame_host below, the kernel (pn_rate_agc.hip pn_rate_agc_kernel) computes
// the same values in the same order, tests/agc_model.py restates them in numpy float32, tests/c/agc_sanitize.cpp runs them under the
// sanitizers over exactly-sized buffers.
// Every fp32 operation is singly rounded (no product is contracted into an add; `/` and sqrtf are the correctly rounded ones) and every
// sum runs in the ONE order written here.  Samples are in the float convention (int16 / 32768).
//
// Parameters, one set per converter (PN_AGC_N_PARAMS = 8 floats; pn_agc_params_check refuses NaN and anything outside a range):
//   0 PN_AGC_MAX_GAIN   Gmax       [1, 1024]     16
//   1 PN_AGC_MIN_GAIN   Gmin       [1/1024, 1]   0.125
//   2 PN_AGC_GATE_RMS   theta      [0, 1]        0.001
//   3 PN_AGC_ATTACK     level rising   (0, 1]    0.5
//   4 PN_AGC_RELEASE    level falling  (0, 1]    0.05
//   5 PN_AGC_STEP_UP    largest gain ratio per frame  [1, 2]   1.0592537 (+0.5 dB)
//   6 PN_AGC_STEP_DOWN  smallest                      (0, 1]   0.8912509 (-1 dB)
//   7 PN_AGC_CEILING    c          (0, 1]        32767/32768
// Target, one fp32 per stream: T, the wanted RMS in (0, 1]; 0 (also -0.0f): the stream is not levelled.
// State of one stream (PN_AGC_STATE_BYTES = 16): lev f32, the smoothed frame energy; gain f32, whose bits 0 mean "fresh" and read as
// 1.0f (the rule keeps a gain that starts in [Gmin, max(Gmax, 1)] there, so 0 is never a live value); adapted u32, the frames that
// adapted, saturating; one spare word, always 0.
//
// One frame of an advancing stream, y = its 480-sample row from the engine; concealed: PLC filled this frame for it.
//   T == 0      row and state are not touched; the report row is {1.0f, +0.0f, 0, +0.0f}
//   E           the energy of y in the mix's order (pn_mix_rules.h pn_mix_level_host): products rounded separately, 120 groups of
//               four from +0.0f in index order, padded to 128, two halves of 64 folded by the xor butterfly 32..1, E = half0[0] + half1[0]
//   p           max |y[j]| from +0.0f with fmaxf: a NaN sample is ignored
//   Eg, Tt      (theta * theta) * 480.0f, (T * T) * 480.0f
//   voiced      E > Eg && E <= FLT_MAX && !concealed
//   lev'        not voiced: lev.  Voiced, lev == 0: E.  Voiced otherwise: a = E > lev ? attack : release, d = E - lev, t = a * d, lev + t
//   g*          voiced: sqrtf(Tt / lev'), then > Gmax -> Gmax (AT_MAX), then < Gmin -> Gmin (AT_MIN).  Otherwise g0: the gain holds
//   slew        g0 = the stored gain, 1.0f when fresh; hi = g0 * step_up, lo = g0 * step_down, g1 = fminf(fmaxf(g*, lo), hi)
//   limiter     m = fmaxf(g0, g1); p <= FLT_MAX && p * m > c (LIMITED): gl = fmaxf(c / p, Gmin), g0' = fminf(g0, gl), g1' = fminf(g1, gl);
//               otherwise g0' = g0, g1' = g1.  A row whose peak exceeds c / Gmin is beyond rescue and CLIPS
//   apply       w_j = (float)(2 j + 1) / 960.0f, d = g1' - g0', out[j] = y[j] * (g0' + w_j * d): a product, an add, a product, none fused.
//               With g0' == g1' == 1.0f the row keeps its bits, -0.0 included
//   state       lev = lev', gain = g1', adapted += voiced
// Report (PN_AGC_REPORT_WORDS = 4): f32 g1', f32 lev', u32 flags (PN_AGC_ON | ADAPTED | LIMITED | AT_MAX | AT_MIN | HELD_LOST), f32 p.
#pragma once
#include "pn_mix_rules.h"    // pn_mix_level_host: E in the one order; pn_ids_check, pn_set_error, the header's PN_AGC_* constants
#include <float.h>
#include <math.h>
#include <string.h>

#define PN_AGC_STATE_BYTES 16
#define PN_AGC_ADAPTED_MAX 0xffffffffu
static_assert(PN_AGC_N_PARAMS == 8 && PN_AGC_REPORT_WORDS == 4 && PN_AGC_STATE_BYTES == 4 * 4 && PN_FRAME == 480, "eight parameters, four words of state and of report");

struct PnAgcParams { float v[PN_AGC_N_PARAMS]; };     // (by value into the kernel: a parameter change is ordered like a launch)

static inline void pn_agc_default_params_host(float *p) {
  p[PN_AGC_MAX_GAIN] = 16.0f; p[PN_AGC_MIN_GAIN] = 0.125f; p[PN_AGC_GATE_RMS] = 0.001f; p[PN_AGC_ATTACK] = 0.5f; p[PN_AGC_RELEASE] = 0.05f;
  p[PN_AGC_STEP_UP] = 1.0592537f; p[PN_AGC_STEP_DOWN] = 0.8912509f; p[PN_AGC_CEILING] = 0.999969482421875f;
}
// -1 with pn_last_error naming the FIRST bad index: NaN, or a value outside its range
static inline int pn_agc_params_check_host(const float *p) {
  if (!p) { pn_set_error("NULL argument"); return -1; }
  static const struct { const char *name, *range; float lo, hi; bool open_lo; } k[PN_AGC_N_PARAMS] = {
      {"max_gain", "[1, 1024]", 1.0f, 1024.0f, false},   {"min_gain", "[1/1024, 1]", 1.0f / 1024.0f, 1.0f, false},
      {"gate_rms", "[0, 1]", 0.0f, 1.0f, false},         {"attack", "(0, 1]", 0.0f, 1.0f, true},
      {"release", "(0, 1]", 0.0f, 1.0f, true},           {"step_up", "[1, 2]", 1.0f, 2.0f, false},
      {"step_down", "(0, 1]", 0.0f, 1.0f, true},         {"ceiling", "(0, 1]", 0.0f, 1.0f, true}};
  for (int i = 0; i < PN_AGC_N_PARAMS; i++)
    if (!((k[i].open_lo ? p[i] > k[i].lo : p[i] >= k[i].lo) && p[i] <= k[i].hi)) {     // (false for NaN)
      pn_set_error("AGC parameter %g at index %d (%s): a value in %s", (double)p[i], i, k[i].name, k[i].range);
      return -1;
    }
  return 0;
}
// targets[0..n): 0 (not levelled; -0.0f is 0) or an RMS in (0, 1].  -1 with pn_last_error naming the FIRST bad index
static inline bool pn_agc_target_ok(float t) { return t >= 0.0f && t <= 1.0f; }           // (false for NaN)
static inline int pn_agc_targets_list_check(const float *targets, int n) {
  if (n < 0 || (n > 0 && !targets)) { pn_set_error("bad argument"); return -1; }
  for (int i = 0; i < n; i++)
    if (!pn_agc_target_ok(targets[i])) { pn_set_error("AGC target %g at index %d: 0 (not levelled) or an RMS in (0, 1]", (double)targets[i], i); return -1; }
  return 0;
}
static inline int pn_agc_targets_set_check(int B, const int32_t *ids, int n, const float *targets) {
  if (pn_ids_check(B, ids, n, true)) return -1;
  return pn_agc_targets_list_check(targets, n);
}

// The scalar half of a frame: from E, p and the state to the two gains the row is scaled between, the new state and the report row.
// The kernel's every lane runs the same statements (pn_rate_agc.hip ag_update).
struct PnAgcStep { float g0, g1, lev, peak; uint32_t adapted, flags; };
#if defined(__GNUC__) && !defined(__clang__)
#define PN_AGC_STRICT __attribute__((optimize("fp-contract=off")))
#else
#define PN_AGC_STRICT
#endif
PN_AGC_STRICT static inline PnAgcStep pn_agc_step_host(const float *P, float T, const uint32_t state[4], float E, float p, bool concealed) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float lev, g0;
  memcpy(&lev, &state[0], 4); memcpy(&g0, &state[1], 4);
  if (state[1] == 0u) g0 = 1.0f;
  const float Gmax = P[PN_AGC_MAX_GAIN], Gmin = P[PN_AGC_MIN_GAIN], th = P[PN_AGC_GATE_RMS], c = P[PN_AGC_CEILING];
  const float th2 = th * th, Eg = th2 * 480.0f, T2 = T * T, Tt = T2 * 480.0f;
  const bool voiced = E > Eg && E <= FLT_MAX && !concealed;
  uint32_t flags = PN_AGC_ON | (concealed ? PN_AGC_HELD_LOST : 0u);
  float gs = g0;
  if (voiced) {
    if (lev == 0.0f) lev = E;
    else { const float a = E > lev ? P[PN_AGC_ATTACK] : P[PN_AGC_RELEASE], d = E - lev, t = a * d; lev = lev + t; }
    const float q = Tt / lev;
    gs = sqrtf(q);
    if (gs > Gmax) { gs = Gmax; flags |= PN_AGC_AT_MAX; }
    if (gs < Gmin) { gs = Gmin; flags |= PN_AGC_AT_MIN; }
    flags |= PN_AGC_ADAPTED;
  }
  const float hi = g0 * P[PN_AGC_STEP_UP], lo = g0 * P[PN_AGC_STEP_DOWN];
  float g1 = fminf(fmaxf(gs, lo), hi);
  const float m = fmaxf(g0, g1), pm = p * m;
  if (p <= FLT_MAX && pm > c) {
    const float gl = fmaxf(c / p, Gmin);
    g0 = fminf(g0, gl); g1 = fminf(g1, gl);
    flags |= PN_AGC_LIMITED;
  }
  PnAgcStep o;
  o.g0 = g0; o.g1 = g1; o.lev = lev; o.peak = p; o.flags = flags;
  o.adapted = state[2] + ((voiced && state[2] != PN_AGC_ADAPTED_MAX) ? 1u : 0u);
  return o;
}
// out[j] = y[j] * (g0 + w_j * (g1 - g0)), w_j = (float)(2 j + 1) / 960.0f
PN_AGC_STRICT static inline float pn_agc_apply_host(float y, float g0, float g1, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float w = (float)(2 * j + 1) / 960.0f, d = g1 - g0, t = w * d, g = g0 + t;
  return y * g;
}
static inline float pn_agc_peak_host(const float *y) {
  float p = 0.0f;
  for (int j = 0; j < PN_FRAME; j++) p = fmaxf(p, fabsf(y[j]));
  return p;
}
// One frame of one stream: state4 is read and written, row_out may be row_in.  Returns the flags (0 for a stream that is not
// levelled, whose row is copied bit for bit), -1 for a bad argument.  report4, optional: the report row
static inline int pn_agc_frame_host(const float *params, float target, uint32_t *state4, const float *row_in, float *row_out, int concealed, uint32_t *report4 = NULL) {
  if (!params || !state4 || !row_in || !row_out) { pn_set_error("NULL argument"); return -1; }
  if (pn_agc_params_check_host(params) || pn_agc_targets_list_check(&target, 1)) return -1;
  if (target == 0.0f) {
    if (row_out != row_in) memmove(row_out, row_in, PN_FRAME * sizeof(float));
    if (report4) { const float one = 1.0f; memcpy(&report4[0], &one, 4); report4[1] = report4[2] = report4[3] = 0u; }
    return 0;
  }
  const PnAgcStep st = pn_agc_step_host(params, target, state4, pn_mix_level_host(row_in), pn_agc_peak_host(row_in), concealed != 0);
  for (int j = 0; j < PN_FRAME; j++) row_out[j] = pn_agc_apply_host(row_in[j], st.g0, st.g1, j);
  memcpy(&state4[0], &st.lev, 4); memcpy(&state4[1], &st.g1, 4); state4[2] = st.adapted; state4[3] = 0u;
  if (report4) { memcpy(&report4[0], &st.g1, 4); memcpy(&report4[1], &st.lev, 4); report4[2] = st.flags; memcpy(&report4[3], &st.peak, 4); }
  return (int)st.flags;
}
