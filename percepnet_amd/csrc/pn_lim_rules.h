// Output limiter on the rate converter (include/percepnet_hip.h "output limiter"), the rule stated once — HIP-free (builds with
// -DPN_NO_HIP): the host's pn_lim_frame is pn_lim_frame_host below, the kernel (pn_rate_lim.hip pn_rate_lim_kernel) computes the same
// values in the same order, tests/lim_model.py restates them in numpy float32, tests/c/lim_sanitize.cpp runs them under the sanitizers
// over exactly-sized buffers.
// Every fp32 operation is singly rounded (no product is contracted into an add; `/` is the correctly rounded one).  The two
// reductions — a max of non-negative values and a min of indices — are free of ordering.  Samples are in the float convention
// (int16 / 32768).
//
// Ceiling, one fp32 per stream: c in [1/1024, 1]; 0 (also -0.0f), the default: the stream is not limited.
// Parameters, one set per converter (PN_LIM_N_PARAMS = 2 floats; pn_lim_params_check refuses NaN and anything outside a range):
//   0 PN_LIM_RELEASE   R   largest gain ratio per frame on the way back to 1    [1, 2]                      1.0592537 (+0.5 dB, the AGC's step)
//   1 PN_LIM_HOLD      H   frames the gain is held after an attack              a whole number in [0, 1000] 2
// State of one stream (PN_LIM_STATE_BYTES = 16): gain f32, whose bits 0 mean "fresh" and read as 1.0f (the rule keeps a gain in
// (0, 1], so 0 is never a live value); hold u32, the frames still to hold; limited u32, the frames whose gain was under 1,
// saturating; one spare word, always 0.  Only the rule writes a state.
//
// One frame of an advancing stream with c > 0, o = the 480-sample row the down-conversion is about to read:
//   g0, h       the stored gain (1.0f when fresh) and hold count
//   p           max |o[j]| from +0.0f with fmaxf: a NaN sample is ignored
//   non-finite  !(p <= FLT_MAX) (NONFINITE): row and state are not touched
//   needed      p > c: q = c / p; if p * q > c then q becomes the float one bit below it; gl = q.  Otherwise gl = 1.0f.
//               (fl(p * q) > c implies q > c / p in the reals — were q <= c / p, p q <= c and rounding, which is monotone and keeps
//               the float c, would give fl(p q) <= c — so the float below q is <= c / p, and p times it rounds to at most c.  q >=
//               2^-10 / FLT_MAX is far above the smallest subnormal, so the step down never reaches 0.)
//   attack      gl < g0 (ATTACK | ACTIVE): k = the first j with |o[j]| * g0 > c, or 480.  out[j] = o[j] * (g0 + ((float)j / (float)k) *
//               (gl - g0)) for j < k — a quotient, a difference, a product, a sum, a product, none fused — and o[j] * gl for j >= k.
//               g1 = gl, h' = H.  The gain leaves the previous row's end value continuously, is at gl exactly where it is first
//               needed, and steps only when k == 0
//   otherwise   h > 0 (HOLDING): g1 = g0, h' = h - 1.  h == 0: g1 = fminf(fminf(g0 * R, 1.0f), gl), h' = 0, RELEASING when g1 > g0.
//               ACTIVE when g0 < 1 or g1 < 1.  The row is scaled by the level control's ramp between g0 and g1 (pn_agc_rules.h
//               pn_agc_apply_host) — unless g0 == g1 == 1.0f: the row is then NOT written and keeps its bits, -0.0 and NaN payloads included
//   state       gain = g1, hold = h', limited += ACTIVE (saturating)
// Report (PN_LIM_REPORT_WORDS = 4): f32 g1 (a non-finite row: g0), f32 p, u32 flags (PN_LIM_ON | ATTACK | HOLDING | RELEASING | ACTIVE |
// NONFINITE), u32 limited.  A stream whose ceiling is 0: {1.0f, +0.0f, 0, 0}, row and state untouched.
//
// The guarantee: for a finite row, |out[j]| <= c as floats for every sample that is not NaN.  Rounding is monotone: a <= b implies
// fl(a) <= fl(b), and fl keeps a float.  (1) With p > c, fl(p * gl) <= c by the step above; with p <= c, gl = 1 and p * gl = p <= c.
// (2) Every gain g the row meets is at most gl — or, in front of index k of an attack, at most g0, which those samples bear:
//     attack, j < k: w = fl(j / k) is in [0, 1), d = fl(gl - g0) is in [-g0, 0) because gl > 0, so t = fl(w d) is in [d, 0] and g = fl(g0 + t)
//     in [0, g0]; by the choice of k, fl(|o[j]| g0) <= c, hence fl(|o[j]| g) <= fl(|o[j]| g0) <= c.  j >= k: g = gl and |o[j]| <= p,
//     hence fl(|o[j]| gl) <= fl(p gl) <= c.
//     otherwise g0 <= g1 <= gl and g1 <= 2 g0 (g0 R rounds to no less than g0 and to no more than 2 g0 because 1 <= R <= 2), so
//     d = g1 - g0 is exact (Sterbenz); w = fl((2j + 1) / 960) < 1, so t = fl(w d) is in [0, d] and g = fl(g0 + t) in [g0, g1]: at most gl;
//     hence fl(|o[j]| g) <= fl(p gl) <= c.
#pragma once
#include "pn_agc_rules.h"    // pn_agc_apply_host: the ramp of a frame that does not attack; pn_agc_peak_host; pn_ids_check, pn_set_error
#include <float.h>
#include <math.h>
#include <string.h>

#define PN_LIM_STATE_BYTES 16
#define PN_LIM_LIMITED_MAX 0xffffffffu
static_assert(PN_LIM_N_PARAMS == 2 && PN_LIM_REPORT_WORDS == 4 && PN_LIM_STATE_BYTES == 4 * 4 && PN_FRAME == 480, "two parameters, four words of state and of report");

struct PnLimParams { float v[PN_LIM_N_PARAMS]; };     // (by value into the kernel: a parameter change is ordered like a launch)

static inline void pn_lim_default_params_host(float *p) { p[PN_LIM_RELEASE] = 1.0592537f; p[PN_LIM_HOLD] = 2.0f; }
// -1 with pn_last_error naming the FIRST bad index: NaN, a value outside its range, a hold that is no whole number
static inline int pn_lim_params_check_host(const float *p) {
  if (!p) { pn_set_error("NULL argument"); return -1; }
  if (!(p[PN_LIM_RELEASE] >= 1.0f && p[PN_LIM_RELEASE] <= 2.0f)) {     // (false for NaN)
    pn_set_error("limiter parameter %g at index %d (release): a value in [1, 2]", (double)p[PN_LIM_RELEASE], PN_LIM_RELEASE);
    return -1;
  }
  if (!(p[PN_LIM_HOLD] >= 0.0f && p[PN_LIM_HOLD] <= 1000.0f && p[PN_LIM_HOLD] == floorf(p[PN_LIM_HOLD]))) {
    pn_set_error("limiter parameter %g at index %d (hold): a whole number in [0, 1000]", (double)p[PN_LIM_HOLD], PN_LIM_HOLD);
    return -1;
  }
  return 0;
}
// ceilings[0..n): 0 (not limited; -0.0f is 0) or a ceiling in [1/1024, 1].  -1 with pn_last_error naming the FIRST bad index
static inline bool pn_lim_ceiling_ok(float c) { return c == 0.0f || (c >= 1.0f / 1024.0f && c <= 1.0f); }           // (false for NaN)
static inline int pn_lim_ceilings_list_check(const float *ceilings, int n) {
  if (n < 0 || (n > 0 && !ceilings)) { pn_set_error("bad argument"); return -1; }
  for (int i = 0; i < n; i++)
    if (!pn_lim_ceiling_ok(ceilings[i])) { pn_set_error("limiter ceiling %g at index %d: 0 (not limited) or a ceiling in [1/1024, 1]", (double)ceilings[i], i); return -1; }
  return 0;
}
static inline int pn_lim_ceilings_set_check(int B, const int32_t *ids, int n, const float *ceilings) {
  if (pn_ids_check(B, ids, n, true)) return -1;
  return pn_lim_ceilings_list_check(ceilings, n);
}

#if defined(__GNUC__) && !defined(__clang__)
#define PN_LIM_STRICT __attribute__((optimize("fp-contract=off")))
#else
#define PN_LIM_STRICT
#endif
// the gain a row of peak p needs under the ceiling c (p finite): the largest the rule trusts with fl(p * gl) <= c, or 1.0f
PN_LIM_STRICT static inline float pn_lim_needed_host(float p, float c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(p > c)) return 1.0f;
  float q = c / p;
  const float pq = p * q;
  if (pq > c) { uint32_t b; memcpy(&b, &q, 4); b -= 1u; memcpy(&q, &b, 4); }      // (q is positive: one bit less is the float below)
  return q;
}
// The scalar half of a frame: from p and the state to the two gains, the new state and the report row.  The kernel's every lane
// runs the same statements (pn_rate_lim.hip lm_update).  attack: the row ramps from g0 to g1 over [0, k) and is g1 behind it;
// otherwise, write: the row takes the level control's ramp between g0 and g1; neither: the row keeps its bits
struct PnLimStep { float g0, g1, peak; uint32_t hold, limited, flags; bool attack, write, keep_state; };
PN_LIM_STRICT static inline PnLimStep pn_lim_step_host(const float *P, float c, const uint32_t state[4], float p) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  PnLimStep o;
  float g0;
  memcpy(&g0, &state[0], 4);
  if (state[0] == 0u) g0 = 1.0f;
  const uint32_t h = state[1];
  o.g0 = g0; o.g1 = g0; o.peak = p; o.hold = h; o.limited = state[2]; o.flags = PN_LIM_ON; o.attack = false; o.write = false; o.keep_state = false;
  if (!(p <= FLT_MAX)) { o.flags |= PN_LIM_NONFINITE; o.keep_state = true; return o; }
  const float gl = pn_lim_needed_host(p, c);
  bool active;
  if (gl < g0) {
    o.g1 = gl; o.hold = (uint32_t)P[PN_LIM_HOLD]; o.attack = true; o.write = true; active = true;
    o.flags |= PN_LIM_ATTACK;
  } else {
    if (h > 0u) { o.hold = h - 1u; o.flags |= PN_LIM_HOLDING; }
    else {
      const float up = g0 * P[PN_LIM_RELEASE];
      o.g1 = fminf(fminf(up, 1.0f), gl);
      if (o.g1 > g0) o.flags |= PN_LIM_RELEASING;
    }
    active = g0 < 1.0f || o.g1 < 1.0f;
    o.write = !(g0 == 1.0f && o.g1 == 1.0f);
  }
  if (active) { o.flags |= PN_LIM_ACTIVE; if (o.limited != PN_LIM_LIMITED_MAX) o.limited += 1u; }
  return o;
}
// the first j with |o[j]| * g0 > c, or 480 (a NaN sample never is one)
PN_LIM_STRICT static inline int pn_lim_first_over_host(const float *o, float g0, float c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int j = 0; j < PN_FRAME; j++) { const float a = fabsf(o[j]) * g0; if (a > c) return j; }
  return PN_FRAME;
}
// out[j] of an attacking row: the ramp from g0 to gl over [0, k), gl from k on
PN_LIM_STRICT static inline float pn_lim_attack_host(float y, float g0, float gl, int j, int k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (j >= k) return y * gl;
  const float w = (float)j / (float)k, d = gl - g0, t = w * d, g = g0 + t;
  return y * g;
}
// One frame of one stream: state4 is read and written, row_out may be row_in.  Returns the flags (0 for a stream that is not
// limited, whose row is copied bit for bit), -1 for a bad argument.  report4, optional: the report row
static inline int pn_lim_frame_host(const float *params, float ceiling, uint32_t *state4, const float *row_in, float *row_out, uint32_t *report4 = NULL) {
  if (!params || !state4 || !row_in || !row_out) { pn_set_error("NULL argument"); return -1; }
  if (pn_lim_params_check_host(params) || pn_lim_ceilings_list_check(&ceiling, 1)) return -1;
  if (ceiling == 0.0f) {
    if (row_out != row_in) memmove(row_out, row_in, PN_FRAME * sizeof(float));
    if (report4) { const float one = 1.0f; memcpy(&report4[0], &one, 4); report4[1] = report4[2] = report4[3] = 0u; }
    return 0;
  }
  const PnLimStep st = pn_lim_step_host(params, ceiling, state4, pn_agc_peak_host(row_in));
  if (st.attack) {
    const int k = pn_lim_first_over_host(row_in, st.g0, ceiling);
    for (int j = 0; j < PN_FRAME; j++) row_out[j] = pn_lim_attack_host(row_in[j], st.g0, st.g1, j, k);
  } else if (st.write) {
    for (int j = 0; j < PN_FRAME; j++) row_out[j] = pn_agc_apply_host(row_in[j], st.g0, st.g1, j);
  } else if (row_out != row_in) memmove(row_out, row_in, PN_FRAME * sizeof(float));
  if (!st.keep_state) { memcpy(&state4[0], &st.g1, 4); state4[1] = st.hold; state4[2] = st.limited; state4[3] = 0u; }
  if (report4) { memcpy(&report4[0], &st.g1, 4); memcpy(&report4[1], &st.peak, 4); report4[2] = st.flags; report4[3] = st.limited; }
  return (int)st.flags;
}
