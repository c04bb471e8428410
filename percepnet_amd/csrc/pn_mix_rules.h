// Loudest-N selection, send gains and the hold of the conference mix (include/percepnet_hip.h "conferences: loudest-N talkers, send
// gains, mix report"), the rules that need no GPU, each stated once for the host — HIP-free (builds with -DPN_NO_HIP), checked on
// the CPU by tests/c/mix_sel_sanitize.cpp under the sanitizers and by tests/test_mix_sel_host.py through the C-ABI: what a gain, a
// cap and a hold factor must be, a talker's level in the ONE order the kernel (pn_rate_mix.hip pn_rate_mix_sel_kernel) sums it in,
// the hold, and who is selected.  The numpy restatement is tests/mix_sel_model.py.
#pragma once
#include "pn_conf.h"
#include <float.h>
#include <math.h>

// gains[0..n): every one finite and >= 0 (-0.0f is 0).  -1 with pn_last_error naming the FIRST bad index; n == 0 is a legal list.
static inline bool pn_mix_gain_ok(float g) { return g >= 0.0f && g <= FLT_MAX; }      // (false for NaN, inf and negatives)
static inline int pn_mix_gains_list_check(const float *gains, int n) {
  if (n < 0 || (n > 0 && !gains)) { pn_set_error("bad argument"); return -1; }
  for (int i = 0; i < n; i++)
    if (!pn_mix_gain_ok(gains[i])) { pn_set_error("mix gain %g at index %d: a finite value >= 0", (double)gains[i], i); return -1; }
  return 0;
}
static inline int pn_mix_gains_set_check(int B, const int32_t *ids, int n, const float *gains) {
  if (pn_ids_check(B, ids, n, true)) return -1;
  return pn_mix_gains_list_check(gains, n);
}
// confs[0..n): distinct conference NUMBERS in [0, B) (the id rule, with its words); max_speakers[i] in [0, PN_CONF_MAX_MEMBERS]
static inline int pn_mix_speakers_set_check(int B, const int32_t *confs, int n, const int32_t *max_speakers) {
  if (n > 0 && !max_speakers) { pn_set_error("bad argument"); return -1; }
  if (pn_ids_check(B, confs, n, true)) return -1;
  for (int i = 0; i < n; i++)
    if (max_speakers[i] < 0 || max_speakers[i] > PN_CONF_MAX_MEMBERS) {
      pn_set_error("%d speakers at index %d: 0 (everybody) or a number up to %d", (int)max_speakers[i], i, PN_CONF_MAX_MEMBERS);
      return -1;
    }
  return 0;
}
static inline int pn_mix_hold_check(float d) {
  if (!(d >= 0.0f && d < 1.0f)) { pn_set_error("mix hold factor %g: a value in [0, 1)", (double)d); return -1; }
  return 0;
}

// E of a row of 480 contributions x (ALREADY scaled by the send gain): the products x*x rounded separately; group q = j / 4 sums its
// four from +0.0f in index order; the 120 group sums, padded with +0.0f to 128, are two halves of 64 that each fold by the xor
// butterfly v[i] = v[i] + v[i ^ stride], stride 32, 16, .., 1; E = half0[0] + half1[0].  No product is contracted into an add.
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
static inline float pn_mix_level_host(const float *x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float v[128], t[64];
  for (int q = 0; q < 128; q++) {
    float e = 0.0f;
    if (q < PN_FRAME / 4)
      for (int i = 0; i < 4; i++) { const float p = x[4 * q + i] * x[4 * q + i]; e = e + p; }
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
static inline uint32_t pn_mix_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
// the peak hold with exponential release: d the hold factor, prev the level of the frame before.  d == 0: E; a non-finite level never sticks
static inline float pn_mix_hold_level(float d, float prev, float E) {
  const float h = d * prev;
  const bool finite = (pn_mix_bits(h) & 0x7f800000u) != 0x7f800000u;
  return (d != 0.0f && finite && h > E) ? h : E;
}
// the rank of a level: its bits without the sign, so NaN ranks above +inf
static inline uint32_t pn_mix_key(float L) { return pn_mix_bits(L) & 0x7fffffffu; }
// levels[0..k): the talkers of one conference in ascending slot order; selected[i] = 1 iff n_max == 0 or fewer than n_max talkers
// q have key(L_q) > key(L_i) or (key(L_q) == key(L_i) and q < i).  Returns how many are selected, -1 for a bad argument.
static inline int pn_mix_select_host(const float *levels, int k, int n_max, uint8_t *selected) {
  if (k < 0 || k > PN_CONF_MAX_MEMBERS || n_max < 0 || n_max > PN_CONF_MAX_MEMBERS || (k > 0 && (!levels || !selected))) { pn_set_error("bad argument"); return -1; }
  int n = 0;
  for (int i = 0; i < k; i++) {
    int ahead = 0;
    for (int q = 0; q < k; q++) {
      const uint32_t a = pn_mix_key(levels[q]), b = pn_mix_key(levels[i]);
      ahead += a > b || (a == b && q < i);
    }
    selected[i] = (n_max == 0 || ahead < n_max) ? 1 : 0;
    n += selected[i];
  }
  return n;
}
