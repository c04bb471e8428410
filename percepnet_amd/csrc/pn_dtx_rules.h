// The DTX send side of the rate converter (include/percepnet_hip.h "DTX send side"), the rule stated once — HIP-free (builds with
// -DPN_NO_HIP): the host's pn_dtx_frame / pn_dtx_sid_from_acorr / pn_dtx_level are these functions, the kernel (pn_rate_dtx.hip
// pn_rate_dtx_kernel) forms the same sums in the same order and runs the SAME scalar statements (pn_dtx_classify, pn_dtx_update,
// pn_dtx_levinson, pn_dtx_level_hd: host and device functions), tests/dtx_model.py restates them in numpy float32 and integers,
// tests/c/dtx_sanitize.cpp runs them under the sanitizers over exactly-sized buffers.  It is the inverse of pn_cng_rules.h: the SID it
// emits is one pn_cng_sid_check accepts, in that file's sign convention and quantisation.
// Every fp32 operation is singly rounded (no product is contracted into an add; the divisions are the correctly rounded ones) and
// runs in the ONE order written here.  The stage only READS the row the caller is about to send; it writes no audio.
//
// Samples x[0..ns): the stream's OUTPUT row at its own rate, ns = 80, 160, 240, 320 or 480, in the float convention.  float: as it is;
// int16: (float)s * 2^-15 (exact); G.711: pn_g711_dec of the stream's law, then as int16.
// Autocorrelation of the row alone, lags j = 0..12: r[j] = sum_{n=j}^{ns-1} x[n] * x[n-j], products rounded separately.  Lane l of 64 sums
//   its terms n = l, l + 64, l + 128, .. (those with j <= n < ns) from +0.0f in ascending order; the 64 partial sums fold by the xor
//   butterfly v[i] = v[i] + v[i ^ s], s = 32, 16, .., 1 (the order of pn_mix_level_host), r[j] = v[0].  No history from the row before:
//   the sequence is positive semi-definite by construction.
//   ZERO PADDING leaves the bits alone.  The kernel holds the row in LDS between 12 zeros in front and zeros behind and forms the
//   products x[n] * x[n-j] for n < j and n >= ns as well.  (a) A partial sum is never -0.0: it starts at +0.0, and in round-to-nearest
//   a + b is -0.0 only where both are.  (b) In a FINITE row a padded product is +-0.0, and s + (+-0.0) = s for every s that is not -0.0.
//   So for finite rows every partial sum, hence every r[j], has the bits of the sum without the padded terms.  (c) r[0] has no padded
//   term that touches a sample (0 * 0 = +0.0), so it is exact for EVERY row; a non-finite sample, or a square that overflows, makes
//   r[0] non-finite (squares cannot cancel), the frame is then NONFINITE, and such a frame reads no other lag.
//   Lags 1..12 are read only on frames that are not active; the kernel skips them on the others.
// Energy: e = r[0] / (float)ns.  Non-finite e: the frame is ACTIVE and NONFINITE and changes NOTHING but the hangover and the mode —
//   not the floor, not the count of analysed frames.
// Floor, per-stream state N: the first analysed frame after a clear sets N = e and IS ACTIVE (there is no floor to hold it against:
//   a stream starts by sending).  Otherwise Nc = N > FLOOR_MIN ? N : FLOOR_MIN, active = e > THR * Nc, then: e < N: N = e; else not
//   active: d = e - N, t = FLOOR_UP * d, N = N + t; else N = Nc * FLOOR_DRIFT.  The count of analysed frames goes up (it stays at 2^32 - 1).
//   Two decisions of this file about digital silence, because N = 0 is a trap: 0 * FLOOR_DRIFT is 0, and every frame above
//   THR * FLOOR_MIN is then active for ever.  (1) The drift multiplies the CLAMPED floor Nc, which is N wherever N >= FLOOR_MIN: a floor
//   that fell under FLOOR_MIN (a row of zeros in a call) climbs back, at the drift's pace — four decades at 1.0023 a frame are 40 s,
//   during which the stream SENDS.  (2) Rows with e == 0 IN FRONT of a stream's first other row are not analysed — ACTIVE, sent,
//   nothing but the hangover and the mode changes: a converter's first output rows are the zeros of its delay, not the call's floor.
// Hangover: active: hang = HANGOVER.  send = active || hang > 0.  Not active and hang > 0: hang -= 1, the frame is a HANGOVER frame.
//   Exactly HANGOVER frames are sent behind the last active one.
// Noise statistics, on every frame that is not active, hangover frames included: q = r[j] / (float)ns, and for j = 0..12 the first such
//   frame after a clear sets R[j] = q, every later one d = q - R[j], t = SMOOTH * d, R[j] = R[j] + t.
// Decision, behind those updates: send: FRAME, the mode becomes VOICE.  Else L = level(R[0]) and: mode VOICE: SID, the mode becomes
//   SILENT, since = 0.  Mode SILENT: |L - L_sent| >= UPDATE_DB, or MAX_INTERVAL > 0 and since + 1 >= MAX_INTERVAL: SID, since = 0;
//   otherwise NONE and since += 1 (it stays at 65535).  L_sent is byte 1 of the last emitted SID.
// Level: L = the number of i in 0..126 with R[0] < EDGE[i], EDGE[i] the fp32 nearest 10^(-(i + 0.5) / 10): 127 literals below, strictly
//   falling, so the count is found by bisection.  No logarithm anywhere.  R[0] = 0 gives 127; a NaN gives 0.
// SID, only on a frame that emits one: Levinson-Durbin in fp32 on R[0..ORDER] in the sign convention of pn_cng_sample's lattice.
//   M = 0 unless R[0] > 0 and finite.  E = R[0].  For i = 1..ORDER:
//     acc = R[i]; for j = 1..i-1 ascending: p = a[j] * R[i-j], acc = acc + p;   k = (-acc) / E
//     stop with M = i - 1 unless |k| < 1 (false for NaN)
//     u = k * PN_DTX_KQ + 127.5f (product, then add; PN_DTX_KQ = the fp32 nearest 32768 / 258), N_i = (int)u clamped to [0, 254]
//     kq = (float)(258 * (N_i - 127)) * 2^-15, exact;   t = kq * kq, o = 1 - t, E' = E * o;   stop with M = i - 1 unless E' > 0
//     from a copy c of a: for j = 1..i-1: p = kq * c[i-j], a[j] = c[j] + p;   a[i] = kq;   E = E';   M = i
//   The emitted SID is (M, L, N_1..N_M, zeros).  M <= 12, L <= 127, N_i <= 254: pn_cng_sid_check accepts it.
// Stream switched off: decision FRAME, eight zero report words, no state touched.  Stream not on the id list: state and report row stay.
//
// Parameters, one set per converter (PN_DTX_N_PARAMS = 9 floats; pn_dtx_params_check refuses NaN and anything outside a range).  The
// defaults are the author's and are NOT tuned on speech:
//   0 PN_DTX_THR           active when e > THR * floor                       finite, > 1                  4.0
//   1 PN_DTX_FLOOR_UP      the floor's step towards a louder quiet frame     (0, 1]                       0.1
//   2 PN_DTX_FLOOR_DRIFT   the floor's growth per active frame               [1, 2)                       1.0023
//   3 PN_DTX_FLOOR_MIN     the least floor the threshold is held against     finite, > 0                  1e-10
//   4 PN_DTX_HANGOVER      frames sent behind the last active one            a whole number in [0, 255]   20
//   5 PN_DTX_SMOOTH        the noise statistics' step                        (0, 1]                       0.1
//   6 PN_DTX_UPDATE_DB     level change that sends a new SID                 a whole number in [1, 127]   2
//   7 PN_DTX_MAX_INTERVAL  frames between two SIDs at the most, 0: never     a whole number in [0, 65535] 0
//   8 PN_DTX_ORDER         reflection coefficients at the most               a whole number in [0, 12]    10
// State of one stream, PN_DTX_STATE_WORDS = 24 words, all zero is fresh: 0..12 R[13] (float), 13 N (float), 14 hang, 15 the mode
// (PN_DTX_MODE_SILENT | PN_DTX_MODE_NOISE: R holds statistics), 16 since, 17 the analysed frames, 18..21 the last emitted SID — its 14
// bytes, little-endian, then the 16-bit count of SIDs emitted since the clear (it WRAPS: a caller compares it for equality) —, 22 and 23
// always 0.
// Report, PN_DTX_REPORT_WORDS = 8 words: 0 the decision (PN_DTX_FRAME 0, PN_DTX_SID 1, PN_DTX_NONE 2); 1 flags (PN_DTX_ON | PN_DTX_ACTIVE |
// PN_DTX_HANGOVER_FRAME | PN_DTX_NONFINITE) | L << 8 | hang << 16, L being the level of this frame's R[0] where the decision is SID or NONE and 0 on a FRAME;
// 2 the bits of e; 3 the bits of N; 4..7 state words 18..21.
#pragma once
#include "pn_cng_rules.h"    // the SID's format and check, pn_cng_row_ok; through it pn_host_rules.h: pn_set_error, pn_ids_check, the header's PN_DTX_* constants
#include <float.h>
#include <math.h>
#include <string.h>

#define PN_DTX_STATE_WORDS 24
#define PN_DTX_LAGS 13
#define PN_DTX_W_N 13
#define PN_DTX_W_HANG 14
#define PN_DTX_W_MODE 15
#define PN_DTX_W_SINCE 16
#define PN_DTX_W_FRAMES 17
#define PN_DTX_W_SID 18
#define PN_DTX_MODE_SILENT 1u
#define PN_DTX_MODE_NOISE 2u
#define PN_DTX_WS_WORDS 32                     // Levinson's workspace: a[0..13) and its copy at 16
#define PN_DTX_KQ 127.007751f                  // 0x42fe03f8, 32768 / 258
#define PN_DTX_SINCE_MAX 0xffffu
#define PN_DTX_SAT 0xffffffffu
static_assert(PN_DTX_N_PARAMS == 9 && PN_DTX_REPORT_WORDS == 8 && PN_DTX_LAGS == PN_CNG_MAX_ORDER + 1 && PN_DTX_W_SID + 4 + 2 == PN_DTX_STATE_WORDS &&
              PN_CNG_SID_BYTES + 2 == 16 && PN_DTX_FRAME == 0, "nine parameters, 24 words of state, eight of report; a SID and its count are four words");

#if defined(__HIPCC__) && !defined(PN_NO_HIP)
#define PN_DTX_HD __host__ __device__ __forceinline__
#else
#define PN_DTX_HD static inline
#endif
#if defined(__GNUC__) && !defined(__clang__)
#define PN_DTX_STRICT __attribute__((optimize("fp-contract=off")))
#else
#define PN_DTX_STRICT
#endif

struct PnDtxParams { float v[PN_DTX_N_PARAMS]; };   // (by value into the kernel: a parameter change is ordered like a launch)

// 10^(-(i + 0.5) / 10), i = 0 .. 126
#define PN_DTX_EDGES { \
    0.891250908f, 0.707945764f, 0.562341332f, 0.446683586f, 0.354813397f, 0.281838298f, 0.22387211f, 0.177827939f, \
    0.141253754f, 0.112201847f, 0.0891250968f, 0.0707945749f, 0.0562341325f, 0.0446683578f, 0.0354813375f, 0.028183829f, \
    0.0223872121f, 0.0177827943f, 0.0141253751f, 0.0112201842f, 0.00891250931f, 0.00707945786f, 0.00562341325f, 0.00446683588f, \
    0.00354813389f, 0.00281838304f, 0.00223872112f, 0.00177827943f, 0.00141253753f, 0.00112201844f, 0.000891250966f, 0.000707945786f, \
    0.000562341302f, 0.000446683582f, 0.000354813383f, 0.000281838293f, 0.000223872121f, 0.00017782794f, 0.000141253753f, 0.000112201844f, \
    8.91250966e-05f, 7.07945801e-05f, 5.62341338e-05f, 4.46683589e-05f, 3.54813383e-05f, 2.81838293e-05f, 2.23872121e-05f, 1.77827933e-05f, \
    1.41253759e-05f, 1.12201842e-05f, 8.91250966e-06f, 7.07945765e-06f, 5.62341347e-06f, 4.46683589e-06f, 3.54813392e-06f, 2.81838288e-06f, \
    2.23872121e-06f, 1.7782794e-06f, 1.41253759e-06f, 1.12201849e-06f, 8.9125092e-07f, 7.07945787e-07f, 5.62341313e-07f, 4.466836e-07f, \
    3.5481338e-07f, 2.81838282e-07f, 2.23872121e-07f, 1.77827943e-07f, 1.4125375e-07f, 1.12201846e-07f, 8.91250949e-08f, 7.07945773e-08f, \
    5.6234132e-08f, 4.46683579e-08f, 3.54813388e-08f, 2.81838286e-08f, 2.23872121e-08f, 1.77827939e-08f, 1.41253755e-08f, 1.12201848e-08f, \
    8.91250895e-09f, 7.07945791e-09f, 5.62341329e-09f, 4.46683579e-09f, 3.54813379e-09f, 2.81838286e-09f, 2.23872121e-09f, 1.77827941e-09f, \
    1.41253753e-09f, 1.12201848e-09f, 8.91250962e-10f, 7.07945758e-10f, 5.6234134e-10f, 4.46683579e-10f, 3.54813401e-10f, 2.81838303e-10f, \
    2.23872115e-10f, 1.77827947e-10f, 1.41253759e-10f, 1.12201845e-10f, 8.91250962e-11f, 7.07945785e-11f, 5.62341319e-11f, 4.46683593e-11f, \
    3.54813401e-11f, 2.81838285e-11f, 2.23872119e-11f, 1.77827943e-11f, 1.41253753e-11f, 1.12201845e-11f, 8.91250962e-12f, 7.07945768e-12f, \
    5.62341319e-12f, 4.46683576e-12f, 3.54813379e-12f, 2.8183829e-12f, 2.23872114e-12f, 1.77827946e-12f, 1.41253751e-12f, 1.12201849e-12f, \
    8.9125094e-13f, 7.07945801e-13f, 5.62341352e-13f, 4.46683597e-13f, 3.54813401e-13f, 2.81838301e-13f, 2.23872109e-13f}

static inline void pn_dtx_default_params_host(float *p) {
  p[PN_DTX_THR] = 4.0f; p[PN_DTX_FLOOR_UP] = 0.1f; p[PN_DTX_FLOOR_DRIFT] = 1.0023f; p[PN_DTX_FLOOR_MIN] = 1e-10f; p[PN_DTX_HANGOVER] = 20.0f;
  p[PN_DTX_SMOOTH] = 0.1f; p[PN_DTX_UPDATE_DB] = 2.0f; p[PN_DTX_MAX_INTERVAL] = 0.0f; p[PN_DTX_ORDER] = 10.0f;
}
// -1 with pn_last_error naming the FIRST bad index: NaN, a value outside its range, or a count that is no whole number
static inline int pn_dtx_params_check_host(const float *p) {
  if (!p) { pn_set_error("NULL argument"); return -1; }
  static const struct { const char *name, *range; float lo, hi; bool open_lo, open_hi, whole; } k[PN_DTX_N_PARAMS] = {
      {"thr", "finite and > 1", 1.0f, FLT_MAX, true, false, false},                   {"floor_up", "in (0, 1]", 0.0f, 1.0f, true, false, false},
      {"floor_drift", "in [1, 2)", 1.0f, 2.0f, false, true, false},                   {"floor_min", "finite and > 0", 0.0f, FLT_MAX, true, false, false},
      {"hangover", "a whole number in [0, 255]", 0.0f, 255.0f, false, false, true},   {"smooth", "in (0, 1]", 0.0f, 1.0f, true, false, false},
      {"update_db", "a whole number in [1, 127]", 1.0f, 127.0f, false, false, true},  {"max_interval", "a whole number in [0, 65535]", 0.0f, 65535.0f, false, false, true},
      {"order", "a whole number in [0, 12]", 0.0f, 12.0f, false, false, true}};
  for (int i = 0; i < PN_DTX_N_PARAMS; i++)
    if (!((k[i].open_lo ? p[i] > k[i].lo : p[i] >= k[i].lo) && (k[i].open_hi ? p[i] < k[i].hi : p[i] <= k[i].hi) && (!k[i].whole || p[i] == floorf(p[i])))) {   // (false for NaN)
      pn_set_error("DTX parameter %g at index %d (%s): a value %s", (double)p[i], i, k[i].name, k[i].range);
      return -1;
    }
  return 0;
}
static inline int pn_dtx_on_set_check(int B, const int32_t *ids, int n, const uint8_t *on) {
  if (n > 0 && !on) { pn_set_error("bad argument"); return -1; }
  return pn_ids_check(B, ids, n, true);
}

PN_DTX_HD uint32_t pn_dtx_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
PN_DTX_HD float pn_dtx_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
PN_DTX_HD bool pn_dtx_finite(float f) { return (pn_dtx_bits(f) & 0x7f800000u) != 0x7f800000u; }

// L of a mean square: how many edges lie above it
PN_DTX_HD int pn_dtx_level_hd(float ms) {
  constexpr float edge[127] = PN_DTX_EDGES;
  int lo = 0, hi = 127;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ms < edge[mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// a frame's class from its energy: PN_DTX_ACTIVE, PN_DTX_NONFINITE or neither.  N, frames: the floor and the count as the frame finds them
PN_DTX_STRICT PN_DTX_HD uint32_t pn_dtx_classify(const float *p, float N, uint32_t frames, float e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!pn_dtx_finite(e)) return PN_DTX_ACTIVE | PN_DTX_NONFINITE;
  if (frames == 0u) return PN_DTX_ACTIVE;
  const float Nc = N > p[PN_DTX_FLOOR_MIN] ? N : p[PN_DTX_FLOOR_MIN], thr = p[PN_DTX_THR] * Nc;
  return e > thr ? PN_DTX_ACTIVE : 0u;
}

// Levinson-Durbin on the words R[0..order] (float bits), quantising as it goes: N_i into bytes 2.. of the four SID words (which the caller
// has zeroed), the order M returned.  ws: PN_DTX_WS_WORDS floats of workspace
PN_DTX_STRICT PN_DTX_HD int pn_dtx_levinson(const uint32_t *R, int order, float *ws, uint32_t *sidw) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float R0 = pn_dtx_float(R[0]);
  if (!(R0 > 0.0f) || !pn_dtx_finite(R0)) return 0;
  float *a = ws, *c = ws + 16, E = R0;
  int M = 0;
  for (int i = 1; i <= order; i++) {
    float acc = pn_dtx_float(R[i]);
    for (int j = 1; j < i; j++) { const float pr = a[j] * pn_dtx_float(R[i - j]); acc = acc + pr; }
    const float k = (-acc) / E;
    if (!(fabsf(k) < 1.0f)) break;
    const float u0 = k * PN_DTX_KQ, u = u0 + 127.5f;
    int Ni = (int)u;
    Ni = Ni < 0 ? 0 : Ni > 254 ? 254 : Ni;
    const float kq = (float)(258 * (Ni - 127)) * (1.0f / 32768.0f), t = kq * kq, o = 1.0f - t, En = E * o;
    if (!(En > 0.0f)) break;
    for (int j = 1; j < i; j++) c[j] = a[j];
    for (int j = 1; j < i; j++) { const float pr = kq * c[i - j]; a[j] = c[j] + pr; }
    a[i] = kq; E = En; M = i;
    sidw[(i + 1) >> 2] |= (uint32_t)Ni << (8 * ((i + 1) & 3));
  }
  return M;
}

// One frame of one enabled stream behind its sums: st[24] in place, r[13] (float bits; lags 1..12 are read only where the frame is not
// active), rep[8] written (NULL: no report).  Returns the decision.
PN_DTX_STRICT PN_DTX_HD int pn_dtx_update(const float *p, uint32_t *st, const uint32_t *r, int ns, float *ws, uint32_t *rep) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float fns = (float)ns, e = pn_dtx_float(r[0]) / fns;
  float N = pn_dtx_float(st[PN_DTX_W_N]);
  uint32_t frames = st[PN_DTX_W_FRAMES], hang = st[PN_DTX_W_HANG], mode = st[PN_DTX_W_MODE], since = st[PN_DTX_W_SINCE];
  const uint32_t cls = pn_dtx_classify(p, N, frames, e);
  const bool active = (cls & PN_DTX_ACTIVE) != 0u;
  if (!(cls & PN_DTX_NONFINITE) && !(frames == 0u && e == 0.0f)) {
    const float Nc = N > p[PN_DTX_FLOOR_MIN] ? N : p[PN_DTX_FLOOR_MIN];
    if (frames == 0u || e < N) N = e;
    else if (!active) { const float d = e - N, t = p[PN_DTX_FLOOR_UP] * d; N = N + t; }
    else N = Nc * p[PN_DTX_FLOOR_DRIFT];
    frames = frames == PN_DTX_SAT ? frames : frames + 1u;
  }
  uint32_t flags = PN_DTX_ON | cls;
  if (active) hang = (uint32_t)p[PN_DTX_HANGOVER];
  const bool send = active || hang > 0u;
  if (!active && hang > 0u) { hang -= 1u; flags |= PN_DTX_HANGOVER_FRAME; }
  if (!active) {
    for (int j = 0; j < PN_DTX_LAGS; j++) {
      const float q = pn_dtx_float(r[j]) / fns;
      if (!(mode & PN_DTX_MODE_NOISE)) st[j] = pn_dtx_bits(q);
      else { const float R = pn_dtx_float(st[j]), d = q - R, t = p[PN_DTX_SMOOTH] * d; st[j] = pn_dtx_bits(R + t); }
    }
    mode |= PN_DTX_MODE_NOISE;
  }
  int decision = PN_DTX_FRAME;
  uint32_t L = 0u;
  if (send) mode &= ~PN_DTX_MODE_SILENT;
  else {
    L = (uint32_t)pn_dtx_level_hd(pn_dtx_float(st[0]));
    const uint32_t Ls = (st[PN_DTX_W_SID] >> 8) & 0xffu, dL = L > Ls ? L - Ls : Ls - L, mi = (uint32_t)p[PN_DTX_MAX_INTERVAL];
    bool emit = true;
    if (mode & PN_DTX_MODE_SILENT) emit = dL >= (uint32_t)p[PN_DTX_UPDATE_DB] || (mi > 0u && since + 1u >= mi);
    mode |= PN_DTX_MODE_SILENT;
    if (emit) {
      const uint32_t count = ((st[PN_DTX_W_SID + 3] >> 16) + 1u) & 0xffffu;
      st[PN_DTX_W_SID] = 0u; st[PN_DTX_W_SID + 1] = 0u; st[PN_DTX_W_SID + 2] = 0u; st[PN_DTX_W_SID + 3] = 0u;
      const uint32_t M = (uint32_t)pn_dtx_levinson(st, (int)p[PN_DTX_ORDER], ws, &st[PN_DTX_W_SID]);
      st[PN_DTX_W_SID] |= M | L << 8;
      st[PN_DTX_W_SID + 3] |= count << 16;
      since = 0u; decision = PN_DTX_SID;
    } else {
      since = since >= PN_DTX_SINCE_MAX ? PN_DTX_SINCE_MAX : since + 1u;
      decision = PN_DTX_NONE;
    }
  }
  st[PN_DTX_W_N] = pn_dtx_bits(N); st[PN_DTX_W_FRAMES] = frames; st[PN_DTX_W_HANG] = hang; st[PN_DTX_W_MODE] = mode; st[PN_DTX_W_SINCE] = since;
  if (rep) {
    rep[0] = (uint32_t)decision; rep[1] = flags | L << 8 | hang << 16; rep[2] = pn_dtx_bits(e); rep[3] = pn_dtx_bits(N);
    rep[4] = st[PN_DTX_W_SID]; rep[5] = st[PN_DTX_W_SID + 1]; rep[6] = st[PN_DTX_W_SID + 2]; rep[7] = st[PN_DTX_W_SID + 3];
  }
  return decision;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// r[0..lags) of a row of ns samples, lane by lane and fold by fold as written above
PN_DTX_STRICT static inline void pn_dtx_acorr_host(const float *x, int ns, int lags, uint32_t *r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float v[64], t[64];
  for (int j = 0; j < lags; j++) {
    for (int l = 0; l < 64; l++) {
      float acc = 0.0f;
      for (int n = l; n < ns; n += 64)
        if (n >= j) { const float pr = x[n] * x[n - j]; acc = acc + pr; }
      v[l] = acc;
    }
    for (int s = 32; s >= 1; s >>= 1) {
      for (int i = 0; i < 64; i++) t[i] = v[i] + v[i ^ s];
      memcpy(v, t, sizeof t);
    }
    r[j] = pn_dtx_bits(v[0]);
  }
}
// the 14 bytes of state words 18..21
static inline void pn_dtx_sid_bytes(const uint32_t *sidw, uint8_t *sid) {
  for (int b = 0; b < PN_CNG_SID_BYTES; b++) sid[b] = (uint8_t)(sidw[b >> 2] >> (8 * (b & 3)));
}
// one float row of one enabled stream: the kernel's twin.  Returns the decision, -1 for a refused argument
static inline int pn_dtx_frame_host(const float *params, uint32_t *st, const float *row, int ns, uint32_t *report) {
  if (!params || !st || !row) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtx_params_check_host(params)) return -1;
  if (!pn_cng_row_ok(ns)) { pn_set_error("a DTX row of %d samples: 80, 160, 240, 320 or 480 (10 ms at a converter's rates)", ns); return -1; }
  uint32_t r[PN_DTX_LAGS];
  float ws[PN_DTX_WS_WORDS] = {};
  pn_dtx_acorr_host(row, ns, PN_DTX_LAGS, r);
  return pn_dtx_update(params, st, r, ns, ws, report);
}
// the Levinson step alone: R[0..12], order 0..12 -> the SID (M, level(R[0]), N_1..N_M, zeros).  Returns M, -1 for a refused argument
static inline int pn_dtx_sid_from_acorr_host(const float *R, int order, uint8_t *sid) {
  if (!R || !sid) { pn_set_error("NULL argument"); return -1; }
  if (order < 0 || order > PN_CNG_MAX_ORDER) { pn_set_error("DTX order %d: a whole number in [0, %d]", order, PN_CNG_MAX_ORDER); return -1; }
  uint32_t Rw[PN_DTX_LAGS], sidw[4] = {0u, 0u, 0u, 0u};
  float ws[PN_DTX_WS_WORDS] = {};
  memcpy(Rw, R, sizeof Rw);
  const int M = pn_dtx_levinson(Rw, order, ws, sidw);
  sidw[0] |= (uint32_t)M | (uint32_t)pn_dtx_level_hd(R[0]) << 8;
  pn_dtx_sid_bytes(sidw, sid);
  return M;
}
