// Comfort noise on the rate converter (include/percepnet_hip.h "comfort noise"), the rule stated once — HIP-free (builds with
// -DPN_NO_HIP): the host's pn_cng_sid_decode / pn_cng_frame are these functions, the kernel (pn_rate_cng.hip pn_rate_cng_kernel) runs the
// SAME sample functions below (they are host and device functions), tests/cng_model.py restates them in numpy integers and float32,
// tests/c/cng_sanitize.cpp runs them under the sanitizers over exactly-sized buffers.
// Every fp32 operation is singly rounded (no product is contracted into an add; the one division is the correctly rounded one) and
// runs in the ONE order written here.  Samples are in the float convention (int16 / 32768), at the STREAM'S OWN rate.
//
// The silence descriptor (SID) of a stream, PN_CNG_SID_BYTES = 14 bytes, fixed: byte 0 = M, the order, 0..12; byte 1 = L, the noise
// level in -dBov, 0..127; bytes 2..13 = N_1..N_12, the quantised reflection coefficients, 0..254 each, of which the first M count.  The
// bytes behind N_M are not looked at and read back as 0.  That is the RFC 3389 payload (L, N_1..N_M) behind a count byte.  Refused: M > 12,
// L > 127, an N_i of 255 among the first M.  The default of a stream nobody gave a SID: level only, M = 0, L = PN_CNG_DEFAULT_LEVEL = 60.
//
// Decode (host, once per setting, in double, then rounded to fp32):
//   k_i = 258 (N_i - 127) / 32768     exact in fp32: |k_i| <= 32766 / 32768.  THIS formula is the contract; it is RFC 3389 section 3.2 as
//                                     remembered, no copy of the RFC was at hand when it was written
//   rms = pn_kCngLevel[L]             128 fp32 literals, 10^(-L / 20) to the nearest fp32
//   g   = (float)((double)rms * sqrt(prod_i (1 - k_i k_i)))   the product from 1.0 in ascending i, every factor in double.  An all-pole
//                                     lattice driven by white noise of variance s^2 gives s^2 / prod (1 - k_i^2): shaped noise of any
//                                     spectrum has the level the SID names
// Excitation, counter-based — sample c of stream slot s under the converter's seed (pn_rate_set_cng_seed, default PN_CNG_DEFAULT_SEED):
//   key = seed ^ (s * 0x9e3779b1)                                  mod 2^32
//   mix(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16          (32-bit, the murmur3 finaliser)
//   h = mix(mix(c) ^ key)
//   u = (h & 0xffff) + (h >> 16) - 65535                           an int in [-65535, 65535], triangular, exact
//   e = (float)u * PN_CNG_C                                        one product; PN_CNG_C = the fp32 nearest 1 / sqrt((2^32 - 1) / 6), so e has unit variance
// Synthesis, an all-pole lattice of order M over b[0..12) (sign convention: f_{i-1} = f_i - k_i b_{i-1}, b_i' = b_{i-1} + k_i f_{i-1}):
//   f = gain(n) * e
//   for i = M down to 1:   p = k_i * b[i-1];  f = f - p;  and where i < M:  q = k_i * f;  b[i] = b[i-1] + q      (b_M is never read: not kept)
//   b[0] = f;  the sample is f
// Gain: a row is CONTINUING when the stream's previous generated row was in the converter's previous frame, otherwise it is the first of a run.
//   first of a run:  gain(n) = g
//   continuing:      w = (float)(n + 1) / (float)n_s,  d = g - prev,  t = w * d,  gain(n) = prev + t     prev: the g of the row before.
//                    An unchanged SID gives d = +0.0 and gain(n) = prev = g exactly; a changed one ramps across the row.  The state then holds g itself
//   (one statement serves both: prev := g on the first row of a run)
//
// State of one stream, PN_CNG_STATE_WORDS = 16 words: b[12] (float), the sample counter (it advances by n_s per generated row and wraps),
// prev (float bits), run = consecutive generated rows, total = generated rows since the state was cleared (both stay at 0xffffffff).
// Whether a row continues is NOT state: the host knows in which frame it last generated a stream's row.  A received, concealed or skipped
// frame ends the run and leaves b and the counter as they are: the noise of the next pause continues the sequence, its gain starts at g.
// Every finite SID gives finite rows; the stage has no audio input, so no NaN can enter.  No bound on |f| is derived here: with all twelve
// k_i at +-32766 / 32768 the filter's gain is 10^23 beside a g of 10^-23, and what holds there is measured on the model.
#pragma once
#include "pn_host_rules.h"   // pn_set_error, pn_ids_check, the header's PN_CNG_* constants
#include <math.h>
#include <string.h>

#define PN_CNG_STATE_WORDS 16
#define PN_CNG_W_CTR 12
#define PN_CNG_W_PREV 13
#define PN_CNG_W_RUN 14
#define PN_CNG_W_TOTAL 15
#define PN_CNG_PARAM_WORDS 16                  // a decoded SID on the device: k[12], g, M, 0, 0
#define PN_CNG_P_G 12
#define PN_CNG_P_M 13
#define PN_CNG_TILE 80                         // samples the kernel stages per stream at a time: the row of 8000 Hz, and it divides every row
#define PN_CNG_C 3.7376248656073585e-05f       // 0x381cc471
#define PN_CNG_SAT 0xffffffffu
static_assert(PN_CNG_MAX_ORDER == 12 && PN_CNG_SID_BYTES == 2 + PN_CNG_MAX_ORDER && PN_CNG_REPORT_WORDS == 4 && PN_CNG_MAX_ORDER + 4 == PN_CNG_STATE_WORDS &&
              PN_FRAME % PN_CNG_TILE == 0 && 80 % PN_CNG_TILE == 0, "twelve coefficients; a tile divides the rows of all five rates (80, 160, 240, 320, 480)");

#if defined(__HIPCC__) && !defined(PN_NO_HIP)
#define PN_CNG_HD __host__ __device__ __forceinline__
#else
#define PN_CNG_HD static inline
#endif
#if defined(__GNUC__) && !defined(__clang__)
#define PN_CNG_STRICT __attribute__((optimize("fp-contract=off")))
#else
#define PN_CNG_STRICT
#endif

// 10^(-L / 20), L = 0 .. 127
static const float pn_kCngLevel[128] = {
    1.0f, 0.891250908f, 0.794328213f, 0.707945764f, 0.630957365f, 0.562341332f, 0.501187205f, 0.446683586f,
    0.398107171f, 0.354813397f, 0.316227764f, 0.281838298f, 0.251188636f, 0.22387211f, 0.199526235f, 0.177827939f,
    0.158489317f, 0.141253754f, 0.125892535f, 0.112201847f, 0.100000001f, 0.0891250968f, 0.0794328228f, 0.0707945749f,
    0.0630957335f, 0.0562341325f, 0.050118722f, 0.0446683578f, 0.0398107171f, 0.0354813375f, 0.0316227749f, 0.028183829f,
    0.0251188651f, 0.0223872121f, 0.0199526232f, 0.0177827943f, 0.0158489328f, 0.0141253751f, 0.0125892544f, 0.0112201842f,
    0.00999999978f, 0.00891250931f, 0.0079432819f, 0.00707945786f, 0.00630957354f, 0.00562341325f, 0.00501187239f, 0.00446683588f,
    0.00398107152f, 0.00354813389f, 0.00316227763f, 0.00281838304f, 0.00251188641f, 0.00223872112f, 0.00199526222f, 0.00177827943f,
    0.00158489321f, 0.00141253753f, 0.00125892542f, 0.00112201844f, 0.00100000005f, 0.000891250966f, 0.000794328225f, 0.000707945786f,
    0.000630957366f, 0.000562341302f, 0.000501187227f, 0.000446683582f, 0.000398107164f, 0.000354813383f, 0.000316227757f, 0.000281838293f,
    0.000251188641f, 0.000223872121f, 0.000199526228f, 0.00017782794f, 0.000158489318f, 0.000141253753f, 0.000125892548f, 0.000112201844f,
    9.99999975e-05f, 8.91250966e-05f, 7.94328225e-05f, 7.07945801e-05f, 6.30957366e-05f, 5.62341338e-05f, 5.01187242e-05f, 4.46683589e-05f,
    3.98107186e-05f, 3.54813383e-05f, 3.16227779e-05f, 2.81838293e-05f, 2.51188649e-05f, 2.23872121e-05f, 1.99526239e-05f, 1.77827933e-05f,
    1.58489311e-05f, 1.41253759e-05f, 1.25892539e-05f, 1.12201842e-05f, 9.99999975e-06f, 8.91250966e-06f, 7.94328207e-06f, 7.07945765e-06f,
    6.30957356e-06f, 5.62341347e-06f, 5.01187242e-06f, 4.46683589e-06f, 3.98107159e-06f, 3.54813392e-06f, 3.16227761e-06f, 2.81838288e-06f,
    2.51188635e-06f, 2.23872121e-06f, 1.99526221e-06f, 1.7782794e-06f, 1.5848932e-06f, 1.41253759e-06f, 1.25892541e-06f, 1.12201849e-06f,
    9.99999997e-07f, 8.9125092e-07f, 7.9432823e-07f, 7.07945787e-07f, 6.30957345e-07f, 5.62341313e-07f, 5.0118723e-07f, 4.466836e-07f,
};

struct PnCngSid { float k[PN_CNG_MAX_ORDER]; float g; int32_t M; };   // a decoded SID; k[M..12) are +0.0

static inline void pn_cng_default_sid(uint8_t *sid) { memset(sid, 0, PN_CNG_SID_BYTES); sid[1] = PN_CNG_DEFAULT_LEVEL; }
// -1 with pn_last_error naming the first bad byte
static inline int pn_cng_sid_check(const uint8_t *sid) {
  if (!sid) { pn_set_error("NULL argument"); return -1; }
  if (sid[0] > PN_CNG_MAX_ORDER) { pn_set_error("SID order %d (byte 0): at most %d reflection coefficients", (int)sid[0], PN_CNG_MAX_ORDER); return -1; }
  if (sid[1] > 127) { pn_set_error("SID level %d (byte 1): a level in [0, 127] -dBov", (int)sid[1]); return -1; }
  for (int i = 0; i < sid[0]; i++)
    if (sid[2 + i] == 255) { pn_set_error("SID reflection coefficient N_%d = 255 (byte %d): a value in [0, 254]", i + 1, 2 + i); return -1; }
  return 0;
}
static inline int pn_cng_sid_decode_host(const uint8_t *sid, PnCngSid *o) {
  if (!o) { pn_set_error("NULL argument"); return -1; }
  if (pn_cng_sid_check(sid)) return -1;
  double prod = 1.0;
  o->M = sid[0];
  for (int i = 0; i < PN_CNG_MAX_ORDER; i++) {
    const double k = i < o->M ? 258.0 * ((int)sid[2 + i] - 127) / 32768.0 : 0.0;
    o->k[i] = (float)k;
    if (i < o->M) prod = prod * (1.0 - k * k);
  }
  o->g = (float)((double)pn_kCngLevel[sid[1]] * sqrt(prod));
  return 0;
}
// what is kept and read back of a SID: the bytes behind N_M as 0
static inline void pn_cng_sid_store(const uint8_t *sid, uint8_t *dst) {
  memset(dst, 0, PN_CNG_SID_BYTES);
  memcpy(dst, sid, 2 + (size_t)sid[0]);
}
// n streams' SIDs, `stride` bytes apart (>= PN_CNG_SID_BYTES), for the ids of a batch of B: -1 naming the first refused one
static inline int pn_cng_sids_set_check(int B, const int32_t *ids, int n, const uint8_t *sids, int stride) {
  if (n > 0 && (!sids || stride < PN_CNG_SID_BYTES)) { pn_set_error("bad argument: n SIDs of %d bytes, at least %d bytes apart", PN_CNG_SID_BYTES, PN_CNG_SID_BYTES); return -1; }
  if (pn_ids_check(B, ids, n, true)) return -1;
  for (int i = 0; i < n; i++)
    if (pn_cng_sid_check(sids + (size_t)i * stride)) {
      std::string why = pn_last_error();
      pn_set_error("SID %d (stream %d) refused: %s", i, (int)ids[i], why.c_str());
      return -1;
    }
  return 0;
}
static inline bool pn_cng_row_ok(int n) { return n == 80 || n == 160 || n == 240 || n == 320 || n == 480; }

PN_CNG_HD uint32_t pn_cng_mix(uint32_t h) { h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16; return h; }
PN_CNG_HD uint32_t pn_cng_key(uint32_t seed, uint32_t slot) { return seed ^ (slot * 0x9e3779b1u); }
PN_CNG_HD int pn_cng_u(uint32_t ctr, uint32_t key) {
  const uint32_t h = pn_cng_mix(pn_cng_mix(ctr) ^ key);
  return (int)(h & 0xffffu) + (int)(h >> 16) - 65535;
}
// one sample: the gain of column n of a row of ns (p0: prev, or g on the first row of a run), the excitation, the lattice in place on b
PN_CNG_STRICT PN_CNG_HD float pn_cng_sample(const float (&k)[PN_CNG_MAX_ORDER], int M, float g, float p0, int n, int ns, uint32_t ctr, uint32_t key, float (&b)[PN_CNG_MAX_ORDER]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float w = (float)(n + 1) / (float)ns, d = g - p0, t = w * d, gain = p0 + t;
  const float e = (float)pn_cng_u(ctr, key) * PN_CNG_C;
  float f = gain * e;
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = PN_CNG_MAX_ORDER; i >= 1; i--) {
    if (i <= M) {
      const float p = k[i - 1] * b[i - 1];
      f = f - p;
      if (i < M) { const float q = k[i - 1] * f; b[i] = b[i - 1] + q; }
    }
  }
  b[0] = f;
  return f;
}
PN_CNG_HD uint32_t pn_cng_count(uint32_t c) { return c == PN_CNG_SAT ? c : c + 1u; }

// One row of one stream: st[16] in place, row[ns] written, report[4] (optional): run, total, the bits of g, the counter behind the row.
// key: pn_cng_key(seed, slot).  cont: the row continues a run.  ns: 80, 160, 240, 320 or 480.
static inline int pn_cng_frame_host(const PnCngSid *sid, uint32_t *st, uint32_t key, int cont, int ns, float *row, uint32_t *report) {
  if (!sid || !st || !row) { pn_set_error("NULL argument"); return -1; }
  if (!pn_cng_row_ok(ns)) { pn_set_error("a comfort-noise row of %d samples: 80, 160, 240, 320 or 480 (10 ms at a converter's rates)", ns); return -1; }
  if (sid->M < 0 || sid->M > PN_CNG_MAX_ORDER) { pn_set_error("SID order %d: at most %d reflection coefficients", (int)sid->M, PN_CNG_MAX_ORDER); return -1; }
  float b[PN_CNG_MAX_ORDER], k[PN_CNG_MAX_ORDER], prev;
  memcpy(b, st, sizeof b); memcpy(k, sid->k, sizeof k); memcpy(&prev, &st[PN_CNG_W_PREV], 4);
  const float p0 = cont ? prev : sid->g;
  const uint32_t ctr = st[PN_CNG_W_CTR];
  for (int n = 0; n < ns; n++) row[n] = pn_cng_sample(k, sid->M, sid->g, p0, n, ns, ctr + (uint32_t)n, key, b);
  memcpy(st, b, sizeof b); memcpy(&st[PN_CNG_W_PREV], &sid->g, 4);
  st[PN_CNG_W_CTR] = ctr + (uint32_t)ns;
  st[PN_CNG_W_RUN] = cont ? pn_cng_count(st[PN_CNG_W_RUN]) : 1u;
  st[PN_CNG_W_TOTAL] = pn_cng_count(st[PN_CNG_W_TOTAL]);
  if (report) { report[0] = st[PN_CNG_W_RUN]; report[1] = st[PN_CNG_W_TOTAL]; report[2] = st[PN_CNG_W_PREV]; report[3] = st[PN_CNG_W_CTR]; }
  return 0;
}
