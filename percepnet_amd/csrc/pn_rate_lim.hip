// Output limiter of the rate converter for gfx950 (include/percepnet_hip.h "output limiter"; the rule, stated once with every rounding
// and the proof of its guarantee: pn_lim_rules.h; host side pn_rate.cpp; numpy model tests/lim_model.py): the last stage in front of
// the down-conversion, in place on the 48 kHz rows it is about to read — the mix rows of conference members, every other stream's own
// (levelled) output.
// The layout of pn_rate_agc.hip: one row per two wavefronts, LM_ROWS rows per block; thread t < 120 of a row owns the float4 of
// columns 4t..4t+3 and KEEPS IT IN REGISTERS between the reduction and the scaling.
//   peak     max |o[j]| from +0.0 by fmaxf, a NaN sample ignored
//   first    the first index with |o[j]| * g0 > c, by integer min of 4t+i, or 480: where an attack's ramp has to have arrived
//            both are free of ordering and run in the same xor-butterfly pass 32, 16, .., 1
//   hand-off the two waves' peaks and indices meet through four LDS words per row behind ONE barrier, which every thread of the block
//            reaches: rows without work (behind the list's end, or not limited) stay as threads that load and store nothing
//   update   every lane runs the scalar rule (lm_update, the statements of pn_lim_step_host) on the same words: no broadcast behind it
// A row that needs no gain — g0 == g1 == 1.0f, the common case — is read once and NEVER written; so is a non-finite row.  A stream
// whose ceiling is 0 costs the read of its ceiling word and no row traffic.  The state words are read in front of the barrier (g0
// enters the index reduction) and written behind it by thread 0 of the row.  No atomics; a row depends on the stream's own state and
// nothing else, so it is the same in every batch size and block.
#include "pn_launch.h"
#include "pn_lim_rules.h"

#define LM_ROW_THREADS 128
#define LM_ROWS 4                              // rows per block, like pn_rate_agc.hip
#define LM_COLS (PN_FRAME / 4)                 // 120 float4 per row
static_assert(PN_FRAME % 4 == 0 && LM_COLS <= LM_ROW_THREADS && LM_ROW_THREADS == 128, "a thread per float4 of a row, two waves per row");

struct LmStep { float g0, g1; uint32_t hold, limited, flags; bool attack, write, keep_state; };
__device__ __forceinline__ float lm_needed(float p, float c) {   // pn_lim_needed_host
  if (!(p > c)) return 1.0f;
  float q = c / p;
  const float pq = p * q;
  if (pq > c) q = __uint_as_float(__float_as_uint(q) - 1u);
  return q;
}
__device__ __forceinline__ LmStep lm_update(const PnLimParams &P, float c, uint4 st, float g0, float p) {   // pn_lim_step_host
  LmStep o;
  const uint32_t h = st.y;
  o.g0 = g0; o.g1 = g0; o.hold = h; o.limited = st.z; o.flags = PN_LIM_ON; o.attack = false; o.write = false; o.keep_state = false;
  if (!(p <= FLT_MAX)) { o.flags |= PN_LIM_NONFINITE; o.keep_state = true; return o; }
  const float gl = lm_needed(p, c);
  bool active;
  if (gl < g0) {
    o.g1 = gl; o.hold = (uint32_t)P.v[PN_LIM_HOLD]; o.attack = true; o.write = true; active = true;
    o.flags |= PN_LIM_ATTACK;
  } else {
    if (h > 0u) { o.hold = h - 1u; o.flags |= PN_LIM_HOLDING; }
    else {
      const float up = g0 * P.v[PN_LIM_RELEASE];
      o.g1 = fminf(fminf(up, 1.0f), gl);
      if (o.g1 > g0) o.flags |= PN_LIM_RELEASING;
    }
    active = g0 < 1.0f || o.g1 < 1.0f;
    o.write = !(g0 == 1.0f && o.g1 == 1.0f);
  }
  if (active) { o.flags |= PN_LIM_ACTIVE; if (o.limited != PN_LIM_LIMITED_MAX) o.limited += 1u; }
  return o;
}
__device__ __forceinline__ float lm_attack(float y, float g0, float gl, float d, int j, int k, float fk) {   // pn_lim_attack_host
  if (j >= k) return y * gl;
  const float w = (float)j / fk, t = w * d, g = g0 + t;
  return y * g;
}
__device__ __forceinline__ float lm_ramp(float y, float g0, float d, int j) {   // pn_agc_apply_host
  const float w = (float)(2 * j + 1) / 960.0f, t = w * d, g = g0 + t;
  return y * g;
}
__device__ __forceinline__ int lm_over(float y, float g0, float c, int j) {     // pn_lim_first_over_host, one sample
  const float a = fabsf(y) * g0;
  return a > c ? j : PN_FRAME;
}

__global__ __launch_bounds__(LM_ROW_THREADS * LM_ROWS) void pn_rate_lim_kernel(
    int n_rows, const int *__restrict__ ids,   // rows to run; ids == NULL: row w is stream w
    const float *__restrict__ ceilings,        // [n_streams] c, +0.0: the stream is not limited
    PnLimParams P,
    float *__restrict__ o48,                   // [n_streams][480], in place
    uint4 *__restrict__ state,                 // [n_streams] gain, hold, limited, 0
    uint4 *__restrict__ report) {              // [n_streams] limiter report records, NULL: off
  __shared__ float s_p[LM_ROWS][2];
  __shared__ int s_k[LM_ROWS][2];
  const int t = threadIdx.x & (LM_ROW_THREADS - 1), lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 7)), wave = __builtin_amdgcn_readfirstlane((t >> 6));
  const int w = (int)blockIdx.x * LM_ROWS + row;
  // everything that decides whether a thread works is the same in both waves of its row; no thread leaves in front of the barrier
  bool live = w < n_rows;
  int s = 0;
  float c = 0.0f;
  if (live) {
    s = __builtin_amdgcn_readfirstlane(ids ? ids[w] : w);
    c = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(ceilings[s])));
    if (c == 0.0f) {
      if (report && t == 0) report[s] = make_uint4(0x3f800000u, 0u, 0u, 0u);
      live = false;
    }
  }
  const bool has_col = live && t < LM_COLS;
  float4 *orow = reinterpret_cast<float4 *>(o48 + (size_t)s * PN_FRAME);
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  uint4 st = make_uint4(0u, 0u, 0u, 0u);
  if (has_col) v = orow[t];
  if (live) st = state[s];
  const float g0 = st.x == 0u ? 1.0f : __uint_as_float(st.x);
  const int j = 4 * t;
  float pk = fmaxf(fmaxf(fmaxf(fmaxf(0.0f, fabsf(v.x)), fabsf(v.y)), fabsf(v.z)), fabsf(v.w));     // (a NaN sample is ignored)
  int kk = has_col ? min(min(lm_over(v.x, g0, c, j), lm_over(v.y, g0, c, j + 1)), min(lm_over(v.z, g0, c, j + 2), lm_over(v.w, g0, c, j + 3))) : PN_FRAME;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { pk = fmaxf(pk, __shfl_xor(pk, m)); kk = min(kk, __shfl_xor(kk, m)); }
  if (lane == 0) { s_p[row][wave] = pk; s_k[row][wave] = kk; }
  __syncthreads();
  if (!live) return;
  const float p = fmaxf(s_p[row][0], s_p[row][1]);
  const int k = min(s_k[row][0], s_k[row][1]);
  const LmStep u = lm_update(P, c, st, g0, p);
  if (has_col && u.write) {
    const float d = u.g1 - u.g0;
    if (u.attack) {
      const float fk = (float)k;
      orow[t] = make_float4(lm_attack(v.x, u.g0, u.g1, d, j, k, fk), lm_attack(v.y, u.g0, u.g1, d, j + 1, k, fk), lm_attack(v.z, u.g0, u.g1, d, j + 2, k, fk),
                            lm_attack(v.w, u.g0, u.g1, d, j + 3, k, fk));
    } else {
      orow[t] = make_float4(lm_ramp(v.x, u.g0, d, j), lm_ramp(v.y, u.g0, d, j + 1), lm_ramp(v.z, u.g0, d, j + 2), lm_ramp(v.w, u.g0, d, j + 3));
    }
  }
  if (t == 0) {
    if (!u.keep_state) state[s] = make_uint4(__float_as_uint(u.g1), u.hold, u.limited, 0u);
    if (report) report[s] = make_uint4(__float_as_uint(u.g1), __float_as_uint(p), u.flags, u.limited);
  }
}

void pn_launch_rate_lim(hipStream_t st, int n_rows, const int *d_ids, const float *d_ceilings, const float *params, float *o48, void *state, void *d_report) {
  if (n_rows <= 0) return;
  PnLimParams P;
  for (int i = 0; i < PN_LIM_N_PARAMS; i++) P.v[i] = params[i];
  hipLaunchKernelGGL(pn_rate_lim_kernel, dim3((n_rows + LM_ROWS - 1) / LM_ROWS), dim3(LM_ROW_THREADS * LM_ROWS), 0, st, n_rows, d_ids, d_ceilings, P, o48,
                     reinterpret_cast<uint4 *>(state), reinterpret_cast<uint4 *>(d_report));
}
