// Automatic level control of the rate converter for gfx950 (include/percepnet_hip.h "automatic level control"; the rule, stated once with
// every rounding and summation order: pn_agc_rules.h; host side pn_rate.cpp; numpy model tests/agc_model.py): between the engine and the
// mix or the down-conversion, in place on the 48 kHz rows.
// One row per two wavefronts, AG_ROWS rows per block.  Thread t < 120 of a row owns the float4 of columns 4t..4t+3, so a row moves in
// 16-byte accesses and whole 128-byte lines, and the float4 STAYS IN REGISTERS between the reduction and the scaling: a row is read
// once and written once.
//   energy   thread t forms the group sum ((((0 + y0 y0) + y1 y1) + y2 y2) + y3 y3) of its columns (threads 120..127: +0.0), each wave
//            folds its 64 group sums by the xor butterfly 32, 16, .., 1 — IEEE adds commute, so every lane ends with the same bits —
//            and E = wave 0's sum + wave 1's: the layout and the order of pn_rate_mix.hip's level, pn_mix_level_host on the host
//   peak     a max of non-negative values, free of ordering, by the same shuffles
//   hand-off the two halves and the two peaks meet through four LDS words per row behind ONE barrier, which every thread of the
//            block reaches: rows without work (behind the list's end, or not levelled) stay as threads that load and store nothing
//   update   every lane runs the scalar rule (ag_update, the statements of pn_agc_step_host) on the same words: no broadcast behind it
// A row that is not levelled costs the read of its target word and no row traffic.  The state words are read in front of the barrier
// and written behind it by thread 0 of the row, so both waves have read what that thread replaces.  No atomics; a row depends on the
// stream's own state and nothing else, so it is the same in every batch size and block.
#include "pn_launch.h"
#include "pn_agc_rules.h"

#define AG_ROW_THREADS 128
#define AG_ROWS 4                              // rows per block, like the row kernels of pn_rate.hip
#define AG_COLS (PN_FRAME / 4)                 // 120 float4 per row
static_assert(PN_FRAME % 4 == 0 && AG_COLS <= AG_ROW_THREADS && AG_ROW_THREADS == 128, "a thread per float4 of a row, two waves per row");

struct AgStep { float g0, g1, lev; uint32_t adapted, flags; };
__device__ __forceinline__ AgStep ag_update(const PnAgcParams &P, float T, uint4 st, float E, float p, bool concealed) {   // pn_agc_step_host
  float lev = __uint_as_float(st.x), g0 = st.y == 0u ? 1.0f : __uint_as_float(st.y);
  const float Gmax = P.v[PN_AGC_MAX_GAIN], Gmin = P.v[PN_AGC_MIN_GAIN], th = P.v[PN_AGC_GATE_RMS], c = P.v[PN_AGC_CEILING];
  const float th2 = th * th, Eg = th2 * 480.0f, T2 = T * T, Tt = T2 * 480.0f;
  const bool voiced = E > Eg && E <= FLT_MAX && !concealed;
  uint32_t flags = PN_AGC_ON | (concealed ? PN_AGC_HELD_LOST : 0u);
  float gs = g0;
  if (voiced) {
    if (lev == 0.0f) lev = E;
    else { const float a = E > lev ? P.v[PN_AGC_ATTACK] : P.v[PN_AGC_RELEASE], d = E - lev, t = a * d; lev = lev + t; }
    const float q = Tt / lev;
    gs = sqrtf(q);
    if (gs > Gmax) { gs = Gmax; flags |= PN_AGC_AT_MAX; }
    if (gs < Gmin) { gs = Gmin; flags |= PN_AGC_AT_MIN; }
    flags |= PN_AGC_ADAPTED;
  }
  const float hi = g0 * P.v[PN_AGC_STEP_UP], lo = g0 * P.v[PN_AGC_STEP_DOWN];
  float g1 = fminf(fmaxf(gs, lo), hi);
  const float m = fmaxf(g0, g1), pm = p * m;
  if (p <= FLT_MAX && pm > c) {
    const float gl = fmaxf(c / p, Gmin);
    g0 = fminf(g0, gl); g1 = fminf(g1, gl);
    flags |= PN_AGC_LIMITED;
  }
  AgStep o;
  o.g0 = g0; o.g1 = g1; o.lev = lev; o.flags = flags;
  o.adapted = st.z + ((voiced && st.z != PN_AGC_ADAPTED_MAX) ? 1u : 0u);
  return o;
}
__device__ __forceinline__ float ag_apply(float y, float g0, float d, int j) {   // pn_agc_apply_host
  const float w = (float)(2 * j + 1) / 960.0f, t = w * d, g = g0 + t;
  return y * g;
}

__global__ __launch_bounds__(AG_ROW_THREADS * AG_ROWS) void pn_rate_agc_kernel(
    int n_rows, const int *__restrict__ ids,   // rows to run; ids == NULL: row w is stream w
    const float *__restrict__ targets,         // [n_streams] T, +0.0: the stream is not levelled
    const uint32_t *__restrict__ lost, uint32_t tick,   // [n_streams] == tick: PLC filled the stream's frame; NULL: nobody is concealed
    PnAgcParams P,
    float *__restrict__ y48,                   // [n_streams][480], in place
    uint4 *__restrict__ state,                 // [n_streams] lev, gain, adapted, 0
    uint4 *__restrict__ report) {              // [n_streams] AGC report records, NULL: off
  __shared__ float s_e[AG_ROWS][2], s_p[AG_ROWS][2];
  const int t = threadIdx.x & (AG_ROW_THREADS - 1), lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 7)), wave = __builtin_amdgcn_readfirstlane((t >> 6));
  const int w = (int)blockIdx.x * AG_ROWS + row;
  // everything that decides whether a thread works is the same in both waves of its row; no thread leaves in front of the barrier
  bool live = w < n_rows;
  int s = 0;
  float T = 0.0f;
  if (live) {
    s = __builtin_amdgcn_readfirstlane(ids ? ids[w] : w);
    T = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(targets[s])));
    if (T == 0.0f) {
      if (report && t == 0) report[s] = make_uint4(0x3f800000u, 0u, 0u, 0u);
      live = false;
    }
  }
  const bool has_col = live && t < AG_COLS;
  float4 *yrow = reinterpret_cast<float4 *>(y48 + (size_t)s * PN_FRAME);
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  uint4 st = make_uint4(0u, 0u, 0u, 0u);
  bool concealed = false;
  if (has_col) v = yrow[t];
  if (live) {
    st = state[s];
    if (lost) concealed = lost[s] == tick;
  }
  float e = 0.0f;
  e = e + v.x * v.x; e = e + v.y * v.y; e = e + v.z * v.z; e = e + v.w * v.w;
  float pk = fmaxf(fmaxf(fmaxf(fmaxf(0.0f, fabsf(v.x)), fabsf(v.y)), fabsf(v.z)), fabsf(v.w));     // (a NaN sample is ignored)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { e = e + __shfl_xor(e, m); pk = fmaxf(pk, __shfl_xor(pk, m)); }
  if (lane == 0) { s_e[row][wave] = e; s_p[row][wave] = pk; }
  __syncthreads();
  if (!live) return;
  const float E = s_e[row][0] + s_e[row][1], p = fmaxf(s_p[row][0], s_p[row][1]);
  const AgStep u = ag_update(P, T, st, E, p, concealed);
  if (has_col) {
    const float d = u.g1 - u.g0;
    const int j = 4 * t;
    yrow[t] = make_float4(ag_apply(v.x, u.g0, d, j), ag_apply(v.y, u.g0, d, j + 1), ag_apply(v.z, u.g0, d, j + 2), ag_apply(v.w, u.g0, d, j + 3));
  }
  if (t == 0) {
    state[s] = make_uint4(__float_as_uint(u.lev), __float_as_uint(u.g1), u.adapted, 0u);
    if (report) report[s] = make_uint4(__float_as_uint(u.g1), __float_as_uint(u.lev), u.flags, __float_as_uint(p));
  }
}

void pn_launch_rate_agc(hipStream_t st, int n_rows, const int *d_ids, const float *d_targets, const uint32_t *d_lost, uint32_t tick, const float *params,
                        float *y48, void *state, void *d_report) {
  if (n_rows <= 0) return;
  PnAgcParams P;
  for (int i = 0; i < PN_AGC_N_PARAMS; i++) P.v[i] = params[i];
  hipLaunchKernelGGL(pn_rate_agc_kernel, dim3((n_rows + AG_ROWS - 1) / AG_ROWS), dim3(AG_ROW_THREADS * AG_ROWS), 0, st, n_rows, d_ids, d_targets, d_lost, tick, P,
                     y48, reinterpret_cast<uint4 *>(state), reinterpret_cast<uint4 *>(d_report));
}
