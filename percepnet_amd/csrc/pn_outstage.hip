// Output stage of the PercepNet frame engine for gfx950 — one wavefront (64 lanes) per stream, launched after the back end
// only while the per-stream frame report (pn_ctx_set_report) or the saturating int16 cast (pn_ctx_set_output_saturate) is on.
//
// It reads the frame's 480 fp32 output samples o (the caller's float rows, or the context's scratch rows that the back end's
// float instantiation wrote for an int16 entry point) and
//   - writes the caller's int16 rows: pn_f2s(o * 32768), the back end's fused cast (wrap), or the saturating cast;
//   - writes the stream's 32-byte report record (include/percepnet_hip.h): peak and energy of o and of the input frame this
//     output frame is about — frame t - 6 of the history ring, the engine's 2880-sample delay — the mean of the network's raw
//     g tap, the pitch period, the count of output samples outside the int16 range and the silence flag.
// Float rows are only read.  The input comes from the ring, never from the caller's `in`, so in / out aliasing cannot matter.
//
// Lane l < 60 owns samples 8l .. 8l + 7: two 16-byte loads per array and one 16-byte store of eight int16.  A lane folds its
// eight samples in index order, the wave folds its lanes by the xor butterfly 32, 16, 8, 4, 2, 1 (lanes 60..63 carry zeros):
// one fixed order, no atomics, no LDS, so a row's report is the same in every batch size, slot and block.  Arithmetic is
// separately rounded fp32 (-ffp-contract=off), like the back end's.
// Memory-bound: per stream 1920 B of o + 1920 B of history + 272 B of g|r, flags and period in, 960 B of PCM + 32 B out.
#include "pn_launch.h"
#include "pn_pcm.h"

#define OS_LANES 64
#define OS_WPB 4                   // wavefronts (= streams) per block
#define OS_OWNERS (PN_FRAME / 8)   // lanes that own samples
static_assert(PN_FRAME % 8 == 0 && OS_OWNERS <= OS_LANES && PN_HIST_STRIDE % 4 == 0 && PN_REPORT_WORDS == 8, "eight samples per lane, 16-byte aligned rows");

__device__ __forceinline__ float os_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float os_wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ int os_wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(OS_LANES * OS_WPB) void pn_outstage_kernel(
    int n_streams,
    const float *__restrict__ o,             // [n_streams][480] output samples before any cast
    const float *__restrict__ hist,          // report only: [n_streams][PN_HIST_STRIDE], the aligned input frame at hist_off
    int hist_off,
    const float *__restrict__ gr,            // report only: [n_streams][68] g | r
    const int *__restrict__ last_period, const int *__restrict__ silence,
    int16_t *__restrict__ pcm,               // [n_streams][480], or NULL: a float entry point
    int saturate,
    uint4 *__restrict__ report) {            // [n_streams][2], or NULL: report off
  const int lane = threadIdx.x & (OS_LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = blockIdx.x * OS_WPB + wave;
  if (s >= n_streams) return;
  const bool own = lane < OS_OWNERS;
  float v[8];
  {
    const float4 *o4 = reinterpret_cast<const float4 *>(o + (size_t)s * PN_FRAME) + 2 * lane;
    const float4 a = own ? o4[0] : make_float4(0.f, 0.f, 0.f, 0.f), b = own ? o4[1] : make_float4(0.f, 0.f, 0.f, 0.f);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  float peak = 0.f, energy = 0.f;
  int clipped = 0;
  union { int16_t h[8]; uint4 q; } p;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const float t = v[i] * 32768;
    peak = fmaxf(peak, fabsf(v[i]));
    energy = energy + v[i] * v[i];
    clipped += !(t > -32769.f && t < 32768.f);      // NaN counts
    p.h[i] = saturate ? pn_f2s_sat(t) : pn_f2s(t);
  }
  if (pcm && own) reinterpret_cast<uint4 *>(pcm + (size_t)s * PN_FRAME)[lane] = p.q;
  if (!report) return;
  float in_peak = 0.f, in_energy = 0.f;
  if (own) {
    const float4 *x4 = reinterpret_cast<const float4 *>(hist + (size_t)s * PN_HIST_STRIDE + hist_off) + 2 * lane;
    const float4 a = x4[0], b = x4[1];
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 8; i++) { in_peak = fmaxf(in_peak, fabsf(x[i])); in_energy = in_energy + x[i] * x[i]; }
  }
  const float g = lane < PN_NB ? gr[(size_t)s * 68 + lane] : 0.f;
  in_peak = os_wave_max(in_peak); in_energy = os_wave_sum(in_energy);
  peak = os_wave_max(peak); energy = os_wave_sum(energy);
  clipped = os_wave_sum(clipped);
  const float gain_mean = os_wave_sum(g) / PN_NB;
  if (lane == 0) {
    report[2 * (size_t)s] = make_uint4(__float_as_uint(in_peak), __float_as_uint(in_energy), __float_as_uint(peak), __float_as_uint(energy));
    report[2 * (size_t)s + 1] = make_uint4(__float_as_uint(gain_mean), (uint32_t)last_period[s], (uint32_t)clipped, silence[s] != 0 ? 1u : 0u);
  }
}

void pn_launch_outstage(hipStream_t st, int n_streams, const float *o, const PnDspSide &s, int hist_slot, const float *gr,
                        int16_t *pcm, int saturate, void *report) {
  const int grid = (n_streams + OS_WPB - 1) / OS_WPB;
  hipLaunchKernelGGL(pn_outstage_kernel, dim3(grid), dim3(OS_LANES * OS_WPB), 0, st, n_streams, o, s.hist, hist_slot * PN_FRAME, gr,
                     s.last_period, s.silence, pcm, saturate, (uint4 *)report);
}
