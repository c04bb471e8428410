// The DTX send side of the rate converter for gfx950 (include/percepnet_hip.h "DTX send side"; the rule, stated once with every rounding
// and summation order: pn_dtx_rules.h, whose scalar functions this kernel calls; host side pn_rate.cpp; numpy model tests/dtx_model.py):
// BEHIND the down-conversion, READ-ONLY on the output rows at the streams' own rates, in the format of the call.
// One wavefront per row, DX_WAVES rows per block; a wave keeps to its own LDS words, and the block's barriers are reached by every thread
// (rows behind the list's end and streams that are switched off stay as waves that load and store nothing).
//   decode     the row once into LDS as floats with 16-byte global loads (4 | 8 | 16 samples each), between DX_PAD = 12 zeros in front
//              and zeros behind up to 512: lane l then owns x[l], x[l + 64], .. in registers, and a lag's partner x[n - j] is one LDS read
//              at a compile-time offset — 64 consecutive words per instruction, no bank conflict, no `n >= j` branch.  That the padded
//              products leave the bits alone is shown in pn_dtx_rules.h
//   r[0]       every lane's partial sum from +0.0f in ascending n, the xor butterfly 32, 16, .., 1 by __shfl_xor: every lane holds r[0],
//              so every lane knows the frame's class (pn_dtx_classify on uniform words) and the wave branches as one
//   r[1..12]   only on a frame that is not active — the others read no lag — the same way, twelve more butterflies
//   rule       lanes 0..23 have read the state row coalesced into LDS; lane 0 runs pn_dtx_update IN PLACE on those words (Levinson only on
//              an emitting frame: rare, and the other lanes wait), with its workspace in LDS too, so no array is indexed in registers and
//              nothing goes to scratch; lanes 0..23 write the state back, lanes 0..7 the report row
// A stream that is switched off costs the read of its switch word and eight zero report words.  No atomics; nothing passes between
// blocks; a row depends on the stream's own state and nothing else, so it is the same in every batch size, block and list position.
#include "pn_launch.h"
#include "pn_dtx_rules.h"
#include "pn_g711.h"
#include "pn_rate_design.h"

#define DX_WAVES 4
#define DX_PAD 12
#define DX_MAX 512                             // 8 terms a lane
#define DX_ROW (DX_PAD + DX_MAX)
static_assert(DX_PAD == PN_DTX_LAGS - 1 && DX_PAD % 4 == 0 && PN_FRAME <= DX_MAX && DX_MAX == 8 * 64 && PN_DTX_STATE_WORDS <= 64 && PN_DTX_REPORT_WORDS <= 64,
              "the padding covers the largest lag and keeps the row 16-byte aligned; a lane owns eight samples");

__device__ __forceinline__ float dx_fold(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}

template <int FMT>
__global__ __launch_bounds__(64 * DX_WAVES) void pn_rate_dtx_kernel(
    int n_rows, const int *__restrict__ ids,   // rows to run; ids == NULL: row w is stream w
    const int *__restrict__ on,                // [n_streams] 0: the stage is off for the stream
    const int *__restrict__ factors, int ns1,  // [n_streams] the factor of every stream (mixed), or NULL and the converter's own n_s
    const int *__restrict__ laws,              // [n_streams] the G.711 law of every stream (FMT == PN_FMT_G711)
    PnDtxParams P,
    const void *__restrict__ rows, int stride, // [n_streams][stride] samples of the format, read only
    uint32_t *__restrict__ state,              // [n_streams][24]
    uint32_t *__restrict__ report) {           // [n_streams][8] DTX report records, NULL: off
  __shared__ __attribute__((aligned(16))) float s_x[DX_WAVES][DX_ROW];
  __shared__ uint32_t s_st[DX_WAVES][PN_DTX_STATE_WORDS], s_r[DX_WAVES][16], s_rep[DX_WAVES][PN_DTX_REPORT_WORDS];
  __shared__ float s_ws[DX_WAVES][PN_DTX_WS_WORDS];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int w = (int)blockIdx.x * DX_WAVES + wv;
  bool live = w < n_rows;
  int s = 0, ns = 0;
  if (live) {
    s = __builtin_amdgcn_readfirstlane(ids ? ids[w] : w);
    if (__builtin_amdgcn_readfirstlane(on[s]) == 0) {
      if (report && lane < PN_DTX_REPORT_WORDS) report[(size_t)s * PN_DTX_REPORT_WORDS + lane] = 0u;
      live = false;
    } else ns = factors ? pn_rate_factor_frame(__builtin_amdgcn_readfirstlane(factors[s])) : ns1;
  }
  float *x = s_x[wv];
  for (int i = lane; i < DX_ROW; i += 64)
    if (i < DX_PAD || i >= DX_PAD + ns) x[i] = 0.0f;
  if (live) {
    float4 *dst = reinterpret_cast<float4 *>(x + DX_PAD);
    if constexpr (FMT == PN_FMT_G711) {
      const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(rows) + (size_t)s * stride);
      const bool alaw = __builtin_amdgcn_readfirstlane(laws[s]) == PN_G711_ALAW;
      for (int i = lane; i < ns / 16; i += 64) {
        const uint4 q = src[i];
        const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
          float f[4];
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const uint32_t b = (u[k] >> (8 * j)) & 0xFFu;
            f[j] = (float)(alaw ? pn_g711_dec_alaw(b) : pn_g711_dec_ulaw(b)) * (1.0f / 32768.0f);
          }
          dst[4 * i + k] = make_float4(f[0], f[1], f[2], f[3]);
        }
      }
    } else if constexpr (FMT == PN_FMT_I16) {
      const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const int16_t *>(rows) + (size_t)s * stride);
      for (int i = lane; i < ns / 8; i += 64) {
        union { uint4 q; int16_t h[8]; } u;
        u.q = src[i];
        dst[2 * i] = make_float4((float)u.h[0] * (1.0f / 32768.0f), (float)u.h[1] * (1.0f / 32768.0f), (float)u.h[2] * (1.0f / 32768.0f), (float)u.h[3] * (1.0f / 32768.0f));
        dst[2 * i + 1] = make_float4((float)u.h[4] * (1.0f / 32768.0f), (float)u.h[5] * (1.0f / 32768.0f), (float)u.h[6] * (1.0f / 32768.0f), (float)u.h[7] * (1.0f / 32768.0f));
      }
    } else {
      const float4 *src = reinterpret_cast<const float4 *>(static_cast<const float *>(rows) + (size_t)s * stride);
      for (int i = lane; i < ns / 4; i += 64) dst[i] = src[i];
    }
    if (lane < PN_DTX_STATE_WORDS) s_st[wv][lane] = state[(size_t)s * PN_DTX_STATE_WORDS + lane];
  }
  __syncthreads();
  if (live) {
    // (64 k < ns is the wave's: ns comes from uniform words.  A skipped k holds zeros only, which would add +0.0)
    const float *xl = x + DX_PAD + lane;
    float xs[8];
#pragma unroll
    for (int k = 0; k < 8; k++) xs[k] = 64 * k < ns ? xl[64 * k] : 0.0f;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (64 * k < ns) { const float pr = xs[k] * xs[k]; acc = acc + pr; }
    const float r0 = dx_fold(acc);
    const float e = r0 / (float)ns;
    const uint32_t cls = pn_dtx_classify(P.v, __uint_as_float(s_st[wv][PN_DTX_W_N]), s_st[wv][PN_DTX_W_FRAMES], e);
    if (lane == 0) s_r[wv][0] = __float_as_uint(r0);
    if (!(cls & PN_DTX_ACTIVE)) {
#pragma unroll
      for (int j = 1; j < PN_DTX_LAGS; j++) {
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; k++)
          if (64 * k < ns) { const float pr = xs[k] * xl[64 * k - j]; a = a + pr; }
        a = dx_fold(a);
        if (lane == 0) s_r[wv][j] = __float_as_uint(a);
      }
    }
    if (lane == 0) pn_dtx_update(P.v, s_st[wv], s_r[wv], ns, s_ws[wv], s_rep[wv]);
  }
  __syncthreads();
  if (live) {
    if (lane < PN_DTX_STATE_WORDS) state[(size_t)s * PN_DTX_STATE_WORDS + lane] = s_st[wv][lane];
    if (report && lane < PN_DTX_REPORT_WORDS) report[(size_t)s * PN_DTX_REPORT_WORDS + lane] = s_rep[wv][lane];
  }
}

int pn_launch_rate_dtx(hipStream_t st, int fmt, int n_rows, const int *d_ids, const int *d_on, const int *d_factors, int ns, const int *d_laws, const float *params,
                       const void *rows, int stride, void *state, void *d_report) {
  if (fmt != PN_FMT_F32 && fmt != PN_FMT_I16 && fmt != PN_FMT_G711) { pn_set_error("pn_rate_dtx: no kernel for sample format %d", fmt); return -1; }
  if (fmt == PN_FMT_G711 && !d_laws) { pn_set_error("pn_rate_dtx: G.711 rows need the law table"); return -1; }
  if (!d_factors && !pn_cng_row_ok(ns)) { pn_set_error("pn_rate_dtx: a row of %d samples", ns); return -1; }
  if (stride < (d_factors ? PN_FRAME : ns) || stride % 16) { pn_set_error("pn_rate_dtx: rows %d samples apart", stride); return -1; }
  if (n_rows <= 0) return 0;
  PnDtxParams P;
  for (int i = 0; i < PN_DTX_N_PARAMS; i++) P.v[i] = params[i];
  const dim3 grid((n_rows + DX_WAVES - 1) / DX_WAVES), block(64 * DX_WAVES);
  uint32_t *s = static_cast<uint32_t *>(state), *rep = static_cast<uint32_t *>(d_report);
  if (fmt == PN_FMT_G711) hipLaunchKernelGGL(HIP_KERNEL_NAME(pn_rate_dtx_kernel<PN_FMT_G711>), grid, block, 0, st, n_rows, d_ids, d_on, d_factors, ns, d_laws, P, rows, stride, s, rep);
  else if (fmt == PN_FMT_I16) hipLaunchKernelGGL(HIP_KERNEL_NAME(pn_rate_dtx_kernel<PN_FMT_I16>), grid, block, 0, st, n_rows, d_ids, d_on, d_factors, ns, d_laws, P, rows, stride, s, rep);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(pn_rate_dtx_kernel<PN_FMT_F32>), grid, block, 0, st, n_rows, d_ids, d_on, d_factors, ns, d_laws, P, rows, stride, s, rep);
  return 0;
}
