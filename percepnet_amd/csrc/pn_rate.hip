// The two kernels of the batched rate converter for gfx950 (include/percepnet_hip.h "batched rate converter"; host side
// pn_rate.cpp; arithmetic and tap design pn_rate_design.h): L = 6 | 3 | 2 takes 8 | 16 | 24 kHz rows of n = 480 / L samples up to
// the engine's 48 kHz rows in front of a frame and back down behind it.  T = 16 taps per phase, D = T * L.
//
// One wavefront (64 lanes) per stream, four streams per block, like the output stage.  A wave stages its row behind the stream's
// tail in LDS — up: 32 + n low-rate samples, down: 2D + 480 samples at 48 kHz — with 16-byte loads, the block stages the 2D + 1
// taps, and then lane l owns the low-rate sample indices l, l + 64, ...:
//   up    index q: the window x[q - 31 .. q] goes to registers once; phase 0 stores x[q - 16] (a copy: the input's bits), phases
//         p = 1..L-1 each run sum_i h[L(15 - i) + p] * x[q - 31 + i], i ascending = oldest sample first.  The tap address is the
//         same in every lane (an LDS broadcast), the window addresses are consecutive.
//   down  index m: sum_j g[D - 1 - j] * o[Lm - 2D + 1 + j], j = 0..2D-2 ascending = oldest first (g[+-D] = 0 is not visited).
// acc starts at 0.0f and every step is acc = acc + c * x with the product and the sum rounded separately (-ffp-contract=off, like
// the DSP kernels), in one order that depends on nothing but the stream's own samples: no atomics, no cross-lane sums, so a
// stream's output is the same in every batch size, slot and block, and numpy float32 reproduces it (tests/rate_model.py).
// The results pass through LDS once more so that the rows leave with 16-byte coalesced stores (every row here is a multiple of
// 16 bytes), and the wave then writes the stream's new tail in place — the last 32 staged low-rate samples / the last 2D staged
// 48 kHz samples — after all of its reads of the old one.
// ids (optional): the rows to run, one per wave; the grid covers only those.  An unlisted stream is neither read nor written,
// which is the converter's whole active-set story: nothing to save, nothing to restore.
// Memory-bound by design.  Per stream and frame — up: n samples + 128 B of tail in, 1920 B out, 32 n (L - 1) multiply-adds
// (12 800 | 10 240 | 7 680); down: 1920 B + 8 D bytes of tail in, n samples out, n (2D - 1) multiply-adds (15 280 | 15 200 | 15 120).
// Below them: the same two kernels with a factor PER STREAM (pn_rate_create_mixed), which call the same row bodies.
#include "pn_launch.h"
#include "pn_pcm.h"
#include "pn_g711.h"
#include "pn_rate_design.h"

#define RT_LANES 64
#define RT_WPB 4                     // wavefronts (= streams) per block
#define RT_T PN_RATE_TAPS
#define RT_UT PN_RATE_UP_TAIL        // 32
static_assert(RT_UT == 2 * RT_T && RT_UT % 4 == 0 && PN_FRAME % (16 * PN_RATE_MAX_L) == 0, "tails and rows are whole 16-byte groups, in every sample format");

// The sample formats of the low-rate rows (pn_launch.h PN_FMT_*): a format enters only where a row is staged into LDS and where it
// leaves, so the row bodies below are the one piece of code every format runs.  int16: x = (float)v / 32768 in, the wrapping or
// saturating cast of t = z * 32768 out.  G.711 (8 bit, pn_g711.h): the int16 format with the companding outside it — in
// x = (float)dec(b) / 32768, out enc(c) of exactly the int16 c the int16 format writes — so a G.711 stream gives bit for bit
// the encoding of what the int16 path gives on the decoded samples.  One 16-byte access carries 4 | 8 | 16 samples.
// int16 x 8 -> two float4 / two float4 -> int16 x 8
__device__ __forceinline__ void rt_i16x8_to_f32(uint4 q, float4 *d) {
  union { uint4 q; int16_t h[8]; } u;
  u.q = q;
  d[0] = make_float4((float)u.h[0] / 32768.f, (float)u.h[1] / 32768.f, (float)u.h[2] / 32768.f, (float)u.h[3] / 32768.f);
  d[1] = make_float4((float)u.h[4] / 32768.f, (float)u.h[5] / 32768.f, (float)u.h[6] / 32768.f, (float)u.h[7] / 32768.f);
}
__device__ __forceinline__ uint4 rt_f32x8_to_i16(const float4 *z, int saturate) {
  const float4 a = z[0], b = z[1];
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  union { int16_t h[8]; uint4 q; } p;
#pragma unroll
  for (int i = 0; i < 8; i++) { const float t = v[i] * 32768; p.h[i] = saturate ? pn_f2s_sat(t) : pn_f2s(t); }
  return p.q;
}
// G.711 x 16 -> four float4 / four float4 -> G.711 x 16: integer ALU on the lane's own 16 bytes, sample i in byte i.  ALAW is
// the wave's law, uniform (rt_wave_law) and branched on by the caller, so that a lane runs one law's formulas.
template <bool ALAW>
__device__ __forceinline__ void rt_g711x16_to_f32(uint4 q, float4 *d) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float f[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t b = (w[k] >> (8 * j)) & 0xFFu;
      f[j] = (float)(ALAW ? pn_g711_dec_alaw(b) : pn_g711_dec_ulaw(b)) / 32768.f;
    }
    d[k] = make_float4(f[0], f[1], f[2], f[3]);
  }
}
template <bool ALAW>
__device__ __forceinline__ uint4 rt_f32x16_to_g711(const float4 *z, int saturate) {
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float4 a = z[k];
    const float v[4] = {a.x, a.y, a.z, a.w};
    w[k] = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float t = v[j] * 32768;
      const int32_t c = saturate ? pn_f2s_sat(t) : pn_f2s(t);
      w[k] |= (ALAW ? pn_g711_enc_alaw(c) : pn_g711_enc_ulaw(c)) << (8 * j);
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// the wave's law from the per-stream table (pn_rate_set_stream_laws), uniform; lanes of dead waves run mu-law on nothing
__device__ __forceinline__ int rt_wave_law(const int *laws, size_t s, bool live) {
  return __builtin_amdgcn_readfirstlane(live ? laws[s] : 0);
}

// The row bodies of the two conversions, shared by the single-rate kernels and the mixed ones (so a stream's arithmetic is one
// piece of code whichever converter runs it).  All pointers are LDS; taps = the table of this L, h[-D..D] / g[-D..D].
// up: buf = 32 tail samples, then the row's N = 480 / L; o receives 480.
template <int L>
__device__ __forceinline__ void rt_up_rows(int lane, const float *buf, float *o, const float *taps) {
  constexpr int N = PN_FRAME / L, D = RT_T * L;
  for (int q = lane; q < N; q += RT_LANES) {
    float x[RT_UT];                            // x[i] = sample q - 31 + i
#pragma unroll
    for (int i = 0; i < RT_UT; i++) x[i] = buf[q + 1 + i];
    o[L * q] = x[RT_T - 1];                    // phase 0: sample q - T
#pragma unroll 1                        // (unrolled, L = 6 keeps all 160 taps in registers: 256 VGPRs)
    for (int p = 1; p < L; p++) {
      float acc = 0.0f;
#pragma unroll
      for (int i = 0; i < RT_UT; i++) acc = acc + taps[D + L * (RT_T - 1 - i) + p] * x[i];
      o[L * q + p] = acc;
    }
  }
}
// down: buf = 2D tail samples, then the 480 of the row; z receives N = 480 / L.
template <int L>
__device__ __forceinline__ void rt_down_rows(int lane, const float *buf, float *z, const float *taps) {
  constexpr int N = PN_FRAME / L, TD = 2 * RT_T * L;
  for (int m = lane; m < N; m += RT_LANES) {
    const float *x = buf + L * m + 1;          // x[j] = 48 kHz sample Lm - 2D + 1 + j
    float acc = 0.0f;
#pragma unroll 8
    for (int j = 0; j < TD - 1; j++) acc = acc + taps[TD - 1 - j] * x[j];
    z[m] = acc;
  }
}

template <int L, int FMT>
__global__ __launch_bounds__(RT_LANES * RT_WPB) void pn_rate_up_kernel(
    int n_rows, const int *__restrict__ ids,   // rows to run; ids == NULL: row w is stream w
    const int *__restrict__ laws,              // [n_streams] G.711 only: the law of every stream
    const void *__restrict__ in,               // [n_streams][N] float, int16 or G.711 bytes
    float *__restrict__ out48,                 // [n_streams][480]
    float *__restrict__ tail,                  // [n_streams][32], read then rewritten
    const float *__restrict__ taps) {          // h[-D..D]
  constexpr int N = PN_FRAME / L, D = RT_T * L, NT = 2 * D + 1;
  static_assert(N % 16 == 0 && N / 4 <= RT_LANES, "one 16-byte load per lane covers a row");
  __shared__ float s_taps[NT];
  __shared__ __align__(16) float s_buf[RT_WPB][RT_UT + N];
  __shared__ __align__(16) float s_out[RT_WPB][PN_FRAME];
  const int lane = threadIdx.x & (RT_LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < NT; i += RT_LANES * RT_WPB) s_taps[i] = taps[i];
  const int w = blockIdx.x * RT_WPB + wave;
  const bool live = w < n_rows;                // (no early return: the block meets at its barriers)
  const size_t s = live ? (size_t)(ids ? ids[w] : w) : 0;
  float *buf = s_buf[wave], *o = s_out[wave];
  if (live) {
    if (lane < RT_UT / 4) reinterpret_cast<float4 *>(buf)[lane] = reinterpret_cast<const float4 *>(tail + s * RT_UT)[lane];
    if constexpr (FMT == PN_FMT_G711) {
      const int law = rt_wave_law(laws, s, live);
      if (lane < N / 16) {
        const uint4 q = reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(in) + s * N)[lane];
        float4 *d = reinterpret_cast<float4 *>(buf + RT_UT) + 4 * lane;
        if (law == PN_G711_ALAW) rt_g711x16_to_f32<true>(q, d); else rt_g711x16_to_f32<false>(q, d);
      }
    } else if constexpr (FMT == PN_FMT_I16) {
      if (lane < N / 8) {
        union { uint4 q; int16_t h[8]; } u;
        u.q = reinterpret_cast<const uint4 *>(static_cast<const int16_t *>(in) + s * N)[lane];
        float4 *d = reinterpret_cast<float4 *>(buf + RT_UT) + 2 * lane;
        d[0] = make_float4((float)u.h[0] / 32768.f, (float)u.h[1] / 32768.f, (float)u.h[2] / 32768.f, (float)u.h[3] / 32768.f);
        d[1] = make_float4((float)u.h[4] / 32768.f, (float)u.h[5] / 32768.f, (float)u.h[6] / 32768.f, (float)u.h[7] / 32768.f);
      }
    } else {
      if (lane < N / 4) reinterpret_cast<float4 *>(buf + RT_UT)[lane] = reinterpret_cast<const float4 *>(static_cast<const float *>(in) + s * N)[lane];
    }
  }
  __syncthreads();
  if (live) {
    rt_up_rows<L>(lane, buf, o, s_taps);
  }
  __syncthreads();
  if (live) {
    float4 *dst = reinterpret_cast<float4 *>(out48 + s * PN_FRAME);
    for (int i = lane; i < PN_FRAME / 4; i += RT_LANES) dst[i] = reinterpret_cast<const float4 *>(o)[i];
    if (lane < RT_UT / 4) reinterpret_cast<float4 *>(tail + s * RT_UT)[lane] = reinterpret_cast<const float4 *>(buf + N)[lane];
  }
}

template <int L, int FMT>
__global__ __launch_bounds__(RT_LANES * RT_WPB) void pn_rate_down_kernel(
    int n_rows, const int *__restrict__ ids,
    const int *__restrict__ laws,              // [n_streams] G.711 only
    const float *__restrict__ in48,            // [n_streams][480]
    void *__restrict__ out,                    // [n_streams][N] float, int16 or G.711 bytes
    int saturate,                              // int16 and G.711: the saturating cast instead of the wrap
    float *__restrict__ tail,                  // [n_streams][2D], read then rewritten
    const float *__restrict__ taps) {          // g[-D..D]
  constexpr int N = PN_FRAME / L, D = RT_T * L, TD = 2 * D, NT = 2 * D + 1;
  static_assert(TD % 4 == 0 && TD / 4 <= RT_LANES && N % 16 == 0 && N / 4 <= RT_LANES, "one 16-byte access per lane covers a tail and an output row");
  __shared__ float s_taps[NT];
  __shared__ __align__(16) float s_buf[RT_WPB][TD + PN_FRAME];
  __shared__ __align__(16) float s_out[RT_WPB][N];
  const int lane = threadIdx.x & (RT_LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < NT; i += RT_LANES * RT_WPB) s_taps[i] = taps[i];
  const int w = blockIdx.x * RT_WPB + wave;
  const bool live = w < n_rows;
  const size_t s = live ? (size_t)(ids ? ids[w] : w) : 0;
  float *buf = s_buf[wave], *z = s_out[wave];
  if (live) {
    if (lane < TD / 4) reinterpret_cast<float4 *>(buf)[lane] = reinterpret_cast<const float4 *>(tail + s * TD)[lane];
    const float4 *src = reinterpret_cast<const float4 *>(in48 + s * PN_FRAME);
    for (int i = lane; i < PN_FRAME / 4; i += RT_LANES) reinterpret_cast<float4 *>(buf + TD)[i] = src[i];
  }
  __syncthreads();
  if (live) {
    rt_down_rows<L>(lane, buf, z, s_taps);
  }
  __syncthreads();
  if (live) {
    if constexpr (FMT == PN_FMT_G711) {
      const int law = rt_wave_law(laws, s, live);
      if (lane < N / 16) {
        const float4 *zz = reinterpret_cast<const float4 *>(z) + 4 * lane;
        reinterpret_cast<uint4 *>(static_cast<uint8_t *>(out) + s * N)[lane] =
            law == PN_G711_ALAW ? rt_f32x16_to_g711<true>(zz, saturate) : rt_f32x16_to_g711<false>(zz, saturate);
      }
    } else if constexpr (FMT == PN_FMT_I16) {
      if (lane < N / 8) {
        const float4 a = reinterpret_cast<const float4 *>(z)[2 * lane], b = reinterpret_cast<const float4 *>(z)[2 * lane + 1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        union { int16_t h[8]; uint4 q; } p;
#pragma unroll
        for (int i = 0; i < 8; i++) { const float t = v[i] * 32768; p.h[i] = saturate ? pn_f2s_sat(t) : pn_f2s(t); }
        reinterpret_cast<uint4 *>(static_cast<int16_t *>(out) + s * N)[lane] = p.q;
      }
    } else {
      if (lane < N / 4) reinterpret_cast<float4 *>(static_cast<float *>(out) + s * N)[lane] = reinterpret_cast<const float4 *>(z)[lane];
    }
    if (lane < TD / 4) reinterpret_cast<float4 *>(tail + s * TD)[lane] = reinterpret_cast<const float4 *>(buf + PN_FRAME)[lane];
  }
}

// ---- mixed rates: a factor per stream ------------------------------------------------------------------------------------------
// The same two kernels with the stream's L in {6, 3, 2, 1} read from a per-stream table (include/percepnet_hip.h "mixed rates").
// Low-rate rows are PN_RATE_MIXED_ROW = 480 samples apart whatever the stream's rate; a stream uses the first 480 / L of its row,
// the rest of an input row is not read and the rest of an output row is not written.  Tails are rows of the largest size (32 up,
// 192 down), of which a stream uses the first 32 / 2D words.  The block stages all three tap tables (the L = 6, 3, 2 tables one
// behind the other: 193 + 97 + 65 words).  A wave makes its L uniform with readfirstlane and runs the row body of that L behind
// a scalar branch; the four waves of a block may take four different branches, so the block's two barriers stand OUTSIDE them:
// stage -> barrier -> compute -> barrier -> store.  L = 1 is a copy: the row goes straight to the output row in LDS (int16 as
// (float)v / 32768), the compute step does nothing, and no tail is read or written.
#define RT_ROW PN_RATE_MIXED_ROW
#define RT_DT_MAX (2 * RT_T * PN_RATE_MAX_L)                   // 192: a stream's down tail row
#define RT_NT(L) (2 * RT_T * (L) + 1)
#define RT_TAPS_ALL (RT_NT(6) + RT_NT(3) + RT_NT(2))           // 355
static_assert(RT_ROW == PN_FRAME && RT_ROW % 8 == 0, "a mixed row is a whole 48 kHz frame");
__device__ __forceinline__ int rt_taps_offset(int L) { return L == 6 ? 0 : L == 3 ? RT_NT(6) : RT_NT(6) + RT_NT(3); }
// the wave's factor: lanes of dead waves and factors the host never writes run nothing (0)
__device__ __forceinline__ int rt_wave_factor(const int *factors, size_t s, bool live) {
  const int L = __builtin_amdgcn_readfirstlane(live ? factors[s] : 0);
  return (L == 6 || L == 3 || L == 2 || L == 1) ? L : 0;
}
template <int FMT>
__global__ __launch_bounds__(RT_LANES * RT_WPB) void pn_rate_up_mixed_kernel(
    int n_rows, const int *__restrict__ ids,
    const int *__restrict__ factors,           // [n_streams] L of every stream
    const int *__restrict__ laws,              // [n_streams] G.711 only: the law of every stream
    const void *__restrict__ in,               // [n_streams][480] float, int16 or G.711 bytes, the first 480 / L used
    float *__restrict__ out48,                 // [n_streams][480]
    float *__restrict__ tail,                  // [n_streams][32], read then rewritten (not for L = 1)
    const float *__restrict__ taps) {          // h of L = 6, 3, 2, one table behind the other
  __shared__ float s_taps[RT_TAPS_ALL];
  __shared__ __align__(16) float s_buf[RT_WPB][RT_UT + PN_FRAME / 2];
  __shared__ __align__(16) float s_out[RT_WPB][PN_FRAME];
  const int lane = threadIdx.x & (RT_LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < RT_TAPS_ALL; i += RT_LANES * RT_WPB) s_taps[i] = taps[i];
  const int w = blockIdx.x * RT_WPB + wave;
  const bool live = w < n_rows;                // (no early return: the block meets at its barriers)
  const size_t s = live ? (size_t)(ids ? ids[w] : w) : 0;
  const int L = rt_wave_factor(factors, s, live);
  const int N = L ? PN_FRAME / L : 0;          // wave-uniform
  float *buf = s_buf[wave], *o = s_out[wave];
  // stage: the tail and the row behind it; L = 1 puts the row where the results go
  float *row = L == 1 ? o : buf + RT_UT;
  if (L > 1 && lane < RT_UT / 4) reinterpret_cast<float4 *>(buf)[lane] = reinterpret_cast<const float4 *>(tail + s * RT_UT)[lane];
  if constexpr (FMT == PN_FMT_G711) {
    const int law = rt_wave_law(laws, s, live);
    const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(in) + s * RT_ROW);
    if (law == PN_G711_ALAW) for (int i = lane; i < N / 16; i += RT_LANES) rt_g711x16_to_f32<true>(src[i], reinterpret_cast<float4 *>(row) + 4 * i);
    else for (int i = lane; i < N / 16; i += RT_LANES) rt_g711x16_to_f32<false>(src[i], reinterpret_cast<float4 *>(row) + 4 * i);
  } else if constexpr (FMT == PN_FMT_I16) {
    const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const int16_t *>(in) + s * RT_ROW);
    for (int i = lane; i < N / 8; i += RT_LANES) rt_i16x8_to_f32(src[i], reinterpret_cast<float4 *>(row) + 2 * i);
  } else {
    const float4 *src = reinterpret_cast<const float4 *>(static_cast<const float *>(in) + s * RT_ROW);
    for (int i = lane; i < N / 4; i += RT_LANES) reinterpret_cast<float4 *>(row)[i] = src[i];
  }
  __syncthreads();
  if (L == 6) rt_up_rows<6>(lane, buf, o, s_taps + rt_taps_offset(6));
  else if (L == 3) rt_up_rows<3>(lane, buf, o, s_taps + rt_taps_offset(3));
  else if (L == 2) rt_up_rows<2>(lane, buf, o, s_taps + rt_taps_offset(2));
  __syncthreads();
  if (L) {
    float4 *dst = reinterpret_cast<float4 *>(out48 + s * PN_FRAME);
    for (int i = lane; i < PN_FRAME / 4; i += RT_LANES) dst[i] = reinterpret_cast<const float4 *>(o)[i];
    if (L > 1 && lane < RT_UT / 4) reinterpret_cast<float4 *>(tail + s * RT_UT)[lane] = reinterpret_cast<const float4 *>(buf + N)[lane];
  }
}

template <int FMT>
__global__ __launch_bounds__(RT_LANES * RT_WPB) void pn_rate_down_mixed_kernel(
    int n_rows, const int *__restrict__ ids,
    const int *__restrict__ factors,           // [n_streams]
    const int *__restrict__ laws,              // [n_streams] G.711 only
    const float *__restrict__ in48,            // [n_streams][480]
    void *__restrict__ out,                    // [n_streams][480] float, int16 or G.711 bytes, the first 480 / L written
    int saturate,
    float *__restrict__ tail,                  // [n_streams][192], the first 2D read then rewritten (not for L = 1)
    const float *__restrict__ taps) {          // g of L = 6, 3, 2, one table behind the other
  __shared__ float s_taps[RT_TAPS_ALL];
  __shared__ __align__(16) float s_buf[RT_WPB][RT_DT_MAX + PN_FRAME];
  __shared__ __align__(16) float s_out[RT_WPB][PN_FRAME];
  const int lane = threadIdx.x & (RT_LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < RT_TAPS_ALL; i += RT_LANES * RT_WPB) s_taps[i] = taps[i];
  const int w = blockIdx.x * RT_WPB + wave;
  const bool live = w < n_rows;
  const size_t s = live ? (size_t)(ids ? ids[w] : w) : 0;
  const int L = rt_wave_factor(factors, s, live);
  const int N = L ? PN_FRAME / L : 0, TD = L > 1 ? 2 * RT_T * L : 0;       // wave-uniform; TD / 4 <= 48 lanes
  float *buf = s_buf[wave], *z = s_out[wave];
  float *row = L == 1 ? z : buf + TD;
  if (lane < TD / 4) reinterpret_cast<float4 *>(buf)[lane] = reinterpret_cast<const float4 *>(tail + s * RT_DT_MAX)[lane];
  if (L) {
    const float4 *src = reinterpret_cast<const float4 *>(in48 + s * PN_FRAME);
    for (int i = lane; i < PN_FRAME / 4; i += RT_LANES) reinterpret_cast<float4 *>(row)[i] = src[i];
  }
  __syncthreads();
  if (L == 6) rt_down_rows<6>(lane, buf, z, s_taps + rt_taps_offset(6));
  else if (L == 3) rt_down_rows<3>(lane, buf, z, s_taps + rt_taps_offset(3));
  else if (L == 2) rt_down_rows<2>(lane, buf, z, s_taps + rt_taps_offset(2));
  __syncthreads();
  if constexpr (FMT == PN_FMT_G711) {
    const int law = rt_wave_law(laws, s, live);
    uint4 *dst = reinterpret_cast<uint4 *>(static_cast<uint8_t *>(out) + s * RT_ROW);
    if (law == PN_G711_ALAW) for (int i = lane; i < N / 16; i += RT_LANES) dst[i] = rt_f32x16_to_g711<true>(reinterpret_cast<const float4 *>(z) + 4 * i, saturate);
    else for (int i = lane; i < N / 16; i += RT_LANES) dst[i] = rt_f32x16_to_g711<false>(reinterpret_cast<const float4 *>(z) + 4 * i, saturate);
  } else if constexpr (FMT == PN_FMT_I16) {
    uint4 *dst = reinterpret_cast<uint4 *>(static_cast<int16_t *>(out) + s * RT_ROW);
    for (int i = lane; i < N / 8; i += RT_LANES) dst[i] = rt_f32x8_to_i16(reinterpret_cast<const float4 *>(z) + 2 * i, saturate);
  } else {
    float4 *dst = reinterpret_cast<float4 *>(static_cast<float *>(out) + s * RT_ROW);
    for (int i = lane; i < N / 4; i += RT_LANES) dst[i] = reinterpret_cast<const float4 *>(z)[i];
  }
  if (lane < TD / 4) reinterpret_cast<float4 *>(tail + s * RT_DT_MAX)[lane] = reinterpret_cast<const float4 *>(buf + PN_FRAME)[lane];
}

// A rate change (pn_rate_set_stream_rates): factors[ids[i]] = vals[i], ids distinct.  The tails are zeroed by the launches behind it.
// A law change (pn_rate_set_stream_laws) writes the law table the same way, in stream order, and touches no tail.
__global__ void pn_rate_set_factors_kernel(const int *__restrict__ ids, const int *__restrict__ vals, int n, int *__restrict__ factors) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) factors[ids[i]] = vals[i];
}

// State records (include/percepnet_hip.h): record i <-> the two tails of stream ids[i]; one block per record.  td = 2D words of a
// down tail row that is td_stride words long (td in a single-rate converter, 192 in a mixed one).  gather writes the header too; scatter trusts it (the host import has checked every header before anything is launched).
__global__ __launch_bounds__(64) void pn_rate_records_kernel(const int *__restrict__ ids, float *__restrict__ tail_up, float *__restrict__ tail_down,
                                                             int td, int td_stride, uint32_t *__restrict__ rec, int rec_words, uint4 hdr, int scatter) {
  const size_t s = (size_t)ids[blockIdx.x];
  uint32_t *r = rec + (size_t)blockIdx.x * rec_words;
  if (!scatter && threadIdx.x == 0) *reinterpret_cast<uint4 *>(r) = hdr;
  float *body = reinterpret_cast<float *>(r + PN_RATE_STATE_HEADER_BYTES / 4);
  for (int i = threadIdx.x; i < RT_UT + td; i += blockDim.x) {
    float *p = i < RT_UT ? tail_up + s * RT_UT + i : tail_down + s * td_stride + (i - RT_UT);
    if (scatter) *p = body[i]; else body[i] = *p;
  }
}

// Device-side records (pn_rate_export_streams / pn_rate_import_streams): record i <-> the two tails of stream ids[i], records
// stride_words apart; one block per record.  The record's rate and tail length are the SLOT's: L = factors[s] in a mixed
// converter (the table a preceding rate change has already written, in stream order), L_all in a single-rate one; a slot without
// a filter (48000, which the host refuses before the launch) moves nothing.
//   gather   the header of the slot's rate, the two tails oldest first, zeros from the record's size up to the stride
//   scatter  lane 0 gives the header's verdict (pn_rate_header_verdict, the host check's own) against the slot's rate and writes
//            it to status[i]; behind the barrier the block copies the tails of an accepted record and leaves those of a refused
//            one untouched — the other records of the call are still imported (the contract of pn_ss_scatter_kernel)
__global__ __launch_bounds__(64) void pn_rate_records_dev_kernel(const int *__restrict__ ids, const int *__restrict__ factors, int L_all, float *__restrict__ tail_up,
                                                                 float *__restrict__ tail_down, int td_stride, uint32_t *__restrict__ rec, int stride_words,
                                                                 int *__restrict__ status, int scatter) {
  const size_t s = (size_t)ids[blockIdx.x];
  int L = factors ? factors[s] : L_all;                      // block-uniform
  if (L != 6 && L != 3 && L != 2) L = 0;
  const int rate = L ? 48000 / L : 0, td = 2 * RT_T * L, body_words = L ? RT_UT + td : 0, hdr_words = PN_RATE_STATE_HEADER_BYTES / 4;
  uint32_t *r = rec + (size_t)blockIdx.x * stride_words;
  float *body = reinterpret_cast<float *>(r + hdr_words);
  __shared__ int verdict;
  if (scatter) {
    if (threadIdx.x == 0) {
      const uint4 h = *reinterpret_cast<const uint4 *>(r);
      verdict = pn_rate_header_verdict(h.x, h.y, h.z, h.w, rate);
      status[blockIdx.x] = verdict;
    }
    __syncthreads();
    if (verdict != PN_SS_OK) return;
  } else {
    if (L && threadIdx.x == 0) *reinterpret_cast<uint4 *>(r) = make_uint4(PN_RATE_STATE_MAGIC, PN_RATE_STATE_VERSION, 4u * (hdr_words + body_words), (uint32_t)rate);
    for (int i = (L ? hdr_words + body_words : 0) + threadIdx.x; i < stride_words; i += blockDim.x) r[i] = 0u;
  }
  for (int i = threadIdx.x; i < body_words; i += blockDim.x) {
    float *p = i < RT_UT ? tail_up + s * RT_UT + i : tail_down + s * td_stride + (i - RT_UT);
    if (scatter) *p = body[i]; else body[i] = *p;
  }
}

#define RT_LAUNCH(kernel, fmt_, ...)                                                                                    \
  do {                                                                                                               \
    if (fmt == PN_FMT_G711) hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<fmt_ PN_FMT_G711>), grid, block, 0, st, __VA_ARGS__);  \
    else if (fmt == PN_FMT_I16) hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<fmt_ PN_FMT_I16>), grid, block, 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<fmt_ PN_FMT_F32>), grid, block, 0, st, __VA_ARGS__);               \
  } while (0)
#define RT_COMMA ,
#define RT_DISPATCH(kernel, ...)                                                                                     \
  do {                                                                                                               \
    const dim3 grid((n_rows + RT_WPB - 1) / RT_WPB), block(RT_LANES * RT_WPB);                                         \
    if (L == 6) RT_LAUNCH(kernel, 6 RT_COMMA, __VA_ARGS__);                                                            \
    else if (L == 3) RT_LAUNCH(kernel, 3 RT_COMMA, __VA_ARGS__);                                                       \
    else RT_LAUNCH(kernel, 2 RT_COMMA, __VA_ARGS__);                                                                   \
  } while (0)
static int rt_fmt_check(const char *who, int fmt, const int *d_laws) {
  if (fmt != PN_FMT_F32 && fmt != PN_FMT_I16 && fmt != PN_FMT_G711) { pn_set_error("%s: no kernel for sample format %d", who, fmt); return -1; }
  if (fmt == PN_FMT_G711 && !d_laws) { pn_set_error("%s: G.711 rows need the law table", who); return -1; }
  return 0;
}

int pn_launch_rate_up(hipStream_t st, int L, int fmt, int n_rows, const int *d_ids, const int *d_laws, const void *in, float *out48, float *tail, const float *taps) {
  if (L != 2 && L != 3 && L != 6) { pn_set_error("pn_launch_rate_up: no kernel for L = %d", L); return -1; }
  if (rt_fmt_check("pn_launch_rate_up", fmt, d_laws)) return -1;
  if (n_rows <= 0) return 0;
  RT_DISPATCH(pn_rate_up_kernel, n_rows, d_ids, d_laws, in, out48, tail, taps);
  return 0;
}
int pn_launch_rate_down(hipStream_t st, int L, int fmt, int n_rows, const int *d_ids, const int *d_laws, const float *in48, void *out, int saturate, float *tail, const float *taps) {
  if (L != 2 && L != 3 && L != 6) { pn_set_error("pn_launch_rate_down: no kernel for L = %d", L); return -1; }
  if (rt_fmt_check("pn_launch_rate_down", fmt, d_laws)) return -1;
  if (n_rows <= 0) return 0;
  RT_DISPATCH(pn_rate_down_kernel, n_rows, d_ids, d_laws, in48, out, saturate, tail, taps);
  return 0;
}
void pn_launch_rate_records(hipStream_t st, int L, int rate_hz, const int *d_ids, int n, float *tail_up, float *tail_down, int td_stride, void *rec, int scatter) {
  if (n <= 0) return;
  uint32_t h[4];
  pn_rate_record_header(h, rate_hz);
  hipLaunchKernelGGL(pn_rate_records_kernel, dim3(n), dim3(64), 0, st, d_ids, tail_up, tail_down, pn_rate_down_tail(L), td_stride, (uint32_t *)rec,
                     (int)pn_rate_record_words(L), make_uint4(h[0], h[1], h[2], h[3]), scatter);
}

// the mixed kernels: rows of 480 samples, the factor of every stream in d_factors, all three tap tables at taps
int pn_launch_rate_up_mixed(hipStream_t st, int fmt, int n_rows, const int *d_ids, const int *d_factors, const int *d_laws, const void *in, float *out48, float *tail, const float *taps) {
  if (rt_fmt_check("pn_launch_rate_up_mixed", fmt, d_laws)) return -1;
  if (n_rows <= 0) return 0;
  const dim3 grid((n_rows + RT_WPB - 1) / RT_WPB), block(RT_LANES * RT_WPB);
  RT_LAUNCH(pn_rate_up_mixed_kernel, , n_rows, d_ids, d_factors, d_laws, in, out48, tail, taps);
  return 0;
}
int pn_launch_rate_down_mixed(hipStream_t st, int fmt, int n_rows, const int *d_ids, const int *d_factors, const int *d_laws, const float *in48, void *out, int saturate, float *tail, const float *taps) {
  if (rt_fmt_check("pn_launch_rate_down_mixed", fmt, d_laws)) return -1;
  if (n_rows <= 0) return 0;
  const dim3 grid((n_rows + RT_WPB - 1) / RT_WPB), block(RT_LANES * RT_WPB);
  RT_LAUNCH(pn_rate_down_mixed_kernel, , n_rows, d_ids, d_factors, d_laws, in48, out, saturate, tail, taps);
  return 0;
}
void pn_launch_rate_set_factors(hipStream_t st, const int *d_ids, const int *d_vals, int n, int *d_factors) {
  if (n <= 0) return;
  hipLaunchKernelGGL(pn_rate_set_factors_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_ids, d_vals, n, d_factors);
}
// the device-side records: d_factors (mixed) or factor (single-rate) gives each slot's rate; stride_words between two records
void pn_launch_rate_records_dev(hipStream_t st, const int *d_ids, int n, const int *d_factors, int factor, float *tail_up, float *tail_down, int td_stride,
                                void *rec, int stride_words, int *d_status, int scatter) {
  if (n <= 0) return;
  hipLaunchKernelGGL(pn_rate_records_dev_kernel, dim3(n), dim3(64), 0, st, d_ids, d_factors, factor, tail_up, tail_down, td_stride, (uint32_t *)rec, stride_words,
                     d_status, scatter);
}
