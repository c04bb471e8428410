// The two kernels of the batched rate converter for gfx950 (include/percepnet_hip.h "batched rate converter"; host side
// pn_rate.cpp; arithmetic and tap design pn_rate_design.h): L = 6 | 3 | 2 takes 8 | 16 | 24 kHz rows of n = 480 / L samples up to
// the engine's 48 kHz rows in front of a frame and back down behind it.  T = 16 taps per phase, D = T * L.  32 kHz rows of
// n = 320 are the rational factor (L, M) = (3, 2): the same kernels around row bodies of their own (rt_up_rows<L, M> below).
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
// The (3, 2) row of 32000 — up: 320 samples + 128 B of tail in, 1920 B out, 32 * 320 = 10 240 multiply-adds (two of a group's
// three outputs are sums); down: 1920 B + 192 B of tail in (2D / M = 48 words), 320 samples out, 160 * (47 + 48) = 15 200.
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

// ---- a rational factor: up by L with every M-th output kept, down from samples M apart on the L-times grid (32000: (3, 2)) ----
// The same sums in the same order — T = 16 taps per phase over the 32 newest inputs going up, every tap of g that meets a
// 48 kHz sample going down — with another lane mapping, since one input no longer owns a whole number of outputs.  M inputs
// make L outputs, so a lane owns GROUPS: group r is the inputs Mr .. Mr + M - 1 and the outputs Lr .. Lr + L - 1.
// up: buf = 32 tail samples, then the row's N = 480 M / L; o receives 480.  Output Lr + t is phase p = (M t) mod L of input
// q = Mr + (M t) div L: p = 0 copies x[q - 16], the others run sum_i h[L(15 - i) + p] * x[q - 31 + i], i ascending.  The group's
// windows overlap in all but M - 1 samples, so the lane reads buf[Mr .. Mr + 32 + M) once, as 8-byte LDS reads: consecutive lanes
// are M = 2 words apart, which four-byte reads would serve two lanes to a bank and eight-byte reads serve without a conflict.
template <int L, int M>
__device__ __forceinline__ void rt_up_rows(int lane, const float *buf, float *o, const float *taps) {
  constexpr int N = PN_FRAME * M / L, D = RT_T * L, G = N / M, W = RT_UT + M;
  static_assert(M == 2 && L > M && L % M != 0, "the window is read in 8-byte pairs: M = 2, and a factor in lowest terms");
  static_assert(PN_FRAME * M % L == 0 && N % M == 0 && G * L == PN_FRAME, "the phase pattern restarts with every frame: none is carried");
  static_assert((L - 1) * M / L + RT_UT < W, "every window of a group lies in the lane's W samples");
  for (int r = lane; r < G; r += RT_LANES) {
    float w[W];                                // w[k] = buf[Mr + k] = sample Mr + k - 32
#pragma unroll
    for (int k = 0; k < W / 2; k++) { const float2 v = reinterpret_cast<const float2 *>(buf)[r + k]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
#pragma unroll
    for (int t = 0; t < L; t++) {
      const int dq = M * t / L, p = M * t % L; // (constants once unrolled) x[i] = w[dq + 1 + i]
      if (p == 0) { o[L * r + t] = w[dq + RT_T]; continue; }
      float acc = 0.0f;
#pragma unroll
      for (int i = 0; i < RT_UT; i++) acc = acc + taps[D + L * (RT_T - 1 - i) + p] * w[dq + 1 + i];
      o[L * r + t] = acc;
    }
  }
}
// down: buf = TD = 2D / M tail samples, then the 480 of the row; z receives N.  Output m = Ma + u sums over every 48 kHz sample
// i = La + i' with |L u - D - M i'| < D, oldest first: i' = lo(u) .. hi(u), tap index (from the table's start) L u - M i'.
// Taps that are exactly 0 are visited like the others.  Consecutive lanes read L = 3 words apart: no two lanes of a half-wave
// on one bank.  The tap address is the same in every lane (a broadcast), since every lane runs the same u at the same time.
constexpr int rt_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
template <int L, int M>
__device__ __forceinline__ void rt_down_rows(int lane, const float *buf, float *z, const float *taps) {
  constexpr int N = PN_FRAME * M / L, D = RT_T * L, TD = 2 * D / M, G = N / M;
  static_assert(2 * D % M == 0 && N % M == 0 && G * L == PN_FRAME, "whole groups, and a tail of whole samples");
  static_assert(rt_floor_div(-2 * D, M) + 1 >= -TD + 1, "nothing older than the tail is read (its oldest sample never)");
  static_assert(L * (G - 1) + (L * (M - 1) + M - 1) / M - 1 < PN_FRAME, "nothing of the next frame is read");
  for (int a = lane; a < G; a += RT_LANES) {
    const float *x = buf + TD + L * a;         // x[i'] = 48 kHz sample La + i'
#pragma unroll
    for (int u = 0; u < M; u++) {
      const int lo = rt_floor_div(L * u - 2 * D, M) + 1, hi = (L * u + M - 1) / M - 1;      // (constants once unrolled)
      float acc = 0.0f;
#pragma unroll 8
      for (int i = lo; i <= hi; i++) acc = acc + taps[L * u - M * i] * x[i];
      z[M * a + u] = acc;
    }
  }
}
// the row bodies of a FACTOR (pn_rate_design.h): the integer ones above for 6, 3, 2, the rational ones for PN_RATE_F_3_2
template <int F>
__device__ __forceinline__ void rt_up_factor(int lane, const float *buf, float *o, const float *taps) {
  if constexpr (pn_rate_factor_M(F) == 1) rt_up_rows<F>(lane, buf, o, taps); else rt_up_rows<pn_rate_factor_L(F), pn_rate_factor_M(F)>(lane, buf, o, taps);
}
template <int F>
__device__ __forceinline__ void rt_down_factor(int lane, const float *buf, float *z, const float *taps) {
  if constexpr (pn_rate_factor_M(F) == 1) rt_down_rows<F>(lane, buf, z, taps); else rt_down_rows<pn_rate_factor_L(F), pn_rate_factor_M(F)>(lane, buf, z, taps);
}

template <int F, int FMT>
__global__ __launch_bounds__(RT_LANES * RT_WPB) void pn_rate_up_kernel(
    int n_rows, const int *__restrict__ ids,   // rows to run; ids == NULL: row w is stream w
    const int *__restrict__ laws,              // [n_streams] G.711 only: the law of every stream
    const void *__restrict__ in,               // [n_streams][N] float, int16 or G.711 bytes
    float *__restrict__ out48,                 // [n_streams][480]
    float *__restrict__ tail,                  // [n_streams][32], read then rewritten
    const float *__restrict__ taps) {          // h[-D..D]
  constexpr int L = pn_rate_factor_L(F), N = pn_rate_factor_frame(F), D = RT_T * L, NT = 2 * D + 1;
  static_assert(N % 16 == 0, "a row is whole 16-byte groups in every format");
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
      for (int i = lane; i < N / 16; i += RT_LANES) {
        const uint4 q = reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(in) + s * N)[i];
        float4 *d = reinterpret_cast<float4 *>(buf + RT_UT) + 4 * i;
        if (law == PN_G711_ALAW) rt_g711x16_to_f32<true>(q, d); else rt_g711x16_to_f32<false>(q, d);
      }
    } else if constexpr (FMT == PN_FMT_I16) {
      for (int i = lane; i < N / 8; i += RT_LANES) {
        union { uint4 q; int16_t h[8]; } u;
        u.q = reinterpret_cast<const uint4 *>(static_cast<const int16_t *>(in) + s * N)[i];
        float4 *d = reinterpret_cast<float4 *>(buf + RT_UT) + 2 * i;
        d[0] = make_float4((float)u.h[0] / 32768.f, (float)u.h[1] / 32768.f, (float)u.h[2] / 32768.f, (float)u.h[3] / 32768.f);
        d[1] = make_float4((float)u.h[4] / 32768.f, (float)u.h[5] / 32768.f, (float)u.h[6] / 32768.f, (float)u.h[7] / 32768.f);
      }
    } else {
      for (int i = lane; i < N / 4; i += RT_LANES) reinterpret_cast<float4 *>(buf + RT_UT)[i] = reinterpret_cast<const float4 *>(static_cast<const float *>(in) + s * N)[i];
    }
  }
  __syncthreads();
  if (live) {
    rt_up_factor<F>(lane, buf, o, s_taps);
  }
  __syncthreads();
  if (live) {
    float4 *dst = reinterpret_cast<float4 *>(out48 + s * PN_FRAME);
    for (int i = lane; i < PN_FRAME / 4; i += RT_LANES) dst[i] = reinterpret_cast<const float4 *>(o)[i];
    if (lane < RT_UT / 4) reinterpret_cast<float4 *>(tail + s * RT_UT)[lane] = reinterpret_cast<const float4 *>(buf + N)[lane];
  }
}

template <int F, int FMT>
__global__ __launch_bounds__(RT_LANES * RT_WPB) void pn_rate_down_kernel(
    int n_rows, const int *__restrict__ ids,
    const int *__restrict__ laws,              // [n_streams] G.711 only
    const float *__restrict__ in48,            // [n_streams][480]
    void *__restrict__ out,                    // [n_streams][N] float, int16 or G.711 bytes
    int saturate,                              // int16 and G.711: the saturating cast instead of the wrap
    float *__restrict__ tail,                  // [n_streams][2D / M], read then rewritten
    const float *__restrict__ taps) {          // g[-D..D]
  constexpr int L = pn_rate_factor_L(F), N = pn_rate_factor_frame(F), D = RT_T * L, TD = pn_rate_down_tail(F), NT = 2 * D + 1;
  static_assert(TD % 4 == 0 && TD / 4 <= RT_LANES && N % 16 == 0, "one 16-byte access per lane covers a tail; a row is whole 16-byte groups in every format");
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
    rt_down_factor<F>(lane, buf, z, s_taps);
  }
  __syncthreads();
  if (live) {
    if constexpr (FMT == PN_FMT_G711) {
      const int law = rt_wave_law(laws, s, live);
      for (int i = lane; i < N / 16; i += RT_LANES) {
        const float4 *zz = reinterpret_cast<const float4 *>(z) + 4 * i;
        reinterpret_cast<uint4 *>(static_cast<uint8_t *>(out) + s * N)[i] =
            law == PN_G711_ALAW ? rt_f32x16_to_g711<true>(zz, saturate) : rt_f32x16_to_g711<false>(zz, saturate);
      }
    } else if constexpr (FMT == PN_FMT_I16) {
      for (int i = lane; i < N / 8; i += RT_LANES) {
        const float4 a = reinterpret_cast<const float4 *>(z)[2 * i], b = reinterpret_cast<const float4 *>(z)[2 * i + 1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        union { int16_t h[8]; uint4 q; } p;
#pragma unroll
        for (int k = 0; k < 8; k++) { const float t = v[k] * 32768; p.h[k] = saturate ? pn_f2s_sat(t) : pn_f2s(t); }
        reinterpret_cast<uint4 *>(static_cast<int16_t *>(out) + s * N)[i] = p.q;
      }
    } else {
      for (int i = lane; i < N / 4; i += RT_LANES) reinterpret_cast<float4 *>(static_cast<float *>(out) + s * N)[i] = reinterpret_cast<const float4 *>(z)[i];
    }
    if (lane < TD / 4) reinterpret_cast<float4 *>(tail + s * TD)[lane] = reinterpret_cast<const float4 *>(buf + PN_FRAME)[lane];
  }
}

// ---- mixed rates: a factor per stream ------------------------------------------------------------------------------------------
// The same two kernels with the stream's factor in {6, 3, 2, 1, PN_RATE_F_3_2} read from a per-stream table (include/percepnet_hip.h "mixed rates").
// Low-rate rows are PN_RATE_MIXED_ROW = 480 samples apart whatever the stream's rate; a stream uses the first n = 480 M / L of its row,
// the rest of an input row is not read and the rest of an output row is not written.  Tails are rows of the largest size (32 up,
// 192 down), of which a stream uses the first 32 / pn_rate_down_tail(factor) words.  The block stages all the tap tables (the
// L = 6, 3, 2 tables one behind the other: 193 + 97 + 65 words; going down the 97 of 32000 behind them, going up a 32000 stream
// reads the L = 3 table).  A wave makes its factor uniform with readfirstlane and runs the row body of that factor behind
// a scalar branch; the four waves of a block may take four different branches, so the block's two barriers stand OUTSIDE them:
// stage -> barrier -> compute -> barrier -> store.  Factor 1 is a copy: the row goes straight to the output row in LDS (int16 as
// (float)v / 32768), the compute step does nothing, and no tail is read or written.
#define RT_ROW PN_RATE_MIXED_ROW
#define RT_DT_MAX (2 * RT_T * PN_RATE_MAX_L)                   // 192: a stream's down tail row
#define RT_NT(L) (2 * RT_T * (L) + 1)
#define RT_TAPS_ALL (RT_NT(6) + RT_NT(3) + RT_NT(2))           // 355: what the up kernel stages — a 32000 stream's h IS the L = 3 table
#define RT_TAPS_ALL_DOWN (RT_TAPS_ALL + RT_NT(3))              // 452: the g of 32000 (h * 2 / 3) behind the other three
#define RT_N_MAX (PN_FRAME * 2 / 3)                            // 320: the longest row with a filter
static_assert(RT_ROW == PN_FRAME && RT_ROW % 8 == 0, "a mixed row is a whole 48 kHz frame");
static_assert(pn_rate_factor_frame(PN_RATE_F_3_2) == RT_N_MAX && pn_rate_down_tail(PN_RATE_F_3_2) <= RT_DT_MAX, "a 32000 stream fits the mixed staging and tail rows");
__device__ __forceinline__ int rt_taps_offset(int f) { return f == 6 ? 0 : f == 3 ? RT_NT(6) : f == 2 ? RT_NT(6) + RT_NT(3) : RT_TAPS_ALL; }
// the wave's factor (pn_rate_design.h: 6, 3, 2, 1 or PN_RATE_F_3_2): lanes of dead waves and factors the host never writes run nothing (0)
__device__ __forceinline__ int rt_wave_factor(const int *factors, size_t s, bool live) {
  const int f = __builtin_amdgcn_readfirstlane(live ? factors[s] : 0);
  return (f == 6 || f == 3 || f == 2 || f == 1 || f == PN_RATE_F_3_2) ? f : 0;
}
// the samples of the wave's row, and the words of its down tail
__device__ __forceinline__ int rt_wave_frame(int f) { return f == PN_RATE_F_3_2 ? RT_N_MAX : f ? PN_FRAME / f : 0; }
__device__ __forceinline__ int rt_wave_down_tail(int f) { return f == PN_RATE_F_3_2 ? pn_rate_down_tail(PN_RATE_F_3_2) : f > 1 ? 2 * RT_T * f : 0; }
template <int FMT>
__global__ __launch_bounds__(RT_LANES * RT_WPB) void pn_rate_up_mixed_kernel(
    int n_rows, const int *__restrict__ ids,
    const int *__restrict__ factors,           // [n_streams] the factor of every stream
    const int *__restrict__ laws,              // [n_streams] G.711 only: the law of every stream
    const void *__restrict__ in,               // [n_streams][480] float, int16 or G.711 bytes, the first pn_rate_factor_frame(factor) used
    float *__restrict__ out48,                 // [n_streams][480]
    float *__restrict__ tail,                  // [n_streams][32], read then rewritten (not for factor 1)
    const float *__restrict__ taps) {          // h of L = 6, 3, 2, one table behind the other (32000 reads the table of 3)
  __shared__ float s_taps[RT_TAPS_ALL];
  __shared__ __align__(16) float s_buf[RT_WPB][RT_UT + RT_N_MAX];
  __shared__ __align__(16) float s_out[RT_WPB][PN_FRAME];
  const int lane = threadIdx.x & (RT_LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < RT_TAPS_ALL; i += RT_LANES * RT_WPB) s_taps[i] = taps[i];
  const int w = blockIdx.x * RT_WPB + wave;
  const bool live = w < n_rows;                // (no early return: the block meets at its barriers)
  const size_t s = live ? (size_t)(ids ? ids[w] : w) : 0;
  const int f = rt_wave_factor(factors, s, live);
  const int N = rt_wave_frame(f);              // wave-uniform
  float *buf = s_buf[wave], *o = s_out[wave];
  // stage: the tail and the row behind it; factor 1 puts the row where the results go
  float *row = f == 1 ? o : buf + RT_UT;
  if (f > 1 && lane < RT_UT / 4) reinterpret_cast<float4 *>(buf)[lane] = reinterpret_cast<const float4 *>(tail + s * RT_UT)[lane];
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
  if (f == 6) rt_up_rows<6>(lane, buf, o, s_taps + rt_taps_offset(6));
  else if (f == 3) rt_up_rows<3>(lane, buf, o, s_taps + rt_taps_offset(3));
  else if (f == 2) rt_up_rows<2>(lane, buf, o, s_taps + rt_taps_offset(2));
  else if (f == PN_RATE_F_3_2) rt_up_rows<3, 2>(lane, buf, o, s_taps + rt_taps_offset(3));
  __syncthreads();
  if (f) {
    float4 *dst = reinterpret_cast<float4 *>(out48 + s * PN_FRAME);
    for (int i = lane; i < PN_FRAME / 4; i += RT_LANES) dst[i] = reinterpret_cast<const float4 *>(o)[i];
    if (f > 1 && lane < RT_UT / 4) reinterpret_cast<float4 *>(tail + s * RT_UT)[lane] = reinterpret_cast<const float4 *>(buf + N)[lane];
  }
}

template <int FMT>
__global__ __launch_bounds__(RT_LANES * RT_WPB) void pn_rate_down_mixed_kernel(
    int n_rows, const int *__restrict__ ids,
    const int *__restrict__ factors,           // [n_streams]
    const int *__restrict__ laws,              // [n_streams] G.711 only
    const float *__restrict__ in48,            // [n_streams][480]
    void *__restrict__ out,                    // [n_streams][480] float, int16 or G.711 bytes, the first pn_rate_factor_frame(factor) written
    int saturate,
    float *__restrict__ tail,                  // [n_streams][192], the first pn_rate_down_tail(factor) read then rewritten (not for factor 1)
    const float *__restrict__ taps) {          // g of L = 6, 3, 2 and of 32000, one table behind the other
  __shared__ float s_taps[RT_TAPS_ALL_DOWN];
  __shared__ __align__(16) float s_buf[RT_WPB][RT_DT_MAX + PN_FRAME];
  __shared__ __align__(16) float s_out[RT_WPB][PN_FRAME];
  const int lane = threadIdx.x & (RT_LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < RT_TAPS_ALL_DOWN; i += RT_LANES * RT_WPB) s_taps[i] = taps[i];
  const int w = blockIdx.x * RT_WPB + wave;
  const bool live = w < n_rows;
  const size_t s = live ? (size_t)(ids ? ids[w] : w) : 0;
  const int f = rt_wave_factor(factors, s, live);
  const int N = rt_wave_frame(f), TD = rt_wave_down_tail(f);               // wave-uniform; TD / 4 <= 48 lanes
  float *buf = s_buf[wave], *z = s_out[wave];
  float *row = f == 1 ? z : buf + TD;
  if (lane < TD / 4) reinterpret_cast<float4 *>(buf)[lane] = reinterpret_cast<const float4 *>(tail + s * RT_DT_MAX)[lane];
  if (f) {
    const float4 *src = reinterpret_cast<const float4 *>(in48 + s * PN_FRAME);
    for (int i = lane; i < PN_FRAME / 4; i += RT_LANES) reinterpret_cast<float4 *>(row)[i] = src[i];
  }
  __syncthreads();
  if (f == 6) rt_down_rows<6>(lane, buf, z, s_taps + rt_taps_offset(6));
  else if (f == 3) rt_down_rows<3>(lane, buf, z, s_taps + rt_taps_offset(3));
  else if (f == 2) rt_down_rows<2>(lane, buf, z, s_taps + rt_taps_offset(2));
  else if (f == PN_RATE_F_3_2) rt_down_rows<3, 2>(lane, buf, z, s_taps + rt_taps_offset(PN_RATE_F_3_2));
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

// State records (include/percepnet_hip.h): record i <-> the two tails of stream ids[i]; one block per record.  td = pn_rate_down_tail(factor) words of a
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
// stride_words apart; one block per record.  The record's rate and tail length are the SLOT's: f = factors[s] in a mixed
// converter (the table a preceding rate change has already written, in stream order), f_all in a single-rate one; a slot without
// a filter (48000, which the host refuses before the launch) moves nothing.
//   gather   the header of the slot's rate, the two tails oldest first, zeros from the record's size up to the stride
//   scatter  lane 0 gives the header's verdict (pn_rate_header_verdict, the host check's own) against the slot's rate and writes
//            it to status[i]; behind the barrier the block copies the tails of an accepted record and leaves those of a refused
//            one untouched — the other records of the call are still imported (the contract of pn_ss_scatter_kernel)
__global__ __launch_bounds__(64) void pn_rate_records_dev_kernel(const int *__restrict__ ids, const int *__restrict__ factors, int f_all, float *__restrict__ tail_up,
                                                                 float *__restrict__ tail_down, int td_stride, uint32_t *__restrict__ rec, int stride_words,
                                                                 int *__restrict__ status, int scatter) {
  const size_t s = (size_t)ids[blockIdx.x];
  int f = factors ? factors[s] : f_all;                      // block-uniform; a factor of pn_rate_design.h
  if (f != 6 && f != 3 && f != 2 && f != PN_RATE_F_3_2) f = 0;
  const int rate = f ? pn_rate_factor_hz(f) : 0, td = f ? pn_rate_down_tail(f) : 0, body_words = f ? RT_UT + td : 0, hdr_words = PN_RATE_STATE_HEADER_BYTES / 4;
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
    if (f && threadIdx.x == 0) *reinterpret_cast<uint4 *>(r) = make_uint4(PN_RATE_STATE_MAGIC, PN_RATE_STATE_VERSION, 4u * (hdr_words + body_words), (uint32_t)rate);
    for (int i = (f ? hdr_words + body_words : 0) + threadIdx.x; i < stride_words; i += blockDim.x) r[i] = 0u;
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
    if (f == 6) RT_LAUNCH(kernel, 6 RT_COMMA, __VA_ARGS__);                                                            \
    else if (f == PN_RATE_F_3_2) RT_LAUNCH(kernel, PN_RATE_F_3_2 RT_COMMA, __VA_ARGS__);                               \
    else if (f == 3) RT_LAUNCH(kernel, 3 RT_COMMA, __VA_ARGS__);                                                       \
    else RT_LAUNCH(kernel, 2 RT_COMMA, __VA_ARGS__);                                                                   \
  } while (0)
static int rt_fmt_check(const char *who, int fmt, const int *d_laws) {
  if (fmt != PN_FMT_F32 && fmt != PN_FMT_I16 && fmt != PN_FMT_G711) { pn_set_error("%s: no kernel for sample format %d", who, fmt); return -1; }
  if (fmt == PN_FMT_G711 && !d_laws) { pn_set_error("%s: G.711 rows need the law table", who); return -1; }
  return 0;
}

int pn_launch_rate_up(hipStream_t st, int f, int fmt, int n_rows, const int *d_ids, const int *d_laws, const void *in, float *out48, float *tail, const float *taps) {
  if (f != 2 && f != 3 && f != 6 && f != PN_RATE_F_3_2) { pn_set_error("pn_launch_rate_up: no kernel for factor %d", f); return -1; }
  if (rt_fmt_check("pn_launch_rate_up", fmt, d_laws)) return -1;
  if (n_rows <= 0) return 0;
  RT_DISPATCH(pn_rate_up_kernel, n_rows, d_ids, d_laws, in, out48, tail, taps);
  return 0;
}
int pn_launch_rate_down(hipStream_t st, int f, int fmt, int n_rows, const int *d_ids, const int *d_laws, const float *in48, void *out, int saturate, float *tail, const float *taps) {
  if (f != 2 && f != 3 && f != 6 && f != PN_RATE_F_3_2) { pn_set_error("pn_launch_rate_down: no kernel for factor %d", f); return -1; }
  if (rt_fmt_check("pn_launch_rate_down", fmt, d_laws)) return -1;
  if (n_rows <= 0) return 0;
  RT_DISPATCH(pn_rate_down_kernel, n_rows, d_ids, d_laws, in48, out, saturate, tail, taps);
  return 0;
}
void pn_launch_rate_records(hipStream_t st, int f, int rate_hz, const int *d_ids, int n, float *tail_up, float *tail_down, int td_stride, void *rec, int scatter) {
  if (n <= 0) return;
  uint32_t h[4];
  pn_rate_record_header(h, rate_hz);
  hipLaunchKernelGGL(pn_rate_records_kernel, dim3(n), dim3(64), 0, st, d_ids, tail_up, tail_down, pn_rate_down_tail(f), td_stride, (uint32_t *)rec,
                     (int)pn_rate_record_words(f), make_uint4(h[0], h[1], h[2], h[3]), scatter);
}

// the mixed kernels: rows of 480 samples, the factor of every stream in d_factors, the tap tables one behind the other at taps
// (up: 6, 3, 2; down: 6, 3, 2 and 32000's)
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
