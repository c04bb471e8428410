// In-band DTMF detection of the rate converter for gfx950 (include/percepnet_hip.h "DTMF detection"; the rule, stated once with every
// rounding and summation order: pn_dtmf_rules.h; host side pn_rate.cpp; numpy model tests/dtmf_model.py): behind the concealer and in
// front of the engine, READ-ONLY on the 48 kHz rows.
// One row per two wavefronts, DT_ROWS rows per block, like pn_rate_agc.hip: thread t < 120 of a row owns the float4 of columns 4t..4t+3.
// A thread's columns never change from row to row, so its 64 twiddles (8 frequencies x cos, sin x 4 columns) are loaded ONCE and stay in
// registers while the block walks over rows base, base + gridDim.x * DT_ROWS, ..: the 30 KB table is read once per block, not once per
// row (that would be sixteen times the row's own bytes).
//   half sums  thread t forms the 17 group sums ((((0 + x0 w0) + x1 w1) + x2 w2) + x3 w3) of its columns (threads 120..127: +0.0), each
//              wave folds its 64 group sums by the xor butterfly 32, 16, .., 1 and a sum = wave 0's + wave 1's: the layout and the
//              order of pn_mix_level_host, pn_dtmf_dot_host on the host.  The energy folds plainly; the 16 tone sums fold TRANSPOSED
//              (below): the same adds of the same tree — IEEE adds commute — with 17 cross-lane moves instead of 96
//   hand-off   the two waves' 17 halves meet through LDS behind ONE barrier per pass, which every thread of the block reaches: the pass
//              count depends on blockIdx alone, and rows without work (behind the list's end, not enabled, concealed) stay as threads
//              that load and store nothing.  The LDS words are double-buffered by the pass's parity: a wave writes buffer p again only
//              behind the barrier of the pass in between, which no wave passes before it has read buffer p
//   rule       every lane of the row's FIRST wave runs the scalar rule (pn_dtmf_power, pn_dtmf_decide, pn_dtmf_held: the one text of
//              pn_dtmf_rules.h) on the same words: no broadcast behind it.  That wave alone reads the state (six 16-byte words), behind
//              the barrier, and its thread 0 writes it — Cp and Sp as soon as the powers exist, the other eight words behind the
//              decision — so the 24 words are never live together with the 17 accumulators or with each other, which keeps the
//              kernel within 128 registers beside its 64 twiddles; no other wave ever reads what thread 0 replaces
// A stream that is not enabled costs the read of its switch word and no row or state traffic; a concealed one no row traffic.  No
// atomics; a row depends on the stream's own state and nothing else, so it is the same in every batch size, block, pass and list position.
#include "pn_launch.h"
#include "pn_dtmf_rules.h"

#define DT_ROW_THREADS 128
#define DT_ROWS 4                              // rows per block and pass
#define DT_COLS (PN_FRAME / 4)                 // 120 float4 per row
static_assert(PN_FRAME % 4 == 0 && DT_COLS <= DT_ROW_THREADS && DT_ROW_THREADS == 128 && PN_DTMF_STATE_WORDS == 24, "a thread per float4 of a row, two waves per row, six uint4 of state");

__global__ __launch_bounds__(DT_ROW_THREADS * DT_ROWS, 4) void pn_rate_dtmf_kernel(
    int n_rows, const int *__restrict__ ids,   // rows to run; ids == NULL: row w is stream w
    const int *__restrict__ on,                // [n_streams] 0: detection is off for the stream
    const uint32_t *__restrict__ lost, uint32_t tick,   // [n_streams] == tick: PLC filled the stream's frame; NULL: nobody is concealed
    PnDtmfParams P_,
    const float4 *__restrict__ tab,            // [16][120] float4: ct[0..7] then st[0..7]
    const float *__restrict__ x48,             // [n_streams][480], read only
    uint4 *__restrict__ state,                 // [n_streams][6]
    uint4 *__restrict__ report) {              // [n_streams] DTMF report records, NULL: off
  __shared__ float s_h[2][DT_ROWS][2][PN_DTMF_NSUM];
  const int t = threadIdx.x & (DT_ROW_THREADS - 1), lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 7)), wave = __builtin_amdgcn_readfirstlane((t >> 6));
  float4 tw[2 * PN_DTMF_NF];
#pragma unroll
  for (int k = 0; k < 2 * PN_DTMF_NF; k++) tw[k] = t < DT_COLS ? tab[k * DT_COLS + t] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  int par = 0;
  for (int base = (int)blockIdx.x * DT_ROWS; base < n_rows; base += (int)gridDim.x * DT_ROWS, par ^= 1) {
    const int w = base + row;
    // everything that decides whether a thread works is the same in both waves of its row; no thread skips the barrier
    bool live = w < n_rows, concealed = false;
    int s = 0;
    if (live) {
      s = __builtin_amdgcn_readfirstlane(ids ? ids[w] : w);
      if (__builtin_amdgcn_readfirstlane(on[s]) == 0) {
        if (report && t == 0) report[s] = make_uint4(0u, 0u, 0u, 0u);
        live = false;
      } else if (lost) concealed = __builtin_amdgcn_readfirstlane((int)(lost[s] == tick)) != 0;
    }
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live && !concealed && t < DT_COLS) v = reinterpret_cast<const float4 *>(x48 + (size_t)s * PN_FRAME)[t];
    if (live && !concealed) {                          // (the same in both waves of the row: a wave without work goes straight to the barrier)
      float a[2 * PN_DTMF_NF], e = 0.0f;
#pragma unroll
      for (int k = 0; k < 2 * PN_DTMF_NF; k++) {
        float c = 0.0f;
        c = c + v.x * tw[k].x; c = c + v.y * tw[k].y; c = c + v.z * tw[k].z; c = c + v.w * tw[k].w;
        a[k] = c;
      }
      e = e + v.x * v.x; e = e + v.y * v.y; e = e + v.z * v.z; e = e + v.w * v.w;
      // The 16 butterflies, transposed.  At stride m a lane needs v[l] + v[l ^ m] of every sum; done plainly, both lanes of a pair
      // then hold the same value twice over.  Instead the pair SPLITS the sums: the lane whose bit m is clear goes on with the even
      // sum of each two, its partner with the odd one, each sending the other the half it gives up — one cross-lane move for two
      // sums, and half as many sums left at the next stride.  Every add is still v[l] + v[l ^ m] of one sum in the order 32, 16, ..,
      // 1, so the bits are the butterfly's.  16 -> 8 -> 4 -> 2 -> 1 sums at strides 32, 16, 8, 4; strides 2 and 1 fold the last one
      // plainly.  Lane l then holds sum k = (l >> 5 & 1) | (l >> 4 & 1) << 1 | (l >> 3 & 1) << 2 | (l >> 2 & 1) << 3
#pragma unroll
      for (int i = 0; i < 8; i++) { const bool up = lane & 32; const float keep = up ? a[2 * i + 1] : a[2 * i], send = up ? a[2 * i] : a[2 * i + 1]; a[i] = keep + __shfl_xor(send, 32); }
#pragma unroll
      for (int i = 0; i < 4; i++) { const bool up = lane & 16; const float keep = up ? a[2 * i + 1] : a[2 * i], send = up ? a[2 * i] : a[2 * i + 1]; a[i] = keep + __shfl_xor(send, 16); }
#pragma unroll
      for (int i = 0; i < 2; i++) { const bool up = lane & 8; const float keep = up ? a[2 * i + 1] : a[2 * i], send = up ? a[2 * i] : a[2 * i + 1]; a[i] = keep + __shfl_xor(send, 8); }
      { const bool up = lane & 4; const float keep = up ? a[1] : a[0], send = up ? a[0] : a[1]; a[0] = keep + __shfl_xor(send, 4); }
      a[0] = a[0] + __shfl_xor(a[0], 2);
      a[0] = a[0] + __shfl_xor(a[0], 1);
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) e = e + __shfl_xor(e, m);
      if ((lane & 3) == 0) s_h[par][row][wave][(lane >> 5 & 1) | (lane >> 4 & 1) << 1 | (lane >> 3 & 1) << 2 | (lane >> 2 & 1) << 3] = a[0];
      if (lane == 0) s_h[par][row][wave][2 * PN_DTMF_NF] = e;
    }
    __syncthreads();
    if (live && wave == 0) {
      uint4 *srow = state + (size_t)s * 6;
      uint32_t tail[8], rep[PN_DTMF_REPORT_WORDS];
      if (concealed) {
        const uint4 u4 = srow[4], u5 = srow[5];
        tail[0] = u4.x; tail[1] = u4.y; tail[2] = u4.z; tail[3] = u4.w; tail[4] = u5.x; tail[5] = u5.y; tail[6] = u5.z; tail[7] = u5.w;
        pn_dtmf_held(tail, rep);
      } else {
        float sums[2 * PN_DTMF_NF], P[PN_DTMF_NF];
        uint32_t prev[2 * PN_DTMF_NF];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint4 u = srow[q];
          prev[4 * q] = u.x; prev[4 * q + 1] = u.y; prev[4 * q + 2] = u.z; prev[4 * q + 3] = u.w;
        }
#pragma unroll
        for (int k = 0; k < 2 * PN_DTMF_NF; k++) sums[k] = s_h[par][row][0][k] + s_h[par][row][1][k];
        pn_dtmf_power(P_.rot, prev, sums, P);
        if (t == 0) {                                  // Cp, Sp = C, S: out of the registers before the decision needs any
#pragma unroll
          for (int q = 0; q < 4; q++) srow[q] = make_uint4(__float_as_uint(sums[4 * q]), __float_as_uint(sums[4 * q + 1]), __float_as_uint(sums[4 * q + 2]), __float_as_uint(sums[4 * q + 3]));
        }
        const uint4 u4 = srow[4], u5 = srow[5];
        tail[0] = u4.x; tail[1] = u4.y; tail[2] = u4.z; tail[3] = u4.w; tail[4] = u5.x; tail[5] = u5.y; tail[6] = u5.z; tail[7] = u5.w;
        pn_dtmf_decide(P_.v, P, s_h[par][row][0][2 * PN_DTMF_NF] + s_h[par][row][1][2 * PN_DTMF_NF], tail, rep);
        if (t == 0) { srow[4] = make_uint4(tail[0], tail[1], tail[2], tail[3]); srow[5] = make_uint4(tail[4], tail[5], tail[6], tail[7]); }
      }
      if (report && t == 0) report[s] = make_uint4(rep[0], rep[1], rep[2], rep[3]);
    }
  }
}

// the grid: a block per DT_ROWS rows up to PN_DTMF_MAX_BLOCKS (two blocks of 512 threads a CU at the kernel's register count, 256 CUs);
// beyond that a block makes further passes with its twiddles still in registers
void pn_launch_rate_dtmf(hipStream_t st, int n_rows, const int *d_ids, const int *d_on, const uint32_t *d_lost, uint32_t tick, const float *params, const float *rot16,
                         const float *d_tab, const float *x48, void *state, void *d_report) {
  if (n_rows <= 0) return;
  PnDtmfParams P;
  for (int i = 0; i < PN_DTMF_N_PARAMS; i++) P.v[i] = params[i];
  for (int i = 0; i < 2 * PN_DTMF_NF; i++) P.rot[i] = rot16[i];
  int blocks = (n_rows + DT_ROWS - 1) / DT_ROWS;
  if (blocks > PN_DTMF_MAX_BLOCKS) blocks = PN_DTMF_MAX_BLOCKS;
  hipLaunchKernelGGL(pn_rate_dtmf_kernel, dim3(blocks), dim3(DT_ROW_THREADS * DT_ROWS), 0, st, n_rows, d_ids, d_on, d_lost, tick, P,
                     reinterpret_cast<const float4 *>(d_tab), x48, reinterpret_cast<uint4 *>(state), reinterpret_cast<uint4 *>(d_report));
}
