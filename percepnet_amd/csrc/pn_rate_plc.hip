// Packet-loss concealment of the rate converter for gfx950 (include/percepnet_hip.h "packet-loss concealment"; the signal rule, stated
// once with every summation order: pn_plc_rules.h; host side pn_rate.cpp; numpy model tests/plc_model.py): between the up-conversion
// and the engine, in place on the 48 kHz rows.  A received row goes into the stream's history; a lost row is filled with a
// pitch-synchronous repetition of the history that fades to silence; the first received row after a loss is cross-faded out of it.
// One block of two wavefronts per listed row, mapped like the mix kernel (pn_rate_mix.hip: a contiguous eighth of the rows per
// group of blocks that share an XCD); thread t < 120 owns the float4 of columns 4t..4t+3, so a row moves in 16-byte accesses and
// whole 128-byte lines.  The stream's case — received / lost, r == 0 / r > 0 — comes from two words every thread of the block reads
// alike, so every branch below, and every barrier behind one, is the whole block's.
//   received, r == 0   the row is read once and written once, into the oldest history row; 16 bytes of meta each way.  Nothing else
//   lost, r == 0       the four history rows come into LDS in their linear order; the search runs there:
//       coarse  d[k] = hist[6k+5] is copied out first, so that the lagged reads d[k - l] of the 81 lag threads are CONSECUTIVE words
//               (64 banks: no conflict) and d[k] is one word for all (a broadcast); read in place at stride 6 the same loop would hit
//               every bank twice.  Thread t < 81 owns lag 40 + t and sums its 160 terms in ascending k, the order of the rule
//       fine    thread (i, j), i < 11 lags, j < 8 parts, sums the 120 terms k = 960 + 8 it + j in ascending it: in one step the 88
//               threads read 8 consecutive words hist[k] and 18 consecutive words hist[k - L]; equal addresses broadcast.  The
//               eight parts of a lag are added in ascending j by ONE thread through LDS
//       best    every thread walks the scores in LDS in ascending lag (broadcast reads): the sequential rule itself, no cross-lane
//               reduction whose order would need stating
//       period  q into LDS and into the state
//   lost, r > 0 and received, r > 0   q comes from the state into LDS; the row is g(m) q[m mod P], or the cross-fade into the real row
// No atomics; a row depends on the stream's own state and nothing else, so it is the same in every batch size and block.
#include "pn_launch.h"
#include "pn_plc_rules.h"

#define PL_THREADS 128
#define PL_COLS (PN_FRAME / 4)                 // 120 float4 per row
#define PL_NCOARSE (PN_PLC_LAG_HI - PN_PLC_LAG_LO + 1)   // 81
static_assert(PL_COLS <= PL_THREADS && PL_NCOARSE <= 96 && PN_PLC_HIST - PN_PLC_P_MAX - PN_PLC_P_MAX / 4 >= PN_PLC_P_MAX && PN_PLC_FINE_MAX * PN_PLC_FINE_PARTS <= PL_THREADS && PN_PLC_P_MAX % 4 == 0,
              "a thread per float4 of a row, per coarse lag, per (fine lag, part)");

__device__ __forceinline__ float pl_gain(int m) {     // pn_plc_gain_host
  if (m < PN_PLC_FADE_START) return 1.0f;
  if (m >= PN_PLC_FADE_END) return 0.0f;
  return (float)(PN_PLC_FADE_END - m) / (float)(PN_PLC_FADE_END - PN_PLC_FADE_START);
}
__device__ __forceinline__ float pl_score(float c, float e) {   // pn_plc_score
  if (!(c > 0.0f && e > 0.0f)) return 0.0f;
  const float cc = c * c, s = cc / e;
  return s == s ? s : 0.0f;
}
__device__ __forceinline__ int pl_best(const float *score, int n) {   // pn_plc_best; score in LDS, the same walk in every thread
  float best = 0.0f;
  int at = 0;
  for (int i = 0; i < n; i++) {
    const float v = score[i];
    if (v > best) { best = v; at = i; }
  }
  return at;
}
__device__ __forceinline__ float pl_syn(const float *q, int P, uint32_t r, int n) {   // pn_plc_syn_host; q in LDS
  if (r >= (uint32_t)(PN_PLC_FADE_END / PN_FRAME) || P < PN_PLC_P_MIN) return 0.0f;   // (a run without a lag: no state the kernel writes)
  const int m = PN_FRAME * (int)r + n;
  return pl_gain(m) * q[m % P];
}

__global__ __launch_bounds__(PL_THREADS) void pn_rate_plc_kernel(
    int n_rows, const int *__restrict__ ids,   // rows to run; ids == NULL: row w is stream w
    const uint32_t *__restrict__ lost, uint32_t tick,   // [n_streams] == tick: the stream's frame is lost
    float *__restrict__ x48,                   // [n_streams][480], in place
    float *__restrict__ hist,                  // [n_streams][4][480]
    float *__restrict__ qbuf,                  // [n_streams][720]
    uint4 *__restrict__ meta,                  // [n_streams] P, r, lost frames, head
    uint4 *__restrict__ report) {              // [n_streams] PLC report records, NULL: off
  // 10 KB a block, so that LDS leaves room for 16 blocks on a CU (the blocks of received streams use none of it, and they are the
  // many).  s_q lies on s_hist[0..720): the period is formed from hist[1920 - P - P/4 ..] >= hist[1020] when the search, whose
  // lagged reads go down to hist[240], is over — a barrier stands between — and a block that loads q from the state has no history
  __shared__ __attribute__((aligned(16))) float s_hist[PN_PLC_HIST];
  float *const s_q = s_hist;
  __shared__ float s_d[PN_PLC_COARSE_N];
  __shared__ float s_score[96];
  __shared__ float s_pc[PN_PLC_FINE_MAX][PN_PLC_FINE_PARTS], s_pe[PN_PLC_FINE_MAX][PN_PLC_FINE_PARTS];
  const int t = threadIdx.x;
  const int chunk = (n_rows + 7) >> 3;
  const int w = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
  if (w >= n_rows) return;                                           // every leave in front of a barrier is the whole block's
  const int s = __builtin_amdgcn_readfirstlane(ids ? ids[w] : w);
  const bool has_col = t < PL_COLS;
  float4 *xrow = reinterpret_cast<float4 *>(x48 + (size_t)s * PN_FRAME);
  // the row is fetched beside the two words that say what to do with it, not behind them: a received stream's block is three
  // dependent round trips otherwise, and at 65 536 streams the launch is bound by that chain, not by bytes.  (A lost stream's row
  // is stale memory of the same buffer; it is fetched and dropped.)
  float4 xv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (has_col) xv = xrow[t];
  const uint32_t lost_word = lost[s];                                // (in front of the meta words: the two fetches overlap)
  const uint4 mt = meta[s];
  int P = __builtin_amdgcn_readfirstlane((int)mt.x);
  const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)mt.y);
  const uint32_t n_lost = (uint32_t)__builtin_amdgcn_readfirstlane((int)mt.z);
  const int head = __builtin_amdgcn_readfirstlane((int)mt.w) & 3;
  const bool is_lost = (uint32_t)__builtin_amdgcn_readfirstlane((int)lost_word) == tick;
  float4 *hrow = reinterpret_cast<float4 *>(hist + (size_t)s * PN_PLC_HIST);
  float4 *newest = hrow + head * PL_COLS;                            // the oldest row: the one this frame's row replaces

  if (!is_lost && r == 0) {                                          // ---- received: into the history
    if (has_col) newest[t] = xv;
    __syncthreads();                                                 // both waves have read the meta words this one replaces
    if (t == 0) {
      meta[s] = make_uint4((uint32_t)P, 0u, n_lost, (uint32_t)((head + 1) & 3));
      if (report) report[s] = make_uint4(0u, (uint32_t)P, 0u, n_lost);
    }
    return;
  }

  if (is_lost && r == 0) {                                           // ---- the first lost frame: the lag and the period
    if (has_col) {
#pragma unroll
      for (int j = 0; j < 4; j++) reinterpret_cast<float4 *>(s_hist)[j * PL_COLS + t] = hrow[((head + j) & 3) * PL_COLS + t];
    }
    __syncthreads();
    for (int k = t; k < PN_PLC_COARSE_N; k += PL_THREADS) s_d[k] = s_hist[6 * k + 5];
    __syncthreads();
    if (t < PL_NCOARSE) {
      const int l = PN_PLC_LAG_LO + t;
      float c = 0.0f, e = 0.0f;
      for (int k = PN_PLC_COARSE_K0; k < PN_PLC_COARSE_N; k++) {
        const float a = s_d[k], b = s_d[k - l];
        const float pc = a * b, pe = b * b;
        c = c + pc; e = e + pe;
      }
      s_score[t] = pl_score(c, e);
    }
    __syncthreads();
    const int l = PN_PLC_LAG_LO + pl_best(s_score, PL_NCOARSE);
    const int lo = 6 * l - 5 < PN_PLC_P_MIN ? PN_PLC_P_MIN : 6 * l - 5, hi = 6 * l + 5 > PN_PLC_P_MAX ? PN_PLC_P_MAX : 6 * l + 5;
    const int nf = hi - lo + 1;
    __syncthreads();                                                 // s_score is written again below
    {
      const int i = t >> 3, j = t & 7;
      if (i < nf) {
        const int L = lo + i;
        float c = 0.0f, e = 0.0f;
        for (int k = PN_PLC_FINE_K0 + j; k < PN_PLC_HIST; k += PN_PLC_FINE_PARTS) {
          const float a = s_hist[k], b = s_hist[k - L];
          const float pc = a * b, pe = b * b;
          c = c + pc; e = e + pe;
        }
        s_pc[i][j] = c; s_pe[i][j] = e;
      }
    }
    __syncthreads();
    if (t < nf) {
      float c = s_pc[t][0], e = s_pe[t][0];
#pragma unroll
      for (int j = 1; j < PN_PLC_FINE_PARTS; j++) { c = c + s_pc[t][j]; e = e + s_pe[t][j]; }
      s_score[t] = pl_score(c, e);
    }
    __syncthreads();
    P = lo + pl_best(s_score, nf);
    const int O = P / 4;
    float *qrow = qbuf + (size_t)s * PN_PLC_P_MAX;
    for (int i = t; i < P; i += PL_THREADS) {
      const float a = s_hist[PN_PLC_HIST - P + i];
      float v = a;
      if (i >= P - O) {
        const float b = s_hist[PN_PLC_HIST - 2 * P + i], wq = ((float)(i - (P - O)) + 0.5f) / (float)O, dba = b - a, tq = wq * dba;
        v = a + tq;
      }
      s_q[i] = v;
      qrow[i] = v;
    }
  } else {                                                           // ---- a loss goes on, or ends: the period from the state
    const float4 *qrow = reinterpret_cast<const float4 *>(qbuf + (size_t)s * PN_PLC_P_MAX);
    for (int i = t; i < PN_PLC_P_MAX / 4; i += PL_THREADS) reinterpret_cast<float4 *>(s_q)[i] = qrow[i];
  }
  __syncthreads();

  if (has_col) {
    const int n0 = 4 * t;
    float4 v = make_float4(pl_syn(s_q, P, r, n0), pl_syn(s_q, P, r, n0 + 1), pl_syn(s_q, P, r, n0 + 2), pl_syn(s_q, P, r, n0 + 3));
    if (!is_lost) {                                                  // the first received row after a loss
      const float4 real = xv;
      if (n0 < PN_PLC_XFADE) {
        const float sy[4] = {v.x, v.y, v.z, v.w}, re[4] = {real.x, real.y, real.z, real.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float wx = (float)(2 * (n0 + j) + 1) / (float)(2 * PN_PLC_XFADE), d = re[j] - sy[j], tx = wx * d;
          o[j] = sy[j] + tx;
        }
        v = make_float4(o[0], o[1], o[2], o[3]);
      } else {
        v = real;
      }
    }
    xrow[t] = v;
    newest[t] = v;
  }
  if (t == 0) {
    const uint32_t r1 = is_lost ? (r < PN_PLC_RUN_MAX ? r + 1 : r) : 0u, nl = n_lost + (is_lost ? 1u : 0u);
    meta[s] = make_uint4((uint32_t)P, r1, nl, (uint32_t)((head + 1) & 3));
    if (report) {
      const uint32_t flags = is_lost ? (PN_PLC_CONCEALED | (r >= (uint32_t)(PN_PLC_FADE_END / PN_FRAME) ? PN_PLC_SILENT : 0u)) : PN_PLC_CROSSFADE;
      report[s] = make_uint4(flags, (uint32_t)P, r1, nl);
    }
  }
}

void pn_launch_rate_plc(hipStream_t st, int n_rows, const int *d_ids, const uint32_t *d_lost, uint32_t tick, float *x48, float *hist, float *q,
                        void *meta, void *d_report) {
  if (n_rows <= 0) return;
  hipLaunchKernelGGL(pn_rate_plc_kernel, dim3(8 * ((n_rows + 7) / 8)), dim3(PL_THREADS), 0, st, n_rows, d_ids, d_lost, tick, x48, hist, q,
                     reinterpret_cast<uint4 *>(meta), reinterpret_cast<uint4 *>(d_report));
}
