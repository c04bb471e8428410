// The conference mix of the rate converter for gfx950 (include/percepnet_hip.h "conferences"; host side pn_rate.cpp; the table's
// rules pn_conf.h): between the engine and the down-conversion every stream of a conference gets the sum of the OTHER members'
// 48 kHz rows ("mix-minus"), a stream without a conference gets its own row, bit for bit.
//   o[s][j] = sum of y[m][j] over the members m != s of s's conference that advance this frame, m ascending,
//             acc = +0.0f, acc = acc + y[m][j]: plain fp32 adds in one order that depends on slots only — no atomics, no cross-lane
//             sums — so a row is the same in every batch size and block and numpy float32 reproduces it (tests/conf_model.py).
// One block of two wavefronts per listed row (a contiguous eighth of the rows per group of blocks that share an XCD); thread
// t < 120 owns the float4 of columns 4t..4t+3, so every access is 16 bytes and a wave reads and writes whole 128-byte lines.  The block of a stream without a conference copies the row.  The block of a
// conference's LEADER — its lowest member that advances — does the whole conference; the blocks of the other members read the
// 128-byte member row, see that they do not lead, and leave.  The leader's threads fetch each member's float4 ONCE into registers
// and then write every listener's row from them, so a member row is read once from memory however many listeners it has.
//   Which members advance: without an id list all of them; with one, those whose stamp word equals this call's tick — the
//   stamp kernel below writes the tick at the listed streams in front of the mix, from the staged id list, so no host pass over
//   the streams is needed and an unlisted (stale) row is never read.
//   The member list lives in lanes 0..31 of each wave (one coalesced load); a ballot of "advances" gives the leader (its lowest
//   bit) and the count k; the k active slots are pulled into scalars with readlane, ascending.
//   Registers, not LDS, and no dynamically indexed array: the body is unrolled over the size classes K = 2, 4, 8, 16, 32 (the
//   smallest K >= k), with the K - k missing members as +0.0f.  That padding is exact: acc starts at +0.0f and a sum of two
//   floats is -0.0f only when both are, so acc is never -0.0f and acc + (+0.0f) == acc for every acc, NaN and inf included.
//   Listener i's sum shares its first i terms with the running prefix p_i = ((0 + y0) + y1) + .. + y(i-1) — the same adds in the
//   same order — and goes on from there over the members behind i.
// Memory-bound by construction: per stream 1920 B in and 1920 B out, k (k - 1) / 2 float4 adds per thread for a conference of k.
#include "pn_launch.h"
#include "../../include/percepnet_hip.h"      // PN_CONF_MAX_MEMBERS

#define MX_THREADS 128
#define MX_COLS (PN_FRAME / 4)                // 120 float4 per row
#define MX_MAX PN_CONF_MAX_MEMBERS
static_assert(PN_FRAME % 4 == 0 && MX_COLS <= MX_THREADS && MX_MAX == 32, "a thread per float4 of a row; the member row fits the low half of a wave");

__device__ __forceinline__ float4 mx_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// One conference of k <= K advancing members; mask: their positions in the member row, member: the row, in lanes 0..31.
template <int K>
__device__ __forceinline__ void mx_conference(int col, int k, uint32_t mask, int member, const float *__restrict__ in48, float *__restrict__ out48) {
  int mem[K];                                  // the advancing members, ascending; wave-uniform
#pragma unroll
  for (int j = 0; j < K; j++) {
    const int bit = __builtin_amdgcn_readfirstlane(mask ? __builtin_ctz(mask) : 0);
    mem[j] = j < k ? __builtin_amdgcn_readlane(member, bit) : -1;
    mask &= mask - 1;
  }
  float4 v[K];
#pragma unroll
  for (int j = 0; j < K; j++)
    v[j] = j < k ? reinterpret_cast<const float4 *>(in48 + (size_t)mem[j] * PN_FRAME)[col] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int i = 0; i < K; i++) {
    if (i < k) {
      float4 acc = p;
#pragma unroll
      for (int m = i + 1; m < K; m++) acc = mx_add(acc, v[m]);
      reinterpret_cast<float4 *>(out48 + (size_t)mem[i] * PN_FRAME)[col] = acc;
    }
    p = mx_add(p, v[i]);
  }
}

__global__ __launch_bounds__(MX_THREADS) void pn_rate_mix_kernel(
    int n_rows, const int *__restrict__ ids,   // rows to run; ids == NULL: row w is stream w
    const int *__restrict__ conf,              // [n_streams] the conference of every stream, -1: none.  NULL: nobody is in one
    const int *__restrict__ members,           // [n_streams][32] row c: the members of conference c, ascending, then -1
    const uint32_t *__restrict__ stamp,        // [n_streams] == tick: the stream advances this frame (read only with an id list)
    uint32_t tick,
    const float *__restrict__ in48,            // [n_streams][480]
    float *__restrict__ out48) {               // [n_streams][480], no row shared with in48
  const int col = threadIdx.x, lane = threadIdx.x & 63;
  // block -> row: blocks whose numbers agree mod 8 share an XCD, and the leaders of conferences of neighbouring slots sit at
  // multiples of the conference size — taken row = block, the leaders of conferences of 8 and more would all run on ONE of the
  // eight XCDs.  So the eight groups each take a contiguous eighth of the rows.  (Speed only: any placement gives the same rows.)
  const int chunk = (n_rows + 7) >> 3;
  const int w = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
  if (col >= MX_COLS || w >= n_rows) return;                         // (no barrier below)
  const int s = __builtin_amdgcn_readfirstlane(ids ? ids[w] : w);
  const int c = __builtin_amdgcn_readfirstlane(conf ? conf[s] : -1);
  if (c < 0) {
    reinterpret_cast<float4 *>(out48 + (size_t)s * PN_FRAME)[col] = reinterpret_cast<const float4 *>(in48 + (size_t)s * PN_FRAME)[col];
    return;
  }
  int member = -1;
  bool adv = false;
  if (lane < MX_MAX) {
    member = members[(size_t)c * MX_MAX + lane];
    adv = member >= 0 && (!ids || stamp[member] == tick);
  }
  const uint32_t mask = (uint32_t)__ballot(adv);                     // (lanes 32..63 vote 0)
  if (!mask) return;                                                 // (a table the host wrote always lists s itself)
  if (__builtin_amdgcn_readlane(member, __builtin_amdgcn_readfirstlane(__builtin_ctz(mask))) != s) return;   // another member's block leads
  const int k = __builtin_popcount(mask);
  if (k <= 2) mx_conference<2>(col, k, mask, member, in48, out48);
  else if (k <= 4) mx_conference<4>(col, k, mask, member, in48, out48);
  else if (k <= 8) mx_conference<8>(col, k, mask, member, in48, out48);
  else if (k <= 16) mx_conference<16>(col, k, mask, member, in48, out48);
  else mx_conference<32>(col, k, mask, member, in48, out48);
}

// ---- the mix with loudest-N selection, send gains and the mix report -------------------------------------------------------------
// include/percepnet_hip.h "conferences: loudest-N talkers, send gains, mix report"; the rules for the host pn_mix_rules.h; the numpy
// model tests/mix_sel_model.py.  Launched instead of the kernel above while any of those settings is off its default (pn_rate.cpp
// rate_mix); same row mapping, leader block and stamps.  What the leader block does for its conference:
//   1  gain and previous level of every member come into lanes 0..31 beside the member row; TALKERS = advancing members with g != 0
//   2  every talker's float4 is loaded once and scaled, x = g * y (a muted member's row is never read), K = 2 .. 32 as above
//   3  level: thread t forms the group sum ((((0 + x0 x0) + x1 x1) + x2 x2) + x3 x3) of its columns 4t..4t+3 (threads 120..127: +0),
//      each wave folds its 64 group sums by the xor butterfly 32, 16, .., 1 — IEEE adds commute, so every lane ends with the same
//      bits — and E = wave 0's sum + wave 1's through LDS.  Every thread of the block reaches the barrier: all leave decisions in
//      front of it are block-uniform, and the threads without a column stay as zero contributors
//   4  hold and selection in lanes 0..31 (both waves compute the same): L from E and the previous level, key = bits(L) & 0x7fffffff,
//      each lane counts the talkers ahead of it with 32 readlane compares; a ballot of "selected" is the mask.  Wave 0 writes L back
//   5  the rows of the talkers that were NOT selected become +0.0 and the prefix scheme of the kernel above runs unchanged: adding
//      +0.0 to an accumulator that starts at +0.0 is exact (it is never -0.0), so listener i gets the sum of the selected talkers
//      m != i, m ascending; a muted member gets the whole sum, the prefix behind the last talker
//   6  the report: peak and clipped count of every written row — a max and an integer sum, free of ordering — per wave by shuffles,
//      across the two waves through LDS behind a second barrier (taken by every thread, or by none when the report is off)
#define MXS_MUTED 32                          // the LDS slot of the row every muted member hears
// Timing aid (tools/rate_conf_times.py with PERCEPNET_LIB at a build.build_variant library): parts of the leader's
// work left out, with WRONG rows as the result — 1: the level sums and their shuffles, 2: the barrier behind them and the LDS
// exchange, 4: the ranking loop.  0 in every build that ships
#ifndef PN_MXS_ABLATE
#define PN_MXS_ABLATE 0
#endif

__device__ __forceinline__ float mxs_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ void mxs_row_report(float4 a, int wave, int lane, int slot, float (*s_pk)[MX_MAX + 1], int (*s_cl)[MX_MAX + 1]) {
  const float e[4] = {a.x, a.y, a.z, a.w};
  float peak = 0.f;
  int clipped = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float t = e[i] * 32768;
    peak = fmaxf(peak, fabsf(e[i]));                                  // (a NaN sample is ignored, as in the frame report)
    clipped += !(t > -32769.f && t < 32768.f);                        // NaN counts
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { peak = fmaxf(peak, __shfl_xor(peak, m)); clipped = clipped + __shfl_xor(clipped, m); }
  if (lane == 0) { s_pk[wave][slot] = peak; s_cl[wave][slot] = clipped; }
}

// One conference of k <= K talkers; tmask: their positions in the member row, amask: the positions of the members that advance
template <int K>
__device__ __forceinline__ void mxs_conference(int col, int k, uint32_t tmask, uint32_t amask, int member, float gain, float prev, int cap, float hold,
                                               const float *__restrict__ in48, float *__restrict__ out48, float *__restrict__ level, uint4 *__restrict__ report,
                                               float (*s_lvl)[MX_MAX], float (*s_pk)[MX_MAX + 1], int (*s_cl)[MX_MAX + 1]) {
  const int lane = col & 63, wave = col >> 6;
  const bool has_col = col < MX_COLS;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 v[K];
  uint32_t m = tmask;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const int bit = __builtin_amdgcn_readfirstlane(m ? __builtin_ctz(m) : 0);
    m &= m - 1;
    v[j] = zero;
    if (j < k) {
      const int mem = __builtin_amdgcn_readlane(member, bit);
      const float g = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gain), bit));
      if (has_col) {
        const float4 y = reinterpret_cast<const float4 *>(in48 + (size_t)mem * PN_FRAME)[col];
        v[j] = make_float4(g * y.x, g * y.y, g * y.z, g * y.w);
      }
    }
  }
  m = tmask;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const int bit = __builtin_amdgcn_readfirstlane(m ? __builtin_ctz(m) : 0);
    m &= m - 1;
    if (j < k && !(PN_MXS_ABLATE & 1)) {
      float e = 0.0f;
      e = e + v[j].x * v[j].x; e = e + v[j].y * v[j].y; e = e + v[j].z * v[j].z; e = e + v[j].w * v[j].w;
      e = mxs_wave_sum(e);
      if (lane == 0) s_lvl[wave][bit] = e;
    }
  }
  if (!(PN_MXS_ABLATE & 2)) __syncthreads();
  const bool talker = lane < MX_MAX && ((tmask >> (lane & 31)) & 1u);
  const bool adv = lane < MX_MAX && ((amask >> (lane & 31)) & 1u);
  float L = 0.0f;
  if (talker) {
    const float E = (PN_MXS_ABLATE & 2) ? (float)lane : s_lvl[0][lane] + s_lvl[1][lane], h = hold * prev;
    const bool finite = (__float_as_uint(h) & 0x7f800000u) != 0x7f800000u;
    L = (hold != 0.0f && finite && h > E) ? h : E;
  }
  const int key = (int)(__float_as_uint(L) & 0x7fffffffu);             // (non-negative as an int: int compares are the unsigned ones)
  int ahead = 0;
#pragma unroll
  for (int q = 0; q < ((PN_MXS_ABLATE & 4) ? 0 : MX_MAX); q++) {
    const int kq = __builtin_amdgcn_readlane(key, q);
    if ((tmask >> q) & 1u) ahead += (kq > key || (kq == key && q < lane)) ? 1 : 0;
  }
  const bool sel = talker && (cap == 0 || ahead < cap);
  const uint32_t smask = (uint32_t)__ballot(sel);
  if (wave == 0 && adv) level[member] = L;                            // (+0.0 for a muted member)
  m = tmask;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const int bit = __builtin_amdgcn_readfirstlane(m ? __builtin_ctz(m) : 0);
    m &= m - 1;
    if (j >= k || !((smask >> bit) & 1u)) v[j] = zero;
  }
  float4 p = zero;
  m = tmask;
#pragma unroll
  for (int i = 0; i < K; i++) {
    const int bit = __builtin_amdgcn_readfirstlane(m ? __builtin_ctz(m) : 0);
    m &= m - 1;
    if (i < k) {
      float4 acc = p;
#pragma unroll
      for (int q = i + 1; q < K; q++) acc = mx_add(acc, v[q]);
      if (has_col) reinterpret_cast<float4 *>(out48 + (size_t)__builtin_amdgcn_readlane(member, bit) * PN_FRAME)[col] = acc;
      if (report) mxs_row_report(acc, wave, lane, bit, s_pk, s_cl);
    }
    p = mx_add(p, v[i]);
  }
  uint32_t muted = amask & ~tmask;
  if (muted && report) mxs_row_report(p, wave, lane, MXS_MUTED, s_pk, s_cl);
  while (muted) {
    const int bit = __builtin_amdgcn_readfirstlane(__builtin_ctz(muted));
    muted &= muted - 1;
    if (has_col) reinterpret_cast<float4 *>(out48 + (size_t)__builtin_amdgcn_readlane(member, bit) * PN_FRAME)[col] = p;
  }
  if (!report) return;                                                // (a kernel argument: the whole block or nobody)
  __syncthreads();
  if (wave == 0 && adv) {
    const int slot = talker ? lane : MXS_MUTED;
    const float peak = fmaxf(s_pk[0][slot], s_pk[1][slot]);
    const int clipped = s_cl[0][slot] + s_cl[1][slot];
    report[member] = make_uint4(__float_as_uint(L), (sel ? 1u : 0u) | (talker ? 0u : 2u) | 4u, __float_as_uint(peak), (uint32_t)clipped);
  }
}

#ifdef PN_MXS_WAVES                           // timing aid: ask for this many waves per SIMD (the default build takes what 210 VGPRs give: 2)
__attribute__((amdgpu_waves_per_eu(PN_MXS_WAVES, PN_MXS_WAVES)))
#endif
__global__ __launch_bounds__(MX_THREADS) void pn_rate_mix_sel_kernel(
    int n_rows, const int *__restrict__ ids, const int *__restrict__ conf, const int *__restrict__ members, const uint32_t *__restrict__ stamp, uint32_t tick,
    const float *__restrict__ in48, float *__restrict__ out48,       // as above
    const float *__restrict__ gains,           // [n_streams] send gains, finite and >= +0.0
    const int *__restrict__ caps,              // [n_streams] N_c by conference number, 0: everybody
    float *__restrict__ level,                 // [n_streams] L, the only state
    float hold,                                // d
    uint4 *__restrict__ report) {              // [n_streams] mix report records, NULL: off
  __shared__ float s_lvl[2][MX_MAX];
  __shared__ float s_pk[2][MX_MAX + 1];
  __shared__ int s_cl[2][MX_MAX + 1];
  const int col = threadIdx.x, lane = threadIdx.x & 63;
  const int chunk = (n_rows + 7) >> 3;
  const int w = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
  if (w >= n_rows) return;                                           // every leave in front of a barrier is the whole block's
  const int s = __builtin_amdgcn_readfirstlane(ids ? ids[w] : w);
  const int c = __builtin_amdgcn_readfirstlane(conf ? conf[s] : -1);
  if (c < 0) {
    if (col < MX_COLS) reinterpret_cast<float4 *>(out48 + (size_t)s * PN_FRAME)[col] = reinterpret_cast<const float4 *>(in48 + (size_t)s * PN_FRAME)[col];
    if (report && col == 0) report[s] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  int member = -1;
  bool adv = false;
  if (lane < MX_MAX) {
    member = members[(size_t)c * MX_MAX + lane];
    adv = member >= 0 && (!ids || stamp[member] == tick);
  }
  const uint32_t amask = (uint32_t)__ballot(adv);                    // (the same in both waves: they read the same words)
  if (!amask) return;
  if (__builtin_amdgcn_readlane(member, __builtin_amdgcn_readfirstlane(__builtin_ctz(amask))) != s) return;   // another member's block leads
  // only the leader fetches gains, levels and the cap (fetched by every block in front of the leader decision, a round trip
  // earlier, the kernel measured 9 % SLOWER at conferences of 32: 63 of 64 blocks then load what they drop)
  float gain = 0.0f, prev = 0.0f;
  if (adv) { gain = gains[member]; prev = level[member]; }
  const uint32_t tmask = (uint32_t)__ballot(adv && gain != 0.0f);
  const int cap = __builtin_amdgcn_readfirstlane(caps[c]);
  const int k = __builtin_popcount(tmask);
#define MXS_ARGS col, k, tmask, amask, member, gain, prev, cap, hold, in48, out48, level, report, s_lvl, s_pk, s_cl
  if (k <= 2) mxs_conference<2>(MXS_ARGS);
  else if (k <= 4) mxs_conference<4>(MXS_ARGS);
  else if (k <= 8) mxs_conference<8>(MXS_ARGS);
  else if (k <= 16) mxs_conference<16>(MXS_ARGS);
  else mxs_conference<32>(MXS_ARGS);
#undef MXS_ARGS
}

// stamp[ids[i]] = tick, i < n: the streams of this frame's id list
__global__ void pn_rate_conf_stamp_kernel(const int *__restrict__ ids, int n, uint32_t *__restrict__ stamp, uint32_t tick) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) stamp[ids[i]] = tick;
}
// A change of the table (pn_rate_set_stream_confs): member row touched[i] = rows[i][0..32), i < k; the conference of every listed
// stream is written by pn_rate_set_factors_kernel in front of it, both in stream order.
__global__ void pn_rate_conf_rows_kernel(const int *__restrict__ touched, const int *__restrict__ rows, int k, int *__restrict__ members) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < k * MX_MAX) members[(size_t)touched[t / MX_MAX] * MX_MAX + (t % MX_MAX)] = rows[t];
}

void pn_launch_rate_mix(hipStream_t st, int n_rows, const int *d_ids, const int *d_conf, const int *d_members, const uint32_t *d_stamp, uint32_t tick,
                        const float *in48, float *out48) {
  if (n_rows <= 0) return;
  hipLaunchKernelGGL(pn_rate_mix_kernel, dim3(8 * ((n_rows + 7) / 8)), dim3(MX_THREADS), 0, st, n_rows, d_ids, d_conf, d_members, d_stamp, tick, in48, out48);
}
void pn_launch_rate_mix_sel(hipStream_t st, int n_rows, const int *d_ids, const int *d_conf, const int *d_members, const uint32_t *d_stamp, uint32_t tick,
                            const float *in48, float *out48, const float *d_gains, const int *d_caps, float *d_level, float hold, void *d_report) {
  if (n_rows <= 0) return;
  hipLaunchKernelGGL(pn_rate_mix_sel_kernel, dim3(8 * ((n_rows + 7) / 8)), dim3(MX_THREADS), 0, st, n_rows, d_ids, d_conf, d_members, d_stamp, tick, in48, out48,
                     d_gains, d_caps, d_level, hold, reinterpret_cast<uint4 *>(d_report));
}
void pn_launch_rate_conf_stamp(hipStream_t st, const int *d_ids, int n, uint32_t *d_stamp, uint32_t tick) {
  if (n <= 0) return;
  hipLaunchKernelGGL(pn_rate_conf_stamp_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_ids, n, d_stamp, tick);
}
void pn_launch_rate_conf_rows(hipStream_t st, const int *d_touched, const int *d_rows, int k, int *d_members) {
  if (k <= 0) return;
  hipLaunchKernelGGL(pn_rate_conf_rows_kernel, dim3((k * MX_MAX + 255) / 256), dim3(256), 0, st, d_touched, d_rows, k, d_members);
}
