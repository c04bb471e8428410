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
void pn_launch_rate_conf_stamp(hipStream_t st, const int *d_ids, int n, uint32_t *d_stamp, uint32_t tick) {
  if (n <= 0) return;
  hipLaunchKernelGGL(pn_rate_conf_stamp_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_ids, n, d_stamp, tick);
}
void pn_launch_rate_conf_rows(hipStream_t st, const int *d_touched, const int *d_rows, int k, int *d_members) {
  if (k <= 0) return;
  hipLaunchKernelGGL(pn_rate_conf_rows_kernel, dim3((k * MX_MAX + 255) / 256), dim3(256), 0, st, d_touched, d_rows, k, d_members);
}
