// Comfort noise of the rate converter for gfx950 (include/percepnet_hip.h "comfort noise"; the rule, stated once with every rounding:
// pn_cng_rules.h, whose sample function this kernel calls; host side pn_rate.cpp; numpy model tests/cng_model.py): in front of the
// up-conversion, it writes the row of every silent stream AT THE STREAM'S OWN RATE into a converter-owned buffer strided like an input
// row, from which the unchanged up kernels of pn_rate.hip take it on.
// The lattice is sequential in time — up to 480 samples of up to 24 dependent fp32 operations — so the parallelism is across streams:
// ONE LANE PER STREAM over a compacted list, one wavefront per block.  The lane keeps b[12] and k[12] in registers (the lattice loop is
// unrolled over the order with the stream's M as a predicate, so every index is a constant and nothing goes to scratch); the
// excitation is a hash of the sample counter and does not depend on the lattice.
// A lane writing a row of its own would put 64 scattered 4-byte stores into every instruction.  Instead the wave stages a TILE of
// PN_CNG_TILE = 80 samples x 64 streams in LDS and then writes it out cooperatively: the tile's 5120 words in flat order, 64 consecutive
// words per store instruction, which are 256 contiguous bytes of one row or the end of one and the start of the next.  80 because it is
// the row of 8000 Hz and divides the rows of all five rates (80, 160, 240, 320, 480): no stream has a partial tile, a converter of 8000 Hz
// runs one tile and leaves the loop, and 64 x 81 words are 20.7 KB, so a CU's 160 KB of LDS holds seven blocks, more than one wave per
// SIMD, while a store instruction still covers two whole 128-byte lines.  Rows are padded to 81 words: lane l writes word 81 l + j, bank (17 l + j) mod 64, all different; the read
// side walks consecutive words with one step of 2 where the row changes, one two-way conflict at the most.
// On a mixed converter the lanes of a wave have different n_s and M.  The tile loop runs while ANY lane has samples left — the bound is the
// wave's, so both barriers of a tile are reached by all 64 lanes — and a lane whose row is complete, or that lies behind the list's end,
// generates nothing and stores nothing; what the cooperative store needs of the other lanes' streams (slot, n_s) goes through LDS.
// Plain vector stores, no atomics; a row depends on the stream's own state, its SID and its slot, so it is the same in every batch size.
#include "pn_launch.h"
#include "pn_cng_rules.h"
#include "pn_rate_design.h"

#define CN_LANES 64
#define CN_PAD (PN_CNG_TILE + 1)
static_assert(CN_LANES * PN_CNG_TILE % CN_LANES == 0 && PN_CNG_PARAM_WORDS == 16 && PN_CNG_STATE_WORDS == 16, "a tile is a whole number of stores; four uint4 of SID, four of state");

__global__ __launch_bounds__(CN_LANES) void pn_rate_cng_kernel(
    int n_rows, const int *__restrict__ ids,   // the compacted list of silent streams, distinct
    const int *__restrict__ cont,              // [n_rows] != 0: the row continues a run
    const int *__restrict__ factors, int ns1,  // [n_streams] the factor of every stream (mixed), or NULL and the converter's own n_s
    uint32_t seed,
    const uint4 *__restrict__ sid,             // [n_streams][4] decoded SIDs: k[12], g, M, 0, 0
    uint4 *__restrict__ state,                 // [n_streams][4] b[12], counter, prev, run, total
    float *__restrict__ out, int stride,       // [n_streams][stride] rows at the streams' own rates
    uint4 *__restrict__ report) {              // [n_streams] CNG report records, NULL: off
  __shared__ float s_tile[CN_LANES][CN_PAD];
  __shared__ int s_slot[CN_LANES], s_ns[CN_LANES];
  const int lane = threadIdx.x, w = (int)blockIdx.x * CN_LANES + lane;
  const bool live = w < n_rows;
  int s = -1, ns = 0, M = 0;
  float k[PN_CNG_MAX_ORDER], b[PN_CNG_MAX_ORDER], g = 0.0f, p0 = 0.0f;
  uint32_t ctr = 0u, run = 0u, total = 0u, key = 0u;
#pragma unroll
  for (int i = 0; i < PN_CNG_MAX_ORDER; i++) { k[i] = 0.0f; b[i] = 0.0f; }
  if (live) {
    s = ids[w];
    ns = factors ? pn_rate_factor_frame(factors[s]) : ns1;
    const uint4 k0 = sid[4 * (size_t)s], k1 = sid[4 * (size_t)s + 1], k2 = sid[4 * (size_t)s + 2], k3 = sid[4 * (size_t)s + 3];
    const uint4 b0 = state[4 * (size_t)s], b1 = state[4 * (size_t)s + 1], b2 = state[4 * (size_t)s + 2], b3 = state[4 * (size_t)s + 3];
    k[0] = __uint_as_float(k0.x); k[1] = __uint_as_float(k0.y); k[2] = __uint_as_float(k0.z); k[3] = __uint_as_float(k0.w);
    k[4] = __uint_as_float(k1.x); k[5] = __uint_as_float(k1.y); k[6] = __uint_as_float(k1.z); k[7] = __uint_as_float(k1.w);
    k[8] = __uint_as_float(k2.x); k[9] = __uint_as_float(k2.y); k[10] = __uint_as_float(k2.z); k[11] = __uint_as_float(k2.w);
    b[0] = __uint_as_float(b0.x); b[1] = __uint_as_float(b0.y); b[2] = __uint_as_float(b0.z); b[3] = __uint_as_float(b0.w);
    b[4] = __uint_as_float(b1.x); b[5] = __uint_as_float(b1.y); b[6] = __uint_as_float(b1.z); b[7] = __uint_as_float(b1.w);
    b[8] = __uint_as_float(b2.x); b[9] = __uint_as_float(b2.y); b[10] = __uint_as_float(b2.z); b[11] = __uint_as_float(b2.w);
    g = __uint_as_float(k3.x); M = min(max((int)k3.y, 0), PN_CNG_MAX_ORDER);
    ctr = b3.x; run = b3.z; total = b3.w;
    p0 = cont[w] ? __uint_as_float(b3.y) : g;
    key = pn_cng_key(seed, (uint32_t)s);
  }
  s_slot[lane] = s; s_ns[lane] = ns;
  for (int t0 = 0; t0 < PN_FRAME; t0 += PN_CNG_TILE) {
    const bool mine = t0 < ns;
    if (__ballot(mine) == 0ull) break;                 // (the wave's verdict: every lane leaves here together)
    if (mine)
      for (int j = 0; j < PN_CNG_TILE; j++) s_tile[lane][j] = pn_cng_sample(k, M, g, p0, t0 + j, ns, ctr + (uint32_t)(t0 + j), key, b);
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < PN_CNG_TILE; i++) {
      const int idx = i * CN_LANES + lane, r = idx / PN_CNG_TILE, c = idx - r * PN_CNG_TILE;
      const int sr = s_slot[r];
      if (sr >= 0 && t0 < s_ns[r]) out[(size_t)sr * stride + t0 + c] = s_tile[r][c];
    }
    __syncthreads();
  }
  if (!live) return;
  run = cont[w] ? pn_cng_count(run) : 1u; total = pn_cng_count(total); ctr += (uint32_t)ns;
  state[4 * (size_t)s] = make_uint4(__float_as_uint(b[0]), __float_as_uint(b[1]), __float_as_uint(b[2]), __float_as_uint(b[3]));
  state[4 * (size_t)s + 1] = make_uint4(__float_as_uint(b[4]), __float_as_uint(b[5]), __float_as_uint(b[6]), __float_as_uint(b[7]));
  state[4 * (size_t)s + 2] = make_uint4(__float_as_uint(b[8]), __float_as_uint(b[9]), __float_as_uint(b[10]), __float_as_uint(b[11]));
  state[4 * (size_t)s + 3] = make_uint4(ctr, __float_as_uint(g), run, total);
  if (report) report[s] = make_uint4(run, total, __float_as_uint(g), ctr);
}

// decoded SIDs into the table: row i of rows[n][16] to stream ids[i]
__global__ void pn_rate_cng_sid_kernel(const int *__restrict__ ids, const uint32_t *__restrict__ rows, int n, uint32_t *__restrict__ sid) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n * PN_CNG_PARAM_WORDS) return;
  sid[(size_t)ids[i / PN_CNG_PARAM_WORDS] * PN_CNG_PARAM_WORDS + i % PN_CNG_PARAM_WORDS] = rows[i];
}

void pn_launch_rate_cng(hipStream_t st, int n_rows, const int *d_ids, const int *d_cont, const int *d_factors, int ns, uint32_t seed, const void *d_sid, void *state,
                        float *out, int stride, void *d_report) {
  if (n_rows <= 0) return;
  hipLaunchKernelGGL(pn_rate_cng_kernel, dim3((n_rows + CN_LANES - 1) / CN_LANES), dim3(CN_LANES), 0, st, n_rows, d_ids, d_cont, d_factors, ns, seed,
                     reinterpret_cast<const uint4 *>(d_sid), reinterpret_cast<uint4 *>(state), out, stride, reinterpret_cast<uint4 *>(d_report));
}
void pn_launch_rate_cng_sids(hipStream_t st, const int *d_ids, const int *d_rows, int n, void *d_sid) {
  if (n <= 0) return;
  const int words = n * PN_CNG_PARAM_WORDS;
  hipLaunchKernelGGL(pn_rate_cng_sid_kernel, dim3((words + 255) / 256), dim3(256), 0, st, d_ids, reinterpret_cast<const uint32_t *>(d_rows), n, reinterpret_cast<uint32_t *>(d_sid));
}
