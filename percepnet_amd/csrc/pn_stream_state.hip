// Per-stream state records (include/percepnet_hip.h, "per-stream state records"): gather the whole state of chosen streams
// into phase-free records, and scatter records into chosen streams of another context at ITS phase.
//
// Every per-stream buffer is a ring or a ping-pong pair indexed by the context's global counters, or in place
// (pn_state_layout.h: the table, the phases, and the check that the record offsets follow from the geometry).  Before the
// frame with counters (t, tn) runs, the live entries of a section sit, oldest first, in slots first, first + 1, ... (mod
// slots) — the host computes `first` per section, the kernels only walk it.  The dead slots of an imported row keep what they
// held: the frame kernels overwrite them before they read them.  Operand shadows are re-derived afterwards for the imported
// rows only, by the row-list forms of the split kernels (pn_launch_split_x3_rows, pn_launch_split_d_rows).
#include "pn_common.h"
#include "pn_launch.h"
#include "../../include/percepnet_hip.h"

#define SS_THREADS 256

// record word i of the body <-> float4 column (rec_off / 4 + e) of record i
__device__ __forceinline__ float4 *ss_body(void *rec, int i) {
  return reinterpret_cast<float4 *>(static_cast<char *>(rec) + (size_t)i * PN_STREAM_STATE_BYTES + PN_STREAM_STATE_HEADER_BYTES);
}

// rows ids[i] -> record i; one block per (record, section), the section's live entries walked oldest first as one flat
// range of float4 columns (each entry is a contiguous 144 B .. 3.2 KB run of the row)
__global__ __launch_bounds__(SS_THREADS) void pn_ss_gather_kernel(PnStreamStateArgs a) {
  const int i = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, s = a.ids[i];
  const PnSsSection S = a.sec[k];
  float4 *rec = ss_body(a.rec, i) + S.rec_off / 4;
  const float *row = S.base + (size_t)s * S.row_stride;
  const int c4 = S.cols / 4;
  for (int e = tid; e < S.live * c4; e += SS_THREADS) {
    const int j = e / c4, c = e - j * c4;
    const int slot = S.first + j < S.slots ? S.first + j : S.first + j - S.slots;
    rec[e] = reinterpret_cast<const float4 *>(row + (size_t)slot * S.slot_stride)[c];
  }
  if (k == 0 && tid < PN_STREAM_STATE_HEADER_BYTES / 4)
    reinterpret_cast<uint32_t *>(static_cast<char *>(a.rec) + (size_t)i * PN_STREAM_STATE_BYTES)[tid] = a.hdr[tid];
  if (k == PN_SS_NSEC - 1 && tid == 0) {                  // the tail rides with the last section (synth)
    uint32_t *tail = reinterpret_cast<uint32_t *>(ss_body(a.rec, i)) + PN_SS_TAIL;
    tail[0] = __float_as_uint(a.last_gain[s]); tail[1] = (uint32_t)a.last_period[s]; tail[2] = 0; tail[3] = 0;
  }
}

// PN_SS_OK or the PN_SS_BAD_* code of record i's header against the context's (magic, version, size, digest); the source's
// nn_mode (word 3) is informational
__device__ __forceinline__ int ss_check(const PnStreamStateArgs &a, int i) {
  const uint32_t *h = reinterpret_cast<const uint32_t *>(static_cast<const char *>(a.rec) + (size_t)i * PN_STREAM_STATE_BYTES);
  if (h[0] != a.hdr[0]) return PN_SS_BAD_MAGIC;
  if (h[1] != a.hdr[1]) return PN_SS_BAD_VERSION;
  if (h[2] != a.hdr[2]) return PN_SS_BAD_SIZE;
  for (int w = 4; w < 12; w++) if (h[w] != a.hdr[w]) return PN_SS_BAD_MODEL;
  return PN_SS_OK;
}

// record i -> row ids[i] at the context's phase (ids distinct: checked on the host).  A record whose header fails leaves its
// row untouched; block (i, 0) reports the verdict in status[i].
__global__ __launch_bounds__(SS_THREADS) void pn_ss_scatter_kernel(PnStreamStateArgs a) {
  const int i = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, s = a.ids[i];
  __shared__ int verdict;
  if (tid == 0) {
    verdict = ss_check(a, i);
    if (k == 0) a.status[i] = verdict;
  }
  __syncthreads();
  if (verdict != PN_SS_OK) return;
  const PnSsSection S = a.sec[k];
  const float4 *rec = ss_body(a.rec, i) + S.rec_off / 4;
  float *row = S.base + (size_t)s * S.row_stride;
  const int c4 = S.cols / 4;
  for (int e = tid; e < S.live * c4; e += SS_THREADS) {
    const int j = e / c4, c = e - j * c4;
    const int slot = S.first + j < S.slots ? S.first + j : S.first + j - S.slots;
    const float4 v = rec[e];
    reinterpret_cast<float4 *>(row + (size_t)slot * S.slot_stride)[c] = v;
    // history: the mirror of the ring's first 8 samples (unaligned comb-tap loads) follows slot 0 — written by the thread
    // that writes those columns (when slot 0 is the dead slot it is not written and its mirror stays right)
    if (k == 0 && slot == 0 && c < 2) reinterpret_cast<float4 *>(row)[PN_HIST / 4 + c] = v;
  }
  if (k == PN_SS_NSEC - 1 && tid == 0) {
    const uint32_t *tail = reinterpret_cast<const uint32_t *>(ss_body(a.rec, i)) + PN_SS_TAIL;
    a.last_gain[s] = __uint_as_float(tail[0]); a.last_period[s] = (int)tail[1];
  }
}

void pn_launch_ss_gather(hipStream_t st, const PnStreamStateArgs &a, int n) {
  if (n > 0) hipLaunchKernelGGL(pn_ss_gather_kernel, dim3(n, PN_SS_NSEC), dim3(SS_THREADS), 0, st, a);
}
void pn_launch_ss_scatter(hipStream_t st, const PnStreamStateArgs &a, int n) {
  if (n > 0) hipLaunchKernelGGL(pn_ss_scatter_kernel, dim3(n, PN_SS_NSEC), dim3(SS_THREADS), 0, st, a);
}
