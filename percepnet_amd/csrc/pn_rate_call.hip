// Call-state records of the rate converter for gfx950 (include/percepnet_hip.h "call-state records"; layout and verdict, stated once:
// pn_call_rules.h; host side pn_rate.cpp; numpy model tests/call_state_model.py): record i <-> the concealer's history, period and
// counters, the level control's and the limiter's four words and the held level of stream ids[i].  One kernel gathers and scatters,
// one block of four wavefronts per record.  A record is 665 groups of 16 bytes — the header and 664 of body — and every group has
// one 16-byte aligned source and destination (the level word apart): a history row is 120 groups, the period 180, and the ring's
// rotation moves whole rows, so thread t walks the groups t, t + 256, t + 512 with one 16-byte load and one 16-byte store each.
// `held`, the states the converter holds, is an argument and so the same in every block; the record's own mask is one word every
// thread of a block reads alike.  Every branch in front of a barrier is therefore the whole block's.
//   gather   the header with mask = held, the held sections — the ring in age order, 0 in the head word — and zeros elsewhere
//   scatter  the block ORs the 660 groups of hist and q when the record claims to have no PLC section (the one part of the verdict
//            that reads the bulk); thread 0 reads the sixteen words behind them and gives pn_call_verdict's verdict, the host
//            check's own, to status[i].  Behind the barrier a refused record leaves its stream exactly as it was — the other records
//            of the call are still imported (the contract of pn_rate_records_dev_kernel).  An accepted one, section by section:
//            present and held: written, the ring at head 0; held and absent: zeroed; present and not held: dropped
// No atomics; ids are distinct on scatter (the host refuses duplicates), so no two blocks write one stream.
#include "pn_launch.h"
#include "pn_call_rules.h"

#define CS_THREADS 256
#define CS_ROW_G (PN_FRAME / 4)                      // 120 groups per history row
#define CS_HIST_G (PN_PLC_HIST / 4)                  // 480
#define CS_Q_G (PN_PLC_P_MAX / 4)                    // 180
#define CS_BULK_G (CS_HIST_G + CS_Q_G)               // 660: hist and q
#define CS_BODY_G (PN_CALL_BODY_WORDS / 4)           // 664
#define CS_REC_G (PN_RATE_CALL_STATE_BYTES / 16)     // 665
static_assert(CS_BULK_G * 4 == PN_CALL_W_META && CS_BODY_G == CS_BULK_G + 4 && CS_REC_G == CS_BODY_G + 1 && PN_PLC_P_MAX % 4 == 0 && PN_FRAME % 4 == 0,
              "a record is a header group, 480 + 180 groups of hist and q and one group each of meta, AGC, limiter and level");

__global__ __launch_bounds__(CS_THREADS) void pn_rate_call_kernel(
    const int *__restrict__ ids,               // stream of record i
    uint32_t held,                             // PN_CALL_*: the states this converter holds; a pointer below is read only under its bit
    uint4 *__restrict__ hist,                  // [n_streams][4][120] groups
    uint4 *__restrict__ qbuf,                  // [n_streams][180]
    uint4 *__restrict__ meta,                  // [n_streams] P, r, lost frames, head
    uint4 *__restrict__ agc,                   // [n_streams]
    uint4 *__restrict__ lim,                   // [n_streams]
    uint32_t *__restrict__ level,              // [n_streams] one word
    uint4 *__restrict__ rec,                   // [n][665] groups
    int *__restrict__ status, int scatter) {
  const int t = threadIdx.x;
  const size_t s = (size_t)ids[blockIdx.x];
  uint4 *r = rec + (size_t)blockIdx.x * CS_REC_G;
  uint4 *body = r + 1;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  if (!scatter) {
    // the head of the ring: one word every thread reads alike (0 while the concealer is not held)
    const int head = (held & PN_CALL_PLC) ? (int)(meta[s].w & 3u) : 0;
    if (t == 0) r[0] = make_uint4(PN_RATE_CALL_MAGIC, PN_RATE_CALL_VERSION, PN_RATE_CALL_STATE_BYTES, held);
    for (int i = t; i < CS_BODY_G; i += CS_THREADS) {
      uint4 v = zero;
      if (i < CS_HIST_G) {
        if (held & PN_CALL_PLC) { const int j = i / CS_ROW_G, col = i - j * CS_ROW_G; v = hist[s * CS_HIST_G + ((head + j) & 3) * CS_ROW_G + col]; }
      } else if (i < CS_BULK_G) {
        if (held & PN_CALL_PLC) v = qbuf[s * CS_Q_G + (i - CS_HIST_G)];
      } else if (i == CS_BULK_G) {
        if (held & PN_CALL_PLC) { v = meta[s]; v.w = 0u; }
      } else if (i == CS_BULK_G + 1) {
        if (held & PN_CALL_AGC) v = agc[s];
      } else if (i == CS_BULK_G + 2) {
        if (held & PN_CALL_LIM) v = lim[s];
      } else if (held & PN_CALL_MIX) v.x = level[s];
      body[i] = v;
    }
    return;
  }

  const uint4 h = r[0];                               // (every thread: one line, broadcast)
  const uint32_t present = h.w;
  int bulk = 0;
  if (!(present & PN_CALL_PLC)) {                     // the record says "no PLC section": then hist and q must be all zero
    uint32_t any = 0u;
    for (int i = t; i < CS_BULK_G; i += CS_THREADS) { const uint4 v = body[i]; any |= v.x | v.y | v.z | v.w; }
    bulk = __syncthreads_or(any != 0u);
  }
  __shared__ int verdict;
  if (t == 0) {
    const uint4 a = body[CS_BULK_G], b = body[CS_BULK_G + 1], c = body[CS_BULK_G + 2], d = body[CS_BULK_G + 3];
    const uint32_t hw[PN_CALL_HEADER_WORDS] = {h.x, h.y, h.z, h.w};
    const uint32_t tw[PN_CALL_TAIL_WORDS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    verdict = pn_call_verdict(hw, tw, bulk != 0);
    status[blockIdx.x] = verdict;
  }
  __syncthreads();
  if (verdict != PN_SS_OK) return;
  for (int i = t; i < CS_BODY_G; i += CS_THREADS) {
    const uint32_t bit = i < CS_BULK_G + 1 ? PN_CALL_PLC : i == CS_BULK_G + 1 ? PN_CALL_AGC : i == CS_BULK_G + 2 ? PN_CALL_LIM : PN_CALL_MIX;
    if (!(held & bit)) continue;                      // not held by this converter: dropped
    const uint4 v = (present & bit) ? body[i] : zero; // held and absent: a fresh state
    if (i < CS_HIST_G) hist[s * CS_HIST_G + i] = v;   // record row j is ring row j: head 0
    else if (i < CS_BULK_G) qbuf[s * CS_Q_G + (i - CS_HIST_G)] = v;
    else if (i == CS_BULK_G) meta[s] = make_uint4(v.x, v.y, v.z, 0u);
    else if (i == CS_BULK_G + 1) agc[s] = v;
    else if (i == CS_BULK_G + 2) lim[s] = v;
    else level[s] = v.x;
  }
}

// held: the PN_CALL_* states of the converter; a state's pointers are read only under its bit.  scatter: d_status[i] receives record
// i's verdict, a refused record moves nothing
void pn_launch_rate_call_state(hipStream_t st, const int *d_ids, int n, uint32_t held, float *hist, float *q, void *meta, void *agc_state, void *lim_state,
                               float *level, void *rec, int *d_status, int scatter) {
  if (n <= 0) return;
  hipLaunchKernelGGL(pn_rate_call_kernel, dim3(n), dim3(CS_THREADS), 0, st, d_ids, held, reinterpret_cast<uint4 *>(hist), reinterpret_cast<uint4 *>(q),
                     reinterpret_cast<uint4 *>(meta), reinterpret_cast<uint4 *>(agc_state), reinterpret_cast<uint4 *>(lim_state),
                     reinterpret_cast<uint32_t *>(level), reinterpret_cast<uint4 *>(rec), d_status, scatter);
}
