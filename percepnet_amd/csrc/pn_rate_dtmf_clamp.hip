// DTMF removal of the rate converter for gfx950 (include/percepnet_hip.h "DTMF removal"; the rule, stated once: pn_dtmf_clamp_rules.h;
// host side pn_rate.cpp; numpy model tests/dtmf_clamp_model.py): behind the engine and in front of the level control, in place on y48.
// Almost every row of a frame is at unity gain, so the cost is the DECISION, not the audio, and the kernel is shaped for that:
//   decide   one THREAD per listed row: it reads the stream's switch word, the detector's report row and its own 16 bytes of state as
//            uint4 — consecutive threads read consecutive 16-byte words where the rows are in stream order, a gather through ids
//            otherwise — runs the scalar rule (pn_dtmf_clamp_decide: the one text of pn_dtmf_clamp_rules.h) and writes state and report
//            back.  A row at unity gain ends here: 32 bytes read, up to 32 written, no audio touched
//   write    the rows that need writing are found by BALLOT: each wave walks over the set bits of its own 64 decisions, lowest first,
//            and works through such a row TOGETHER — the stream and the kind come from the deciding lane, the wave covers the row's 120
//            float4 in two steps of 64 lanes.  Zeros are stored without a load (a NaN in a removed row is gone), a ramp is one load,
//            four products and one store per float4
// A wave works on the rows its own lanes decided: no LDS, no barrier, no atomics, nothing depends on an order between waves or blocks.
// A row depends on its stream's own report row and state alone, so it is the same in every batch size, block and list position.
// A stream whose switch is off costs the read of its switch word (and a zero report row while the report is on).
#include "pn_launch.h"
#include "pn_dtmf_clamp_rules.h"

#define DC_THREADS 256                         // rows per block
#define DC_COLS (PN_FRAME / 4)                 // 120 float4 per row
static_assert(PN_FRAME % 4 == 0 && DC_COLS <= 128 && DC_THREADS % 64 == 0, "a row is two steps of a wave's 64 float4");

__global__ __launch_bounds__(DC_THREADS) void pn_rate_dtmf_clamp_kernel(
    int n_rows, const int *__restrict__ ids,   // rows to run; ids == NULL: row w is stream w
    const int *__restrict__ on,                // [n_streams] 0: removal is off for the stream
    PnDtmfClampParams P,
    const uint4 *__restrict__ det,             // [n_streams] the detector's report rows of this frame; NULL: detection is off for everybody
    float *__restrict__ y48,                   // [n_streams][480], in place
    uint4 *__restrict__ state,                 // [n_streams] marks, cut, muted, previous dur
    uint4 *__restrict__ report) {              // [n_streams] removal report records, NULL: off
  const int w = (int)blockIdx.x * DC_THREADS + (int)threadIdx.x, lane = (int)threadIdx.x & 63;
  int s = 0, kind = PN_DTMF_CLAMP_KEEP;
  if (w < n_rows) {
    s = ids ? ids[w] : w;
    if (on[s] == 0) {
      if (report) report[s] = make_uint4(0u, 0u, 0u, 0u);
    } else {
      const uint4 u = state[s], d = det ? det[s] : make_uint4(0u, 0u, 0u, 0u);
      uint32_t st[PN_DTMF_CLAMP_STATE_WORDS] = {u.x, u.y, u.z, u.w}, dr[PN_DTMF_REPORT_WORDS] = {d.x, d.y, d.z, d.w}, rep[PN_DTMF_CLAMP_REPORT_WORDS];
      kind = pn_dtmf_clamp_decide(P.v, st, dr, rep);
      state[s] = make_uint4(st[0], st[1], st[2], st[3]);
      if (report) report[s] = make_uint4(rep[0], rep[1], rep[2], rep[3]);
    }
  }
  // the wave's rows that need writing, lowest lane first; todo is the same in every lane of the wave
  unsigned long long todo = __ballot(kind != PN_DTMF_CLAMP_KEEP);
  while (todo) {
    const int from = __ffsll(todo) - 1;
    todo &= todo - 1ull;
    const int rs = __shfl(s, from), rk = __shfl(kind, from);
    float4 *row = reinterpret_cast<float4 *>(y48 + (size_t)rs * PN_FRAME);
#pragma unroll
    for (int q = lane; q < DC_COLS; q += 64) {
      if (rk == PN_DTMF_CLAMP_ZERO) row[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      else {
        const float4 v = row[q];
        const int j = 4 * q;
        row[q] = make_float4(pn_dtmf_clamp_sample(rk, v.x, j), pn_dtmf_clamp_sample(rk, v.y, j + 1), pn_dtmf_clamp_sample(rk, v.z, j + 2), pn_dtmf_clamp_sample(rk, v.w, j + 3));
      }
    }
  }
}

void pn_launch_rate_dtmf_clamp(hipStream_t st, int n_rows, const int *d_ids, const int *d_on, const int32_t *params, const void *d_det_report, float *y48,
                               void *state, void *d_report) {
  if (n_rows <= 0) return;
  PnDtmfClampParams P;
  for (int i = 0; i < PN_DTMF_CLAMP_N_PARAMS; i++) P.v[i] = params[i];
  hipLaunchKernelGGL(pn_rate_dtmf_clamp_kernel, dim3((n_rows + DC_THREADS - 1) / DC_THREADS), dim3(DC_THREADS), 0, st, n_rows, d_ids, d_on, P,
                     reinterpret_cast<const uint4 *>(d_det_report), y48, reinterpret_cast<uint4 *>(state), reinterpret_cast<uint4 *>(d_report));
}
