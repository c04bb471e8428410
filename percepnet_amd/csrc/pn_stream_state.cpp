// State I/O of a batched context: the network state as host arrays in the reference's RNNState layout, and the per-stream state
// records (kernels: pn_stream_state.hip; rules: pn_host_rules.h), device and host forms.
#include "pn_context.h"

// ---- network state <-> host arrays in the reference's RNNState layout (nnet_data.h:28-38) ---------------------------
// The same walk as a record section: an entry's live slots, oldest first (the ks-1 previous layer inputs of a conv FIFO, the
// half of a GRU pair that the next step reads), one host row = live * cols floats.  host[i]: the i-th ring of the network
// (conv1, conv2, gru1..gru_gb, gru_rb, in table order), or NULL.
enum { PN_ST_NNET = 7 };
static int rnn_state_copy(pn_ctx *c, bool to_device, float *const host[PN_ST_NNET]) {
  PN_ON_DEVICE(c);
  if (pipe_drain(c)) return -1;
  // fp16-operand, split-precision and direct-operand contexts: the fp32 buffers are complete (every layer stores fp32 next to its
  // operand shadow), so a store reads them as in the plain fp32 mode and a load re-derives the shadows from the loaded fp32 values
  const size_t B = c->B;
  int split_rc = 0;
  for (int e = PN_ST_C1RING, i = 0; e <= PN_ST_RB; e++) {
    const PnStateEntry &L = pn_kState[e];
    if (L.cls != PN_CLS_RING) continue;
    float *const hrow = host[i++];
    const size_t hp = (size_t)L.live * L.cols * 4, dp = (size_t)L.row_words * 4, w = (size_t)L.cols * 4;
    for (int j = 0; hrow && j < L.live; j++) {
      float *d = state_at(c, e, j), *h = hrow + j * L.cols;
      PN_HIP_CHECK(to_device ? hipMemcpy2DAsync(d, dp, h, hp, w, B, hipMemcpyHostToDevice, c->stream)
                             : hipMemcpy2DAsync(h, hp, d, dp, w, B, hipMemcpyDeviceToHost, c->stream));
      if (to_device) split_rc |= reshadow(c, c->stream, e, d);
    }
  }
  PN_HIP_CHECK(hipStreamSynchronize(c->stream));
  return split_rc ? -1 : 0;                  // a refused shadow-operand split (pn_launch_split_x3) fails the call, like any refused launch
}
extern "C" int pn_ctx_set_rnn_state_host(pn_ctx *c, const float *conv1, const float *conv2, const float *gru1, const float *gru2,
                                         const float *gru3, const float *gru_gb, const float *gru_rb) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  float *h[PN_ST_NNET] = {(float *)conv1, (float *)conv2, (float *)gru1, (float *)gru2, (float *)gru3, (float *)gru_gb, (float *)gru_rb};
  return rnn_state_copy(c, true, h);
}
extern "C" int pn_ctx_get_rnn_state_host(pn_ctx *c, float *conv1, float *conv2, float *gru1, float *gru2, float *gru3,
                                         float *gru_gb, float *gru_rb) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  float *h[PN_ST_NNET] = {conv1, conv2, gru1, gru2, gru3, gru_gb, gru_rb};
  return rnn_state_copy(c, false, h);
}

// ---- per-stream state records (pn_stream_state.hip; layout in include/percepnet_hip.h; header and check in pn_host_rules.h) ----
extern "C" size_t pn_stream_state_bytes(void) { return PN_STREAM_STATE_BYTES; }
extern "C" int pn_stream_state_check(const void *record, size_t bytes, const pn_model *m) {
  if (!record || !m) { pn_set_error("NULL argument"); return PN_SS_BAD_ARG; }
  return ss_check_host(record, bytes, m->sha256);
}
static const unsigned char *ctx_digest(const pn_ctx *c) { return std::get<0>(c->weights_key).data(); }
static void ss_args(pn_ctx *c, PnStreamStateArgs &a) {
  memset(&a, 0, sizeof(a));
  state_sections(c, a.sec);
  a.last_gain = c->side.last_gain; a.last_period = c->side.last_period;
  ss_header(a.hdr, ctx_digest(c), c->nn_mode);
}

extern "C" int pn_ctx_export_streams(pn_ctx *c, const int32_t *ids, int n, void *d_records) {
  if (!c || n < 0 || (n > 0 && (!ids || !d_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if ((uintptr_t)d_records & 15) { pn_set_error("records must be 16-byte aligned"); return -1; }
  if (pn_ids_check(c->B, ids, n, false)) return -1;
  PN_ON_DEVICE(c);
  const int *d = stage_ids(c, ids, n);
  if (!d) return -1;
  PnStreamStateArgs a;
  ss_args(c, a);
  a.ids = d; a.rec = d_records;
  pn_launch_ss_gather(c->stream, a, n);
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int pn_ctx_import_streams(pn_ctx *c, const int32_t *ids, int n, const void *d_records, int32_t *d_status) {
  if (!c || n < 0 || (n > 0 && (!ids || !d_records || !d_status))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if ((uintptr_t)d_records & 15) { pn_set_error("records must be 16-byte aligned"); return -1; }
  if (pn_ids_check(c->B, ids, n, true)) return -1;
  PN_ON_DEVICE(c);
  const int *d = stage_ids(c, ids, n);
  if (!d) return -1;
  PnStreamStateArgs a;
  ss_args(c, a);
  a.ids = d; a.rec = const_cast<void *>(d_records); a.status = d_status;
  pn_launch_ss_scatter(c->stream, a, n);
  // operand shadows of the live entries, imported rows only (status 0), in this context's layout: fp16 / hi + lo planes of the
  // conv FIFOs and the GRU / rb states (shadow-operand modes), fp32 fragments of the GRU / rb states (direct-operand family)
  int rc = 0;
  for (int e = PN_ST_C1RING; e <= PN_ST_RB; e++)
    for (int j = 0; pn_kState[e].cls == PN_CLS_RING && j < pn_kState[e].live; j++) rc |= reshadow(c, c->stream, e, state_at(c, e, j), d, d_status, n);
  PN_HIP_CHECK(hipGetLastError());
  return rc ? -1 : 0;
}

int host_records_sync(pn_ctx *c, bool import, void *h_records, size_t bytes, const std::function<int(void *d_records)> &launch,
                      void *h_extra, size_t extra_bytes) {
  PN_ON_DEVICE(c);
  if (pipe_drain(c)) return -1;
  void *d = NULL;
  PN_HIP_CHECK(hipMalloc(&d, bytes + extra_bytes));
  int rc = 0;
  if (import && hipMemcpyAsync(d, h_records, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { pn_set_error("record copy failed"); rc = -1; }
  if (!rc) rc = launch(d);
  if (!rc && !import && hipMemcpyAsync(h_records, d, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) { pn_set_error("record copy failed"); rc = -1; }
  if (!rc && extra_bytes && hipMemcpyAsync(h_extra, static_cast<char *>(d) + bytes, extra_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) { pn_set_error("status copy failed"); rc = -1; }
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) { pn_set_error(import ? "import failed" : "export failed"); rc = -1; }
  hipFree(d);
  return rc;
}

// Host forms: synchronous, frames in flight on the pipelined path are completed first (like rnn_state_copy).  The records
// pass through a device buffer of their own size, freed before returning (host_records_sync).
extern "C" int pn_ctx_export_streams_host(pn_ctx *c, const int32_t *ids, int n, void *h_records) {
  if (!c || n < 0 || (n > 0 && (!ids || !h_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if (pn_ids_check(c->B, ids, n, false)) return -1;
  return host_records_sync(c, false, h_records, (size_t)n * PN_STREAM_STATE_BYTES, [&](void *d) { return pn_ctx_export_streams(c, ids, n, d); });
}
extern "C" int pn_ctx_import_streams_host(pn_ctx *c, const int32_t *ids, int n, const void *h_records) {
  if (!c || n < 0 || (n > 0 && (!ids || !h_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if (pn_ids_check(c->B, ids, n, true)) return -1;
  if (pn_records_check(h_records, n, PN_STREAM_STATE_BYTES, [&](const void *r, size_t b) { return ss_check_host(r, b, ctx_digest(c)); })) return -1;
  const size_t bytes = (size_t)n * PN_STREAM_STATE_BYTES;
  std::vector<int32_t> status(n, 0);
  int rc = host_records_sync(c, true, const_cast<void *>(h_records), bytes, [&](void *d) {
    return pn_ctx_import_streams(c, ids, n, d, reinterpret_cast<int32_t *>(static_cast<char *>(d) + bytes)); }, status.data(), (size_t)n * sizeof(int32_t));
  for (int i = 0; i < n && !rc; i++)
    if (status[i]) { pn_set_error("record %d refused on the device (%d) after passing the host check", i, status[i]); rc = -1; }
  return rc;
}
