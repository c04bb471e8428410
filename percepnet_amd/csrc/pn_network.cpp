// The gain network of a context: the shared device copy of a model's weights, the ten layers of compute_rnn (rnn.cpp:42-81)
// launched from the table of pn_network.h, and the row-range chains of large fp32 batches.
#include "pn_context.h"
#include <map>
#include <mutex>

// Device copy of a model's biases and (re-packed) weights, shared by every context of one (model content, device, network
// mode, narrow-layer packing): the reference binds all its states to ONE static model (denoise.cpp:49-51,267: a borrowed
// pointer, zero copies); here N contexts — N legacy rnnoise_create handles, the shards of a CLI run, a service that opens
// and closes contexts — share one 32 MB upload and one re-pack instead of N.  Reference-counted, freed with its last user.
struct SharedWeights {
  int refs = 0;
  DevLayer L[PN_NLAYERS];
  std::vector<void *> allocs;
  size_t bytes = 0;
};
static std::mutex g_weights_mu;                              // guards g_weights and every refs counter
static std::mutex g_weights_build_mu[16];                    // per device (mod 16): uploads and re-packs of DIFFERENT devices run
                                                             // side by side (percepnet_run --devices creates its contexts from one thread per device)
static std::map<WeightsKey, SharedWeights *> g_weights;

// into the shared weight copy under construction (uploads run on the creating context's stream)
static int upload_w(pn_ctx *c, SharedWeights *w, float **dst, const float *src, size_t n) {
  if (dev_alloc_into(w->allocs, w->bytes, c->stream, (void **)dst, n * sizeof(float), false)) return -1;
  PN_HIP_CHECK(hipMemcpyAsync(*dst, src, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// Biases + weights of `model` on the context's device in the format each layer's kernel reads (pn_network.h): STRICT the
// nnet_data.h arrays as they are, the MFMA modes re-packed tile orders (pn_pack.cpp, pn_nn_x3.hip).  NULL (pn_set_error) on failure.
static SharedWeights *build_weights(pn_ctx *c, const pn_model *model, int nn_mode, int narrow) {
  SharedWeights *w = new SharedWeights();
  memset(w->L, 0, sizeof(w->L));
  for (int li = 0; li < PN_NLAYERS; li++) {
    const PnLayerHost &H = model->L[li]; DevLayer &D = w->L[li];
    size_t nb, nw, nr; pn_layer_floats(H.kind, H.nin, H.nn, H.ks, &nb, &nw, &nr);
    const int fmt = pn_layer_weight_format(nn_mode, narrow, li), gru = H.kind == PN_KIND_GRU, np = pn_weight_planes(nn_mode);
    const int K = H.nin * H.ks, ncols = H.nn * (gru ? 3 : 1);
    // a packed array: its host copy dies with this scope, so the copy has executed when this returns
    auto put = [&](float **dst, const void *src, size_t n_floats) { return upload_w(c, w, dst, (const float *)src, n_floats) || hipStreamSynchronize(c->stream) != hipSuccess; };
    // one matrix (k rows, k_alloc swept; ctr: column-tile rounding of the layer's kernel) in the tile order of the layer's format
    auto pack = [&](float **dst, const float *W, int k, int k_alloc, int ctr, const char *what) {
      if (fmt != PN_WF_X3) {
        std::vector<float> f(pn_packed_floats(k_alloc, ncols, ctr));
        pn_pack_weights(W, k, k_alloc, ncols, ctr, f.data());
        return put(dst, f.data(), f.size());
      }
      std::vector<uint16_t> h(pn_packed_halfs_x3(k, ncols, ctr, np));
      if (pn_pack_weights_x3(W, k, k, ncols, ctr, np, h.data())) { pn_set_error("layer %d has a %sweight outside the fp16 range: the fp16-operand and split-precision modes cannot represent it", li, what); return true; }
      return put(dst, h.data(), h.size() / 2);
    };
    if (upload_w(c, w, &D.bias, H.bias, nb)) goto fail_w;
    if (fmt == PN_WF_RAW) {
      if (upload_w(c, w, &D.w, H.w, nw) || (nr && upload_w(c, w, &D.rw, H.rw, nr))) goto fail_w;
      continue;
    }
    if (pack(&D.wp, H.w, K, pn_net_k(li), pn_layer_ct_round(nn_mode, narrow, li), "")) goto fail_w;   // (fc sweeps the zero-padded feature panel)
    if (fmt == PN_WF_F32_N16) {
      std::vector<float> pq(pn_packed_floats_n16(K, ncols));
      pn_pack_weights_n16(H.w, K, ncols, pq.data());
      if (put(&D.wq, pq.data(), pq.size())) goto fail_w;
    }
    if (nr && pack(&D.rwp, H.rw, H.nn, H.nn, 1, "recurrent ")) goto fail_w;
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess) { pn_set_error("weight upload failed"); goto fail_w; }
  return w;
fail_w:
  hipStreamSynchronize(c->stream);
  for (void *p : w->allocs) hipFree(p);
  delete w;
  return NULL;
}

// the device copy of the weights: shared with every other context of this model content on this device in this mode
int weights_acquire(pn_ctx *c, const pn_model *model) {
  std::array<unsigned char, 32> dig; memcpy(dig.data(), model->sha256, 32);
  c->weights_key = std::make_tuple(dig, model->n_floats, c->device, c->nn_mode, c->plan.narrow);
  std::lock_guard<std::mutex> build_lk(g_weights_build_mu[c->device & 15]);   // one build per device at a time; the map lock is never held across a build
  {
    std::lock_guard<std::mutex> lk(g_weights_mu);
    auto it = g_weights.find(c->weights_key);
    if (it != g_weights.end()) { c->weights = it->second; c->weights->refs++; c->weights_were_cached = true; }
  }
  if (!c->weights) {
    SharedWeights *w = build_weights(c, model, c->nn_mode, c->plan.narrow);
    if (!w) return -1;
    w->refs = 1; c->weights = w;
    std::lock_guard<std::mutex> lk(g_weights_mu);
    g_weights[c->weights_key] = w;
  }
  memcpy(c->L, c->weights->L, sizeof(c->L));
  c->weight_bytes = c->weights->bytes;
  return 0;
}
void weights_release(pn_ctx *c) {
  std::lock_guard<std::mutex> lk(g_weights_mu);
  if (!c->weights || --c->weights->refs) return;
  for (void *p : c->weights->allocs) hipFree(p);
  g_weights.erase(c->weights_key);
  delete c->weights;
}

// ---- the per-frame launch sequence -----------------------------------------------------------------------
// the launchers of a kernel kind (pn_network.h: pn_kKernelRule names the same forms)
static constexpr struct { PnLayerLauncher *dense, *gru; } kLaunchers[] = {
    {pn_launch_dense_strict, pn_launch_gru_strict}, {pn_launch_dense, pn_launch_gru}, {pn_launch_dense, NULL}, {pn_launch_dense_small, pn_launch_gru_small},
    {pn_launch_dense_n16, NULL}, {pn_launch_dense_n48, NULL}, {pn_launch_dense_x3, pn_launch_gru_x3}, {NULL, pn_launch_gru_d}};
constexpr bool launchers_match_rules() {
  for (int k = 0; k < PN_K_COUNT; k++)
    if ((kLaunchers[k].dense != nullptr) != (pn_kKernelRule[k].dense != nullptr) || (kLaunchers[k].gru != nullptr) != (pn_kKernelRule[k].gru != nullptr)) return false;
  return true;
}
static_assert(sizeof(kLaunchers) / sizeof(kLaunchers[0]) == PN_K_COUNT && launchers_match_rules(), "one launcher per form of every kernel kind (pn_kKernelRule)");

int reshadow(pn_ctx *c, hipStream_t st, int e, const float *p, const int *d_ids, const int *d_status, int n) {
  void *S = shadow_at(c, e, p); const int w = pn_kState[e].cols, np = pn_weight_planes(c->nn_mode);
  if (!S) return 0;
  if (pn_mode_x3(c->nn_mode)) return d_ids ? pn_launch_split_x3_rows(st, p, w, w, S, d_ids, d_status, n, np) : pn_launch_split_x3(st, p, w, w, S, (int)c->Bp, np);
  return d_ids ? pn_launch_split_d_rows(st, p, w, w, S, d_ids, d_status, n) : pn_launch_split_d(st, p, w, w, S, (int)c->Bp);   // the direct-operand family
}

// Returns 0, or -1 when a launcher refused its geometry (pn_set_error names it): the refused layer is not launched (later
// layers of the frame may be — their results are never reported) and the caller fails the frame.
// The ten layers for the rows [r0, r0 + nrows) of the batch on stream `st`.  Every activation buffer is row-major, so a row range
// is the same launch with every base pointer moved down by r0 rows.  Wiring, kernel and shadows of each layer are pn_network.h's,
// under c->plan.  The shadow-operand and STRICT modes always run the whole batch.
static int launch_rnn_rows(pn_ctx *c, size_t r0, size_t nrows, hipStream_t st) {
  const bool strict = c->nn_mode == PN_NN_STRICT;
  int rc = 0;
  for (int li = 0; li < PN_NLAYERS; li++) {
    const PnNetLayer &R = pn_kNet[li]; const DevLayer &W = c->L[li];
    const int k = pn_layer_kernel(c->plan, c->nn_mode, li), fmt = pn_kernel_weight_format(k); const bool gru = R.state >= 0;
    if (rc && R.fam == KF_GRU512) continue;   // gru1 -> gru2 -> gru3 -> gru_gb, each fed the UPDATED state of its predecessor: the sequence stops at a refusal
    // every chain's launches are bracketed on the stream they go to (pn_ctx_kernel_times averages over all launches of a family;
    // with N chains the launches of one family overlap in time: bench.py prices the CONCURRENT launches together)
    Scope sc(c, R.fam, st);
    PnLayerLaunch L = {};
    PnSegs &A = L.A, &S = L.S; A.n = S.n = R.n_in;     // the input panels, and their operand shadows for the kernels that read those
    for (int j = 0; j < R.n_in; j++) {
      const int e = R.in[j].entry;
      A.p[j] = state_at(c, e, R.in[j].j, r0); A.ld[j] = S.ld[j] = pn_kState[e].row_words; A.width[j] = S.width[j] = pn_kState[e].cols;
      S.p[j] = reinterpret_cast<const float *>(shadow_at(c, e, A.p[j]));
    }
    if (li == PN_L_FC && strict) A.width[0] = pn_kGeom[li].nin;               // (the MFMA kernels sweep the zero-padded panel: cols 70..127 are zero)
    if (li == PN_L_FC && c->inject_bad_launch && !strict) A.width[0] = 96;     // test hook: three K-tiles, which every MFMA dense launcher refuses
    L.bias = W.bias;
    L.w = fmt == PN_WF_RAW ? W.w : (fmt == PN_WF_F32_N16 ? W.wq : W.wp); L.rw = fmt == PN_WF_RAW ? W.rw : W.rwp;
    L.N = pn_kGeom[li].nn; L.act = c->geom[li].act; L.tansig = c->tansig;
    L.out = state_at(c, R.out.entry, R.out.j, r0) + R.out_col; L.ldo = pn_kState[R.out.entry].row_words;
    L.outS = pn_kernel_writes_shadow(k) ? shadow_at(c, R.out.entry, L.out) : NULL;       // (fc_gb's output keeps none)
    L.nts_out = L.outS ? pn_kState[R.out.entry].cols / 32 : 0;                           // column tiles of the output's shadow
    if (gru) { L.h_old = state_at(c, R.state, 0, r0); L.h_oldS = shadow_at(c, R.state, L.h_old); }   // GRU pairs: live half read, the other written
    L.n_rows = (int)nrows; L.rg = c->plan.rg; L.np = pn_weight_planes(c->nn_mode);
    PnLayerLauncher *launch = gru ? kLaunchers[k].gru : kLaunchers[k].dense;
    rc |= launch ? launch(st, L) : pn_kernel_geometry_ok(k, gru, A.n, A.width, L.N);   // (no such form: the rule's refusal says so)
    // an output whose entry keeps a shadow that the kernel does not write: fc in the shadow-operand modes runs in fp32 (70 inputs),
    // its output enters the shadow-operand layers
    if (!pn_kernel_writes_shadow(k)) rc |= reshadow(c, st, R.out.entry, L.out);
  }
  return rc ? -1 : 0;
}

// compute_rnn for the whole batch.  Large fp32 MFMA contexts run it as ROW-RANGE CHAINS (round 6, round-5 verdict item 3).
// The batch-GEMM kernels run in rounds of 512 co-resident blocks (two per CU) — 4096 rows of a 512-wide layer, 65 536 rows of a
// 34-wide one — and on ONE in-order stream every layer pays whole rounds: 65 536 streams = 16 rounds per 512-wide layer, 66 048 = 17
// (+0.45 ms per frame; the reference has no such step, its cost is per stream: nnet.cpp:120-180), and even an exact fit leaves the
// ramp and drain of ten launches idle.  No layer mixes rows, so the batch is cut into PN_NN_CHAINS row ranges (multiples of 128
// rows) whose ten layers are independent chains of the SAME kernels on streams of their own: while one chain drains a layer the
// blocks of another fill the slots.  One fork (the features are ready) and one join (before the back end) per frame; results
// are bit-identical by construction (the same launches over sub-ranges of the rows).  The chain count and the shares are
// pn_plan.h's (measured: profiles/r06_row_chains.log).
// The first attempts — the rows past the last whole round on the small-batch kernels, in the same stream or beside the body —
// cost 2-3x the tail's share: a small block holds a block slot for a single latency-bound MFMA chain, and any slot taken from
// an exactly fitting body pushes that layer into an extra round.
// Every extra chain's stream must have a HARDWARE queue of its own: HIP multiplexes the streams of one priority over a few queues,
// and on a queue shared with the context's stream a chain runs in front of the others instead of beside them.  Same remedy as for
// the copy streams of the pipelined host path: default-priority streams PROBED against the streams they must not share a queue
// with, a high-priority one as the fallback (pipe_make_stream).
int chain_streams_init(pn_ctx *c) {
  int lo = 0, hi = 0;
  PN_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  for (int k = 1; k < c->plan.chains; k++) {
    if (pipe_make_stream(c, &c->chain_stream[k], 'a', hi, 'h', busy_streams(c), &c->chain_kind[k])) return -1;
    PN_HIP_CHECK(hipEventCreateWithFlags(&c->chain_join[k], hipEventDisableTiming));
  }
  PN_HIP_CHECK(hipEventCreateWithFlags(&c->chain_fork, hipEventDisableTiming));
  return 0;
}
// hipSuccess, or the error recorded as the frame's (pn_set_error) unless an earlier one already is
static bool chain_ok(hipError_t e, const char *what, int &rc) {
  if (e == hipSuccess) return true;
  if (!rc) pn_set_error("%s failed: %s", what, hipGetErrorString(e));
  rc = -1;
  return false;
}
int launch_rnn(pn_ctx *c) {
  const int n = c->plan.chains;
  if (n <= 1) return launch_rnn_rows(c, 0, c->B, c->stream);
  const size_t B = c->B, share = pn_plan_share(c->plan, B);
  PN_HIP_CHECK(hipEventRecord(c->chain_fork, c->stream));                 // the front end's features (and last frame's state) are in place
  // Once forked, every chain that started is joined back into the context's stream whatever fails after it (a refused launch,
  // a HIP error): nothing stays unordered.  No chain starts after a failure; the first error is the one returned.
  int rc = 0;
  bool started[PN_MAX_CHAINS] = {};
  for (int k = n - 1; k >= 0 && !rc; k--) {                               // the context's own stream last: the others are already queued
    const size_t r0 = share * k, nr = r0 >= B ? 0 : (B - r0 < share ? B - r0 : share);
    if (!nr) continue;
    hipStream_t st = k ? c->chain_stream[k] : c->stream;
    if (k && !(started[k] = chain_ok(hipStreamWaitEvent(st, c->chain_fork, 0), "hipStreamWaitEvent(chain, fork)", rc))) break;
    if (launch_rnn_rows(c, r0, nr, st)) rc = -1;
  }
  for (int k = 1; k < n; k++)
    if (started[k] && chain_ok(hipEventRecord(c->chain_join[k], c->chain_stream[k]), "hipEventRecord(join)", rc))
      chain_ok(hipStreamWaitEvent(c->stream, c->chain_join[k], 0), "hipStreamWaitEvent(stream, join)", rc);
  return rc;
}
