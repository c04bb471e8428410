// Private to the host side of libpercepnet_hip: a batched context and the few helpers its files share — pn_context.cpp (lifecycle,
// settings, the frame's launch sequence, active set), pn_selftest.cpp (the create-time self-tests), pn_host_pipe.cpp (pipelined
// host-buffer path, host-thread helpers), pn_stream_state.cpp (RNN-state and stream-state I/O) and pn_network.cpp (shared weights,
// the ten-layer launch loop, row-range chains).  The training-feature generator (pn_featgen.cpp) shares the allocator, the table
// upload and the device preamble; the rate converter (pn_rate.cpp) the id ring, the host form of a record transfer and the pipelined
// path's frame (pipe_submit).
#pragma once
#include <array>
#include <functional>
#include <tuple>
#include <vector>
#include "pn_host_rules.h"   // the id-list rule, the record-header rule
#include "pn_launch.h"       // pn_common.h, pn_network.h (plan, state table, DSP side, kernel families), the public header

struct SharedWeights;             // pn_network.cpp
// SHA-256 of the model content (pn_model_from_sources: arrays + activations + reset_after), array length, device, nn_mode, narrow
// layers packed for the n16 kernel.  The digest IS the identity: no host copy of the model is kept and nothing is compared byte for
// byte on a hit (round 5 kept 32 MB per entry and memcmp'ed it under the build lock).
typedef std::tuple<std::array<unsigned char, 32>, size_t, int, int, int> WeightsKey;

struct pn_ctx {
  int device, B, nn_mode;
  PnPlan plan;                     // the kernel families (pn_plan.h), fixed at creation
  size_t Bp;                       // B rounded up to the largest GEMM M tile (256): row count of every network buffer
  hipStream_t stream; bool own_stream;
  hipStream_t chain_stream[4] = {nullptr, nullptr, nullptr, nullptr};      // launch_rnn (pn_network.cpp): streams of the row-range chains 1..3 (chain 0 = stream), created with the context
  hipEvent_t chain_fork = nullptr, chain_join[4] = {nullptr, nullptr, nullptr, nullptr};
  char chain_kind[5] = {'-', '-', '-', '-', 0};   // how each chain stream was obtained (n: default priority, probed; h: priority stream)
  int64_t t;                       // frames done: the counter of the DSP rings (pn_state_layout.h)
  int64_t tn;                      // network steps done: the counter of the conv FIFOs and the GRU pairs.
                                   // == t unless pn_ctx_compute_rnn_host advanced the network on its own (rnn.cpp:42 is
                                   // callable on an RNNState without a DenoiseState in the reference too)
  size_t bytes;
  PnLayerHost geom[PN_NLAYERS];
  DevLayer L[PN_NLAYERS];           // = weights->L (pointers into the shared copy)
  SharedWeights *weights = NULL; WeightsKey weights_key; bool weights_were_cached = false; size_t weight_bytes = 0;   // (of the shared copy)
  // a list of stream ids on the device, and a ring of pinned host copies (the H2D copy runs when the stream gets to it —
  // frames may be in flight — so its source must outlive the call; slot k is reused once its copy has executed)
  struct IdRing { int *d = NULL; int cap = 0; unsigned calls = 0; struct { int *h = NULL; hipEvent_t ev = nullptr; } slot[4]; };
  IdRing ids;                      // pn_ctx_reset_streams, pn_ctx_set_atten_limit, stream-state export / import
  // pn_process_*_active: the inactive rows (a ring of its own: a reset's list may still be in flight) and the save area of the
  // in-place state of those rows, grown on demand
  struct Active {
    IdRing ids;
    float *save_synth = NULL, *save_gr = NULL, *save_gain = NULL; uint32_t *save_out = NULL; int *save_period = NULL;
    std::vector<uint8_t> mark; std::vector<int32_t> inactive;
  } act;
  PnTables *tables; float *tansig;
  // the per-stream state: pn_kState (pn_state_layout.h) resolved for this context's size, mode and plan.  sh: the operand shadow
  // (same element index, shadow_halfs_per_element halfs per element), NULL where the mode / family keeps none
  struct StateBuf { float *p; uint16_t *sh; size_t words; long long slot_stride; } st[PN_ST_COUNT] = {};
  PnDspSide side;                  // the front end's entries of st[] (pn_dsp_layout.h), resolved once; no aux rows
  float *io_in, *io_out;           // staging rows of the host-buffer paths
  bool postfilter = false;         // optional envelope post-filter in the back end (pn_ctx_set_postfilter)
  // per-stream attenuation limit (pn_ctx_set_atten_limit): (lam, mu) per stream on the device, allocated by the first set; the
  // host mirror of the dB values (the getter) and the count of streams with lam != 0 (the launch decision: while it is 0 the
  // back end is the plain kernel and lam_mu is not read)
  float2 *lam_mu = NULL;
  std::vector<float> atten_db;
  int n_limited = 0;
  // the output stage (pn_outstage.hip; pn_ctx_set_report, pn_ctx_set_output_saturate): launched after the back end while either
  // setting is on.  stage_o: [B][480] fp32 rows the back end's float kernel writes for an int16 entry point; report: [B][8] words.
  // Both are allocated by the two setters.  next_report: pn_host_next_report's pending host destination (one-shot)
  bool report_on = false, saturate = false;
  float *stage_o = NULL; uint32_t *report = NULL;
  void *next_report = NULL;
  bool x3_sat = false;            // PERCEPNET_X3_SATCOUNT=1 (shadow-operand modes): count operand values clamped to the fp16 range
  int dsp_grid_cap = 0;            // > 0 only in the DSP self-test's temporary context: its DSP launches use that many blocks
  bool inject_bad_launch = false;  // pn_ctx_debug_inject_launch_failure (tests): the next frames hand fc a geometry its launcher refuses
  std::vector<void *> allocs;
  bool profiling;
  struct Ev { int fam; hipEvent_t a, b; };
  std::vector<Ev> events;
  std::vector<hipEvent_t> event_pool;   // recycled timing events: no hipEventCreate/Destroy inside a timed region
  double fam_ms[KF_COUNT]; int64_t fam_n[KF_COUNT];
  // pipelined host-buffer path (pn_submit_host_*): created on first use
  struct Pipe {
    bool init = false;
    hipStream_t h2d = nullptr, d2h = nullptr;
    hipEvent_t in_ready[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr}, delivered[2] = {nullptr, nullptr};
    void *in[2] = {nullptr, nullptr}, *out[2] = {nullptr, nullptr};
    float *gr[2] = {nullptr, nullptr};
    uint32_t *report[2] = {nullptr, nullptr};   // per-slot copy of the frame's report records (pn_host_next_report allocates them)
    int64_t submitted = 0;
    char kind[3] = {'?', '?', 0};             // how each copy stream was obtained: n (default priority, probed) / h / l (priority stream)
  } pipe;
};

// ---- pn_context.cpp ---------------------------------------------------------------------------------------------------------
// device count and range, then the guard (entered, the caller's to hold), then the stream: the caller's own, or a new non-blocking
// one (*own_stream).  What pn_ctx_create and pn_featgen_create do before they allocate anything; -1 with the error set.
int open_device(int device, void *hip_stream, DeviceGuard &guard, hipStream_t *stream, bool *own_stream);
// plan: NULL = pn_plan_for(n_streams, nn_mode) (the public behaviour); the self-tests' temporary contexts run the SAME families
// as the context under test whatever their own size.
pn_ctx *ctx_create(const pn_model *model, int device, int n_streams, int nn_mode, void *hip_stream, bool selftest, const PnPlan *plan);
int dev_alloc_into(std::vector<void *> &allocs, size_t &total, hipStream_t stream, void **p, size_t bytes, bool zero);
static inline int dev_alloc(pn_ctx *c, void **p, size_t bytes, bool zero) { return dev_alloc_into(c->allocs, c->bytes, c->stream, p, bytes, zero); }
bool &last_alloc_oom();      // this thread's last dev_alloc_into failure was hipErrorOutOfMemory (the self-tests: skipped, not failed)
// the shared tables built on the host and copied to a new device buffer (synchronous); tansig (optional): the activation table alone
int tables_upload(std::vector<void *> &allocs, size_t &total, hipStream_t stream, PnTables **tables, float **tansig);
// ids[0..n) (host) -> the context's id ring on the device, asynchronously on the context's stream; NULL on failure.  For the
// objects beside a context that take id lists under its rules (pn_rate.cpp)
const int *stage_ids(pn_ctx *c, const int32_t *ids, int n, const void *payload = NULL, int payload_words = 0);
// one frame for every stream / for the listed ones (device rows); active_check: the list's verdict alone, leaves c->act.mark
int process_dev(pn_ctx *c, const void *d_in, void *d_out, float *d_gr, int is_i16);
int active_check(pn_ctx *c, const int32_t *ids, int n);
int process_active(pn_ctx *c, const void *d_in, void *d_out, float *d_gr, int is_i16, const int32_t *ids, int n);
// ---- pn_selftest.cpp --------------------------------------------------------------------------------------------------------
int nn_selftest(pn_ctx *c);
int dsp_selftest(pn_ctx *c);
// ---- pn_host_pipe.cpp -------------------------------------------------------------------------------------------------------
int pipe_make_stream(pn_ctx *c, hipStream_t *out, char how, int prio, char fallback, const std::vector<hipStream_t> &others, char *kind);
// One frame of the pipelined path for whoever owns a frame body (the context's own frame; a rate converter's, pn_rate.cpp): the
// owner's two staging pairs and the bytes of its rows, and the launches between them.  pipe_submit builds the pipeline when it
// is the first frame (the caller is on the context's device).
struct PipeStaging { void *in[2], *out[2]; size_t bytes; };
typedef int (*PipeBody)(void *arg, void *d_in, void *d_out, float *d_gr);
int pipe_submit(pn_ctx *c, const PipeStaging &st, const void *h_in, void *h_out, float *h_gr, PipeBody body, void *arg);
int pipe_drain(pn_ctx *c);       // frames in flight on the pipelined path complete (the caller is on the context's device)
void pipe_destroy(pn_ctx *c);    // the pipeline's streams and events, whole or partly built; its device buffers stay with the context
// ---- pn_stream_state.cpp ----------------------------------------------------------------------------------------------------
// The synchronous host form of a record transfer, for the context's records and for those of the objects beside it (pn_rate.cpp):
// frames in flight on the pipelined path complete first; the records pass through a device buffer of their own size (+ extra_bytes
// behind them, copied to h_extra after the launch: the context's import keeps its status words there) that is freed on every path.
// import: h_records -> device before launch(d_records); else device -> h_records after it.  launch returns 0, or -1 with the error set.
int host_records_sync(pn_ctx *c, bool import, void *h_records, size_t bytes, const std::function<int(void *d_records)> &launch,
                      void *h_extra = NULL, size_t extra_bytes = 0);
// ---- pn_network.cpp ---------------------------------------------------------------------------------------------------------
int weights_acquire(pn_ctx *c, const pn_model *model);     // c->weights, c->L: the shared device copy for c's key, built by its first user
void weights_release(pn_ctx *c);                           // ... freed with its last one
int chain_streams_init(pn_ctx *c);
int launch_rnn(pn_ctx *c);                                 // compute_rnn (rnn.cpp:42-81) for all streams; features in st[PN_ST_FEAT], result in st[PN_ST_GR]
// the operand shadow of entry e at p (a pointer into the entry) re-derived from its fp32 values, in this context's mode and
// family: the whole batch, or the rows ids[i] with status[i] == 0 (status may be NULL).  Launches nothing where e keeps no shadow.
int reshadow(pn_ctx *c, hipStream_t st, int e, const float *p, const int *d_ids = NULL, const int *d_status = NULL, int n = 0);

// operand shadows: 1 half per element (fp16-operand mode) or a hi and a lo plane (split-precision mode)
// (the fp32 shadows of the direct-operand family are 4 bytes per element, laid out in the same 16-byte slab entries)
static inline size_t shadow_halfs_per_element(const pn_ctx *c) { return (c->nn_mode == PN_NN_MFMA_X3 || c->plan.direct) ? 2 : 1; }
// the shadow of the element of entry e that p points at (same element index in the twin buffer), NULL where the entry keeps none
static inline uint16_t *shadow_at(const pn_ctx *c, int e, const float *p) { return c->st[e].sh ? c->st[e].sh + shadow_halfs_per_element(c) * (size_t)(p - c->st[e].p) : NULL; }
// entry e of the state: its j-th live entry, oldest first, before the step with the context's counters runs (j == live: the slot
// that step writes), from row r0 on
static inline float *state_at(const pn_ctx *c, int e, int j, size_t r0 = 0) {
  const PnStateEntry &L = pn_kState[e];
  const int slot = j < L.live ? (pn_state_first(L, c->t, c->tn) + j) % L.slots : pn_state_write(L, c->t, c->tn);
  return c->st[e].p + slot * c->st[e].slot_stride + r0 * L.row_words;
}
// The record sections (= the rings the active-set fix-up shifts, and synth) at the context's CURRENT counters, those of the next
// frame to run: DSP rings follow t, the network's follow tn (they differ after pn_ctx_compute_rnn_host)
static inline void state_sections(const pn_ctx *c, PnSsSection sec[PN_SS_NSEC]) {
  for (int e = 0; e < PN_ST_COUNT; e++) {
    const PnStateEntry &L = pn_kState[e]; const pn_ctx::StateBuf &b = c->st[e];
    if (L.rec_off >= 0) sec[pn_state_section(e)] = PnSsSection{b.p, (uint4 *)b.sh, L.row_words, b.slot_stride, L.slots, pn_state_first(L, c->t, c->tn), L.live, L.cols, L.rec_off,
                         b.sh ? (int)shadow_halfs_per_element(c) : 0};
  }
}
// every stream of this context that carries kernels or copies of a frame: a new one must share a hardware queue with none of them
static inline std::vector<hipStream_t> busy_streams(const pn_ctx *c) {
  std::vector<hipStream_t> v{c->stream};
  for (int k = 1; k < 4; k++) if (c->chain_stream[k]) v.push_back(c->chain_stream[k]);
  if (c->pipe.h2d) v.push_back(c->pipe.h2d);
  if (c->pipe.d2h) v.push_back(c->pipe.d2h);
  return v;
}

// ---- profiling ------------------------------------------------------------------------------------------
struct Scope {
  pn_ctx *c; int fam; hipEvent_t a, b; bool on; hipStream_t st;      // st: the stream the bracketed launches go to (a row-range chain's own)
  Scope(pn_ctx *c_, int fam_, hipStream_t st_ = nullptr) : c(c_), fam(fam_), on(c_->profiling), st(st_ ? st_ : c_->stream) {
    if (on) {
      auto take = [&](hipEvent_t &e) { if (c->event_pool.empty()) hipEventCreate(&e); else { e = c->event_pool.back(); c->event_pool.pop_back(); } };
      take(a); take(b); hipEventRecord(a, st);
    }
  }
  ~Scope() {
    if (on) { hipEventRecord(b, st); c->events.push_back({fam, a, b}); }
    // debugging aid: PERCEPNET_SYNC_EACH=<bit mask over kernel families, -1 = all>: host sync after those launches
    static const long sync_mask = getenv("PERCEPNET_SYNC_EACH") ? strtol(getenv("PERCEPNET_SYNC_EACH"), NULL, 0) : 0;
    if (sync_mask & (1L << fam)) hipStreamSynchronize(st);
  }
};
