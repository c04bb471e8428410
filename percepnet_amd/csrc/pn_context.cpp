// Host side of libpercepnet_hip: models, batched contexts, the per-frame launch sequence and the
// C-ABI declared in include/percepnet_hip.h.  Mirrors the reference's frame engine
// (rnnoise_create/init/process_frame, denoise.cpp:252-280,508-547) for B streams in lock-step.
#include "pn_context.h"
#include <stdio.h>
#include <float.h>
#include <math.h>
#include <map>
#include <mutex>
#include <string>

#include "pn_selftest_golden.h"

extern "C" int pn_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

// ---- contexts -----------------------------------------------------------------------------------------

static thread_local bool g_last_alloc_oom = false;     // the last dev_alloc failure on this thread was hipErrorOutOfMemory
int dev_alloc_into(std::vector<void *> &allocs, size_t &total, hipStream_t stream, void **p, size_t bytes, bool zero) {
  // PERCEPNET_GUARD=1 (debugging aid): every buffer is followed by 1 MB of 0xFF (NaN as fp32 and as fp16), so that a
  // read past the end of a buffer shows up as NaN in the outputs instead of as run-to-run noise
  static const bool guard = getenv("PERCEPNET_GUARD") != NULL;
  const size_t pad = guard ? (1u << 20) : 0, body = (bytes + 255) & ~(size_t)255;
  {
    const hipError_t e = hipMalloc(p, guard ? body + pad : bytes);
    if (e != hipSuccess) {
      g_last_alloc_oom = (e == hipErrorOutOfMemory);
      (void)hipGetLastError();
      pn_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
      return -1;
    }
  }
  allocs.push_back(*p);
  total += bytes;
  if (zero) PN_HIP_CHECK(hipMemsetAsync(*p, 0, bytes, stream));
  if (guard) PN_HIP_CHECK(hipMemsetAsync((char *)*p + body, 0xFF, pad, stream));
  return 0;
}
static int dev_alloc(pn_ctx *c, void **p, size_t bytes, bool zero) { return dev_alloc_into(c->allocs, c->bytes, c->stream, p, bytes, zero); }
#define DEV_ALLOC(ptr, count, zero) \
  do { if (dev_alloc(c, (void **)&(ptr), sizeof(*(ptr)) * (size_t)(count), zero)) goto fail; } while (0)
int tables_upload(std::vector<void *> &allocs, size_t &total, hipStream_t stream, PnTables **tables, float **tansig) {
  PnTables *ht = new PnTables();
  hipError_t e = hipSuccess;
  int rc = pn_build_tables(ht);                          // these two set the error themselves
  if (!rc) rc = dev_alloc_into(allocs, total, stream, (void **)tables, sizeof(PnTables), false);
  if (!rc) e = hipMemcpyAsync(*tables, ht, sizeof(PnTables), hipMemcpyHostToDevice, stream);
  if (!rc && e == hipSuccess && tansig) {
    rc = dev_alloc_into(allocs, total, stream, (void **)tansig, sizeof(ht->tansig), false);
    if (!rc) e = hipMemcpyAsync(*tansig, ht->tansig, sizeof(ht->tansig), hipMemcpyHostToDevice, stream);
  }
  const hipError_t es = hipStreamSynchronize(stream);    // always: ht must outlive the copies
  if (e == hipSuccess) e = es;
  if (!rc && e != hipSuccess) { pn_set_error("table upload failed: %s", hipGetErrorString(e)); rc = -1; }
  delete ht;
  return rc;
}

// "fresh context", pn_ctx_reset and "every stream reset" are one statement: every word of every entry and shadow is zero
static int zero_state(pn_ctx *c) {
  for (const pn_ctx::StateBuf &b : c->st) {
    PN_HIP_CHECK(hipMemsetAsync(b.p, 0, b.words * 4, c->stream));
    if (b.sh) PN_HIP_CHECK(hipMemsetAsync(b.sh, 0, b.words * 2 * shadow_halfs_per_element(c), c->stream));
  }
  if (c->lam_mu) PN_HIP_CHECK(hipMemsetAsync(c->lam_mu, 0, (size_t)c->B * sizeof(float2), c->stream));   // every stream back to off
  c->atten_db.assign(c->B, INFINITY); c->n_limited = 0;
  c->t = 0; c->tn = 0;
  return 0;
}
// The record sections (= the rings the active-set fix-up shifts, and synth) at the context's CURRENT counters, those of the next
// frame to run: DSP rings follow t, the network's follow tn (they differ after pn_ctx_compute_rnn_host)
static void state_sections(const pn_ctx *c, PnSsSection sec[PN_SS_NSEC]) {
  for (int e = 0; e < PN_ST_COUNT; e++) {
    const PnStateEntry &L = pn_kState[e]; const pn_ctx::StateBuf &b = c->st[e];
    if (L.rec_off >= 0) sec[pn_state_section(e)] = PnSsSection{b.p, (uint4 *)b.sh, L.row_words, b.slot_stride, L.slots, pn_state_first(L, c->t, c->tn), L.live, L.cols, L.rec_off,
                         b.sh ? (int)shadow_halfs_per_element(c) : 0};
  }
}

static int nn_selftest(pn_ctx *c);
static int dsp_selftest(pn_ctx *c);
static pn_ctx *ctx_create(const pn_model *model, int device, int n_streams, int nn_mode, void *hip_stream, bool selftest, const PnPlan *plan);

extern "C" void pn_ctx_destroy(pn_ctx *c) {
  if (!c) return;
  DeviceGuard _dg(c->device);
  hipStreamSynchronize(c->stream);
  if (c->pipe.init) {
    hipStreamSynchronize(c->pipe.h2d); hipStreamSynchronize(c->pipe.d2h);
    for (int k = 0; k < 2; k++) { hipEventDestroy(c->pipe.in_ready[k]); hipEventDestroy(c->pipe.done[k]); hipEventDestroy(c->pipe.delivered[k]); }
    hipStreamDestroy(c->pipe.h2d); hipStreamDestroy(c->pipe.d2h);
  }
  for (int k = 1; k < 4; k++) if (c->chain_stream[k]) { hipStreamSynchronize(c->chain_stream[k]); hipStreamDestroy(c->chain_stream[k]); if (c->chain_join[k]) hipEventDestroy(c->chain_join[k]); }
  if (c->chain_fork) hipEventDestroy(c->chain_fork);
  for (auto &e : c->events) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
  for (hipEvent_t e : c->event_pool) hipEventDestroy(e);
  for (void *p : c->allocs) hipFree(p);
  for (pn_ctx::IdRing *r : {&c->ids, &c->act.ids})
    for (auto &sl : r->slot) { if (sl.h) hipHostFree(sl.h); if (sl.ev) hipEventDestroy(sl.ev); }
  weights_release(c);
  if (c->own_stream) hipStreamDestroy(c->stream);
  delete c;
}

extern "C" pn_ctx *pn_ctx_create(const pn_model *model, int device, int n_streams, int nn_mode, void *hip_stream) {
  return ctx_create(model, device, n_streams, nn_mode, hip_stream, true, NULL);
}

// plan: NULL = pn_plan_for(n_streams, nn_mode) (the public behaviour); the self-tests' temporary contexts run the SAME families
// as the context under test whatever their own size.
static pn_ctx *ctx_create(const pn_model *model, int device, int n_streams, int nn_mode, void *hip_stream, bool selftest, const PnPlan *plan) {
  if (!model) { pn_set_error("NULL model"); return NULL; }
  if (n_streams < 1) { pn_set_error("n_streams must be >= 1"); return NULL; }
  if (nn_mode != PN_NN_MFMA && nn_mode != PN_NN_STRICT && nn_mode != PN_NN_MFMA_F16 && nn_mode != PN_NN_MFMA_X3) { pn_set_error("bad nn_mode %d", nn_mode); return NULL; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    pn_set_error("no HIP device available (this library has no CPU fallback)");
    return NULL;
  }
  if (device < 0 || device >= ndev) { pn_set_error("device %d out of range (%d devices)", device, ndev); return NULL; }
  DeviceGuard _dg(device);
  if (!_dg.ok) { pn_set_error("hipSetDevice(%d) failed", device); return NULL; }
  pn_ctx *c = new pn_ctx();
  c->device = device; c->B = n_streams; c->Bp = ((size_t)n_streams + 255) / 256 * 256; c->nn_mode = nn_mode; c->plan = plan ? *plan : pn_plan_for(n_streams, nn_mode);
  c->t = 0; c->tn = 0; c->bytes = 0; c->profiling = false;
  memset(c->fam_ms, 0, sizeof(c->fam_ms)); memset(c->fam_n, 0, sizeof(c->fam_n));
  memset(c->L, 0, sizeof(c->L));

  if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = false; }
  else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { pn_set_error("hipStreamCreate failed"); delete c; return NULL; }
    c->own_stream = true;
  }
  const size_t B = n_streams, Bp = c->Bp;
  float *base[PN_ST_COUNT];
  if (tables_upload(c->allocs, c->bytes, c->stream, &c->tables, &c->tansig)) goto fail;
  for (int e = 0; e < PN_ST_COUNT; e++) {
    pn_ctx::StateBuf &b = c->st[e];
    const PnStateSize z = pn_state_size(pn_kState[e], pn_kState[e].padded ? Bp : B);
    b.words = z.words; b.slot_stride = z.slot_stride;
    DEV_ALLOC(b.p, b.words, false);
    base[e] = b.p;
  }
  c->side = pn_dsp_side(base, nullptr, B);
  // operand shadows: of the shadow-operand modes (1 half per element: fp16 operands; hi + lo planes: split precision), and of the
  // direct-operand family (fp32 fragments), which keeps its dense layers on the batch kernels: no shadows of the conv FIFOs
  for (int e = 0; e < PN_ST_COUNT; e++)
    if (pn_state_shadowed(e, c->plan, nn_mode)) DEV_ALLOC(c->st[e].sh, shadow_halfs_per_element(c) * c->st[e].words, false);
  DEV_ALLOC(c->io_in, B * PN_FRAME, false);
  DEV_ALLOC(c->io_out, B * PN_FRAME, false);
  if (zero_state(c)) goto fail;
  for (int li = 0; li < PN_NLAYERS; li++) { c->geom[li] = model->L[li]; c->geom[li].bias = c->geom[li].w = c->geom[li].rw = NULL; }
  if (weights_acquire(c, model)) goto fail;
  if (hipStreamSynchronize(c->stream) != hipSuccess) { pn_set_error("initial upload failed"); goto fail; }
  if (selftest && (nn_mode == PN_NN_MFMA_X3 || nn_mode == PN_NN_MFMA_F16)) {       // (not for the self-tests' temporary contexts)
    const char *e = getenv("PERCEPNET_X3_SATCOUNT");
    c->x3_sat = e && atoi(e);
  }
  if (selftest && nn_mode != PN_NN_STRICT && nn_selftest(c)) goto fail;
  if (selftest && dsp_selftest(c)) goto fail;
  if (c->x3_sat && pn_x3_sat_set(1)) { pn_set_error("cannot enable the operand-saturation counter"); goto fail; }   // after the self-tests: starts at zero
  if (c->plan.chains > 1 && chain_streams_init(c)) goto fail;      // probed now, not inside a frame
  return c;
fail:
  pn_ctx_destroy(c);
  return NULL;
}

static int pipe_drain(pn_ctx *c);
extern "C" int pn_ctx_reset(pn_ctx *c) { if (!c) return -1; PN_ON_DEVICE(c); if (pipe_drain(c)) return -1; return zero_state(c); }
// The pinned id ring, for both of its users.  (The caller is on the context's device.)
static int stage_payload_offset(int n) { return (n + 3) & ~3; }      // 16-byte aligned
// room for `cap` ints in ring r (the old, smaller buffers stay in allocs until destroy: kernels of an earlier call may still be reading them)
static int id_ring_reserve(pn_ctx *c, pn_ctx::IdRing &r, int cap) {
  if (r.cap >= cap) return 0;
  if (dev_alloc(c, (void **)&r.d, (size_t)cap * sizeof(int), false)) return -1;
  for (auto &sl : r.slot) {
    if (sl.ev) PN_HIP_CHECK(hipEventSynchronize(sl.ev));
    if (sl.h) hipHostFree(sl.h);
    sl.h = NULL;
    PN_HIP_CHECK(hipHostMalloc((void **)&sl.h, (size_t)cap * sizeof(int), hipHostMallocDefault));
    if (!sl.ev) PN_HIP_CHECK(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
  }
  r.cap = cap;
  return 0;
}
// ids[0..n) (+ the payload) -> r.d through the next pinned slot, asynchronously on the context's stream; r holds `words` ints
static int id_ring_stage(pn_ctx *c, pn_ctx::IdRing &r, const int32_t *ids, int n, const void *payload, int payload_words, int words) {
  auto &sl = r.slot[r.calls++ & 3];
  PN_HIP_CHECK(hipEventSynchronize(sl.ev));                 // the copy issued from this slot four calls ago has executed
  memcpy(sl.h, ids, (size_t)n * sizeof(int));
  if (payload_words) memcpy(sl.h + stage_payload_offset(n), payload, (size_t)payload_words * 4);
  PN_HIP_CHECK(hipMemcpyAsync(r.d, sl.h, (size_t)words * sizeof(int), hipMemcpyHostToDevice, c->stream));
  PN_HIP_CHECK(hipEventRecord(sl.ev, c->stream));
  return 0;
}
// ids[0..n) (host) -> c->ids.d, asynchronously on the context's stream (frames may be in flight); the launches that read it follow
// on the same stream.  NULL on failure.  payload (optional): payload_words more 32-bit words staged in the same copy, at
// c->ids.d + stage_payload_offset(n)
const int *stage_ids(pn_ctx *c, const int32_t *ids, int n, const void *payload, int payload_words) {
  const int words = payload_words ? stage_payload_offset(n) + payload_words : n;
  if (id_ring_reserve(c, c->ids, words < 1024 ? 1024 : words) || id_ring_stage(c, c->ids, ids, n, payload, payload_words, words)) return NULL;
  return c->ids.d;
}
// rnnoise_init for a subset of the streams (denoise.cpp:259-280): every row of stream s in every ring slot / ping-pong half
// of every state buffer goes to zero (pn_state.hip says why that is a fresh stream whatever the ring phases are)
extern "C" int pn_ctx_reset_streams(pn_ctx *c, const int32_t *ids, int n) {
  if (!c || n < 0 || (n > 0 && !ids)) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  for (int i = 0; i < n; i++) if (ids[i] < 0 || ids[i] >= c->B) { pn_set_error("stream id %d out of range [0, %d)", ids[i], c->B); return -1; }
  PN_ON_DEVICE(c);
  const int *d = stage_ids(c, ids, n);
  if (!d) return -1;
  const int np = (int)shadow_halfs_per_element(c);
  for (int e = 0; e < PN_ST_COUNT; e++) {                    // the rows in every slot of every entry, and of its shadow (a NULL one is skipped)
    const PnStateEntry &L = pn_kState[e]; const pn_ctx::StateBuf &b = c->st[e];
    const int outer = L.in_row ? 1 : L.slots;
    pn_launch_zero_rows(c->stream, b.p, L.row_words, L.row_words, outer, b.slot_stride, d, n);
    pn_launch_zero_shadow_rows(c->stream, b.sh, L.cols, np, outer, np * b.slot_stride, d, n);
  }
  if (c->lam_mu) pn_launch_zero_rows(c->stream, c->lam_mu, 2, 2, 1, 0, d, n);   // a reset slot is a new call: attenuation limit off
  PN_HIP_CHECK(hipGetLastError());
  for (int i = 0; i < n; i++) {                            // (duplicates allowed: the second sees the stream already off)
    if (pn_atten_limit_factor(c->atten_db[ids[i]]) != 0.f) c->n_limited--;
    c->atten_db[ids[i]] = INFINITY;
  }
  return 0;
}
extern "C" int pn_ctx_n_streams(const pn_ctx *c) { return c ? c->B : -1; }
extern "C" int64_t pn_ctx_frames_done(const pn_ctx *c) { return c ? c->t : -1; }
// state (+ tables) of this context, plus the weights if this context created their device copy (a context that found them
// in the cache adds nothing: the copy is shared)
extern "C" size_t pn_ctx_device_bytes(const pn_ctx *c) { return c ? c->bytes + ((c->weights && !c->weights_were_cached) ? c->weight_bytes : 0) : 0; }
// bytes of the packed weight copy this context reads, whoever created it: a process's footprint is the sum of
// pn_ctx_device_bytes over its contexts plus every DISTINCT shared copy that no live context reports as its own
extern "C" size_t pn_ctx_weight_bytes(const pn_ctx *c) { return (c && c->weights) ? c->weight_bytes : 0; }
extern "C" int pn_ctx_describe(const pn_ctx *c, char *buf, size_t n) {
  if (!c || !buf || !n) return -1;
  const int f = pn_plan_describe(c->plan, c->nn_mode, buf, n);
  if (f < 0 || (size_t)f >= n) return -1;
  const int k = c->plan.chains;
  const int w = f + snprintf(buf + f, n - f, " weights=%s nn_chains=%d%s%s", c->weights_were_cached ? "shared" : "own", k, k > 1 ? ":" : "", k > 1 ? c->chain_kind + 1 : "");
  if (w < 0 || (size_t)w >= n) return -1;
  if (c->x3_sat) {                                        // debug: operand values clamped to +-65504 so far (device-wide counter)
    DeviceGuard _dg(c->device);
    hipStreamSynchronize(c->stream);
    const int w2 = snprintf(buf + w, n - w, " x3_saturated=%lld", pn_x3_sat_read());
    return (w2 < 0 || (size_t)(w + w2) >= n) ? -1 : w + w2;
  }
  return w;
}
extern "C" int pn_ctx_synchronize(pn_ctx *c) { if (!c) return -1; PN_ON_DEVICE(c); PN_HIP_CHECK(hipStreamSynchronize(c->stream)); return 0; }


static int flush_events(pn_ctx *c) {
  PN_HIP_CHECK(hipStreamSynchronize(c->stream));
  for (int k = 1; k < 4; k++) if (c->chain_stream[k]) PN_HIP_CHECK(hipStreamSynchronize(c->chain_stream[k]));
  for (auto &e : c->events) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { c->fam_ms[e.fam] += ms; c->fam_n[e.fam]++; }
    c->event_pool.push_back(e.a); c->event_pool.push_back(e.b);
  }
  c->events.clear();
  return 0;
}

extern "C" int pn_ctx_set_profiling(pn_ctx *c, int enable) {
  if (!c) return -1;
  if (enable && c->event_pool.size() < 2048) {        // enough for ~75 frames between two reads; created outside any timed region
    PN_ON_DEVICE(c);
    while (c->event_pool.size() < 2048) { hipEvent_t e; PN_HIP_CHECK(hipEventCreate(&e)); c->event_pool.push_back(e); }
  }
  c->profiling = enable != 0;
  return 0;
}
extern "C" int pn_kernel_count(void) { return KF_COUNT; }
extern "C" const char *pn_kernel_name(int i) { return (i >= 0 && i < KF_COUNT) ? pn_kFamilyName[i] : NULL; }
extern "C" int pn_ctx_kernel_time(pn_ctx *c, const char *name, double *total_ms, int64_t *launches) {
  if (!c || !name) return -1;
  if (flush_events(c)) return -1;
  for (int i = 0; i < KF_COUNT; i++)
    if (!strcmp(name, pn_kFamilyName[i])) { if (total_ms) *total_ms = c->fam_ms[i]; if (launches) *launches = c->fam_n[i]; return 0; }
  pn_set_error("unknown kernel family '%s'", name);
  return -1;
}
extern "C" int pn_ctx_reset_profile(pn_ctx *c) {
  if (!c) return -1;
  if (flush_events(c)) return -1;
  memset(c->fam_ms, 0, sizeof(c->fam_ms)); memset(c->fam_n, 0, sizeof(c->fam_n));
  return 0;
}


// Known-answer self-test of the MFMA network kernels (PERCEPNET_SELFTEST=0 skips it).
// The MFMA paths (fp32 and fp16 operands) depend on the compiler's wait-state insertion and on pinned instruction
// order; a toolchain that schedules them differently could lose accumulator updates silently (the
// failure once seen hit output rows 27/31 mod 32 only).  So the first context of every (device, nn_mode, kernel
// family) in a process triggers one check of THE KERNELS — not of the caller's model: a fixed built-in synthetic weight
// set (uniform +-3/sqrt(fan_in), LCG-generated: gates from saturated to linear; the expected MFMA-vs-reference-order
// difference over two steps from the zero state is known and small; PERCEPNET_SELFTEST=2 prints it) is
// run for two network steps over 192 rows (six 32-row wave tiles, two M tiles) through two temporary contexts — the
// kernel family under test and the reference-order STRICT kernels — and the context is refused if any g/r output
// differs by more than 2e-5 (fp32 operands) / 4e-3 (fp16 operands, whose rounding the x3 weights amplify).  The verdict is cached for
// the process; a self-test that cannot allocate its ~70 MB of temporaries is reported as SKIPPED, not as a failure.
static std::mutex g_selftest_mu;
static std::map<std::tuple<int, int, int, int, int, int, int>, int> g_selftest_done;     // key -> 0 passed, 1 skipped

pn_model *pn_model_from_sources(const struct PnLayerSrc *src);
static pn_model *selftest_model() {
  static std::vector<float> store;
  PnLayerSrc s[PN_NLAYERS];
  size_t total = 0, nb, nw, nr;
  for (int li = 0; li < PN_NLAYERS; li++) total += pn_layer_floats(pn_kGeom[li].kind, pn_kGeom[li].nin, pn_kGeom[li].nn, pn_kGeom[li].ks, &nb, &nw, &nr);
  store.resize(total);
  unsigned x = 2463534242u;
  size_t off = 0;
  static const int act[PN_NLAYERS] = {3, 3, 2, 2, 2, 2, 2, 2, 1, 1};        // relu relu tanh tanh*5 sigmoid sigmoid (rnn_train.py:105-121)
  for (int li = 0; li < PN_NLAYERS; li++) {
    pn_layer_floats(pn_kGeom[li].kind, pn_kGeom[li].nin, pn_kGeom[li].nn, pn_kGeom[li].ks, &nb, &nw, &nr);
    const float bound_w = 1.f / sqrtf((float)(pn_kGeom[li].kind == PN_KIND_GRU ? pn_kGeom[li].nn : pn_kGeom[li].nin * pn_kGeom[li].ks));
    for (size_t i = 0; i < nb + nw + nr; i++) {
      x = x * 1664525u + 1013904223u;
      // x3: a good share of the GRU gates and tanh outputs saturate, so the clamped end of the activation table
      // (indices 192..200: a 192-thread block once failed to stage them) is exercised, not only its linear middle
      store[off + i] = ((int)(x >> 8) % 20001 - 10000) * 1e-4f * bound_w * (i < nb ? 1.f : 3.f);
    }
    s[li] = {pn_kGeom[li].kind, pn_kGeom[li].nin, pn_kGeom[li].nn, pn_kGeom[li].ks, act[li], 1, &store[off], &store[off + nb], nr ? &store[off + nb + nw] : NULL};
    off += nb + nw + nr;
  }
  pn_model *m = pn_model_from_sources(s);
  store.clear(); store.shrink_to_fit();
  return m;
}

static int nn_selftest(pn_ctx *c) {
  const char *env = getenv("PERCEPNET_SELFTEST");
  if (env && !atoi(env)) return 0;
  const PnPlan &p = c->plan;      // the kernel-selecting fields; the front end and the chains select no network kernel
  const auto key = std::make_tuple(c->device, c->nn_mode, p.small, p.small_gru, p.direct, p.rg, p.narrow);
  std::lock_guard<std::mutex> lk(g_selftest_mu);
  if (g_selftest_done.count(key)) return 0;
  const int rows = 192;
  const float tol = c->nn_mode == PN_NN_MFMA_F16 ? 4e-3f : 2e-5f;    // measured on the built-in set: 8.3e-7 (fp32), 1.03e-3 (fp16 operands); a lost k-step is O(0.1)
  pn_model *m = selftest_model();
  pn_ctx *cx[2] = {NULL, NULL};
  std::vector<float> feat((size_t)rows * PN_NFEAT), gr[2][2];
  int rc = m ? 0 : -1;
  bool oom = false;
  PnPlan plan[2] = {p, pn_plan_for(rows, PN_NN_STRICT)};
  plan[0].chains = 1;                                    // (192 rows are one chain)
  for (int pass = 0; pass < 2 && !rc; pass++) {          // pass 0: the kernel family under test; pass 1: STRICT kernels
    g_last_alloc_oom = false;
    cx[pass] = ctx_create(m, c->device, rows, pass ? PN_NN_STRICT : c->nn_mode, NULL, false, &plan[pass]);
    if (!cx[pass]) { rc = -1; oom = g_last_alloc_oom; break; }
    unsigned x = 12345u;
    for (int step = 0; step < 2 && !rc; step++) {
      for (float &v : feat) { x = x * 1664525u + 1013904223u; v = ((int)(x >> 8) % 2001 - 1000) * 1.5e-3f; }
      gr[pass][step].resize((size_t)rows * 68);
      if (pn_ctx_compute_rnn_host(cx[pass], feat.data(), gr[pass][step].data())) rc = -1;
    }
  }
  pn_ctx_destroy(cx[0]); pn_ctx_destroy(cx[1]); pn_model_free(m);
  if (rc && oom) {
    fprintf(stderr, "percepnet_hip: network self-test SKIPPED on device %d (not enough free memory for its temporaries): %s\n", c->device, pn_last_error());
    g_selftest_done[key] = 1;
    return 0;
  }
  if (rc) { std::string why = pn_last_error(); pn_set_error("network self-test could not run: %s", why.c_str()); return -1; }
  float worst = 0; int wrow = 0, wcol = 0;
  for (int step = 0; step < 2; step++)
    for (size_t i = 0; i < gr[0][step].size(); i++) {
      const float d = fabsf(gr[0][step][i] - gr[1][step][i]);
      if (!(d <= worst)) { worst = d; wrow = (int)(i / 68); wcol = (int)(i % 68); }     // NaN lands here too
    }
  if (env && atoi(env) >= 2)
    fprintf(stderr, "percepnet_hip: network self-test device %d nn_mode %d dense=%s gru=%s: worst |delta g,r| %g (tolerance %g) at row %d output %d\n",
            c->device, c->nn_mode, p.small ? "small" : "batch", p.small_gru ? "small" : "batch", (double)worst, (double)tol, wrow, wcol);
  if (!(worst <= tol)) {
    pn_set_error("network self-test FAILED (nn_mode %d, dense=%s gru=%s): the MFMA kernels differ from the reference-order kernels by %g "
                 "(> %g) at row %d (row %% 32 = %d), output %d on the built-in weight set — the build's instruction schedule is "
                 "not the validated one (DESIGN.md 4.3); refusing to run", c->nn_mode, p.small ? "small" : "batch",
                 p.small_gru ? "small" : "batch", (double)worst, (double)tol, wrow, wrow % 32, wcol);
    return -1;
  }
  g_selftest_done[key] = 0;
  return 0;
}

// Known-answer self-test of the DSP kernels, the counterpart of nn_selftest (PERCEPNET_SELFTEST=0 skips both).
// The first context of every (device, front-end family) in a process runs a fixed integer-generated waveform
// (two triangle waves + LCG noise, quiet and clipping stretches) through a temporary 40-stream context whose DSP
// launches are capped at ONE block (pn_ctx::dsp_grid_cap, an argument of the DSP launchers): every stream is fed the same PCM, so the 40 streams of 3 to 10
// grid-stride rounds must agree with each other word for word, the silence flags of all 14 frames (a full wrap of
// the 12-frame history ring) and the 70 features of the last frame must equal the CPU oracle's bit patterns stored in
// pn_selftest_golden.h (tools/make_dsp_selftest_golden.py; the features never touch the network).
static void selftest_pcm(std::vector<int16_t> &out) {     // in step with tools/make_dsp_selftest_golden.py
  const int n = PN_SELFTEST_FRAMES * PN_FRAME;
  out.resize(n);
  uint32_t x = 2463534242u;
  for (int i = 0; i < n; i++) {
    const int p1 = (i * 7) % 960, t1 = p1 < 480 ? p1 - 480 : 1440 - p1 - 480;
    const int p2 = (i * 31) % 960, t2 = p2 < 480 ? p2 - 480 : 1440 - p2 - 480;
    x = x * 1664525u + 1013904223u;
    const int noise = (int)((x >> 16) % 2001u) - 1000;
    const int amp = (i / 2400) % 2 == 1 ? 200 : 24;
    int v = amp * t1 + (amp / 3) * t2 + noise;
    v = v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
    out[i] = (int16_t)v;
  }
}

static int dsp_selftest(pn_ctx *c) {
  const char *env = getenv("PERCEPNET_SELFTEST");
  if (env && !atoi(env)) return 0;
  static std::map<std::pair<int, int>, int> done;
  const auto key = std::make_pair(c->device, c->plan.fe);
  std::lock_guard<std::mutex> lk(g_selftest_mu);
  if (done.count(key)) return 0;
  const int Bt = 40;
  std::vector<int16_t> pcm;
  selftest_pcm(pcm);
  pn_model *m = selftest_model();
  g_last_alloc_oom = false;
  PnPlan plan = pn_plan_for(Bt, PN_NN_MFMA);
  plan.fe = c->plan.fe;
  pn_ctx *t = m ? ctx_create(m, c->device, Bt, PN_NN_MFMA, NULL, false, &plan) : NULL;
  if (!t) {
    const bool oom = g_last_alloc_oom;
    pn_model_free(m);
    if (oom) { fprintf(stderr, "percepnet_hip: DSP self-test SKIPPED on device %d (no memory for its temporaries)\n", c->device); done[key] = 1; return 0; }
    std::string why = pn_last_error(); pn_set_error("DSP self-test could not run: %s", why.c_str()); return -1;
  }
  std::vector<int16_t> in((size_t)Bt * PN_FRAME), out((size_t)Bt * PN_FRAME);
  std::vector<float> feat((size_t)Bt * PN_NFEAT);
  std::vector<int32_t> sil(Bt);
  int rc = 0; std::string msg;
  t->dsp_grid_cap = 1;
  for (int f = 0; f < PN_SELFTEST_FRAMES && !rc; f++) {
    for (int s = 0; s < Bt; s++) memcpy(&in[(size_t)s * PN_FRAME], &pcm[(size_t)f * PN_FRAME], PN_FRAME * sizeof(int16_t));
    if (pn_process_host_i16(t, in.data(), out.data(), NULL) || pn_ctx_read_features(t, feat.data(), sil.data())) { rc = -1; msg = pn_last_error(); break; }
    for (int s = 0; s < Bt && !rc; s++) {
      if (sil[s] != kSelftestSilence[f]) { rc = -2; msg = "silence flag of frame " + std::to_string(f) + ", stream " + std::to_string(s); }
      if (memcmp(&feat[(size_t)s * PN_NFEAT], &feat[0], PN_NFEAT * 4)) { rc = -2; msg = "stream " + std::to_string(s) + " differs from stream 0 at frame " + std::to_string(f) + " (same input)"; }
    }
    if (!rc && f == PN_SELFTEST_FRAMES - 1)
      for (int k = 0; k < PN_NFEAT; k++) {
        uint32_t w; memcpy(&w, &feat[k], 4);
        if (w != kSelftestFeat[k]) { rc = -2; msg = "feature " + std::to_string(k) + " of the last frame"; break; }
      }
  }
  pn_ctx_destroy(t); pn_model_free(m);
  if (env && atoi(env) >= 2) fprintf(stderr, "percepnet_hip: DSP self-test device %d front end %d: %s\n", c->device, c->plan.fe, rc ? msg.c_str() : "70 features + 14 silence flags bit-equal to the CPU oracle, 40 streams identical");
  if (rc == -1) { pn_set_error("DSP self-test could not run: %s", msg.c_str()); return -1; }
  if (rc) {
    pn_set_error("DSP self-test FAILED (front end %s): %s does not match the CPU reference's known answer — this build of the DSP "
                 "kernels is not bit-exact (DESIGN.md 4.4); refusing to run", pn_kFe[c->plan.fe].name, msg.c_str());
    return -1;
  }
  done[key] = 0;
  return 0;
}

// launch k of front-end family fe: row fe of this table is row fe of pn_kFe, its launchers in the order of that row's fam[]
void pn_launch_fe(hipStream_t st, const PnTables *T, int n_streams, int fe, int k, const PnDspSide &s, const PnDspSlots &sl, const PnDspIn &in, int grid_cap) {
  static PnFeLaunch *const launch[][3] = {{pn_launch_frontend}, {pn_launch_frontend_g2}, {pn_launch_fe_spec_in, pn_launch_fe_pitch, pn_launch_fe_spec_out}};
  static_assert(sizeof(launch) / sizeof(launch[0]) == sizeof(pn_kFe) / sizeof(pn_kFe[0]) && sizeof(launch[0]) / sizeof(launch[0][0]) == sizeof(pn_kFe[0].fam) / sizeof(int),
                "one row of launchers per front-end family of pn_kFe");
  launch[fe][k](st, T, n_streams, s, sl, in, grid_cap);
}

static int process_dev(pn_ctx *c, const void *d_in, void *d_out, float *d_gr, int is_i16) {
  if (!c || !d_in || !d_out) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(c);
  const PnDspSide &s = c->side;
  const PnDspSlots k = pn_dsp_slots(c->t);
  const PnDspIn in = {d_in, is_i16, PN_FRAME, 1.f / 32768.f};
  float *const gr = c->st[PN_ST_GR].p;
  for (int i = 0; i < pn_kFe[c->plan.fe].n; i++) {
    Scope sc(c, pn_kFe[c->plan.fe].fam[i]);
    pn_launch_fe(c->stream, c->tables, c->B, c->plan.fe, i, s, k, in, c->dsp_grid_cap);
  }
  if (launch_rnn(c)) return -1;                        // a refused launch fails the frame (pn_last_error says which layer)
  // the output stage runs while it has something to do: a report to write, or int16 rows to saturate.  It then owns the int16
  // cast: the back end's float kernel writes the context's own rows and the stage casts them into the caller's
  const bool stage = c->report_on || (c->saturate && is_i16), staged_cast = stage && is_i16;
  { Scope sc(c, KF_BACKEND);
    // X(t), and Ex(t) for the post-filter: the oldest live look-ahead slot
    pn_launch_backend(c->stream, c->tables, c->B, pn_dsp_spec(s, k.slot_r), s.Ps, gr, c->postfilter ? pn_dsp_bands(s, k.slot_r) : nullptr, s.silence,
                      c->st[PN_ST_SYNTH].p, staged_cast ? (void *)c->stage_o : d_out, staged_cast ? 0 : is_i16, c->dsp_grid_cap,
                      c->n_limited > 0 ? c->lam_mu : nullptr); }      // no stream limited: the plain back end
  if (stage) {
    Scope sc(c, KF_BACKEND);
    // the input frame this output frame is about: frame t - 6 of the history ring (the engine's delay)
    pn_launch_outstage(c->stream, c->B, staged_cast ? c->stage_o : (const float *)d_out, s, (k.frame_t + 6) % PN_HIST_FRAMES, gr,
                       is_i16 ? (int16_t *)d_out : nullptr, c->saturate, c->report_on ? c->report : nullptr);
  }
  if (d_gr) PN_HIP_CHECK(hipMemcpyAsync(d_gr, gr, (size_t)c->B * 68 * 4, hipMemcpyDeviceToDevice, c->stream));
  PN_HIP_CHECK(hipGetLastError());
  c->t++; c->tn++;
  if (c->events.size() >= 4096 && flush_events(c)) return -1;   // profiling left on: bound the pending events
  return 0;
}

// Test hook (tests/test_gpu_lifecycle.py): while enabled, every frame asks the fc layer's launcher for a geometry it refuses —
// pn_process_* / pn_submit_host_* / pn_ctx_compute_rnn_host must then return -1 with pn_last_error() naming the launcher,
// never 0 with stale outputs (STRICT contexts have no such refusal: their kernels take any geometry).
extern "C" int pn_ctx_debug_inject_launch_failure(pn_ctx *c, int enable) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  c->inject_bad_launch = enable != 0;
  return 0;
}

extern "C" int pn_ctx_set_postfilter(pn_ctx *c, int enable) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  c->postfilter = enable != 0;
  return 0;
}

// ---- per-stream frame report, saturating int16 output (pn_outstage.hip) ---------------------------------------------------
// Context-wide settings; what the stage needs is allocated here, never inside a frame (the lam_mu pattern).
static int stage_buffers(pn_ctx *c, bool report) {
  if (!c->stage_o && dev_alloc(c, (void **)&c->stage_o, (size_t)c->B * PN_FRAME * sizeof(float), false)) return -1;
  if (report && !c->report && dev_alloc(c, (void **)&c->report, (size_t)c->B * PN_REPORT_WORDS * 4, true)) return -1;
  return 0;
}
extern "C" int pn_ctx_set_report(pn_ctx *c, int enable) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  if (enable) { PN_ON_DEVICE(c); if (stage_buffers(c, true)) return -1; }
  else c->next_report = NULL;                            // a pending pn_host_next_report goes with it
  c->report_on = enable != 0;
  return 0;
}
extern "C" int pn_ctx_set_output_saturate(pn_ctx *c, int enable) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  if (enable) { PN_ON_DEVICE(c); if (stage_buffers(c, false)) return -1; }
  c->saturate = enable != 0;
  return 0;
}
static int report_copy(pn_ctx *c, void *dst, hipMemcpyKind kind) {
  if (!c || !dst) { pn_set_error("NULL argument"); return -1; }
  if (!c->report_on) { pn_set_error("the frame report is off (pn_ctx_set_report)"); return -1; }
  PN_ON_DEVICE(c);
  PN_HIP_CHECK(hipMemcpyAsync(dst, c->report, (size_t)c->B * PN_REPORT_WORDS * 4, kind, c->stream));
  if (kind == hipMemcpyDeviceToHost) PN_HIP_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int pn_ctx_read_report(pn_ctx *c, void *h_report) { return report_copy(c, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_ctx_read_report_dev(pn_ctx *c, void *d_report) { return report_copy(c, d_report, hipMemcpyDeviceToDevice); }
// The next pn_submit_host_* call copies its frame's records into its pipeline slot on the context's stream and from there to
// h_report on the device-to-host stream, behind h_out.  (NULL cancels; the slot copies are allocated here.)
extern "C" int pn_host_next_report(pn_ctx *c, void *h_report) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  if (!c->report_on) { pn_set_error("the frame report is off (pn_ctx_set_report)"); return -1; }
  if (h_report) {
    PN_ON_DEVICE(c);
    for (int k = 0; k < 2; k++)
      if (!c->pipe.report[k] && dev_alloc(c, (void **)&c->pipe.report[k], (size_t)c->B * PN_REPORT_WORDS * 4, false)) return -1;
  }
  c->next_report = h_report;
  return 0;
}

// ---- per-stream attenuation limit ----------------------------------------------------------------------------------------
// lam = 10^(-L/20) in double, rounded to fp32 once; a factor below FLT_MIN is 0 (off), so no subnormal reaches the device
extern "C" float pn_atten_limit_factor(float db) {
  if (!(db >= 0.f)) return NAN;                          // negative or NaN
  const float lam = (float)pow(10.0, -(double)db / 20.0);
  return lam < FLT_MIN ? 0.f : lam;
}
// ids distinct and in range, every value >= 0 (+inf = off): else -1 before anything is staged or launched.  The (lam, mu) pairs
// travel with the ids through the pinned slot ring and are scattered on the context's stream, between the frames submitted
// before and after the call, like pn_ctx_reset_streams.
extern "C" int pn_ctx_set_atten_limit(pn_ctx *c, const int32_t *ids, int n, const float *db) {
  if (!c || n < 0 || (n > 0 && (!ids || !db))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if (n > c->B) { pn_set_error("%d stream ids in a context of %d", n, c->B); return -1; }
  std::vector<uint8_t> seen((size_t)c->B, 0);
  for (int i = 0; i < n; i++) {
    if (ids[i] < 0 || ids[i] >= c->B) { pn_set_error("stream id %d out of range [0, %d)", ids[i], c->B); return -1; }
    if (seen[ids[i]]++) { pn_set_error("stream id %d listed twice", ids[i]); return -1; }
    if (!(db[i] >= 0.f)) { pn_set_error("attenuation limit %g dB for stream %d: must be >= 0 (+inf = off)", (double)db[i], ids[i]); return -1; }
  }
  PN_ON_DEVICE(c);
  if (!c->lam_mu && dev_alloc(c, (void **)&c->lam_mu, (size_t)c->B * sizeof(float2), true)) return -1;   // zero = every stream off
  std::vector<float2> lm(n);
  for (int i = 0; i < n; i++) { const float lam = pn_atten_limit_factor(db[i]); lm[i] = make_float2(lam, 1.0f - lam); }
  const int *d = stage_ids(c, ids, n, lm.data(), 2 * n);
  if (!d) return -1;
  pn_launch_scatter_pairs(c->stream, c->lam_mu, d, reinterpret_cast<const float2 *>(d + stage_payload_offset(n)), n);
  PN_HIP_CHECK(hipGetLastError());
  for (int i = 0; i < n; i++) {
    c->n_limited += (lm[i].x != 0.f) - (pn_atten_limit_factor(c->atten_db[ids[i]]) != 0.f);
    c->atten_db[ids[i]] = db[i];
  }
  return 0;
}
extern "C" int pn_ctx_get_atten_limit(const pn_ctx *c, float *h_db) {
  if (!c || !h_db) { pn_set_error("bad argument"); return -1; }
  memcpy(h_db, c->atten_db.data(), (size_t)c->B * sizeof(float));
  return 0;
}

extern "C" int pn_process_f32(pn_ctx *c, const float *d_in, float *d_out, float *d_gr) { return process_dev(c, d_in, d_out, d_gr, 0); }
extern "C" int pn_process_i16(pn_ctx *c, const int16_t *d_in, int16_t *d_out, float *d_gr) { return process_dev(c, d_in, d_out, d_gr, 1); }
extern "C" int pn_process_i16_multi(pn_ctx *c, const int16_t *d_in, int16_t *d_out, float *d_gr, int n_frames) {
  if (!c) return -1;
  const size_t fs = (size_t)c->B * PN_FRAME;
  for (int f = 0; f < n_frames; f++)
    if (process_dev(c, d_in + f * fs, d_out + f * fs, d_gr ? d_gr + (size_t)f * c->B * 68 : NULL, 1)) return -1;
  return 0;
}

// ---- per-call active set (pn_active.hip) -----------------------------------------------------------------------------
// ids[0..n): the streams that receive a frame in this call (distinct, any order).  Every other stream keeps ALL of its
// state — as if its rnnoise_process_frame had not been called (denoise.cpp:508-547) — and its rows of d_out / d_gr are
// left as they were; its row of d_in is ignored.  n == n_streams is exactly pn_process_*.
// the active list must name distinct streams of this context; leaves c->act.mark[s] = 1 for the listed ones
static int active_check(pn_ctx *c, const int32_t *ids, int n) {
  if (!c || n < 0 || (n > 0 && !ids)) { pn_set_error("bad argument"); return -1; }
  const int B = c->B;
  if (n > B) { pn_set_error("%d active streams in a context of %d", n, B); return -1; }
  pn_ctx::Active &A = c->act;
  A.mark.assign((size_t)B, 0);
  for (int i = 0; i < n; i++) {
    if (ids[i] < 0 || ids[i] >= B) { pn_set_error("stream id %d out of range [0, %d)", ids[i], B); return -1; }
    if (A.mark[ids[i]]) { pn_set_error("stream id %d listed twice", ids[i]); return -1; }
    A.mark[ids[i]] = 1;
  }
  return 0;
}
static int process_active(pn_ctx *c, const void *d_in, void *d_out, float *d_gr, int is_i16, const int32_t *ids, int n) {
  if (!c || !d_in || !d_out) { pn_set_error("NULL argument"); return -1; }
  if (active_check(c, ids, n)) return -1;
  const int B = c->B;
  pn_ctx::Active &A = c->act;
  if (n == B) return process_dev(c, d_in, d_out, d_gr, is_i16);
  A.inactive.clear();
  for (int s = 0; s < B; s++) if (!A.mark[s]) A.inactive.push_back(s);
  const int ni = (int)A.inactive.size();
  PN_ON_DEVICE(c);
  if (A.ids.cap < ni) {
    int cap = 1024; while (cap < ni) cap *= 2; if (cap > B) cap = B;
    if (dev_alloc(c, (void **)&A.save_synth, (size_t)cap * PN_FRAME * 4, false) ||
        dev_alloc(c, (void **)&A.save_out, (size_t)cap * PN_FRAME * 4, false) || dev_alloc(c, (void **)&A.save_gr, (size_t)cap * 68 * 4, false) ||
        dev_alloc(c, (void **)&A.save_period, (size_t)cap * 4, false) || dev_alloc(c, (void **)&A.save_gain, (size_t)cap * 4, false) ||
        id_ring_reserve(c, A.ids, cap)) return -1;
  }
  if (id_ring_stage(c, A.ids, A.inactive.data(), ni, NULL, 0, ni)) return -1;
  PnActiveArgs a; memset(&a, 0, sizeof(a));
  a.ids = A.ids.d; a.synth = c->st[PN_ST_SYNTH].p; a.last_period = c->side.last_period; a.last_gain = c->side.last_gain;
  a.out = d_out; a.out_row_words = is_i16 ? PN_FRAME / 2 : PN_FRAME; a.d_gr = d_gr;
  a.save_synth = A.save_synth; a.save_out = A.save_out; a.save_gr = A.save_gr; a.save_period = A.save_period; a.save_gain = A.save_gain;
  state_sections(c, a.sec);                             // at the counters the frame below runs with
  pn_launch_inactive_save(c->stream, a, ni);
  if (process_dev(c, d_in, d_out, d_gr, is_i16)) {
    // a refused launch: the frame did not complete and the counters did not advance, but the front end may already have
    // written last_period / last_gain and the caller's rows may hold anything — the SKIPPED streams still get their in-place
    // state and their output rows back, as the header promises (the error message of the refusal is kept)
    a.restore_only = 1;
    pn_launch_inactive_fixup(c->stream, a, ni);
    return -1;
  }
  pn_launch_inactive_fixup(c->stream, a, ni);
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
extern "C" int pn_process_f32_active(pn_ctx *c, const float *d_in, float *d_out, float *d_gr, const int32_t *ids, int n) { return process_active(c, d_in, d_out, d_gr, 0, ids, n); }
extern "C" int pn_process_i16_active(pn_ctx *c, const int16_t *d_in, int16_t *d_out, float *d_gr, const int32_t *ids, int n) { return process_active(c, d_in, d_out, d_gr, 1, ids, n); }

static int process_host(pn_ctx *c, const void *h_in, void *h_out, float *h_gr, int is_i16) {
  if (!c || !h_in || !h_out) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(c);
  if (pipe_drain(c)) return -1;                      // frames still in flight on the pipelined path use io_in/io_out
  const size_t nbytes = (size_t)c->B * PN_FRAME * (is_i16 ? 2 : 4);
  PN_HIP_CHECK(hipMemcpyAsync(c->io_in, h_in, nbytes, hipMemcpyHostToDevice, c->stream));
  if (process_dev(c, c->io_in, c->io_out, NULL, is_i16)) return -1;
  PN_HIP_CHECK(hipMemcpyAsync(h_out, c->io_out, nbytes, hipMemcpyDeviceToHost, c->stream));
  if (h_gr) PN_HIP_CHECK(hipMemcpyAsync(h_gr, c->st[PN_ST_GR].p, (size_t)c->B * 68 * 4, hipMemcpyDeviceToHost, c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int pn_process_host_f32(pn_ctx *c, const float *h_in, float *h_out, float *h_gr) { return process_host(c, h_in, h_out, h_gr, 0); }
extern "C" int pn_process_host_i16(pn_ctx *c, const int16_t *h_in, int16_t *h_out, float *h_gr) { return process_host(c, h_in, h_out, h_gr, 1); }

// ---- pipelined host-buffer path ----------------------------------------------------------------------------
// Copy-in, the 13 launches and copy-out of consecutive frames on three streams with double-buffered device staging:
//   h2d stream:     H2D(t) ........ H2D(t+1) ......
//   compute stream:        frame(t) ........ frame(t+1) ...
//   d2h stream:                     D2H(t) ......... D2H(t+1)
// Slot k = t & 1 is reused by frame t+2 only after the host has seen frame t delivered, which also bounds the frames
// in flight to two.
// Do `busy` and `cand` share a hardware queue?  A 1 ms sleeper goes to `busy`, then a 64-byte copy to `cand`: on a queue of
// its own the copy lands while the sleeper runs; on a shared queue it lands after it.
static int pipe_streams_share(pn_ctx *c, hipStream_t busy, hipStream_t cand, void *d_scratch, void *h_scratch, bool *shared) {
  struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) hipEventDestroy(e); } } ek, ec;     // destroyed on every exit path
  PN_HIP_CHECK(hipEventCreateWithFlags(&ek.e, hipEventDisableTiming));
  PN_HIP_CHECK(hipEventCreateWithFlags(&ec.e, hipEventDisableTiming));
  if (pn_launch_spin(busy, 100000)) { pn_set_error("queue probe: launch failed"); return -1; }
  PN_HIP_CHECK(hipEventRecord(ek.e, busy));
  PN_HIP_CHECK(hipMemcpyAsync(d_scratch, h_scratch, 64, hipMemcpyHostToDevice, cand));
  PN_HIP_CHECK(hipEventRecord(ec.e, cand));
  PN_HIP_CHECK(hipEventSynchronize(ec.e));
  *shared = hipEventQuery(ek.e) == hipSuccess;
  PN_HIP_CHECK(hipEventSynchronize(ek.e));
  (void)c;
  return 0;
}

// One copy stream.  how: 'n' default priority unprobed, 'h' / 'l' a priority stream, 'a' (the default) a default-priority
// stream that shares its queue with none of `others` — up to 6 candidates (the rejected ones stay alive until the end, so
// that the runtime's least-used-queue choice moves on), else the priority stream `fallback`.
int pipe_make_stream(pn_ctx *c, hipStream_t *out, char how, int prio, char fallback, const std::vector<hipStream_t> &others, char *kind) {
  if (how == 'h' || how == 'l') {
    int lo = 0, hi = 0;
    PN_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    PN_HIP_CHECK(hipStreamCreateWithPriority(out, hipStreamNonBlocking, how == 'h' ? hi : lo));
    *kind = how;
    return 0;
  }
  if (how == 'n') { PN_HIP_CHECK(hipStreamCreateWithFlags(out, hipStreamNonBlocking)); *kind = 'n'; return 0; }
  // everything the probe owns is released on EVERY exit path (advisor, round 5: the early returns of PN_HIP_CHECK leaked the
  // scratch buffers and the rejected streams)
  struct Probe {
    void *h_scratch = NULL, *d_scratch = NULL; std::vector<hipStream_t> rejected; hipStream_t cur = nullptr;
    ~Probe() { for (hipStream_t s : rejected) hipStreamDestroy(s); if (cur) hipStreamDestroy(cur); if (d_scratch) hipFree(d_scratch); if (h_scratch) hipHostFree(h_scratch); }
  } pr;
  PN_HIP_CHECK(hipHostMalloc(&pr.h_scratch, 64, hipHostMallocDefault));
  memset(pr.h_scratch, 0, 64);
  PN_HIP_CHECK(hipMalloc(&pr.d_scratch, 64));
  for (int attempt = 0; attempt < 6; attempt++) {
    PN_HIP_CHECK(hipStreamCreateWithFlags(&pr.cur, hipStreamNonBlocking));
    PN_HIP_CHECK(hipMemcpyAsync(pr.d_scratch, pr.h_scratch, 64, hipMemcpyHostToDevice, pr.cur));       // first use of the stream, not timed
    PN_HIP_CHECK(hipStreamSynchronize(pr.cur));
    bool bad = false;
    for (hipStream_t o : others) {
      bool sh = false;
      if (pipe_streams_share(c, o, pr.cur, pr.d_scratch, pr.h_scratch, &sh)) return -1;
      if (sh) { bad = true; break; }
    }
    if (!bad) { *out = pr.cur; pr.cur = nullptr; *kind = 'n'; return 0; }
    pr.rejected.push_back(pr.cur); pr.cur = nullptr;
  }
  PN_HIP_CHECK(hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio));
  *kind = fallback;
  return 0;
}

static int pipe_init_body(pn_ctx *c) {
  pn_ctx::Pipe &P = c->pipe;
  // Each of the three streams of the pipeline needs a hardware queue of its own.  HIP multiplexes the streams of one
  // priority over a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default): in a process that already owns a handful of
  // streams (torch's pools) a copy stream can land on the queue of the compute stream, and the copy of frame t - 1 then
  // runs BEHIND the kernels of frame t instead of beside them (10.6 instead of 9.5 ms per frame at 65 536 streams,
  // profiles/r04q_host_pipeline_queues.log).  Queues of different priorities are never shared — but two copy streams at
  // the non-default priorities cost every kernel of the compute stream ~50 us (back-to-back frames 10.06 instead of
  // 9.48 ms at 65 536 streams; one priority stream costs nothing: profiles/r05_host_pipeline.log).  So: default-priority
  // streams, each PROBED against the streams it must not share a queue with (pipe_make_stream), a priority stream only
  // as the fallback.  PN_PIPE_PRIO = two letters (h2d, d2h) of h / n / l overrides (tools/host_pipeline_probe.py).
  int prio_least = 0, prio_greatest = 0;
  PN_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
  const char *pp = getenv("PN_PIPE_PRIO");
  if (pp && strlen(pp) != 2) pp = NULL;
  if (pipe_make_stream(c, &P.h2d, pp ? pp[0] : 'a', prio_greatest, 'h', busy_streams(c), &P.kind[0])) return -1;     // incl. the row-range chains' streams
  if (pipe_make_stream(c, &P.d2h, pp ? pp[1] : 'a', prio_least, 'l', busy_streams(c), &P.kind[1])) return -1;
  for (int k = 0; k < 2; k++) {
    PN_HIP_CHECK(hipEventCreateWithFlags(&P.in_ready[k], hipEventDisableTiming));
    PN_HIP_CHECK(hipEventCreateWithFlags(&P.done[k], hipEventDisableTiming));
    PN_HIP_CHECK(hipEventCreateWithFlags(&P.delivered[k], hipEventDisableTiming));
  }
  const size_t io_bytes = (size_t)c->B * PN_FRAME * 4, gr_bytes = (size_t)c->B * 68 * 4;
  P.in[0] = c->io_in; P.out[0] = c->io_out;
  if (!P.in[1] && dev_alloc(c, &P.in[1], io_bytes, false)) return -1;          // device buffers belong to the context (freed with it): a retry reuses them
  if (!P.out[1] && dev_alloc(c, &P.out[1], io_bytes, false)) return -1;
  for (int k = 0; k < 2; k++) if (!P.gr[k] && dev_alloc(c, (void **)&P.gr[k], gr_bytes, false)) return -1;
  return 0;
}
// The first pn_submit_host_* call (or pn_host_pipeline_prepare) builds the pipeline: up to 6 attempts x 3 pairings of a 1 ms
// probe on the context's stream — tens of milliseconds, and not legal while that stream is being captured.  A caller on a
// real-time clock calls pn_host_pipeline_prepare once, before its first frame arrives.  A failed build leaves NOTHING behind
// (streams and events of the partial pipeline are destroyed; the next call starts over).
static int pipe_init(pn_ctx *c) {
  pn_ctx::Pipe &P = c->pipe;
  if (P.init) return 0;
  if (pipe_init_body(c)) {
    if (P.h2d) { hipStreamDestroy(P.h2d); P.h2d = nullptr; }
    if (P.d2h) { hipStreamDestroy(P.d2h); P.d2h = nullptr; }
    for (int k = 0; k < 2; k++) {
      if (P.in_ready[k]) { hipEventDestroy(P.in_ready[k]); P.in_ready[k] = nullptr; }
      if (P.done[k]) { hipEventDestroy(P.done[k]); P.done[k] = nullptr; }
      if (P.delivered[k]) { hipEventDestroy(P.delivered[k]); P.delivered[k] = nullptr; }
    }
    return -1;
  }
  P.init = true;
  return 0;
}
extern "C" int pn_host_pipeline_prepare(pn_ctx *c) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(c);
  return pipe_init(c);
}

static int pipe_drain(pn_ctx *c) {
  if (!c->pipe.init) return 0;
  PN_HIP_CHECK(hipStreamSynchronize(c->pipe.h2d));
  PN_HIP_CHECK(hipStreamSynchronize(c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(c->pipe.d2h));
  return 0;
}

// ids != NULL or n >= 0 with active = true: only the listed streams advance (pn_submit_host_*_active)
static int submit_host(pn_ctx *c, const void *h_in, void *h_out, float *h_gr, int is_i16, bool active = false, const int32_t *ids = NULL, int n = 0) {
  if (!c || !h_in || !h_out) { pn_set_error("NULL argument"); return -1; }
  if (active && active_check(c, ids, n)) return -1;          // refused before the frame takes a pipeline slot
  PN_ON_DEVICE(c);
  if (pipe_init(c)) return -1;
  pn_ctx::Pipe &P = c->pipe;
  const int k = (int)(P.submitted & 1);
  void *const h_report = c->next_report;                     // pn_host_next_report: this call's, whatever becomes of it
  c->next_report = NULL;
  if (P.submitted >= 2) PN_HIP_CHECK(hipEventSynchronize(P.delivered[k]));     // frame submitted-2 delivered: slot k is free
  const size_t nbytes = (size_t)c->B * PN_FRAME * (is_i16 ? 2 : 4);
  PN_HIP_CHECK(hipMemcpyAsync(P.in[k], h_in, nbytes, hipMemcpyHostToDevice, P.h2d));
  PN_HIP_CHECK(hipEventRecord(P.in_ready[k], P.h2d));
  PN_HIP_CHECK(hipStreamWaitEvent(c->stream, P.in_ready[k], 0));
  if (active ? process_active(c, P.in[k], P.out[k], h_gr ? P.gr[k] : NULL, is_i16, ids, n)
             : process_dev(c, P.in[k], P.out[k], h_gr ? P.gr[k] : NULL, is_i16)) return -1;
  const size_t report_bytes = (size_t)c->B * PN_REPORT_WORDS * 4;
  if (h_report) PN_HIP_CHECK(hipMemcpyAsync(P.report[k], c->report, report_bytes, hipMemcpyDeviceToDevice, c->stream));   // the next frame rewrites c->report
  PN_HIP_CHECK(hipEventRecord(P.done[k], c->stream));
  PN_HIP_CHECK(hipStreamWaitEvent(P.d2h, P.done[k], 0));
  PN_HIP_CHECK(hipMemcpyAsync(h_out, P.out[k], nbytes, hipMemcpyDeviceToHost, P.d2h));
  if (h_gr) PN_HIP_CHECK(hipMemcpyAsync(h_gr, P.gr[k], (size_t)c->B * 68 * 4, hipMemcpyDeviceToHost, P.d2h));
  if (h_report) PN_HIP_CHECK(hipMemcpyAsync(h_report, P.report[k], report_bytes, hipMemcpyDeviceToHost, P.d2h));
  PN_HIP_CHECK(hipEventRecord(P.delivered[k], P.d2h));
  P.submitted++;
  return 0;
}
// "nn" / "hl" / ...: how the two copy streams of the pipelined path were obtained (pipe_init); "" before the first submit
extern "C" const char *pn_ctx_pipe_streams(pn_ctx *c) { return (c && c->pipe.init) ? c->pipe.kind : ""; }
extern "C" int pn_submit_host_f32(pn_ctx *c, const float *h_in, float *h_out, float *h_gr) { return submit_host(c, h_in, h_out, h_gr, 0); }
extern "C" int pn_submit_host_i16(pn_ctx *c, const int16_t *h_in, int16_t *h_out, float *h_gr) { return submit_host(c, h_in, h_out, h_gr, 1); }
// The pipelined path with a per-call active set: rows of h_in of skipped streams are ignored; their rows of h_out / h_gr are
// UNSPECIFIED (the device staging rows are restored to what they held two frames earlier and copied out with the rest).
extern "C" int pn_submit_host_f32_active(pn_ctx *c, const float *h_in, float *h_out, float *h_gr, const int32_t *ids, int n) { return submit_host(c, h_in, h_out, h_gr, 0, true, ids, n); }
extern "C" int pn_submit_host_i16_active(pn_ctx *c, const int16_t *h_in, int16_t *h_out, float *h_gr, const int32_t *ids, int n) { return submit_host(c, h_in, h_out, h_gr, 1, true, ids, n); }
extern "C" int pn_host_wait(pn_ctx *c) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(c);
  return pipe_drain(c);
}
// Frames of the pipelined host path whose output copy has landed in the caller's buffer (non-blocking: event queries on the
// at most two frames in flight; delivery is in order).  A caller on a real-time clock polls this between arrivals to
// timestamp each frame's delivery (bench.py: arrival-to-delivery latency), which the blocking pn_submit_host_* cannot show.
extern "C" int64_t pn_host_frames_delivered(pn_ctx *c) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  pn_ctx::Pipe &P = c->pipe;
  if (!P.init || P.submitted == 0) return 0;
  DeviceGuard _dg(c->device);
  if (!_dg.ok) { pn_set_error("hipSetDevice(%d) failed", c->device); return -1; }
  int64_t done = P.submitted >= 2 ? P.submitted - 2 : 0;     // everything older than the two newest was waited for by a submit
  for (int64_t f = done; f < P.submitted; f++) {
    const hipError_t e = hipEventQuery(P.delivered[f & 1]);
    if (e == hipSuccess) done = f + 1;
    else { if (e != hipErrorNotReady) { pn_set_error("hipEventQuery failed: %s", hipGetErrorString(e)); return -1; } (void)hipGetLastError(); break; }
  }
  return done;
}
// NUMA placement of a host thread that feeds one device: bind the CALLING THREAD to the CPUs of the NUMA node the device hangs
// off (read from /sys/bus/pci/devices/<bdf>/numa_node), BEFORE it allocates its pinned buffers — first touch then places
// them next to the GPU's root port.  Returns the node (>= 0) when bound, -1 when nothing was changed (msg says why: no
// affinity reported, sysfs unreadable, ...).  Never an error for the caller: an unbound thread is merely slower.
#include <sched.h>
extern "C" int pn_bind_thread_to_device_numa(int device, char *msg, size_t msg_bytes) {
#define PN_SAY(...) do { if (msg && msg_bytes) snprintf(msg, msg_bytes, __VA_ARGS__); } while (0)
  char bdf[64] = {0};
  if (hipDeviceGetPCIBusId(bdf, sizeof(bdf), device) != hipSuccess) { (void)hipGetLastError(); PN_SAY("device %d: no PCI bus id", device); return -1; }
  for (char *p = bdf; *p; p++) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');      // sysfs spells it lower-case
  char path[256];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
  FILE *f = fopen(path, "r");
  int node = -1;
  if (!f || fscanf(f, "%d", &node) != 1) { if (f) fclose(f); PN_SAY("device %d (%s): %s unreadable", device, bdf, path); return -1; }
  fclose(f);
  if (node < 0) { PN_SAY("device %d (%s): the platform reports no NUMA affinity (numa_node = -1)", device, bdf); return -1; }
  snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
  f = fopen(path, "r");
  char list[4096] = {0};
  if (!f || !fgets(list, sizeof(list), f)) { if (f) fclose(f); PN_SAY("device %d (%s): node %d has no cpulist", device, bdf, node); return -1; }
  fclose(f);
  cpu_set_t allowed, want;
  CPU_ZERO(&want);
  if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) { PN_SAY("sched_getaffinity failed"); return -1; }
  int n = 0;
  for (char *p = list; *p && *p != '\n';) {              // "0-3,8,10-11"
    char *e; const long lo = strtol(p, &e, 10); long hi = lo;
    if (e == p) break;
    if (*e == '-') { p = e + 1; hi = strtol(p, &e, 10); }
    for (long c = lo; c <= hi && c < CPU_SETSIZE; c++) if (CPU_ISSET(c, &allowed)) { CPU_SET(c, &want); n++; }
    p = (*e == ',') ? e + 1 : e;
    if (*e != ',') break;
  }
  if (!n) { PN_SAY("device %d (%s): node %d has no CPU inside this thread's affinity mask", device, bdf, node); return -1; }
  if (sched_setaffinity(0, sizeof(want), &want) != 0) { PN_SAY("device %d (%s): sched_setaffinity failed", device, bdf); return -1; }
  PN_SAY("device %d (%s): thread bound to the %d CPUs of NUMA node %d", device, bdf, n, node);
  return node;
}
#undef PN_SAY
extern "C" void *pn_host_alloc(size_t bytes) {
  void *p = NULL;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { pn_set_error("hipHostMalloc(%zu) failed", bytes); return NULL; }
  return p;
}
extern "C" void pn_host_free(void *p) { if (p) hipHostFree(p); }

extern "C" int pn_ctx_read_features(pn_ctx *c, float *h_feat, int32_t *h_silence) {
  if (!c) return -1;
  PN_ON_DEVICE(c);
  if (h_feat)
    PN_HIP_CHECK(hipMemcpy2DAsync(h_feat, PN_NFEAT * 4, c->side.feat, PN_FEAT_STRIDE * 4, PN_NFEAT * 4, c->B, hipMemcpyDeviceToHost, c->stream));
  if (h_silence) PN_HIP_CHECK(hipMemcpyAsync(h_silence, c->side.silence, (size_t)c->B * 4, hipMemcpyDeviceToHost, c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}

// Device-side twin of pn_ctx_read_features: asynchronous copies on the context's stream into caller-owned device
// buffers (d_feat [n_streams][70], d_silence [n_streams] int32; either may be NULL).
extern "C" int pn_ctx_read_features_dev(pn_ctx *c, float *d_feat, int32_t *d_silence) {
  if (!c) return -1;
  PN_ON_DEVICE(c);
  if (d_feat)
    PN_HIP_CHECK(hipMemcpy2DAsync(d_feat, PN_NFEAT * 4, c->side.feat, PN_FEAT_STRIDE * 4, PN_NFEAT * 4, c->B, hipMemcpyDeviceToDevice, c->stream));
  if (d_silence) PN_HIP_CHECK(hipMemcpyAsync(d_silence, c->side.silence, (size_t)c->B * 4, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

extern "C" int pn_ctx_compute_rnn_host(pn_ctx *c, const float *h_feat, float *h_gr) {
  if (!c || !h_feat || !h_gr) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(c);
  if (pipe_drain(c)) return -1;                      // frames in flight on the pipelined path own feat/gr
  PN_HIP_CHECK(hipMemcpy2DAsync(c->side.feat, PN_FEAT_STRIDE * 4, h_feat, PN_NFEAT * 4, PN_NFEAT * 4, c->B, hipMemcpyHostToDevice, c->stream));
  if (launch_rnn(c)) return -1;
  PN_HIP_CHECK(hipMemcpyAsync(h_gr, c->st[PN_ST_GR].p, (size_t)c->B * 68 * 4, hipMemcpyDeviceToHost, c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(c->stream));
  PN_HIP_CHECK(hipGetLastError());
  c->tn++;                                           // only the network's rings advance; the DSP rings keep their frame
  return 0;
}

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

// ---- per-stream state records (pn_stream_state.hip; layout in include/percepnet_hip.h) ------------------------------
// The header words a context writes (export) and expects (import; word 3, the source's nn_mode, is not compared).
static void ss_header(uint32_t hdr[16], const unsigned char digest[32], int nn_mode) {
  memset(hdr, 0, 16 * sizeof(uint32_t));
  hdr[0] = PN_STREAM_STATE_MAGIC; hdr[1] = PN_STREAM_STATE_VERSION; hdr[2] = PN_STREAM_STATE_BYTES; hdr[3] = (uint32_t)nn_mode;
  memcpy(&hdr[4], digest, 32);
}
static uint32_t ss_le32(const unsigned char *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// host twin of the import kernel's check (pn_stream_state.hip ss_check), same order of verdicts
static int ss_check_host(const void *record, size_t bytes, const unsigned char digest[32]) {
  const unsigned char *r = static_cast<const unsigned char *>(record);
  if (bytes < 16) { pn_set_error("stream-state record of %zu bytes: a record has %d", bytes, PN_STREAM_STATE_BYTES); return PN_SS_BAD_SIZE; }
  if (ss_le32(r) != PN_STREAM_STATE_MAGIC) { pn_set_error("not a stream-state record (magic 0x%08x)", ss_le32(r)); return PN_SS_BAD_MAGIC; }
  if (ss_le32(r + 4) != PN_STREAM_STATE_VERSION) { pn_set_error("stream-state record version %u, this library reads %d", ss_le32(r + 4), PN_STREAM_STATE_VERSION); return PN_SS_BAD_VERSION; }
  if (ss_le32(r + 8) != PN_STREAM_STATE_BYTES || bytes != PN_STREAM_STATE_BYTES) {
    pn_set_error("stream-state record of %zu bytes (header: %u), a record has %d", bytes, ss_le32(r + 8), PN_STREAM_STATE_BYTES);
    return PN_SS_BAD_SIZE;
  }
  if (memcmp(r + 16, digest, 32)) { pn_set_error("stream-state record written under another model (pn_model_digest differs)"); return PN_SS_BAD_MODEL; }
  return PN_SS_OK;
}
extern "C" size_t pn_stream_state_bytes(void) { return PN_STREAM_STATE_BYTES; }
extern "C" int pn_stream_state_check(const void *record, size_t bytes, const pn_model *m) {
  if (!record || !m) { pn_set_error("NULL argument"); return PN_SS_BAD_ARG; }
  return ss_check_host(record, bytes, m->sha256);
}
static const unsigned char *ctx_digest(const pn_ctx *c) { return std::get<0>(c->weights_key).data(); }

// ids in range (and distinct when `distinct`)
static int ss_ids_check(pn_ctx *c, const int32_t *ids, int n, bool distinct) {
  std::vector<uint8_t> seen(distinct ? (size_t)c->B : 0, 0);
  for (int i = 0; i < n; i++) {
    if (ids[i] < 0 || ids[i] >= c->B) { pn_set_error("stream id %d out of range [0, %d)", ids[i], c->B); return -1; }
    if (distinct && seen[ids[i]]++) { pn_set_error("stream id %d listed twice", ids[i]); return -1; }
  }
  return 0;
}
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
  if (ss_ids_check(c, ids, n, false)) return -1;
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
  if (ss_ids_check(c, ids, n, true)) return -1;
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

// Host forms: synchronous, frames in flight on the pipelined path are completed first (like rnn_state_copy).  The records
// pass through a device buffer of their own size, freed before returning.
extern "C" int pn_ctx_export_streams_host(pn_ctx *c, const int32_t *ids, int n, void *h_records) {
  if (!c || n < 0 || (n > 0 && (!ids || !h_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if (ss_ids_check(c, ids, n, false)) return -1;
  PN_ON_DEVICE(c);
  if (pipe_drain(c)) return -1;
  const size_t bytes = (size_t)n * PN_STREAM_STATE_BYTES;
  void *d = NULL;
  PN_HIP_CHECK(hipMalloc(&d, bytes));
  int rc = pn_ctx_export_streams(c, ids, n, d);
  if (!rc && hipMemcpyAsync(h_records, d, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) { pn_set_error("record copy failed"); rc = -1; }
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) { pn_set_error("export failed"); rc = -1; }
  hipFree(d);
  return rc;
}
extern "C" int pn_ctx_import_streams_host(pn_ctx *c, const int32_t *ids, int n, const void *h_records) {
  if (!c || n < 0 || (n > 0 && (!ids || !h_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if (ss_ids_check(c, ids, n, true)) return -1;
  for (int i = 0; i < n; i++)                          // all or nothing: every header before anything is launched
    if (ss_check_host(static_cast<const char *>(h_records) + (size_t)i * PN_STREAM_STATE_BYTES, PN_STREAM_STATE_BYTES, ctx_digest(c))) {
      std::string why = pn_last_error();
      pn_set_error("record %d refused: %s", i, why.c_str());
      return -1;
    }
  PN_ON_DEVICE(c);
  if (pipe_drain(c)) return -1;
  const size_t bytes = (size_t)n * PN_STREAM_STATE_BYTES;
  void *d = NULL;
  PN_HIP_CHECK(hipMalloc(&d, bytes + (size_t)n * sizeof(int32_t)));
  int32_t *d_status = reinterpret_cast<int32_t *>(static_cast<char *>(d) + bytes);
  std::vector<int32_t> status(n, 0);
  int rc = hipMemcpyAsync(d, h_records, bytes, hipMemcpyHostToDevice, c->stream) == hipSuccess ? 0 : -1;
  if (rc) pn_set_error("record copy failed");
  if (!rc) rc = pn_ctx_import_streams(c, ids, n, d, d_status);
  if (!rc && hipMemcpyAsync(status.data(), d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess) { pn_set_error("status copy failed"); rc = -1; }
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) { pn_set_error("import failed"); rc = -1; }
  hipFree(d);
  for (int i = 0; i < n && !rc; i++)
    if (status[i]) { pn_set_error("record %d refused on the device (%d) after passing the host check", i, status[i]); rc = -1; }
  return rc;
}

// Debug tap (tests/tools only): copy an internal device buffer to the host.
// which: 0 feat[B][128], 1 c1ring[5][B][128], 2 c2ring[3][B][512], 3 c2out[B][512],
//        4..7 gru[i][2][B][512], 8 rb[2][B][128], 9 gr[B][68], 10 look-ahead spectra ring, 11 comb-filtered spectrum,
//        12 history ring, 13 last_period int32 [B].  Returns the byte count.
extern "C" long long pn_ctx_debug_copy(pn_ctx *c, int which, void *dst, long long max_bytes) {
  if (!c || !dst) return -1;
  static const int entry[14] = {PN_ST_FEAT, PN_ST_C1RING, PN_ST_C2RING, PN_ST_C2OUT, PN_ST_GRU1, PN_ST_GRU2, PN_ST_GRU3, PN_ST_GRU_GB, PN_ST_RB,
                                PN_ST_GR, PN_ST_YRING, PN_ST_PS, PN_ST_HIST, PN_ST_LAST_PERIOD};
  if (which < 0 || which >= 14) { pn_set_error("bad debug buffer id"); return -1; }
  const void *src = c->st[entry[which]].p; const size_t n = c->st[entry[which]].words * 4;
  if ((long long)n > max_bytes) { pn_set_error("debug buffer needs %zu bytes", n); return -1; }
  PN_ON_DEVICE(c);
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  if (hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) { pn_set_error("debug copy failed"); return -1; }
  return (long long)n;
}
