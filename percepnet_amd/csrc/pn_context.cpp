// Host side of libpercepnet_hip: batched contexts — lifecycle, settings, the per-frame launch sequence, the active set — and
// their part of the C-ABI declared in include/percepnet_hip.h.  Mirrors the reference's frame engine
// (rnnoise_create/init/process_frame, denoise.cpp:252-280,508-547) for B streams in lock-step.  (Self-tests: pn_selftest.cpp;
// pipelined host path: pn_host_pipe.cpp; state I/O: pn_stream_state.cpp.)
#include "pn_context.h"
#include <stdio.h>
#include <float.h>
#include <math.h>

extern "C" int pn_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

// ---- contexts -----------------------------------------------------------------------------------------

static thread_local bool g_last_alloc_oom = false;     // the last dev_alloc failure on this thread was hipErrorOutOfMemory
bool &last_alloc_oom() { return g_last_alloc_oom; }
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
extern "C" void pn_ctx_destroy(pn_ctx *c) {
  if (!c) return;
  DeviceGuard _dg(c->device);
  hipStreamSynchronize(c->stream);
  pipe_destroy(c);
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

int open_device(int device, void *hip_stream, DeviceGuard &guard, hipStream_t *stream, bool *own_stream) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    pn_set_error("no HIP device available (this library has no CPU fallback)");
    return -1;
  }
  if (device < 0 || device >= ndev) { pn_set_error("device %d out of range (%d devices)", device, ndev); return -1; }
  guard.enter(device);
  if (!guard.ok) { pn_set_error("hipSetDevice(%d) failed", device); return -1; }
  *stream = (hipStream_t)hip_stream; *own_stream = !hip_stream;
  if (!hip_stream && hipStreamCreateWithFlags(stream, hipStreamNonBlocking) != hipSuccess) { pn_set_error("hipStreamCreate failed"); return -1; }
  return 0;
}

pn_ctx *ctx_create(const pn_model *model, int device, int n_streams, int nn_mode, void *hip_stream, bool selftest, const PnPlan *plan) {
  if (!model) { pn_set_error("NULL model"); return NULL; }
  if (n_streams < 1) { pn_set_error("n_streams must be >= 1"); return NULL; }
  if (nn_mode != PN_NN_MFMA && nn_mode != PN_NN_STRICT && nn_mode != PN_NN_MFMA_F16 && nn_mode != PN_NN_MFMA_X3) { pn_set_error("bad nn_mode %d", nn_mode); return NULL; }
  DeviceGuard _dg; hipStream_t stream; bool own_stream;
  if (open_device(device, hip_stream, _dg, &stream, &own_stream)) return NULL;
  pn_ctx *c = new pn_ctx();
  c->stream = stream; c->own_stream = own_stream;
  c->device = device; c->B = n_streams; c->Bp = ((size_t)n_streams + 255) / 256 * 256; c->nn_mode = nn_mode; c->plan = plan ? *plan : pn_plan_for(n_streams, nn_mode);
  c->t = 0; c->tn = 0; c->bytes = 0; c->profiling = false;
  memset(c->fam_ms, 0, sizeof(c->fam_ms)); memset(c->fam_n, 0, sizeof(c->fam_n));
  memset(c->L, 0, sizeof(c->L));
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
  if (!c) { pn_set_error("bad argument"); return -1; }
  if (pn_ids_check(c->B, ids, n, false)) return -1;
  if (n == 0) return 0;
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

// launch k of front-end family fe: row fe of this table is row fe of pn_kFe, its launchers in the order of that row's fam[]
void pn_launch_fe(hipStream_t st, const PnTables *T, int n_streams, int fe, int k, const PnDspSide &s, const PnDspSlots &sl, const PnDspIn &in, int grid_cap) {
  static PnFeLaunch *const launch[][3] = {{pn_launch_frontend}, {pn_launch_frontend_g2}, {pn_launch_fe_spec_in, pn_launch_fe_pitch, pn_launch_fe_spec_out}};
  static_assert(sizeof(launch) / sizeof(launch[0]) == sizeof(pn_kFe) / sizeof(pn_kFe[0]) && sizeof(launch[0]) / sizeof(launch[0][0]) == sizeof(pn_kFe[0].fam) / sizeof(int),
                "one row of launchers per front-end family of pn_kFe");
  launch[fe][k](st, T, n_streams, s, sl, in, grid_cap);
}

int process_dev(pn_ctx *c, const void *d_in, void *d_out, float *d_gr, int is_i16) {
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
  if (!c || (n > 0 && !db)) { pn_set_error("bad argument"); return -1; }
  if (pn_ids_check(c->B, ids, n, true)) return -1;
  if (n == 0) return 0;
  for (int i = 0; i < n; i++) {
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
int active_check(pn_ctx *c, const int32_t *ids, int n) {
  if (!c) { pn_set_error("bad argument"); return -1; }
  return pn_ids_check(c->B, ids, n, true, &c->act.mark);
}
int process_active(pn_ctx *c, const void *d_in, void *d_out, float *d_gr, int is_i16, const int32_t *ids, int n) {
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
