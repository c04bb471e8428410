// The host-buffer side of a batched context beyond the synchronous pn_process_host_*: the pipelined path (pn_submit_host_*) with
// the queue probe its copy streams are chosen by, and the helpers of the host thread that feeds it (NUMA binding, pinned buffers).
#include "pn_context.h"
#include <stdio.h>

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
// the streams and events of the pipeline, whole (pn_ctx_destroy) or partly built (a failed pipe_init)
void pipe_destroy(pn_ctx *c) {
  pn_ctx::Pipe &P = c->pipe;
  for (hipStream_t *s : {&P.h2d, &P.d2h}) if (*s) hipStreamSynchronize(*s);
  for (int k = 0; k < 2; k++)
    for (hipEvent_t *e : {&P.in_ready[k], &P.done[k], &P.delivered[k]}) if (*e) { hipEventDestroy(*e); *e = nullptr; }
  for (hipStream_t *s : {&P.h2d, &P.d2h}) if (*s) { hipStreamDestroy(*s); *s = nullptr; }
  P.init = false;
}
// The first pn_submit_host_* call (or pn_host_pipeline_prepare) builds the pipeline: up to 6 attempts x 3 pairings of a 1 ms
// probe on the context's stream — tens of milliseconds, and not legal while that stream is being captured.  A caller on a
// real-time clock calls pn_host_pipeline_prepare once, before its first frame arrives.  A failed build leaves NOTHING behind
// (streams and events of the partial pipeline are destroyed; the next call starts over).
static int pipe_init(pn_ctx *c) {
  pn_ctx::Pipe &P = c->pipe;
  if (P.init) return 0;
  if (pipe_init_body(c)) { pipe_destroy(c); return -1; }
  P.init = true;
  return 0;
}
extern "C" int pn_host_pipeline_prepare(pn_ctx *c) {
  if (!c) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(c);
  return pipe_init(c);
}

int pipe_drain(pn_ctx *c) {
  if (!c->pipe.init) return 0;
  PN_HIP_CHECK(hipStreamSynchronize(c->pipe.h2d));
  PN_HIP_CHECK(hipStreamSynchronize(c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(c->pipe.d2h));
  return 0;
}
// One frame of the pipeline, whoever's it is (the context's own frame, or a rate converter's: pn_rate.cpp).  st: the two device
// staging pairs of its owner and the bytes of a whole batch of rows; body(arg, d_in, d_out, d_gr) queues the frame's launches
// on the context's stream from st.in[k] to st.out[k] (d_gr: the slot's g|r rows, or NULL).  The streams, the slot counter, the
// events, the g|r and report slots and the two-frames-in-flight bound are the context's, so frames of either kind count in
// submission order.  The caller has refused everything it refuses BEFORE this call: from here on the frame owns slot k.
int pipe_submit(pn_ctx *c, const PipeStaging &st, const void *h_in, void *h_out, float *h_gr, PipeBody body, void *arg) {
  if (pipe_init(c)) return -1;
  pn_ctx::Pipe &P = c->pipe;
  const int k = (int)(P.submitted & 1);
  void *const h_report = c->next_report;                     // pn_host_next_report: this call's, whatever becomes of it
  c->next_report = NULL;
  if (P.submitted >= 2) PN_HIP_CHECK(hipEventSynchronize(P.delivered[k]));     // frame submitted-2 delivered: slot k is free
  PN_HIP_CHECK(hipMemcpyAsync(st.in[k], h_in, st.bytes, hipMemcpyHostToDevice, P.h2d));
  PN_HIP_CHECK(hipEventRecord(P.in_ready[k], P.h2d));
  PN_HIP_CHECK(hipStreamWaitEvent(c->stream, P.in_ready[k], 0));
  if (body(arg, st.in[k], st.out[k], h_gr ? P.gr[k] : NULL)) return -1;
  const size_t report_bytes = (size_t)c->B * PN_REPORT_WORDS * 4;
  if (h_report) PN_HIP_CHECK(hipMemcpyAsync(P.report[k], c->report, report_bytes, hipMemcpyDeviceToDevice, c->stream));   // the next frame rewrites c->report
  PN_HIP_CHECK(hipEventRecord(P.done[k], c->stream));
  PN_HIP_CHECK(hipStreamWaitEvent(P.d2h, P.done[k], 0));
  PN_HIP_CHECK(hipMemcpyAsync(h_out, st.out[k], st.bytes, hipMemcpyDeviceToHost, P.d2h));
  if (h_gr) PN_HIP_CHECK(hipMemcpyAsync(h_gr, P.gr[k], (size_t)c->B * 68 * 4, hipMemcpyDeviceToHost, P.d2h));
  if (h_report) PN_HIP_CHECK(hipMemcpyAsync(h_report, P.report[k], report_bytes, hipMemcpyDeviceToHost, P.d2h));
  PN_HIP_CHECK(hipEventRecord(P.delivered[k], P.d2h));
  P.submitted++;
  return 0;
}
// the context's own frame: ids != NULL or n >= 0 with active = true: only the listed streams advance (pn_submit_host_*_active)
struct CtxFrame { pn_ctx *c; int is_i16; bool active; const int32_t *ids; int n; };
static int ctx_frame_body(void *arg, void *d_in, void *d_out, float *d_gr) {
  const CtxFrame &f = *static_cast<const CtxFrame *>(arg);
  return f.active ? process_active(f.c, d_in, d_out, d_gr, f.is_i16, f.ids, f.n) : process_dev(f.c, d_in, d_out, d_gr, f.is_i16);
}
static int submit_host(pn_ctx *c, const void *h_in, void *h_out, float *h_gr, int is_i16, bool active = false, const int32_t *ids = NULL, int n = 0) {
  if (!c || !h_in || !h_out) { pn_set_error("NULL argument"); return -1; }
  if (active && active_check(c, ids, n)) return -1;          // refused before the frame takes a pipeline slot
  PN_ON_DEVICE(c);
  if (pipe_init(c)) return -1;                               // (P.in[1] / P.out[1] exist from here on)
  const pn_ctx::Pipe &P = c->pipe;
  const PipeStaging st = {{P.in[0], P.in[1]}, {P.out[0], P.out[1]}, (size_t)c->B * PN_FRAME * (is_i16 ? 2 : 4)};
  CtxFrame f = {c, is_i16, active, ids, n};
  return pipe_submit(c, st, h_in, h_out, h_gr, ctx_frame_body, &f);
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
