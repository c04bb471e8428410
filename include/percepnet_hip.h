/* libpercepnet_hip.so — C-ABI of the MI355X-native batched PercepNet inference path.
 *
 * Two layers of entry points:
 *
 *  (1) The reference's own frame-engine interface (reference src/rnnoise.h:49-68), same names,
 *      argument meaning and return values, so existing callers (reference src/main.cpp:30-39)
 *      re-link unchanged.  The reference compiles its "C" API as C++ (no extern "C" in
 *      rnnoise.h), so its exported symbols are Itanium-mangled; this library exports BOTH the
 *      mangled names (csrc/rnnoise_compat.cpp) and the extern "C" ones declared below with a
 *      pn_ prefix-free alias set (`rnnoise_*_c`).
 *
 *  (2) The batched interface the GPU needs: one context = B independent 48 kHz streams advanced
 *      in lock-step, one 10 ms frame (480 samples) per stream per call.  Plain pointers and
 *      sizes only; device pointers are raw HIP device addresses (e.g. torch's data_ptr()).
 *      8, 16, 24 and 32 kHz streams go through a pn_rate beside the context (the rate converter, below), all at one rate or, with
 *      a mixed converter, each stream at its own, 48 kHz included.
 *
 * All functions are thread-compatible per context; one context belongs to one HIP device.
 * Errors: functions returning int give 0 on success, <0 on failure; pn_last_error() returns a
 * thread-local description.  The library never falls back to a CPU path: if no HIP device is
 * usable, context creation fails.
 */
#ifndef PERCEPNET_HIP_H
#define PERCEPNET_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "percepnet_nnet_data.h"

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared between this push and its pop (plus the
   reference's nine C++-mangled names, csrc/rnnoise_compat.cpp) are exported.  Harmless for callers. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define PN_FRAME_SIZE 480      /* reference denoise.cpp:19 */
#define PN_NB_BANDS 34         /* reference denoise.cpp:35 */
#define PN_NB_FEATURES 70      /* reference denoise.cpp:40 */

typedef struct pn_ctx pn_ctx;
typedef struct pn_model pn_model;

/* Network evaluation mode. */
enum {
  PN_NN_MFMA = 0,    /* fp32 MFMA GEMM over the stream batch (v_mfma_f32_32x32x2_f32): each output
                        is a k-ascending fmaf chain from the bias — the reference's summation
                        order (nnet.cpp:59-72) with fused instead of separate rounding */
  PN_NN_STRICT = 1,  /* one lane per (stream, neuron), separate mul and add in the reference's
                        order: bit-identical to the CPU reference; slow, for parity tests */
  PN_NN_MFMA_F16 = 2,/* BASELINE configs[4]: the GEMM operands (weights and activations) of conv1, conv2, the five
                        GRUs and fc_gb rounded to fp16, fp32 accumulation (v_mfma_f32_32x32x16_f16); fc (70 inputs)
                        and fc_rb (K = 128) run on the fp32 kernels; bias, activations, gating, state, DSP fp32.
                        Operands beyond +-65504 saturate (PERCEPNET_X3_SATCOUNT=1 counts them).
                        Tolerance re-stated: DESIGN.md 4.2b (6 LSB bound, 4 measured) */
  PN_NN_MFMA_X3 = 3  /* split precision: every fp32 GEMM operand is carried as an fp16 (hi, lo) pair and every
                        product formed as lo*hi + hi*lo + hi*hi by three v_mfma_f32_32x32x16_f16 into an fp32
                        accumulator (operand error ~2^-22, below the reference's own accumulation rounding);
                        state, gating and activations fp32.  Same parity bounds as PN_NN_MFMA */
};

/* ---- models ------------------------------------------------------------------------------ */
/* Borrow an in-memory RNNModel laid out as nnet_data.h lays it out (replaces the reference's
   link-time `percepnet_model_orig`, denoise.cpp:49-51,267).  The arrays are copied. */
pn_model *pn_model_from_rnnmodel(const RNNModel *m);
/* Load the PNW1 container (percepnet_amd/weights.py) — this library's implementation of the
   declared-but-undefined rnnoise_model_from_file (rnnoise.h:62). */
pn_model *pn_model_from_blob(const void *blob, size_t nbytes);
pn_model *pn_model_from_file(FILE *f);
void pn_model_free(pn_model *m);

/* ---- batched contexts ---------------------------------------------------------------------- */
/* device: HIP device ordinal; n_streams >= 1; stream: a hipStream_t to launch on (NULL = the
   context creates its own non-blocking stream).  State starts all-zero (rnnoise_init,
   denoise.cpp:259-280). */
pn_ctx *pn_ctx_create(const pn_model *model, int device, int n_streams, int nn_mode, void *hip_stream);
void pn_ctx_destroy(pn_ctx *ctx);
int pn_ctx_reset(pn_ctx *ctx);                       /* zero all stream state, frame counter = 0 */
/* Per-stream lifecycle: put the n streams ids[0..n) (host array, each in [0, n_streams), duplicates allowed) back into
   the state rnnoise_init leaves ONE DenoiseState in (denoise.cpp:259-280: all-zero DSP and network state) while every
   other stream of the context keeps its state and the context keeps its frame counter — the batched counterpart of
   rnnoise_destroy + rnnoise_create for a slot whose call has ended and whose next call begins.  Asynchronous on the
   context's stream: it takes effect between the frames submitted before and after it (also on the pipelined host path).
   The first frame processed after it is that stream's frame 0 (its first output frame is the one main.cpp:37 skips). */
int pn_ctx_reset_streams(pn_ctx *ctx, const int32_t *ids, int n);
int pn_ctx_n_streams(const pn_ctx *ctx);
int64_t pn_ctx_frames_done(const pn_ctx *ctx);
size_t pn_ctx_device_bytes(const pn_ctx *ctx);       /* HBM footprint of state + weights (weights only if this context created their device copy) */
/* Bytes of the packed weight copy this context reads — its own or one shared with other contexts of the same model content,
   device and network mode (pn_ctx_describe: weights=own|shared).  A shared copy outlives its creator while any user lives,
   and is then reported by no context's pn_ctx_device_bytes: add it once per distinct copy when summing a process. */
size_t pn_ctx_weight_bytes(const pn_ctx *ctx);
/* Which kernel families this context launches (chosen at creation from its batch size and nn_mode), as a
   NUL-terminated "key=value ..." string, e.g. "nn=mfma_f32 dense=batch gru=batch gru_rb=batch narrow=n16 frontend=split".
   gru / gru_rb: small | batch | direct_rows32 | direct_rows64 (fp32 mode from 24 576 streams: the GRU steps read fragment-order
   fp32 shadows of their inputs, +19 KB of device memory per stream, results bit-identical) | x3_* / f16_* in the shadow-operand
   modes; narrow: n16 | batch | small | fc_gb:n48+fc_rb:batch.  Returns the length written (excluding the NUL) or -1. */
int pn_ctx_describe(const pn_ctx *ctx, char *buf, size_t buf_bytes);

/* Advance every stream by one frame.  Device-resident buffers, asynchronous on the context's
   stream.  in: [n_streams][480]; out: [n_streams][480]; gr (optional, may be NULL):
   [n_streams][68] = g[34] | r[34], the reference's feature_test.raw tap (denoise.cpp:533-534).
   f32 = the rnnoise_process_frame sample convention (nominal [-1,1));
   i16 = the CLI convention (main.cpp:34,36): in/32768.f, out = trunc(x*32768) wrapped to 16 bit
   (saturated instead after pn_ctx_set_output_saturate).
   in and out may alias.
   Ordering is the caller's: the launches only see what is complete on the context's stream.  A
   context created with hip_stream = NULL runs on its own NON-BLOCKING stream, which does not
   synchronise with the null stream or with any other stream: buffers filled by another stream
   (or by hipMemcpyAsync) must be ordered first (hipStreamWaitEvent / a synchronise), and the
   outputs consumed after pn_ctx_synchronize or an event on that stream. */
int pn_process_f32(pn_ctx *ctx, const float *d_in, float *d_out, float *d_gr);
int pn_process_i16(pn_ctx *ctx, const int16_t *d_in, int16_t *d_out, float *d_gr);
/* Per-call ACTIVE SET.  In the reference a stream's state advances only when ITS rnnoise_process_frame is called
   (src/denoise.cpp:508-547, src/rnnoise.h:60); these calls advance only the n streams listed in ids[] (host array,
   distinct ids, any order).  Every other stream keeps all of its state — history, look-ahead, pitch memory, synthesis
   memory, conv FIFOs, GRU states — bit for bit as if the call had not happened for it: its row of d_in is ignored, its rows
   of d_out and d_gr are left untouched, and when it is listed again it continues exactly like a reference stream that was
   only fed the frames it received.  (pn_ctx_read_features rows of a skipped stream are undefined for that tick.)
   n == n_streams is pn_process_*; the cost is paid per SKIPPED stream (two small launches over those rows: ~4 KB saved
   and ~52 KB of ring entries shifted per skipped stream-tick), nothing is added to an all-active call. */
int pn_process_f32_active(pn_ctx *ctx, const float *d_in, float *d_out, float *d_gr, const int32_t *ids, int n);
int pn_process_i16_active(pn_ctx *ctx, const int16_t *d_in, int16_t *d_out, float *d_gr, const int32_t *ids, int n);
/* The same on the pipelined host path (see pn_submit_host_* below): rows of h_in of skipped streams are ignored; their rows of
   h_out / h_gr are UNSPECIFIED for that frame (the caller knows which streams it listed).  A refused id list consumes no slot. */
int pn_submit_host_f32_active(pn_ctx *ctx, const float *h_in, float *h_out, float *h_gr, const int32_t *ids, int n);
int pn_submit_host_i16_active(pn_ctx *ctx, const int16_t *h_in, int16_t *h_out, float *h_gr, const int32_t *ids, int n);
/* Optional output stage: the reference's envelope post-filter
   (post_filtering, denoise.cpp:216-250), which it only runs on train()'s TEST synthesis (743),
   applied to the gains inside the back-end kernel between the g/r tap and pitch_filter — the same
   place.  Off by default (= rnnoise_process_frame exactly); the tap keeps the network's raw g.
   Takes effect from the next frame. */
int pn_ctx_set_postfilter(pn_ctx *ctx, int enable);
/* Per-stream ATTENUATION LIMIT (suppression strength per call).  Stream s has a limit L_s in dB, 0 <= L_s <= +inf, default
   +inf = off.  The host turns it into lam_s = (float)pow(10.0, -(double)L_s / 20.0) (double, rounded to fp32 once; a factor
   below FLT_MIN, i.e. L_s > ~758.6 dB, becomes 0 = off, so +inf gives 0 and 0 dB gives 1) and mu_s = 1.0f - lam_s (fp32).
   In the back end, for every bin k < 400 and both the real and the imaginary part, with a = X_k as analysed (before
   pitch_filter) and y the value after pitch_filter (non-silent frames) and the gain stage, before the 1/960 scale:
       lam_s != 0:  y <- (mu_s * y) + (lam_s * a)     (two fp32 products, then the fp32 sum; no FMA)
   lam_s == 0 runs the unlimited arithmetic exactly.  Bins >= 400 stay exactly 0 (the engine keeps bins 0..399), so 0 dB is a
   BYPASS: the input band-limited to 20 kHz and delayed like the enhanced signal, by 2880 samples from input frame t to output
   frame t.  The mix
   applies to silent frames too (y is then the gained X) and after the optional post-filter; the g|r tap stays the network's
   raw output, and nothing upstream of the synthesis (features, pitch, network state) depends on the limit.
   pn_atten_limit_factor: host only, needs no GPU: lam for `db` as above; NaN for db < 0 or NaN.
   pn_ctx_set_atten_limit: streams ids[0..n) (host array, DISTINCT, in range) get the limits db[0..n) (host array).  An id out of
   range, a duplicate id or a db that is NaN or negative refuses the call: -1, pn_last_error set, nothing changed or launched.
   n == 0 is a no-op.  Ordered exactly like pn_ctx_reset_streams: asynchronous on the context's stream, frames submitted before
   the call use the old values and frames submitted after it the new ones (also on the pipelined host path); the caller may
   reuse its arrays when the call returns.  While no stream of the context is limited, a frame runs the same back-end kernel
   as a context that never set a limit.
   pn_ctx_get_atten_limit: the values as last set, [n_streams] floats (+INFINITY = off).
   Lifecycle: pn_ctx_reset sets every stream back to off; pn_ctx_reset_streams sets the listed streams back to off (a reset
   slot is a new call); streams skipped by pn_process_*_active keep their limit (a setting, not per-tick state); stream-state
   records do not carry it (format, version and size unchanged): an imported stream continues under the target slot's own
   setting. */
float pn_atten_limit_factor(float db);
int pn_ctx_set_atten_limit(pn_ctx *ctx, const int32_t *ids, int n, const float *db);
int pn_ctx_get_atten_limit(const pn_ctx *ctx, float *h_db);
/* Per-stream FRAME REPORT and SATURATING int16 output: one more kernel after the back end (csrc/pn_outstage.hip), launched only
   while one of the two is on; with both off (the default) a frame launches exactly what it always did.
   pn_ctx_set_report(ctx, 1): every following frame also leaves one record per stream on the device, PN_REPORT_WORDS = 8
   little-endian 32-bit words, [n_streams][8]:
     0  f32  in_peak       max |x| over the 480 input samples this output frame is about: the stream's input frame 6 frames
                           (2880 samples, the engine's delay: INTEGRATION.md §2) back, in the float convention (int16 / 32768),
                           read from the history ring; 0 for the first 6 frames of a stream after a reset.  The ring holds
                           whatever a float entry point was given: a NaN sample is ignored here (0 for a frame of 480 NaNs),
                           an infinite one gives +inf
     1  f32  in_energy     sum of x * x over those samples: the fixed-order fp32 sum of fp32 products, so NaN as soon as one
                           sample is NaN, +inf otherwise when a product or the sum overflows (|x| > ~1.8e19)
     2  f32  out_peak      max |o| over the 480 output samples o before any cast (a NaN sample is ignored here: 0 for a frame
                           of 480 NaNs; an infinite sample gives +inf)
     3  f32  out_energy    sum of o * o, with in_energy's rules: NaN as soon as one sample is NaN, +inf on overflow otherwise
     4  f32  gain_mean     (sum of g_b) / 34 over the network's raw g (the first 34 words of the g|r tap)
     5  i32  pitch_period  the period this frame's comb filter used (pn_ctx_debug_copy's buffer 13)
     6  i32  out_clipped   output samples whose t = o * 32768 (fp32) lies outside the open interval (-32769, 32768), i.e. that do
                           not fit an int16 after truncation; NaN counts.  Computed for the float entry points too
     7  u32  flags         bit 0: the frame's silence flag; the other bits are 0
   The sums are fp32 in one fixed order, so a stream's record does not depend on the batch size, its slot or the kernel family.
   pn_ctx_set_output_saturate(ctx, 1): the int16 entry points cast t = o * 32768 as  t >= 32768 -> 32767,  t <= -32769 -> -32768,
   NaN -> 0, otherwise trunc(t), instead of the reference CLI's wrap to the low 16 bits (main.cpp:36), which turns a sample
   that lands on +32768 into -32768.  A sample in range is cast exactly as before.  Float outputs are never altered (with only
   this setting on, a float frame launches nothing more).
   Both are context-wide settings like pn_ctx_set_postfilter: they take effect from the next frame submitted and survive
   pn_ctx_reset, pn_ctx_reset_streams and imports; the device buffers they need are allocated inside these two calls, never inside
   a frame.  While the stage is on, the int16 entry points run the back end's float kernel into a context-owned buffer and the
   stage casts it: the same fp32 arithmetic, so wrap-mode PCM is bit for bit what the fused cast gives.  The stage is profiled
   under the "backend" family, which then counts two launches per frame.
   pn_ctx_read_report: the last frame's records to h_report [n_streams][8] words (synchronising, like pn_ctx_read_features);
   pn_ctx_read_report_dev: the same into a device buffer, asynchronous on the context's stream.  Both return -1 while the report
   is off.  Rows of streams skipped by pn_process_*_active are unspecified for that tick; a listed stream's input figures follow
   its own received frames.  After pn_process_i16_multi the records are the last frame's.
   pn_host_next_report: the next pn_submit_host_* call (any of the four) also delivers ITS frame's records to h_report
   [n_streams][8] words, copied on the device-to-host stream with h_out and under h_out's lifetime rule.  One-shot; NULL cancels a
   pending request; -1 while the report is off. */
#define PN_REPORT_WORDS 8
int pn_ctx_set_report(pn_ctx *ctx, int enable);
int pn_ctx_set_output_saturate(pn_ctx *ctx, int enable);
int pn_ctx_read_report(pn_ctx *ctx, void *h_report);
int pn_ctx_read_report_dev(pn_ctx *ctx, void *d_report);
int pn_host_next_report(pn_ctx *ctx, void *h_report);
/* n_frames consecutive frames per call: in/out are [n_frames][n_streams][480] (frame-major). */
int pn_process_i16_multi(pn_ctx *ctx, const int16_t *d_in, int16_t *d_out, float *d_gr, int n_frames);
/* Host-buffer convenience wrappers (H2D, process, D2H, synchronise). */
int pn_process_host_f32(pn_ctx *ctx, const float *h_in, float *h_out, float *h_gr);
int pn_process_host_i16(pn_ctx *ctx, const int16_t *h_in, int16_t *h_out, float *h_gr);
/* Pipelined host-buffer entry points: the same work as pn_process_host_*, but the call returns
   once the frame is queued.  Copy-in, the launches and copy-out of consecutive frames overlap on
   three streams with double-buffered device staging, so a caller feeding frames back to back gets
   the device rate instead of the serial copy+compute+copy rate.  At most two frames are in
   flight: the call blocks until the frame submitted two calls earlier has been delivered.
   Lifetime: h_in must stay unmodified, and h_out / h_gr are undefined, until THAT frame is
   delivered — after pn_host_wait(ctx), or once the second next pn_submit_host_* call has
   returned.  Use pinned host memory (pn_host_alloc / hipHostMalloc / hipHostRegister): with
   pageable memory the runtime stages the copies and nothing overlaps.  Results are identical to
   pn_process_host_*; the two families may be mixed (the synchronous one drains the pipeline). */
int pn_submit_host_f32(pn_ctx *ctx, const float *h_in, float *h_out, float *h_gr);
int pn_submit_host_i16(pn_ctx *ctx, const int16_t *h_in, int16_t *h_out, float *h_gr);
int pn_host_wait(pn_ctx *ctx);               /* every submitted frame delivered */
/* Builds the three-stream pipeline NOW instead of inside the first pn_submit_host_* call: the copy streams are probed against
   the context's stream (a 1 ms sleeper kernel on it, up to 6 attempts x 3 pairings: tens of milliseconds; not legal while that
   stream is being captured).  A caller on a real-time clock calls this once before its first frame arrives. */
int pn_host_pipeline_prepare(pn_ctx *ctx);
/* Non-blocking: how many submitted frames have been DELIVERED (output copy complete) so far; -1 on error.  For callers on a
   real-time clock that timestamp each frame's delivery between arrivals (reference contract: src/main.cpp:30-39). */
int64_t pn_host_frames_delivered(pn_ctx *ctx);
/* How the two copy streams (host-to-device, device-to-host) of the pipelined path were obtained, one letter each: "n" a
   default-priority stream probed to share its hardware queue with neither the compute stream nor the other copy stream, "h" /
   "l" a high- / low-priority stream (the fallback); "" before the first pn_submit_host_* call.  Diagnostics (bench.py). */
const char *pn_ctx_pipe_streams(pn_ctx *ctx);
void *pn_host_alloc(size_t bytes);           /* pinned host memory (hipHostMalloc); NULL on failure */
/* One host feeding several GPUs: bind the CALLING THREAD to the CPUs of the NUMA node `device` hangs off (sysfs
   /sys/bus/pci/devices/<bdf>/numa_node) — call it in the thread that will own the device BEFORE pn_ctx_create / pn_host_alloc,
   so that first touch places its pinned buffers next to that GPU.  Returns the node (>= 0) when bound, -1 when the affinity
   was left alone; msg (optional) receives one line saying what was done or why not.  Never fatal.  (The reference's
   fan-out, utils/run.sh:49,65,99, places nothing.) */
int pn_bind_thread_to_device_numa(int device, char *msg, size_t msg_bytes);
void pn_host_free(void *p);
int pn_ctx_synchronize(pn_ctx *ctx);

/* Mid-pipeline taps for per-stage parity tests (device -> host copies, synchronising).
   features: [n_streams][70] of the last frame; silence: [n_streams] int32. */
int pn_ctx_read_features(pn_ctx *ctx, float *h_feat, int32_t *h_silence);
/* The same tap into caller-owned DEVICE buffers, asynchronous on the context's stream (either may be NULL). */
int pn_ctx_read_features_dev(pn_ctx *ctx, float *d_feat, int32_t *d_silence);
/* Run only the network on host-supplied features [n_streams][70] -> g,r [n_streams][68]: compute_rnn (rnn.cpp:42-81)
   on the context's RNN state.  Advances only the network's state (conv FIFOs, GRUs), like calling the reference's
   compute_rnn on an RNNState directly; the DSP state and frame counter of pn_process_* are untouched. */
int pn_ctx_compute_rnn_host(pn_ctx *ctx, const float *h_feat, float *h_gr);
/* Load / store the network state of every stream from / to host arrays in the reference's RNNState layout
   (nnet_data.h:28-38): conv1 [n_streams][4*128] and conv2 [n_streams][2*512] = the live part of the FIFOs, oldest
   frame first (nnet.cpp:191-199); gru1, gru2, gru3, gru_gb [n_streams][512]; gru_rb [n_streams][128].  NULL
   arrays are skipped.  Synchronous.  (Checkpoint/resume of the recurrent state, and what the exported
   compute_rnn(RNNState*, ...) uses.)  Available in every network mode: the fp16-operand and split-precision modes keep
   the fp32 values next to their operand shadows and re-derive the shadows on a load. */
int pn_ctx_set_rnn_state_host(pn_ctx *ctx, const float *conv1, const float *conv2, const float *gru1, const float *gru2,
                              const float *gru3, const float *gru_gb, const float *gru_rb);
int pn_ctx_get_rnn_state_host(pn_ctx *ctx, float *conv1, float *conv2, float *gru1, float *gru2, float *gru3,
                              float *gru_gb, float *gru_rb);

/* ---- per-stream state records: moving a live stream between slots, contexts, devices, processes ------------------- */
/* One record holds ALL the state of ONE stream — the DSP half (history, look-ahead, pitch and synthesis memory) and the
   network half — so that a stream exported from one context and imported into another (any batch size, kernel family,
   network mode, device, process) continues from exactly that state on the target's kernels: between contexts of one
   network mode (in PN_NN_MFMA: any of its bit-identical kernel families) the moved stream's outputs are bit for bit those
   it would have produced in its source context.  The record does not depend on the ring phases of the source: every ring is written in AGE order (oldest
   entry first) and is scattered at the target's own frame counters.  Scratch (features, silence flags, the comb-filtered
   spectrum, conv2 output, g|r, dead ring slots) and the operand shadows of the fp16 / split-precision / direct-operand
   kernels are not state: the target re-derives the shadows of the imported rows from their fp32 values.

   Layout (PN_STREAM_STATE_BYTES = 54 688 bytes, little-endian; every section starts on a 16-byte boundary):
     header, 64 bytes: uint32 magic PN_STREAM_STATE_MAGIC | uint32 version PN_STREAM_STATE_VERSION | uint32 record bytes |
                       int32 nn_mode of the source (informational, never checked) | 32-byte pn_model_digest of the model |
                       16 zero bytes
     body, fp32 (int32 where noted) words from PN_STREAM_STATE_HEADER_BYTES on, at these word offsets:
       PN_SS_HIST        11 x 480   the last 11 input frames (the reference's comb_buf minus the frame to come)
       PN_SS_SPEC         5 x 800   look-ahead spectra of the last 5 frames, bins 0..399 as (re, im) pairs
       PN_SS_EY           5 x 36    their band energies (34 bands + 2 padding words)
       PN_SS_CONV1        4 x 128   conv1 FIFO (RNNState layout, nnet_data.h:28-38; the same as pn_ctx_get_rnn_state_host)
       PN_SS_CONV2        2 x 512   conv2 FIFO
       PN_SS_GRU          4 x 512   gru1, gru2, gru3, gru_gb states
       PN_SS_GRU_RB       128       gru_rb state
       PN_SS_SYNTH        480       synthesis overlap memory
       PN_SS_TAIL         4         last_gain (fp32) | last_period (int32) | 2 zero words */
#define PN_STREAM_STATE_MAGIC 0x53534e50u      /* "PNSS" */
#define PN_STREAM_STATE_VERSION 1
#define PN_STREAM_STATE_HEADER_BYTES 64
#define PN_SS_HIST 0
#define PN_SS_SPEC 5280
#define PN_SS_EY 9280
#define PN_SS_CONV1 9460
#define PN_SS_CONV2 9972
#define PN_SS_GRU 10996
#define PN_SS_GRU_RB 13044
#define PN_SS_SYNTH 13172
#define PN_SS_TAIL 13652
#define PN_SS_BODY_WORDS 13656
#define PN_STREAM_STATE_BYTES (PN_STREAM_STATE_HEADER_BYTES + 4 * PN_SS_BODY_WORDS)
/* Why a record is refused (pn_stream_state_check's return value, d_status of pn_ctx_import_streams). */
enum {
  PN_SS_OK = 0,
  PN_SS_BAD_MAGIC = -1,
  PN_SS_BAD_VERSION = -2,
  PN_SS_BAD_SIZE = -3,      /* a buffer of the wrong size, or a header that names another record size */
  PN_SS_BAD_MODEL = -4,     /* written under another model (pn_model_digest differs) */
  PN_SS_BAD_ARG = -5,       /* NULL record or model */
  PN_SS_BAD_RATE = -6,      /* pn_rate_state_check: written by a converter of another rate, or a rate no converter has */
  PN_SS_BAD_STATE = -7      /* pn_rate_call_state_check: a body that breaks an invariant its kernels rely on, or an unknown section */
};
size_t pn_stream_state_bytes(void);            /* PN_STREAM_STATE_BYTES */
/* Host only, needs no GPU: is `bytes` bytes at `record` one record that a context of `model` accepts?  PN_SS_OK or a
   PN_SS_BAD_* code (pn_last_error says why).  For callers that receive records from elsewhere. */
int pn_stream_state_check(const void *record, size_t bytes, const pn_model *model);
/* Export streams ids[0..n) (host array, in range, duplicates allowed) into records [n][PN_STREAM_STATE_BYTES] at the
   16-byte aligned DEVICE address d_records.  Asynchronous on the context's stream, ordered like pn_ctx_reset_streams: the
   records hold the state between the frames submitted before and after the call (on the pipelined host path too); the
   caller orders its own use of d_records (pn_ctx_synchronize or an event on the context's stream). */
int pn_ctx_export_streams(pn_ctx *ctx, const int32_t *ids, int n, void *d_records);
/* Import records [n][PN_STREAM_STATE_BYTES] (16-byte aligned device address) into streams ids[0..n) (host array, DISTINCT
   ids in range: otherwise -1 and nothing is launched).  Asynchronous and ordered like the export.  Each header is checked
   on the device against this context's model digest, the version and the size: d_status[i] (device int32 [n], required)
   receives PN_SS_OK when record i was imported, a PN_SS_BAD_* code when it was refused — a refused record leaves its
   stream exactly as it was.  The other streams of the context are not touched (their operand shadows neither).  The
   first frame processed after the import continues the imported streams. */
int pn_ctx_import_streams(pn_ctx *ctx, const int32_t *ids, int n, const void *d_records, int32_t *d_status);
/* The same with host records, synchronous (frames in flight on the pipelined host path are completed first).  The host
   import checks every header BEFORE anything is launched and is all-or-nothing: one bad record (or id) refuses the call
   and leaves the context untouched. */
int pn_ctx_export_streams_host(pn_ctx *ctx, const int32_t *ids, int n, void *h_records);
int pn_ctx_import_streams_host(pn_ctx *ctx, const int32_t *ids, int n, const void *h_records);

/* ---- per-kernel timing (HIP events on the context's stream) ------------------------------- */
/* When enabled, every launch of the named kernel families is bracketed by events. */
int pn_ctx_set_profiling(pn_ctx *ctx, int enable);
/* name: one of pn_kernel_name(i), i in [0, pn_kernel_count()).  Returns total milliseconds and
   launch count since the last pn_ctx_reset_profile (synchronises the stream). */
int pn_kernel_count(void);
const char *pn_kernel_name(int i);
int pn_ctx_kernel_time(pn_ctx *ctx, const char *name, double *total_ms, int64_t *launches);
int pn_ctx_reset_profile(pn_ctx *ctx);

/* Debug tap (tests/tools): copy an internal device buffer to the host; which = 0 feat, 1 c1ring,
   2 c2ring, 3 c2out, 4..7 gru1..gb (ping-pong pair), 8 rb, 9 g|r, 10 look-ahead spectra ring, 11 comb-filtered
   spectrum, 12 history ring, 13 the pitch period the last frame's comb filter used (int32 per stream).  Returns bytes copied
   or -1. */
long long pn_ctx_debug_copy(pn_ctx *ctx, int which, void *dst, long long max_bytes);
/* Launch-refusal hooks (tests).  A network launcher that is asked for a geometry its software pipeline cannot run returns
   an error WITHOUT launching and the frame fails: pn_process_* / pn_submit_host_* / pn_ctx_compute_rnn_host return -1 with
   pn_last_error() naming the launcher — never 0 with stale layer outputs.  (The context's stream state is undefined after
   a failed frame: pn_ctx_reset before reuse.)
   pn_debug_check_launch runs the launchers' geometry predicates without a GPU: kind 0 dense on the fp32 MFMA kernels,
   1 dense / 2 GRU (n_out neurons) on the shadow-operand kernels, 3 narrow dense on 16x16x4 tiles; n_panels panels of
   `width` columns.  0 = accepted, -1 = refused (pn_last_error()).
   pn_ctx_debug_inject_launch_failure(ctx, 1) makes every following frame of a non-STRICT context ask the fc layer's
   launcher for a refused geometry. */
int pn_debug_check_launch(int kind, int n_panels, int width, int n_out);
/* The kernel families a context of n_streams streams in nn_mode would run under the current environment, without a GPU (every
   family override is read once, when a context is created: csrc/pn_plan.h).  Writes describe()'s family fields ("nn=" through
   "frontend=") then " nn_chains=N tile=T share=S" (T: rows per block of the chained kernels; S: the first row of chain 1, 0 with
   one chain).  Returns the length written, or -1 (pn_last_error()). */
int pn_debug_plan(int n_streams, int nn_mode, char *buf, size_t n);
int pn_ctx_debug_inject_launch_failure(pn_ctx *ctx, int enable);
/* The digest function behind the shared-weights cache key (SHA-256, FIPS 180-4), exposed so that the CPU tests can check it
   against known answers: a model's packed device copy is shared by every context whose model has the same digest. */
void pn_debug_sha256(const void *data, size_t len, unsigned char out[32]);
/* SHA-256 of a model's content (arrays in storage order, then each layer's activation and reset_after as two int32). */
void pn_model_digest(const pn_model *model, unsigned char out[32]);

/* ---- batched training-feature generator ----------------------------------- */
/* The reference's `percepNet <speech> <noisy> <count> <output>` binary (train(), denoise.cpp:603-787,
   declared rnnoise.h:66) for n_pairs (speech, noisy) pairs in lock-step.  Samples are int16 at
   NORM_RATIO 1 (denoise.cpp:41,697: the float sample IS the int16 value).  One record = 138 float32:
   Ey_lookahead[34] | Ephaty[34] | T | pitch_corr | g[34] | r[34] (denoise.cpp:764-773), g being
   envelope-post-filtered as in the reference's default (TEST) build (45-47, 743).  The optional PCM is
   that build's test_output.pcm.  No model is involved. */
typedef struct pn_featgen pn_featgen;
pn_featgen *pn_featgen_create(int device, int n_pairs, void *hip_stream);
void pn_featgen_destroy(pn_featgen *fg);
int pn_featgen_reset(pn_featgen *fg);
int pn_featgen_n_pairs(const pn_featgen *fg);
int64_t pn_featgen_frames_done(const pn_featgen *fg);
size_t pn_featgen_device_bytes(const pn_featgen *fg);
int pn_featgen_synchronize(pn_featgen *fg);
/* One frame, device buffers, asynchronous: speech/noisy [n_pairs][480]; records [n_pairs][138];
   test_pcm (may be NULL) [n_pairs][480]. */
int pn_featgen_process_i16(pn_featgen *fg, const int16_t *d_speech, const int16_t *d_noisy, float *d_records,
                           int16_t *d_test_pcm);
/* n_frames frames, pair-major "file images": speech/noisy [n_pairs][n_frames][480], records
   [n_pairs][n_frames][138] (= each pair's output file), test_pcm [n_pairs][n_frames][480] or NULL. */
int pn_featgen_process_i16_files(pn_featgen *fg, const int16_t *d_speech, const int16_t *d_noisy, int n_frames,
                                 float *d_records, int16_t *d_test_pcm);
int pn_featgen_process_host_i16_files(pn_featgen *fg, const int16_t *h_speech, const int16_t *h_noisy, int n_frames,
                                      float *h_records, int16_t *h_test_pcm);
/* File-level driver with train()'s file semantics (whole frames cycled at EOF, 693-715) for n_jobs
   jobs at once; test_out_paths / test_in_paths may be NULL (or hold NULL entries). */
int pn_featgen_run_files(int device, int n_jobs, const char *const *speech_paths, const char *const *noisy_paths,
                         const int *counts, const char *const *out_paths, const char *const *test_out_paths,
                         const char *const *test_in_paths);

/* ---- batched rate converter: 8, 16, 24 and 32 kHz streams through a 48 kHz context --------------------------------------- */
/* The engine runs at 48 kHz; a pn_rate is an object BESIDE a context (like pn_featgen: it adds nothing to the context's state)
   that converts all of the context's streams from ONE low rate up to 48 kHz in front of a frame and back down behind it, on the
   GPU (csrc/pn_rate.hip).  rate_hz is 8000, 16000 or 24000 — L = 48000 / rate_hz = 6, 3, 2 — or 32000, the rational rate
   48000 * M / L with (L, M) = (3, 2) ("32000 Hz", below); any other rate is refused.  A caller
   with mixed rates uses a MIXED converter (pn_rate_create_mixed, below: a rate per stream, 48000 included, in one context), or
   one context and converter per rate.  A frame is still 10 ms: n = 480 M / L = 80 | 160 | 240 | 320 samples per stream.

   Arithmetic (fixed, so that a float32 model reproduces it bit for bit: tests/rate_model.py, and tests/rate32_model.py for
   32000).  T = PN_RATE_TAPS = 16, D = T * L.  For the integer factors (M = 1):
   Prototype filter, k = -D..D:  h[k] = sinc(k / L) * I0(8 * sqrt(1 - (k / D)^2)) / I0(8)  (a Kaiser-windowed sinc, beta = 8),
   computed in double for k >= 0, mirrored, h[0] = 1 and h[jL] = 0 (j != 0) exactly, rounded to fp32 once; the down-converter's taps
   are g[k] = (float)(h_double[k] / L).
     up    y[Lq + p] = sum_m x[m] * h[L(q - T - m) + p]:  phase p = 0 is the copy y[Lq] = x[q - T] (the input's bits), phases
           1..L-1 sum over the 32 samples x[q - 2T + 1 .. q].  Per-stream state: the last 32 low-rate input samples.
     down  z[m] = sum_{i = Lm - 2D + 1}^{Lm - 1} g[Lm - D - i] * o[i].  Per-stream state: the last 2D 48 kHz samples (192 | 96 | 64).
   32000 Hz: up by L = 3 with every M = 2nd output kept, and down from 48 kHz samples that sit M apart on the L-times grid.  The
   prototype h is the L = 3 table (16000's), bit for bit; the down taps are g[k] = (float)(h_double[k] * 2 / 3).
     up    output j of a frame: q = (2j) div 3, p = (2j) mod 3 (480 * 2 / 3 is whole, so the pattern restarts with every frame and
           no phase is carried).  p = 0 is the copy y[j] = x[q - T]; p = 1, 2: y[j] = sum_{i = 0..31} h[3(15 - i) + p] * x[q - 31 + i]
           — the 16 kHz interpolation of the same samples with every second output kept.  State: the last 32 input samples.
     down  z[m] = sum_i g[3m - 48 - 2i] * o[i] over every i with (3m - 96) / 2 < i < 3m / 2, ascending: 47 terms for even m, 48 for
           odd m, taps that are exactly 0 included.  State: the last 2D / M = 48 samples at 48 kHz (the oldest is never read).
   Every sum runs oldest sample first from acc = 0.0f as acc = acc + c * x, product and sum separately rounded (no FMA), so a
   stream's output does not depend on the batch size, its slot or the block it ran in.
   Delay from an input sample to the same sample in the output, in low-rate samples: 2880 M / L + 2T

       rate_hz   (L, M)   n     delay (samples)   delay (ms)   state record (bytes)
        8000     (6, 1)   80        512              64           912
       16000     (3, 1)  160        992              62           528
       24000     (2, 1)  240       1472              61.33        400
       32000     (3, 2)  320       1952              61           336

   The engine runs in float between the two conversions; int16 exists only at the edges: input (float)v / 32768, output
   trunc(z * 32768) wrapped to 16 bit, or saturated while pn_ctx_set_output_saturate is on.  The frame report (pn_ctx_set_report)
   stays that of the 48 kHz signal inside the engine: 480 samples per frame, the engine's own 2880-sample delay, levels before the
   down-conversion.  8-bit G.711 rows are the int16 edge with the companding outside it ("G.711 streams", below).
   The model was trained on full-band speech; its quality on 32 kHz input (as on the other low rates) is not measured here.
   NOT provided: other rates.  44100, 12000, 96000 and every rate not named above are refused.

   Host only, needing no GPU:
   pn_rate_frame_samples: n, -1 for a refused rate.  pn_rate_delay_samples: the table above, -1.  pn_rate_taps: the fp32 table,
   2D + 1 values for k = -D..D (down == 0: h; otherwise g), into taps[0..cap); returns the count, -1 for a refused rate or
   cap < 2D + 1.  pn_rate_state_bytes: the record size, 0 for a refused rate.  pn_rate_state_check: is `bytes` bytes at `record`
   one state record of a converter of rate_hz?  PN_SS_OK or a PN_SS_BAD_* code (pn_last_error says why).
   State record (little-endian): 16-byte header — uint32 magic PN_RATE_STATE_MAGIC | uint32 version PN_RATE_STATE_VERSION |
   uint32 record bytes | int32 rate_hz — then the 32 fp32 words of the up-converter's tail and the 2D / M words (192 | 96 | 64 |
   48) of the down-converter's, each oldest sample first. */
#define PN_RATE_TAPS 16
#define PN_RATE_STATE_MAGIC 0x53524e50u        /* "PNRS" */
#define PN_RATE_STATE_VERSION 1
#define PN_RATE_STATE_HEADER_BYTES 16
typedef struct pn_rate pn_rate;
int pn_rate_frame_samples(int rate_hz);
int pn_rate_delay_samples(int rate_hz);
int pn_rate_taps(int rate_hz, int down, float *taps, int cap);
size_t pn_rate_state_bytes(int rate_hz);
int pn_rate_state_check(const void *record, size_t bytes, int rate_hz);
/* A converter for every stream of ctx.  It BORROWS ctx — its device, n_streams and HIP stream — and owns its state, its tap
   tables and the 48 kHz rows between the conversions: destroy the converter before ctx.  State starts all-zero.  Everything
   below runs on the context's stream, so it is ordered against pn_process_*, pn_ctx_reset_streams and the rest like they are
   against each other.  Id lists are host arrays under the context's rules (in range and, where streams advance or are imported,
   distinct; otherwise -1 and nothing is launched); the caller may reuse them when the call returns. */
pn_rate *pn_rate_create(pn_ctx *ctx, int rate_hz);
void pn_rate_destroy(pn_rate *r);
int pn_rate_reset(pn_rate *r);                       /* zero every stream's tails */
/* The converter's half of a slot reset, asynchronous like pn_ctx_reset_streams (duplicates allowed): a caller whose slot starts a
   new call calls both. */
int pn_rate_reset_streams(pn_rate *r, const int32_t *ids, int n);
/* The two kernels on their own, device buffers (16-byte aligned), asynchronous.  d_in [n_streams][n] -> d_out48 [n_streams][480],
   and d_in48 [n_streams][480] -> d_out [n_streams][n].  ids == NULL: every stream; otherwise only the n_ids listed rows are
   read, written and advanced — an unlisted stream's tails and output row are not touched. */
int pn_rate_up_f32(pn_rate *r, const float *d_in, float *d_out48, const int32_t *ids, int n_ids);
int pn_rate_up_i16(pn_rate *r, const int16_t *d_in, float *d_out48, const int32_t *ids, int n_ids);
int pn_rate_down_f32(pn_rate *r, const float *d_in48, float *d_out, const int32_t *ids, int n_ids);
int pn_rate_down_i16(pn_rate *r, const float *d_in48, int16_t *d_out, const int32_t *ids, int n_ids);
/* One whole frame of every stream: up, pn_process_f32 on converter-owned 48 kHz rows, down.  d_in, d_out [n_streams][n] at the
   low rate; d_gr (optional) [n_streams][68] as for pn_process_*.  When the frame fails inside pn_process_f32 the call returns -1
   with the context's error kept: reset the context AND the converter before reuse.
   _active: only the n listed streams advance (pn_process_f32_active in the middle); the converter has no save and restore —
   its kernels simply run over the listed rows.  _host: host buffers, synchronous (H2D, frame, D2H, synchronise), like
   pn_process_host_*; frames in flight on the context's pipelined host path are completed first. */
int pn_rate_process_f32(pn_rate *r, const float *d_in, float *d_out, float *d_gr);
int pn_rate_process_i16(pn_rate *r, const int16_t *d_in, int16_t *d_out, float *d_gr);
int pn_rate_process_f32_active(pn_rate *r, const float *d_in, float *d_out, float *d_gr, const int32_t *ids, int n);
int pn_rate_process_i16_active(pn_rate *r, const int16_t *d_in, int16_t *d_out, float *d_gr, const int32_t *ids, int n);
int pn_rate_process_host_f32(pn_rate *r, const float *h_in, float *h_out, float *h_gr);
int pn_rate_process_host_i16(pn_rate *r, const int16_t *h_in, int16_t *h_out, float *h_gr);
/* State records of streams ids[0..n) to / from host memory [n][pn_rate_state_bytes(rate)], synchronous.  The import checks every
   header before anything is launched and is all-or-nothing (distinct ids): a record of another rate, or any other bad record or
   id, refuses the call and leaves the converter untouched.  With pn_ctx_export_streams_host / pn_ctx_import_streams_host this
   moves a narrowband stream between slots, contexts, devices and processes bit for bit. */
int pn_rate_export_streams_host(pn_rate *r, const int32_t *ids, int n, void *h_records);
int pn_rate_import_streams_host(pn_rate *r, const int32_t *ids, int n, const void *h_records);
/* The pipelined host path for a converter's frames (single-rate or mixed): pn_submit_host_* with the converter's frame in the
   middle.  One frame is H2D of the low-rate rows on the context's h2d stream into a staging slot of the converter, then on the
   context's stream the frame of pn_rate_process_* (up, pn_process_f32[_active], down), then D2H of the low-rate rows and of g|r
   on the d2h stream.  It runs through the CONTEXT's pipeline — its two copy streams, slot counter, events and its bound of two
   frames in flight — so pn_host_wait(ctx), pn_host_frames_delivered(ctx), pn_ctx_pipe_streams(ctx) and pn_host_next_report(ctx,
   h_report) work unchanged and count frames of either kind in submission order (the next submit of either kind delivers its
   frame's 48 kHz report records), and pn_submit_host_* and pn_rate_submit_host_* may be interleaved on one context.
   Rows are [n_streams][pn_rate_row_samples(r)].  On a mixed converter whole rows of 480 travel both ways: the rest of an input
   row is ignored and the rest of an output row is UNSPECIFIED on this path (no landing buffer, no per-stream host copy).  Rows of
   streams skipped by an _active call are unspecified.  h_in / h_out / h_gr live by the rule of pn_submit_host_*.
   pn_rate_host_pipeline_prepare: allocates the converter's second staging pair and does pn_host_pipeline_prepare(ctx); otherwise
   the first submit does both; no later frame allocates.  pn_rate_set_stream_rates, pn_rate_reset_streams, pn_ctx_reset_streams,
   pn_ctx_set_atten_limit and the record calls are ordered on the context's stream: frames submitted before them run under the
   old values, frames after them under the new ones, with no wait in between.  A refused id list consumes no slot; a frame that
   fails inside the engine returns -1 with the context's error kept.  pn_rate_destroy completes the frames in flight;
   pn_rate_process_host_* keeps draining the pipeline first.  Results are bit for bit those of the synchronous path. */
int pn_rate_submit_host_f32(pn_rate *r, const float *h_in, float *h_out, float *h_gr);
int pn_rate_submit_host_i16(pn_rate *r, const int16_t *h_in, int16_t *h_out, float *h_gr);
int pn_rate_submit_host_f32_active(pn_rate *r, const float *h_in, float *h_out, float *h_gr, const int32_t *ids, int n);
int pn_rate_submit_host_i16_active(pn_rate *r, const int16_t *h_in, int16_t *h_out, float *h_gr, const int32_t *ids, int n);
int pn_rate_host_pipeline_prepare(pn_rate *r);
/* Device-side records: asynchronous on the context's stream, ordered like pn_ctx_export_streams / pn_ctx_import_streams.  Records
   go to a 16-byte aligned device address, pn_rate_record_stride(r) bytes apart: pn_rate_state_bytes(rate) on a single-rate
   converter, PN_RATE_STATE_MAX_BYTES on a mixed one, where the fixed stride lifts the one-rate-per-call rule of the host forms —
   each record carries its own stream's rate.  Format, version and sizes are those above.
   Export (duplicates allowed): record i gets the header of stream ids[i]'s current rate, that rate's size, the two tails oldest
   first, and zeros from the record's size up to the stride.
   Import (distinct ids, d_status required): every header is checked on the device against the SLOT's rate — the converter's, or
   the per-stream rate a preceding pn_rate_set_stream_rates has set, in stream order — and d_status[i] receives exactly
   pn_rate_state_check(record_i, pn_rate_state_bytes(R), R) for the slot's rate R.  A refused record leaves both tails of its
   stream untouched; the other records of the call are imported.
   Refused on the host with -1, nothing written or launched: a bad or (import) duplicate id, a misaligned pointer, a listed stream
   that runs at 48000 (it has no converter state).  n == 0 is a no-op. */
#define PN_RATE_STATE_MAX_BYTES 912
size_t pn_rate_state_max_bytes(void);                 /* host only */
size_t pn_rate_record_stride(const pn_rate *r);
int pn_rate_export_streams(pn_rate *r, const int32_t *ids, int n, void *d_records);
int pn_rate_import_streams(pn_rate *r, const int32_t *ids, int n, const void *d_records, int32_t *d_status);
/* Timing of the converter's two kernels inside a frame: HIP events around their launches, like pn_ctx_set_profiling but owned by
   the converter (the context's family list does not change).  Off by default; off, no event is created or recorded.  name:
   "rate_up" | "rate_down" | "rate_mix" (the conference mix, below) | "rate_plc" (packet-loss concealment, below) | "rate_agc" (automatic level control, below) | "rate_lim" (the output limiter, below) | "rate_dtmf" (DTMF detection, below) | "rate_clamp" (DTMF removal, below) | "rate_cng" (comfort noise, below) | "rate_dtx" (the DTX send side, below).  pn_rate_kernel_time synchronises the context's stream. */
int pn_rate_set_profiling(pn_rate *r, int enable);
int pn_rate_kernel_time(pn_rate *r, const char *name, double *total_ms, int64_t *launches);
int pn_rate_reset_profile(pn_rate *r);

/* ---- mixed rates: 8, 16, 24 and 48 kHz streams, and 32 kHz ones, in ONE context --------------------------------------------- */
/* A mixed converter IS a pn_rate — every entry point above takes it — whose streams each have a rate of their own out of 8000,
   16000, 24000, 32000 and 48000 (L = 6, 3, 2, the rational (3, 2), and 1), so that any free slot of a context takes the next call whatever its rate.  The rate
   per stream lives in the converter; pn_ctx, its state and its records know nothing of it.  It differs from a single-rate
   converter in two things only:
   Rows.  Low-rate rows are [n_streams][PN_RATE_MIXED_ROW = 480] samples (1920 bytes in float, 960 in int16) whatever the rates,
   because a slot's rate may change at any time; stream s at rate R uses the first n_s = pn_rate_mixed_frame_samples(R) samples
   of its row.  The rest of an input row is ignored, the rest of an output row is left untouched (also by the _host forms).  Base
   pointers stay 16-byte aligned.
   A factor per stream.  For 8000, 16000, 24000 and 32000 the arithmetic is exactly the one above for that rate — same taps, same order, same tails
   — so a stream gives bit for bit what it gives in a single-rate converter of its rate.  L = 1 is a copy: float rows carry the
   input's bits up and down; int16 is (float)v / 32768 on the way up and t = o * 32768 through the wrapping or saturating cast
   (pn_ctx_set_output_saturate) on the way down.  A 48000 stream has no tails and no record; its delay is the engine's 2880 samples.

       rate_hz   (L, M)   n_s   delay (samples)
        8000     (6, 1)   80        512
       16000     (3, 1)  160        992
       24000     (2, 1)  240       1472
       32000     (3, 2)  320       1952
       48000     (1, 1)  480       2880

   Host only, needing no GPU: pn_rate_mixed_frame_samples and pn_rate_mixed_delay_samples, the table above, -1 for another rate
   (pn_rate_frame_samples(48000) and the rest of the single-rate surface keep refusing 48000); pn_rate_mixed_rates_check: 0 when
   rates_hz[0..n) are all out of the five, else -1 with pn_last_error naming the first bad index.
   pn_rate_create_mixed: rates_hz [n_streams] (NULL: all 48000); a bad rate returns NULL.  pn_rate_is_mixed: 1 | 0.
   pn_rate_row_samples: samples between two rows at the low rate — n for a single-rate converter, 480 for a mixed one.
   pn_rate_set_stream_rates: streams ids[i] (distinct, in range) continue at rates_hz[i] (out of the five); anything else refuses
   the call with -1, nothing changed or launched; n == 0 is a no-op; refused on a single-rate converter.  Asynchronous on the
   context's stream and ordered exactly like pn_rate_reset_streams: frames submitted before it run at the old rates, frames after
   it at the new ones; the caller may reuse its arrays on return.  It ZEROES both tails of the listed streams — a rate change is a
   new call, and setting a stream's current rate equals pn_rate_reset_streams — and does not touch the context: a caller whose
   slot starts a new call also calls pn_ctx_reset_streams.  pn_rate_reset and pn_rate_reset_streams keep the rates.
   pn_rate_get_stream_rates: the rates as last set, h_rates [n_streams]; a single-rate converter gives its rate for every stream.
   Records: format, version and sizes are those above, so streams move between mixed and single-rate converters.  One export or
   import call on a mixed converter handles ONE rate: the listed streams must share a rate R != 48000 now, and the records are
   [n][pn_rate_state_bytes(R)].  Refused all-or-nothing, nothing written or launched: a list spanning two rates; a 48000 slot (it
   has no converter state to move); on import, a record whose header names another rate than the slot's (PN_SS_BAD_RATE) — the
   importing caller sets the slot's rate first. */
#define PN_RATE_MIXED_ROW 480
int pn_rate_mixed_frame_samples(int rate_hz);
int pn_rate_mixed_delay_samples(int rate_hz);
int pn_rate_mixed_rates_check(const int32_t *rates_hz, int n);
pn_rate *pn_rate_create_mixed(pn_ctx *ctx, const int32_t *rates_hz);
int pn_rate_is_mixed(const pn_rate *r);
int pn_rate_row_samples(const pn_rate *r);
int pn_rate_set_stream_rates(pn_rate *r, const int32_t *ids, int n, const int32_t *rates_hz);
int pn_rate_get_stream_rates(const pn_rate *r, int32_t *h_rates);

/* ---- G.711 streams: 8-bit mu-law and A-law rows at the converter's edges ------------------------------------------------------- */
/* A third sample format beside _f32 and _i16 on a pn_rate, single-rate or mixed: one byte per sample, G.711 mu-law (PCMU) or
   A-law (PCMA), with a law PER STREAM.  The engine, the filters, the tails, the delays, the records (format, version, sizes)
   and the _f32 / _i16 entry points are untouched: the 8-bit format is the int16 format with the companding outside it,
       in    x = (float)dec(b) / 32768
       out   enc(c), c = exactly the int16 the _i16 down-conversion writes for that sample from t = z * 32768 — through the
             wrapping cast, or the saturating one while pn_ctx_set_output_saturate is on
   so a G.711 stream gives, bit for bit, the encoding of what the _i16 path gives on the decoded samples.  It applies at whatever
   rate a stream runs, 48000 in a mixed converter included (L = 1: decode, engine, encode).  A G.711 caller should turn
   pn_ctx_set_output_saturate ON: in wrap mode a clipped sample wraps before it is encoded, exactly as on the int16 path.

   Arithmetic (csrc/pn_g711.h; integer formulas with one answer per input, reproduced by tests/g711_model.py; all values int32,
   b the byte, v the linear value in the int16 range).
     decode  mu-law  u = ~b & 0xFF, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 132) << e) - 132, v = (u & 0x80) ? -mag : mag
                     range +-32124; 0xFF and 0x7F both give 0
             A-law   a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15, mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 264) << (e - 1),
                     v = (a & 0x80) ? mag : -mag;  range +-32256, never 0 (0xD5 -> +8, 0x55 -> -8)
     encode  neg = v < 0, mag = neg ? ~v : v (the one's-complement magnitude of the ITU software tool library, both laws)
             mu-law  p = min((mag >> 2) + 33, 8191), e = floor(log2 p) - 5, m = (p >> (e + 1)) & 15,
                     b = ~((neg ? 0x80 : 0) | e << 4 | m) & 0xFF
             A-law   e = mag < 256 ? 0 : floor(log2 mag) - 7, m = (e == 0 ? mag >> 4 : mag >> (e + 3)) & 15,
                     b = ((neg ? 0 : 0x80) | e << 4 | m) ^ 0x55
   enc(dec(b)) == b for every byte except mu-law 0x7F -> 0xFF; both decoders equal CPython's audioop.ulaw2lin / alaw2lin, the
   A-law encoder equals audioop.lin2alaw, the mu-law encoder equals audioop.lin2ulaw(v) for v >= 0 and audioop.lin2ulaw(~v) ^ 0x80
   for v < 0 (audioop negates after shifting and so differs for 381 negative values).

   Host only, needing no GPU: pn_g711_decode / pn_g711_encode, n samples of one law; -1 for a law that is neither of the two or a
   NULL pointer.  pn_rate_laws_check: 0 when laws[0..n) are all out of the two, else -1 with pn_last_error naming the first bad index.

   The law per stream lives in the converter, like a mixed converter's rates.  It is a SETTING, not state: mu-law for every stream
   of a new converter; records do not carry it; pn_rate_reset, pn_rate_reset_streams, pn_rate_set_stream_rates and the record
   calls keep it — the importing caller sets the slot's law, as it sets the slot's rate.
   pn_rate_set_stream_laws: streams ids[i] (distinct, in range) continue under laws[i] (out of the two), on either kind of
   converter; anything else refuses the call with -1, nothing changed or launched; n == 0 is a no-op.  Asynchronous on the
   context's stream and ordered exactly like pn_rate_set_stream_rates: frames submitted before it run under the old law, frames
   after it under the new one, on the pipelined path too; the caller may reuse its arrays on return.  It touches no tail.
   pn_rate_get_stream_laws: the laws as last set, h_laws [n_streams].

   Frames and kernels: the byte twins of the _i16 entry points above, with the same ordering, id-list, failure and lifetime rules.
   Rows are [n_streams][pn_rate_row_samples(r)] BYTES — 80 | 160 | 240 on a single-rate converter, 480 on a mixed one, each a
   multiple of 16 — at 16-byte aligned addresses.  In a mixed converter the rest of an input row is ignored, the rest of an output
   row is left untouched on the synchronous paths and is unspecified on the pipelined one.  pn_rate_submit_host_g711* go through
   the context's pipeline and may be interleaved with the other pn_rate_submit_host_* calls and with pn_submit_host_*;
   pn_host_next_report works unchanged.
   NOT provided: linear and companded rows in one call; G.711 on pn_process_* without a converter (a mixed converter whose slots
   run at 48000 covers it).  (Packet-loss concealment and comfort noise: their own sections below.)  How well the model, trained on
   full-band linear speech, cleans companded narrowband input is not measured. */
#define PN_G711_ULAW 0
#define PN_G711_ALAW 1
int pn_g711_decode(int law, const uint8_t *in, int16_t *out, size_t n);
int pn_g711_encode(int law, const int16_t *in, uint8_t *out, size_t n);
int pn_rate_laws_check(const int32_t *laws, int n);
int pn_rate_set_stream_laws(pn_rate *r, const int32_t *ids, int n, const int32_t *laws);
int pn_rate_get_stream_laws(const pn_rate *r, int32_t *h_laws);
int pn_rate_up_g711(pn_rate *r, const uint8_t *d_in, float *d_out48, const int32_t *ids, int n_ids);
int pn_rate_down_g711(pn_rate *r, const float *d_in48, uint8_t *d_out, const int32_t *ids, int n_ids);
int pn_rate_process_g711(pn_rate *r, const uint8_t *d_in, uint8_t *d_out, float *d_gr);
int pn_rate_process_g711_active(pn_rate *r, const uint8_t *d_in, uint8_t *d_out, float *d_gr, const int32_t *ids, int n);
int pn_rate_process_host_g711(pn_rate *r, const uint8_t *h_in, uint8_t *h_out, float *h_gr);
int pn_rate_submit_host_g711(pn_rate *r, const uint8_t *h_in, uint8_t *h_out, float *h_gr);
int pn_rate_submit_host_g711_active(pn_rate *r, const uint8_t *h_in, uint8_t *h_out, float *h_gr, const int32_t *ids, int n);

/* ---- conferences: every stream hears the sum of the others --------------------------------------------------------------------- */
/* A conference id PER STREAM on a pn_rate, single-rate or mixed: between the engine and the down-conversion, where every stream's
   enhanced frame is a 48 kHz float row whatever its rate and coding, each member of a conference gets the sum of the OTHER
   members' rows ("mix-minus"), on the GPU (csrc/pn_rate_mix.hip).  An 8 kHz A-law, a 16 kHz linear and a 48 kHz float
   participant meet there in one format.  No new sample format, row shape or entry point for frames: every pn_rate_process_*,
   _active, pn_rate_process_host_* and pn_rate_submit_host_* call in f32 / i16 / g711 runs it.

   Arithmetic.  For a frame, A = the streams that advance (all of them, or the _active list); y[m][0..480) = the engine's float
   output row of stream m.
     stream s in A, conference c:  o[s][j] = sum of y[m][j] over the members m of c with m != s and m in A, m ASCENDING,
                                   in fp32 as acc = +0.0f, acc = acc + y[m][j].  A lone member hears +0.0.
     stream s in A, PN_CONF_NONE:  o[s] = y[s], bit for bit — what every stream gets while no conference exists.
     stream not in A:              contributes nothing (its y row is stale and is not read) and gets no output, as everywhere.
   The order depends on slots only — no atomics, no cross-lane sums — so a row is the same in every batch size and block, and a
   float32 model reproduces it, NaN, inf and -0.0 included (tests/conf_model.py).  The down-conversion (or the 48000 copy) then
   reads o instead of y, with the stream's own rate, format, law and the context's wrapping or saturating cast.  A sum of
   voices clips where one voice does not: a conference caller should turn pn_ctx_set_output_saturate ON.
   A participant who only LISTENS (muted, DTX) must still advance to hear: feed it frames of silence and keep it on the list.
   The mix has no state and nothing upstream depends on it: the engine's state, the delays, the converter's tails and records and
   the g|r tap are unchanged, and the frame report (pn_ctx_set_report) stays about the stream's OWN output before the mix.
   The down-converter's tail holds, as always, the last 2D samples of what it converted — for a conference member that is the mix —
   so the first 2T = 32 low-rate samples of a stream's first frame after joining or leaving a conference still filter the signal
   it heard before (nothing at 48000, which has no filter); pn_rate_reset_streams clears that where it matters.

   A conference is a number in [0, n_streams); PN_CONF_NONE (every stream of a new converter) is none; a conference holds at most
   PN_CONF_MAX_MEMBERS streams.  The id is a SETTING, not state: records do not carry it; pn_rate_reset, pn_rate_reset_streams,
   pn_rate_set_stream_rates and the record calls keep it — a slot that starts a new call is taken out of its conference by the
   caller.  Conferences live in one converter: none spans two contexts or devices.
   pn_rate_confs_check (host only, needs no GPU): 0 when confs[0..n) are all PN_CONF_NONE or in [0, n_streams), else -1 with
   pn_last_error naming the first bad index.
   pn_rate_set_stream_confs: streams ids[i] (distinct, in range) continue in conference confs[i].  Refused with -1, nothing
   changed or launched: a bad or duplicate id, a bad value, or a conference that would hold more than PN_CONF_MAX_MEMBERS streams
   AFTER the change (pn_last_error names it and its size) — so one call may swap members of two full conferences.  n == 0 is a
   no-op.  Asynchronous on the context's stream and ordered exactly like pn_rate_set_stream_laws: frames submitted before it use
   the old table, frames after it the new one, on the pipelined path too, with no wait; the caller may reuse its arrays on return.
   The first call that puts a stream into a conference allocates the device buffers (a second [n_streams][480] row set, the member
   table: 128 bytes per stream, a stamp per stream); no frame ever allocates.
   pn_rate_get_stream_confs: the table as last set, h_confs [n_streams].
   While no stream of the converter is in a conference a frame launches exactly what it launches without this section.
   pn_rate_mix_f32: the kernel on its own, like pn_rate_up_* / pn_rate_down_*: d_in48 -> d_out48, both [n_streams][480] float at
   16-byte aligned device addresses, asynchronous.  d_in48 == d_out48, or row sets that overlap, are refused.  ids == NULL: every
   stream advances; otherwise only the n_ids listed rows are read and written, and unlisted members contribute nothing.
   pn_rate_kernel_time takes "rate_mix" beside "rate_up" and "rate_down".
   Loudest-N selection, per-member gains and a report of the mix: the next section.
   NOT provided: conferences of more than 32 members or across contexts. */
#define PN_CONF_NONE (-1)
#define PN_CONF_MAX_MEMBERS 32
int pn_rate_confs_check(const int32_t *confs, int n, int n_streams);
int pn_rate_set_stream_confs(pn_rate *r, const int32_t *ids, int n, const int32_t *confs);
int pn_rate_get_stream_confs(const pn_rate *r, int32_t *h_confs);
int pn_rate_mix_f32(pn_rate *r, const float *d_in48, float *d_out48, const int32_t *ids, int n_ids);

/* ---- conferences: loudest-N talkers, send gains, mix report ---------------------------------------------------------------------- */
/* A bridge mixes the few loudest talkers, lets an operator mute or trim a member, and tells the application who speaks and whether
   the sum clipped.  Three settings of the conference mix above and one report, all on the GPU in the mix's own launch
   (csrc/pn_rate_mix.hip pn_rate_mix_sel_kernel), with fixed arithmetic that a float32 model reproduces bit for bit
   (tests/mix_sel_model.py; the host's statement of the level and the selection: csrc/pn_mix_rules.h).

   Arithmetic, for one frame: A = the streams that advance, y[m] = the engine's float row of stream m, c = a conference.
     send gain g_m: fp32, finite, >= 0, default 1.0f.  g_m == 0 MUTES the member: it is no talker, its row is not read (an inf or
       NaN in it reaches nobody), it contributes nothing, it is never selected — and it still hears.  Otherwise its contribution
       is x[m][j] = g_m * y[m][j], one fp32 product, never fused with the add behind it.  Gains act inside a conference only: a
       PN_CONF_NONE stream gets y[s] bit for bit whatever its gain.
     talkers of c: its members in A with g_m != 0.
     level of a talker: E_m = the sum of x*x over its 480 samples in ONE order: the products rounded separately; group q = j / 4
       (120 groups) sums its four products in index order from +0.0f; the 120 group sums, padded with +0.0f to 128, are two halves
       of 64; each half folds by the xor butterfly v[i] = v[i] + v[i ^ stride] with strides 32, 16, 8, 4, 2, 1; E = half0[0] +
       half1[0].  That is the order of the mix kernel's layout (thread t owns columns 4t..4t+3, two wavefronts) and NOT the order
       of the frame report's out_energy, whose last bits differ.
     hold: one factor d per converter, fp32 in [0, 1), default 0.  h = d * L_prev[m];  L_m = (d != 0 && isfinite(h) && h > E_m) ?
       h : E_m — a peak hold with exponential release.  d == 0: L = E exactly; a non-finite level never sticks.  L is the only new
       STATE: one float per stream.  An advancing muted member's level becomes +0.0.
     selection: every conference NUMBER c has N_c in [0, 32], default 0 = everybody.  key(L) = the uint32 bits of L with the sign
       bit cleared (NaN ranks above +inf; two NaNs rank by their bits).  Talker m is selected iff N_c == 0, or fewer than N_c
       talkers q of c have key(L_q) > key(L_m) or (key(L_q) == key(L_m) and q < m): ties go to the lower slot.
     mix: listener s in A of conference c gets o[s][j] = the sum of x[m][j] over the SELECTED talkers m != s, m ascending, from
       acc = +0.0f in plain fp32 adds — the rule of the section above with "advancing member" replaced by "selected talker".  A
       selected talker hears the other selected ones, everybody else all of them.  With all gains 1 and N_c 0 or at least the
       number of talkers the rows are bit for bit those of the section above.
   Mix report (optional): PN_MIX_REPORT_WORDS = 4 little-endian words per stream, [n_streams][4], written for every stream in A;
   the rows of other streams are left as they were:
     word 0  f32 level        L_s; +0.0 for a muted member and for a stream without a conference
     word 1  u32 flags        bit 0 selected this frame, bit 1 muted, bit 2 in a conference
     word 2  f32 mix_peak     max |o[s][j]| from 0 with fmax, so a NaN sample is ignored (the frame report's peak rule); 0 without a
                              conference
     word 3  i32 mix_clipped  the samples of o[s] whose t = o * 32768 lies outside (-32769, 32768), NaN counting: the frame report's
                              out_clipped rule applied to what the stream HEARS; 0 without a conference

   Setting calls.  Id lists follow the context's rules (distinct, in range); a bad id, a duplicate or a bad value refuses the call
   with -1, pn_last_error names the first offender, and nothing is changed or launched; n == 0 is a no-op.  Asynchronous on the
   context's stream and ordered exactly like pn_rate_set_stream_confs: frames submitted before the call use the old values, frames
   after it the new ones, on the pipelined path too, with no wait; the caller may reuse its arrays on return.
     pn_rate_set_stream_mix_gains: gains[i] for stream ids[i]; NaN, inf and negative gains are refused, -0.0f is 0.
     pn_rate_get_stream_mix_gains: h_gains [n_streams].
     pn_rate_set_conf_speakers: confs[i] distinct conference numbers in [0, n_streams), max_speakers[i] in [0, PN_CONF_MAX_MEMBERS].
     pn_rate_get_conf_speakers: h_n [n_streams], indexed by conference number.
     pn_rate_set_mix_hold: d outside [0, 1) or NaN is refused; zeroes every stream's level, in stream order.  pn_rate_get_mix_hold.
     pn_rate_set_mix_report(r, enable); pn_rate_read_mix_report: the last frame's records to h_report [n_streams][4] words,
     synchronising like pn_ctx_read_report; pn_rate_read_mix_report_dev: the same into a device buffer, asynchronous on the
     context's stream.  Both return -1 while the report is off.  Delivery through pn_host_next_report is NOT provided: on the
     pipelined path read the records with pn_rate_read_mix_report_dev between two submits, or after pn_host_wait.
   Host only, needing no GPU: pn_rate_mix_gains_check (0, or -1 naming the first bad index); pn_mix_level: E of a row of 480
   contributions x (the gain already applied; NaN and pn_last_error for a NULL row); pn_mix_select: levels[0..k) of one
   conference's talkers in ascending slot order, n_max = N_c, selected[i] = 1 | 0; returns how many are selected, -1 for k or
   n_max outside [0, 32].
   Lifecycle.  Gains, N_c, the hold factor and the report switch are SETTINGS: records do not carry them (format, version and sizes
   are unchanged); pn_rate_reset, pn_rate_reset_streams, rate changes and the record calls keep them; N_c belongs to the conference
   number and survives the conference emptying.  The level L is state that records do not carry: zeroed by pn_rate_reset, and for
   the listed streams by pn_rate_reset_streams, pn_rate_set_stream_rates and pn_rate_set_stream_confs, for all streams by
   pn_rate_set_mix_hold; a stream that does not advance keeps it; an import leaves the slot's own level.  The device buffers
   (gains, N_c, levels, report rows) are allocated inside the setting calls, never inside a frame.
   When it runs.  While every gain is 1.0f, every N_c is 0, d is 0 and the mix report is off, a frame (and pn_rate_mix_f32) launches
   exactly what it launches without this section, and the levels are not touched.  Otherwise the mix is the selecting kernel, in
   every entry point the mix runs in, pn_rate_mix_f32 included, which then also advances the levels; while a setting is off its
   default the mix runs even when no stream is in a conference (every row is then a copy, every record zero).  It is timed under
   "rate_mix".
   NOT provided: conferences of more than 32 members or across contexts, selection by voice activity rather than energy, the mix
   report on pn_host_next_report. */
#define PN_MIX_REPORT_WORDS 4
int pn_rate_mix_gains_check(const float *gains, int n);
float pn_mix_level(const float *row480);
int pn_mix_select(const float *levels, int k, int n_max, uint8_t *selected);
int pn_rate_set_stream_mix_gains(pn_rate *r, const int32_t *ids, int n, const float *gains);
int pn_rate_get_stream_mix_gains(const pn_rate *r, float *h_gains);
int pn_rate_set_conf_speakers(pn_rate *r, const int32_t *confs, int n, const int32_t *max_speakers);
int pn_rate_get_conf_speakers(const pn_rate *r, int32_t *h_n);
int pn_rate_set_mix_hold(pn_rate *r, float d);
float pn_rate_get_mix_hold(const pn_rate *r);
int pn_rate_set_mix_report(pn_rate *r, int enable);
int pn_rate_read_mix_report(pn_rate *r, void *h_report);
int pn_rate_read_mix_report_dev(pn_rate *r, void *d_report);

/* ---- packet-loss concealment: lost frames filled on the GPU ---------------------------------------------------------------------- */
/* A stream whose packet did not arrive for a 10 ms tick is neither left off the id list (a hole, the engine's state spliced across
   it) nor fed zeros (a click into the pitch and GRU state): its 48 kHz row is SYNTHESISED, a waveform substitution in the spirit of
   G.711 Appendix I restated for 48 kHz float rows, with no added delay.  It runs in one kernel (csrc/pn_rate_plc.hip) between the
   up-conversion and the engine, in place on the rows the engine reads, on a pn_rate of any kind (a mixed converter at 48000 covers
   streams that need no conversion).  The engine sees a signal that is continuous in time; the mix, the down-conversion, the frame
   report and the mix report need no change and are unchanged.  OFF by default: a converter that never enables it launches exactly
   what it launches without this section, and one that enables it and loses nothing produces the same bits.

   The rule, with every rounding and summation order, is csrc/pn_plc_rules.h (HIP-free); tests/plc_model.py restates it in numpy
   float32 and the kernel matches both bit for bit.  Every fp32 operation is singly rounded, no product is contracted into an add.
   State per stream (PN_PLC_STATE_BYTES = 10576 bytes, allocated by the first enable, never inside a frame): hist[1920], the last
   four rows the engine was given, real or synthetic, newest at hist[1919] (a ring of four rows with a head per stream); q[720],
   the period buffer; the lag P; r, the consecutive lost frames so far; the lost frames since reset.
     received, r == 0:  the row goes into the history and is not altered.
     first lost frame:  the lag.  Coarse: d[k] = hist[6k+5], k < 320; for l = 40..120, c = sum over k = 160..319 ascending of
                        d[k] d[k-l], e = the sum of d[k-l]^2; score = c*c / e where c > 0, e > 0 and the quotient is no NaN, else 0;
                        the best score wins, strictly greater in ascending l (ties and all zeros: the smallest lag).  Fine: L over
                        [max(240, 6l-5), min(720, 6l+5)], the same score over k = 960..1919, summed as 8 interleaved parts
                        (k = 960 + 8i + j, i ascending) that are then added in ascending j; same tie rule: P.
                        The period: q[i] = hist[1920-P+i] for i < P - O, O = P/4; behind that a = hist[1920-P+i],
                        b = hist[1920-2P+i], w = ((i - (P-O)) + 0.5) / O, q[i] = a + w (b - a).
     lost frame:        x[n] = g(m) q[m mod P], m = 480 r + n; g = 1 for m < 480, (2880 - m) / 2400 up to 2880, then the sample is
                        +0.0: 20 % per 10 ms, silence after 60 ms.  The row goes into the history; r += 1.
     first received frame after a loss: n < 240: x[n] = syn + w (real - syn), w = (2n+1) / 480; n >= 240: the real bits; r = 0.
   A lost stream's INPUT row is never read (NaN in it is harmless) and its up-conversion tail is left as it was: the up kernel is
   launched over the advancing streams minus the lost ones.  A frame with nothing lost launches the up kernel exactly as before.

   pn_rate_set_plc(r, enable): the first enable allocates and zeroes the state, and makes room in the context's id ring for a list
     of n_streams ids, so that no frame allocates.  While on, every frame launches the concealer between the up-conversion and the
     engine; while off nothing new is launched or read, and marks are dropped.  The frames of a pause are missing from the
     histories, so enabling again after a disable zeroes the PLC state of every stream (lost counts included), like pn_rate_reset.
   pn_rate_set_lost(r, ids, n): the listed streams are lost in the NEXT frame submitted on this converter (any pn_rate_process_*,
     _active, _host or pn_rate_submit_host_* call, or pn_rate_plc_f32), and only in that one.  Calls before one frame add up.
     Asynchronous on the context's stream and ordered exactly like pn_rate_set_stream_laws, on the pipelined path too, with no
     wait.  Refused with -1, nothing changed or launched: a bad or duplicate id, or while PLC is off.  A marked stream that does
     not advance in that frame (it is not on the _active list) keeps all its state; its mark is dropped.  A list goes to the device
     in chunks of 16384 ids; should the device refuse a later chunk (-1, a HIP error), the streams of the chunks before it are
     marked, on the host and on the device alike.
   pn_rate_plc_f32(r, d_x48, ids, n_ids): the kernel on its own, in place on [n_streams][480] float rows at a 16-byte aligned
     device address, ids as for pn_rate_up_*; it consumes the marks.  Refused while PLC is off.
   pn_rate_kernel_time takes "rate_plc".
   PLC report (optional; pn_rate_set_plc_report, pn_rate_read_plc_report synchronising, pn_rate_read_plc_report_dev asynchronous on
     the context's stream; -1 while off): PN_PLC_REPORT_WORDS = 4 little-endian uint32 words per stream, [n_streams][4], written for
     every stream that advances:
     word 0  flags   PN_PLC_CONCEALED the row is synthetic, PN_PLC_CROSSFADE it is the cross-fade out of a loss, PN_PLC_SILENT the
                     synthetic row lies wholly behind the fade (all +0.0)
     word 1  P       the lag of the last search, 0 before the first
     word 2  run     consecutive lost frames including this one; 0 for a received frame
     word 3  lost    lost frames since reset
   Lifecycle.  pn_rate_reset zeroes the PLC state of every stream; pn_rate_reset_streams and pn_rate_set_stream_rates that of the
   listed ones: a following loss conceals from an empty history, that is with silence.  Law, conference and mix settings do not touch
   it.  The tails records (pn_rate_export_streams*) do not carry it: pn_rate_import_streams and pn_rate_import_streams_host zero the
   PLC state of the slots they write (the device form whatever status a record gets), so the slot hears nothing of its previous
   stream; the call-state record ("call-state records", below), imported behind them, brings the moved stream's own history.
   Host only, needing no GPU: pn_plc_pitch (hist[1920] -> P), pn_plc_period (hist, P in [240, 720] -> q[0..P); -1 otherwise),
   pn_plc_gain (m -> g(m)).
   NOT provided: Appendix I's lengthening of the repeated segment to two and three periods on long losses (comfort noise for DTX streams: the next section);
   concealment on pn_process_* without a converter; lost marks set for the next frame in any record (a mover sets them again).  How
   the model's output quality fares on concealed frames is not measured. */
#define PN_PLC_HIST 1920
#define PN_PLC_P_MIN 240
#define PN_PLC_P_MAX 720
#define PN_PLC_REPORT_WORDS 4
#define PN_PLC_CONCEALED 1
#define PN_PLC_CROSSFADE 2
#define PN_PLC_SILENT 4
int pn_plc_pitch(const float *hist1920);
int pn_plc_period(const float *hist1920, int P, float *q);
float pn_plc_gain(int64_t m);
int pn_rate_set_plc(pn_rate *r, int enable);
int pn_rate_set_lost(pn_rate *r, const int32_t *ids, int n);
int pn_rate_plc_f32(pn_rate *r, float *d_x48, const int32_t *ids, int n_ids);
int pn_rate_set_plc_report(pn_rate *r, int enable);
int pn_rate_read_plc_report(pn_rate *r, void *h_report);
int pn_rate_read_plc_report_dev(pn_rate *r, void *d_report);

/* ---- comfort noise: DTX streams filled on the GPU --------------------------------------------------------------------------------- */
/* An endpoint with silence suppression (DTX) stops sending in a pause and sends only a silence descriptor (SID, RFC 3389 / G.711
   Appendix II): a noise level and a spectral shape.  Such a stream is neither left off the id list (the talker stops hearing the
   conference), nor marked lost (the concealer repeats speech and fades to digital silence), nor fed zeros (the noise floor the engine
   leaves under speech drops out in every pause and pumps): the row of a SILENT stream is filled with the noise its SID describes, IN
   FRONT of the engine, so the noise of a pause passes the same suppressor as the noise under speech.  One kernel (csrc/pn_rate_cng.hip)
   writes the row AT THE STREAM'S OWN RATE — the SID's spectrum is defined there — into a converter-owned buffer, and the stream's own,
   unchanged up-conversion (float) takes it to 48 kHz: the noise is band-limited like the stream's speech, and the filter tail runs
   continuously across speech, noise and speech.  Everything behind sees an ordinary row: the concealer (a received row of its
   history), the detector, the engine, level control, the mix, the reports.  A silent frame is bit for bit the frame of a float
   converter whose caller had supplied the same noise row.  OFF by default: a converter that never enables it, or enables it and marks
   nobody, launches exactly what it launches without this section and gives the same bits.

   The rule, with every rounding, is csrc/pn_cng_rules.h (HIP-free); tests/cng_model.py restates it in numpy integers and float32 and
   the kernel matches both bit for bit.  Samples are in the float convention (int16 / 32768).
   SID of a stream: PN_CNG_SID_BYTES = 14 bytes, FIXED: byte 0 = M, the number of reflection coefficients, 0..12; byte 1 = L, the level in
     -dBov, 0..127; bytes 2..13 = N_1..N_12, 0..254 each, of which the first M count (the rest is not looked at and reads back as 0).
     That is the RFC 3389 payload behind a count byte.  Refused: M > 12, L > 127, N_i = 255 for an i <= M.  A stream nobody gave a SID
     has the DEFAULT: level only, M = 0, L = PN_CNG_DEFAULT_LEVEL = 60 (-60 dBov).
   Decode (host, double, rounded once to fp32): k_i = 258 (N_i - 127) / 32768 — this formula is the contract; it is RFC 3389 section 3.2
     as remembered, no copy of the RFC was at hand —, rms = 10^(-L/20) from a table of 128 fp32 literals, g = rms sqrt(prod (1 - k_i^2)),
     so shaped noise of any spectrum has the level the SID names.
   Excitation: h = mix(mix(c) ^ key), c the stream's sample counter, key = seed ^ slot * 0x9e3779b1, mix the 32-bit murmur3 finaliser;
     u = (h & 0xffff) + (h >> 16) - 65535, triangular; e = (float)u * (1 / sqrt((2^32 - 1) / 6)).  Gaussian it is not.
   Synthesis: f = gain(n) e; for i = M..1: f = f - k_i b[i-1], and where i < M: b[i] = b[i-1] + k_i f; b[0] = f; the sample is f.
   Gain: g on the first row of a run; on a row that continues a run, prev + ((n+1) / n_s) (g - prev), prev the g of the row before: an
     unchanged SID gives g exactly, a changed one ramps across one row.  A row CONTINUES a run when the stream's row was generated in the
     converter's previous frame too; a frame in which it was received, concealed or did not advance ends the run.
   State per stream, 16 words, allocated by the first enable: b[12], the sample counter (+ n_s per generated row, wrapping), prev, the
     run, the generated rows since the state was cleared.  The end of a run leaves b and the counter: the next pause continues the
     sequence.  Every finite SID gives finite rows.  The state is zeroed by pn_rate_reset, for the listed streams by
     pn_rate_reset_streams, pn_rate_set_stream_rates, pn_rate_import_streams[_host], and by "on again"; it travels in NO record.

   pn_rate_set_cng(r, enable): the first enable allocates the state, the decoded SIDs and the rows, and makes room in the id ring, so no
     frame allocates.  Enabling again after a disable zeroes every stream's state.  Disabling drops the marks.
   pn_rate_set_cng_seed / pn_rate_get_cng_seed: the converter's seed, default PN_CNG_DEFAULT_SEED; an argument of every launch.
   pn_rate_set_stream_sid(r, ids, n, sids, stride): SID i, at sids + i * stride (stride >= 14), becomes stream ids[i]'s.  A setting,
     asynchronous and ordered like pn_rate_set_stream_laws, on the pipelined path too; valid with the switch off or never on (the
     first enable decodes what was set).  All or nothing: a bad or duplicate id or a refused SID changes nothing; every refusal
     stands in front of the first launch.  A list goes to the device in pieces of 1024 SIDs; should the device itself fail at a later
     piece (-1, a HIP error), the pieces before it are written on the device and pn_rate_get_stream_sid still gives the SIDs of before.
     pn_rate_get_stream_sid(r, h_sids): [n_streams][14] bytes as last set.
   pn_rate_set_silent(r, ids, n): the listed streams are silent in the NEXT frame submitted on this converter, and only in that one,
     with the lifetime of pn_rate_set_lost's marks; calls before one frame add up.  Refused while the switch is off.  A silent stream's
     INPUT row is never read.  A stream marked lost AND silent is concealed (lost wins); its silent mark is consumed all the same.  A
     marked stream that does not advance keeps all its state; its mark is dropped.
   pn_rate_cng_f32(r, d_x48, ids, n_ids): the stage on its own: the row of every LISTED stream (NULL: all), marked or not, is generated
     and up-converted into its row of d_x48 [n_streams][480]; other rows are not touched.  It counts as a frame: marks are dropped.
   pn_rate_kernel_time takes "rate_cng"; the second up-conversion launch counts under "rate_up".  (With the two launches a frame can
     have ten timed scopes, eleven with the DTX send side below: pn_rate_set_profiling creates 1408 events up front, on every converter.)
   CNG report (pn_rate_set_cng_report, pn_rate_read_cng_report[_dev]; -1 while off): PN_CNG_REPORT_WORDS = 4 words per stream, written
     when the stream's row is generated (other streams' records keep what they had):
     word 0  run     consecutive generated rows including this one      word 2  g     the gain in use, float bits
     word 1  total   generated rows since the state was cleared         word 3  ctr   the sample counter behind the row
   Host only, needing no GPU: pn_cng_sid_decode (14 bytes -> g, k[12], M; -1 for a refused SID), pn_cng_level (L -> the table's rms),
     pn_cng_frame (one row of one stream: the twin of the kernel, as pn_agc_frame is; cont: the row continues a run).
   The send side (VAD, the DTX decision, SID generation for outgoing streams) is the next section, "DTX send side".
   NOT provided: noise state in any record (a moved call's
   noise restarts under the new slot's key); comfort noise without a converter, or in the gap behind DTMF removal; Gaussian excitation;
   any measurement of how the model treats synthetic noise, or of perceived quality. */
#define PN_CNG_MAX_ORDER 12
#define PN_CNG_SID_BYTES 14
#define PN_CNG_DEFAULT_LEVEL 60
#define PN_CNG_DEFAULT_SEED 0x434e4731u
#define PN_CNG_REPORT_WORDS 4
int pn_cng_sid_decode(const uint8_t *sid14, float *g, float *k12, int32_t *M);
float pn_cng_level(int level);
int pn_cng_frame(const uint8_t *sid14, uint32_t *state16, uint32_t seed, int slot, int cont, int n, float *row, uint32_t *report4);
int pn_rate_set_cng(pn_rate *r, int enable);
int pn_rate_set_cng_seed(pn_rate *r, uint32_t seed);
int pn_rate_get_cng_seed(const pn_rate *r, uint32_t *seed);
int pn_rate_set_stream_sid(pn_rate *r, const int32_t *ids, int n, const uint8_t *sids, int stride);
int pn_rate_get_stream_sid(const pn_rate *r, uint8_t *h_sids);
int pn_rate_set_silent(pn_rate *r, const int32_t *ids, int n);
int pn_rate_cng_f32(pn_rate *r, float *d_x48, const int32_t *ids, int n_ids);
int pn_rate_set_cng_report(pn_rate *r, int enable);
int pn_rate_read_cng_report(pn_rate *r, void *h_report);
int pn_rate_read_cng_report_dev(pn_rate *r, void *d_report);
int pn_rate_debug_cng_state(pn_rate *r, void *h_state);                /* tests: [n_streams][16] words, synchronising */

/* ---- DTX send side: VAD, the DTX decision and SIDs for outgoing streams, on the GPU ------------------------------------------------ */
/* The section above lets a bridge HEAR an endpoint that suppresses silence; this one lets it SEND that way.  Most legs of a conference
   listen to a pause most of the time, and without this every leg is sent all 100 packets a second — or every output row goes to the
   host for a detector there, the per-stream CPU loop this library exists to replace.  With the stage ON for a stream, one kernel
   (csrc/pn_rate_dtx.hip) reads the stream's OUTPUT row BEHIND the down-conversion — behind the suppressor, the mix and the limiter,
   at the stream's own rate, in the format of the call — and leaves a decision per frame in a report row: send the frame, send this
   SID instead, or send nothing.  It WRITES NO AUDIO: a converter with streams switched on gives bit for bit the audio of one without.
   OFF by default, a switch per stream like DTMF detection: a converter on which nobody was ever switched on launches exactly what it
   launches without this section.  The SID is the 14 bytes of the section above (M, L, N_1..N_12), always one pn_rate_set_stream_sid of
   another converter accepts: the send side is the inverse of csrc/pn_cng_rules.h.

   The rule, with every rounding and summation order, is csrc/pn_dtx_rules.h (HIP-free); tests/dtx_model.py restates it in numpy float32
   and integers; the kernel, pn_dtx_frame and the model agree bit for bit.  Every fp32 operation is singly rounded.
   Samples: the output row, n_s = 80, 160, 240, 320 or 480, float as it is, int16 times 2^-15, G.711 decoded with the stream's law.
   Autocorrelation of the row alone, r[j] = sum_{n >= j} x[n] x[n-j], j = 0..12, 64 lanes' partial sums folded by the xor butterfly (the
     order of the mix level).  No history from the row before: the sequence is positive semi-definite.
   Energy e = r[0] / n_s.  A non-finite e (NaN or inf in a float row) makes the frame ACTIVE with PN_DTX_NONFINITE and changes nothing
     but the hangover and the mode.
   Floor N: the first analysed frame after a clear sets N = e and counts as ACTIVE (a stream starts by sending).  Then
     active = e > THR max(N, FLOOR_MIN), and N = e where e < N, else N += FLOOR_UP (e - N) where not active, else
     N = max(N, FLOOR_MIN) FLOOR_DRIFT.  Digital silence: rows with e == 0 in front of a stream's first other row (the zeros of the
     converter's delay) are sent and not analysed; a row of zeros later in a call takes the floor to 0, from where it climbs back at
     the drift's pace — about 40 s from FLOOR_MIN to a floor of -60 dBov at the defaults, during which the stream sends every frame.
   Hangover: an active frame sets hang = HANGOVER; a frame is sent while active or hang > 0; a frame that is not active takes one off
     hang: exactly HANGOVER frames are sent behind the last active one.
   Noise statistics R[0..12], on every frame that is not active (hangover frames included): R[j] += SMOOTH (r[j] / n_s - R[j]); the first
     such frame after a clear sets them.
   Decision: sent -> PN_DTX_FRAME, mode VOICE.  Else from VOICE -> PN_DTX_SID, mode SILENT.  Else, L being the level of R[0]:
     |L - L_sent| >= UPDATE_DB, or MAX_INTERVAL > 0 and MAX_INTERVAL frames since the last SID -> PN_DTX_SID; otherwise PN_DTX_NONE.
   Level L, -dBov: the number of i in 0..126 with R[0] < 10^(-(i + 0.5) / 10), from 127 fp32 literals; no logarithm.  R[0] = 0: 127.
   SID, on a frame that emits one: Levinson-Durbin in fp32 on R[0..ORDER] in the sign convention of the comfort-noise lattice, each k_i
     quantised inside the loop (N_i = (int)(k_i 32768/258 + 127.5)) and the recursion continued with the quantised value; it stops early
     (a smaller M) where |k_i| < 1 or the residual > 0 fails, and with M = 0 unless R[0] > 0 and finite.
   A stream that is switched off: decision FRAME, eight zero report words, no state touched.  A stream off the id list keeps both.
   Parameters, one set per converter, PN_DTX_N_PARAMS = 9 floats.  THE DEFAULTS ARE THE AUTHOR'S AND ARE NOT TUNED ON SPEECH:
     0 PN_DTX_THR 4.0 (finite, > 1)   1 PN_DTX_FLOOR_UP 0.1 ((0, 1])   2 PN_DTX_FLOOR_DRIFT 1.0023 ([1, 2))   3 PN_DTX_FLOOR_MIN 1e-10
     (finite, > 0)   4 PN_DTX_HANGOVER 20 (whole, 0..255)   5 PN_DTX_SMOOTH 0.1 ((0, 1])   6 PN_DTX_UPDATE_DB 2 (whole, 1..127)
     7 PN_DTX_MAX_INTERVAL 0 (whole, 0..65535; 0: never)   8 PN_DTX_ORDER 10 (whole, 0..12).  They travel as an argument of every launch.
   State per stream, 24 words, allocated by the first enabling, never inside a frame: R[13], N, hang, the mode, the frames since the
     last SID, the analysed frames, the last emitted SID with its count.  Zeroed by pn_rate_reset, for the listed streams by
     pn_rate_reset_streams, pn_rate_set_stream_rates, pn_rate_import_streams[_host], and for a stream that is switched on from off; a
     conference or hold change leaves it.  It travels in NO record.

   pn_rate_set_stream_dtx(r, ids, n, on) / pn_rate_get_stream_dtx: the switch, a setting ordered like pn_rate_set_stream_dtmf.
   pn_rate_set_dtx_params / pn_rate_get_dtx_params: the converter's nine parameters; refused like pn_dtx_params_check.
   A frame (pn_rate_process_*, pn_rate_submit_host_*), while somebody is switched on: one launch behind the down-conversion over the
     frame's rows, on the caller's output rows in the frame's format.
   pn_rate_dtx_f32 / _i16 / _g711(r, d_out_rows, ids, n_ids): the stage on its own over caller-supplied OUTPUT rows [n_streams][n] (a
     mixed converter: [n_streams][480]) at a 16-byte aligned device address, ids as for pn_rate_down_*.
   DTX report (pn_rate_set_dtx_report, pn_rate_read_dtx_report synchronising, pn_rate_read_dtx_report_dev asynchronous on the context's
     stream; -1 while off): PN_DTX_REPORT_WORDS = 8 little-endian 32-bit words per stream, written for every stream on a launch's list:
     word 0  the decision: PN_DTX_FRAME 0, PN_DTX_SID 1, PN_DTX_NONE 2
     word 1  PN_DTX_ON | PN_DTX_ACTIVE | PN_DTX_HANGOVER_FRAME | PN_DTX_NONFINITE in the low byte; L in bits 8..14 (the level of this frame's
             R[0] where the decision is SID or NONE, 0 on a FRAME); hang in bits 16..31
     word 2  the bits of e          word 3  the bits of N
     words 4..7  the last emitted SID's 14 bytes, then a 16-bit count of the SIDs emitted since the clear (it wraps): a caller that
             reads less often than every frame tells a new SID from the old one
   pn_rate_kernel_time takes "rate_dtx".  (A frame can now have eleven timed scopes, so pn_rate_set_profiling creates 1408 events up
     front where it created 1280, on every converter.)
   Host only, needing no GPU: pn_dtx_default_params, pn_dtx_params_check, pn_dtx_frame (one float row of one enabled stream, the twin of
     the kernel: -> the decision, -1 for a refused argument; state24 read and written, report8 may be NULL), pn_dtx_sid_from_acorr (the
     Levinson step alone on R[0..12]: -> M, the SID's level byte being that of R[0]), pn_dtx_level (a mean square -> L).
   Known limit.  The detector is an energy detector behind a suppressor.  On the comfort-noise model's most strongly shaped noise (all
     twelve coefficients large) at 80-sample rows the frame energy fluctuates enough that THR = 4 fires on about 2 % of pure-noise
     frames (12 of 535 on the numpy model); at 160 samples, or on white noise, on none.
   NOT provided: the report on pn_host_next_report; DTX state in any record (a moved call starts in VOICE and relearns its floor); a
   model-based or spectral VAD; packetisation and RTP; the send side without a converter; any measurement of detection quality on speech
   or of perceived quality. */
#define PN_DTX_N_PARAMS 9
#define PN_DTX_THR 0
#define PN_DTX_FLOOR_UP 1
#define PN_DTX_FLOOR_DRIFT 2
#define PN_DTX_FLOOR_MIN 3
#define PN_DTX_HANGOVER 4
#define PN_DTX_SMOOTH 5
#define PN_DTX_UPDATE_DB 6
#define PN_DTX_MAX_INTERVAL 7
#define PN_DTX_ORDER 8
#define PN_DTX_REPORT_WORDS 8
#define PN_DTX_FRAME 0
#define PN_DTX_SID 1
#define PN_DTX_NONE 2
#define PN_DTX_ON 1
#define PN_DTX_ACTIVE 2
#define PN_DTX_HANGOVER_FRAME 4
#define PN_DTX_NONFINITE 8
int pn_dtx_default_params(float *params9);                /* host only */
int pn_dtx_params_check(const float *params9);            /* host only */
int pn_dtx_frame(const float *params9, uint32_t *state24, const float *row, int n, uint32_t *report8);   /* host only */
int pn_dtx_sid_from_acorr(const float *R13, int order, uint8_t *sid14);                                  /* host only */
int pn_dtx_level(float mean_square);                      /* host only */
int pn_rate_set_stream_dtx(pn_rate *r, const int32_t *ids, int n, const uint8_t *on);
int pn_rate_get_stream_dtx(const pn_rate *r, uint8_t *h_on);
int pn_rate_set_dtx_params(pn_rate *r, const float *params9);
int pn_rate_get_dtx_params(const pn_rate *r, float *params9);
int pn_rate_dtx_f32(pn_rate *r, const float *d_out_rows, const int32_t *ids, int n_ids);
int pn_rate_dtx_i16(pn_rate *r, const int16_t *d_out_rows, const int32_t *ids, int n_ids);
int pn_rate_dtx_g711(pn_rate *r, const uint8_t *d_out_rows, const int32_t *ids, int n_ids);
int pn_rate_set_dtx_report(pn_rate *r, int enable);
int pn_rate_read_dtx_report(pn_rate *r, void *h_report);
int pn_rate_read_dtx_report_dev(pn_rate *r, void *d_report);
int pn_rate_debug_dtx_state(pn_rate *r, void *h_state);                /* tests: [n_streams][24] words, synchronising; zeros while no stream was ever enabled */

/* ---- automatic level control: talkers levelled on the GPU ------------------------------------------------------------------------ */
/* A quiet phone caller and a hot headset otherwise enter a conference at whatever level they arrive: loudest-N ranks raw frame
   energy, the fp32 sum of several voices clips, and the only lever is the static send gain.  Automatic gain control (AGC) brings each
   LEVELLED stream's enhanced 48 kHz row towards a target RMS of its own.  It runs in one kernel (csrc/pn_rate_agc.hip) behind the
   engine — the noise is gone there, so a plain energy gate separates speech from pauses, and every stream is a 48 kHz float row
   whatever its rate or coding — and in front of the mix or the down-conversion, in place on the engine's output rows, on a pn_rate of
   any kind.  So the mix, its levels, loudest-N selection and the send gains all see levelled rows; a stream without a conference
   hears its own levelled output; the engine's frame report (pn_ctx_set_report) and the g|r tap stay about the row BEFORE AGC.
   OFF by default: a converter that never enables it launches exactly what it launches without this section.  While on, a frame
   launches the kernel only while at least one stream's target is non-zero (the host keeps that count).

   The rule, with every rounding and summation order, is csrc/pn_agc_rules.h (HIP-free); tests/agc_model.py restates it in numpy
   float32 and the kernel matches both bit for bit.  Every fp32 operation is singly rounded, no product is contracted into an add,
   `/` and sqrtf are the correctly rounded ones.  Samples are in the float convention (int16 / 32768).
   Parameters, one set per converter, PN_AGC_N_PARAMS = 8 floats:
     0 PN_AGC_MAX_GAIN  Gmax [1, 1024] 16          1 PN_AGC_MIN_GAIN  Gmin [1/1024, 1] 0.125       2 PN_AGC_GATE_RMS theta [0, 1] 0.001
     3 PN_AGC_ATTACK    (level rising) (0, 1] 0.5  4 PN_AGC_RELEASE   (level falling) (0, 1] 0.05
     5 PN_AGC_STEP_UP   largest gain ratio per frame [1, 2] 1.0592537 (+0.5 dB)    6 PN_AGC_STEP_DOWN (0, 1] 0.8912509 (-1 dB)
     7 PN_AGC_CEILING   c (0, 1] 32767/32768
   Target, one fp32 per stream: T, the wanted RMS in (0, 1]; 0 (also -0.0f), the default of every stream: not levelled.
   State per stream (16 bytes, allocated by the first enable, never inside a frame): lev, the smoothed frame energy; gain, whose bits
   0 mean "fresh" and read as 1.0f; adapted, the frames that adapted (saturating); one spare word, always 0.
   One frame of an advancing stream, y = its 480-sample row from the engine; concealed = PLC filled this frame for it:
     T == 0:   the row and the state are not touched; the report row is {1.0f, +0.0f, 0, +0.0f}.
     E:        the energy of y in the mix's order (pn_mix_level): products rounded separately, 120 groups of four from +0.0f in index
               order, padded to 128, two halves of 64 folded by the xor butterfly 32..1, E = half0[0] + half1[0].
     p:        max |y[j]| from +0.0f with fmaxf, so a NaN sample is ignored.     Eg = (theta*theta)*480.0f, Tt = (T*T)*480.0f.
     voiced:   E > Eg && E <= FLT_MAX && !concealed.
     level:    not voiced: lev' = lev.  Voiced, lev == 0: lev' = E.  Voiced otherwise: a = E > lev ? attack : release, d = E - lev,
               t = a*d, lev' = lev + t.
     desired:  voiced: g* = sqrtf(Tt / lev'), then g* > Gmax -> Gmax (AT_MAX), then g* < Gmin -> Gmin (AT_MIN).  Otherwise g* = g0, the
               stored gain (1.0f when fresh): a pause, a concealed frame and a row of NaN or inf HOLD the gain.
     slew:     hi = g0*step_up, lo = g0*step_down, g1 = fminf(fmaxf(g*, lo), hi).
     limiter:  m = fmaxf(g0, g1); if p <= FLT_MAX && p*m > c (LIMITED): gl = fmaxf(c / p, Gmin), g0' = fminf(g0, gl),
               g1' = fminf(g1, gl); otherwise g0' = g0, g1' = g1.  A row whose peak exceeds c / Gmin is beyond rescue and CLIPS.
     apply:    w_j = (float)(2j+1) / 960.0f, d = g1' - g0', out[j] = y[j] * (g0' + w_j*d): one product, one add, one product, none
               fused.  With g0' == g1' == 1.0f the row keeps its bits, -0.0 included.
     state:    lev = lev', gain = g1', adapted += voiced.

   pn_rate_set_agc(r, enable): the first enable allocates and zeroes the state and the target table; a frame never allocates.
     Enabling again after a disable zeroes every stream's state (the frames of the pause are missing from the levels); targets and
     parameters stay.  While off nothing new is launched or read.
   pn_rate_set_agc_params(r, params[8]) / pn_rate_get_agc_params: one set for the converter, from the next frame submitted on (they
     travel as an argument of every launch, so they are ordered like one).  Refused with -1, nothing changed: NaN or a value outside
     its range, pn_last_error naming the FIRST bad index.  Host only: pn_agc_default_params(params[8]), pn_agc_params_check(params[8]).
   pn_rate_set_stream_agc_targets(r, ids, n, targets) / pn_rate_get_stream_agc_targets / pn_rate_agc_targets_check(targets, n): the id
     list rules of pn_rate_set_stream_mix_gains (distinct ids in range, the first offender named, n == 0 a no-op); every target 0 or in
     (0, 1], NaN refused.  Asynchronous on the context's stream and ordered against frames exactly like the mix gains, on the pipelined
     path too.  It changes the target only; the state stays.  Refused while AGC is off.
   pn_rate_agc_f32(r, d_y48, ids, n_ids): the kernel on its own, in place on [n_streams][480] float rows at a 16-byte aligned device
     address, ids as for pn_rate_up_*; nobody counts as concealed.  Refused while AGC is off.
   pn_agc_frame(params, target, state4, row_in480, row_out480, concealed) -> flags, or -1 for a bad argument: host only, the rule above
     on one row (row_out may be row_in); state4: the four state words, read and written.
   pn_rate_kernel_time takes "rate_agc".
   AGC report (optional; pn_rate_set_agc_report, pn_rate_read_agc_report synchronising, pn_rate_read_agc_report_dev asynchronous on
     the context's stream; -1 while off): PN_AGC_REPORT_WORDS = 4 little-endian 32-bit words per stream, [n_streams][4], written for
     every stream that advances in a frame that launches the kernel:
     word 0  f32 g1'     the gain at the row's end, the stored one
     word 1  f32 lev'    the smoothed energy
     word 2  u32 flags   PN_AGC_ON the stream is levelled, PN_AGC_ADAPTED the frame was voiced, PN_AGC_LIMITED the limiter acted,
                         PN_AGC_AT_MAX / PN_AGC_AT_MIN the desired gain was clamped, PN_AGC_HELD_LOST the frame was concealed
     word 3  f32 p       the row's peak before the gain
   Lifecycle.  pn_rate_reset zeroes the AGC state of every stream; pn_rate_reset_streams, pn_rate_set_stream_rates and both import
   forms (pn_rate_import_streams, pn_rate_import_streams_host) that of the listed slots.  A stream that does not advance keeps its
   state.  Targets, parameters and the switches are settings that survive all of those.  The tails records do not carry the AGC
   state and their format and sizes are untouched; the call-state record ("call-state records", below) carries it.  With PLC on, a stream is concealed in the frame whose marks the concealer consumed; once in 2^32
   frames, when the concealer's tick wraps, that frame's concealed streams count as received.
   A sum of levelled voices can still pass full scale: the output limiter (next section) keeps the mix under a ceiling.
   NOT provided: targets in dBFS; targets and parameters in any record (they are settings: a mover sets them on the target); AGC
   without a converter; loudness weighting (K-weighting); any measurement of perceived quality. */
#define PN_AGC_N_PARAMS 8
#define PN_AGC_MAX_GAIN 0
#define PN_AGC_MIN_GAIN 1
#define PN_AGC_GATE_RMS 2
#define PN_AGC_ATTACK 3
#define PN_AGC_RELEASE 4
#define PN_AGC_STEP_UP 5
#define PN_AGC_STEP_DOWN 6
#define PN_AGC_CEILING 7
#define PN_AGC_REPORT_WORDS 4
#define PN_AGC_ON 1
#define PN_AGC_ADAPTED 2
#define PN_AGC_LIMITED 4
#define PN_AGC_AT_MAX 8
#define PN_AGC_AT_MIN 16
#define PN_AGC_HELD_LOST 32
int pn_agc_default_params(float *params8);                /* host only */
int pn_agc_params_check(const float *params8);            /* host only */
int pn_agc_frame(const float *params8, float target, uint32_t *state4, const float *row_in480, float *row_out480, int concealed);   /* host only */
int pn_rate_agc_targets_check(const float *targets, int n);   /* host only */
int pn_rate_set_agc(pn_rate *r, int enable);
int pn_rate_set_agc_params(pn_rate *r, const float *params8);
int pn_rate_get_agc_params(const pn_rate *r, float *params8);
int pn_rate_set_stream_agc_targets(pn_rate *r, const int32_t *ids, int n, const float *targets);
int pn_rate_get_stream_agc_targets(const pn_rate *r, float *h_targets);
int pn_rate_agc_f32(pn_rate *r, float *d_y48, const int32_t *ids, int n_ids);
int pn_rate_set_agc_report(pn_rate *r, int enable);
int pn_rate_read_agc_report(pn_rate *r, void *h_report);
int pn_rate_read_agc_report_dev(pn_rate *r, void *d_report);

/* ---- output limiter: a mix that does not clip ------------------------------------------------------------------------------------- */
/* The level control brings every talker to the same RMS and the mix then sums up to 31 of them, so the sum leaves the int16 / G.711
   range; pn_ctx_set_output_saturate turns the wrap into hard clipping, which is audible.  The output limiter is a per-stream gain
   as the LAST stage in front of the down-conversion, in one kernel (csrc/pn_rate_lim.hip), in place on the 48 kHz float row the
   down-conversion is about to read: the mix row of a conference member, every other stream's own (levelled) output, on a pn_rate of
   any kind.  The whole 10 ms row is in hand there, so the gain looks ahead INSIDE the row without adding delay: it ramps down from
   the previous row's end value and is at the needed gain exactly at the first sample that needs it.
   OFF by default: a converter that never sets a ceiling launches exactly what it launches without this section, and a frame launches
   the kernel only while at least one stream's ceiling is non-zero (the host keeps that count).  The mix report's mix_peak /
   mix_clipped stay about the mix BEFORE the limiter, the frame report and the g|r tap about the stream's own output; the limiter's
   report is the new information.

   The rule, with every rounding and the proof of the guarantee, is csrc/pn_lim_rules.h (HIP-free); tests/lim_model.py restates it in
   numpy float32 and the kernel matches both bit for bit.  Every fp32 operation is singly rounded, `/` is the correctly rounded one.
   Ceiling, one fp32 per stream: c in [1/1024, 1] (float convention, int16 / 32768); 0 (also -0.0f), the default: not limited.
   Parameters, one set per converter, PN_LIM_N_PARAMS = 2 floats:
     0 PN_LIM_RELEASE  R, the largest gain ratio per frame on the way back to 1   [1, 2]   1.0592537 (+0.5 dB, the AGC's step)
     1 PN_LIM_HOLD     H, the frames the gain is held after an attack             a whole number in [0, 1000]   2
   State per stream (16 bytes, allocated by the first pn_rate_set_stream_limiter that sets a ceiling, never inside a frame): gain,
   whose bits 0 mean "fresh" and read as 1.0f; hold, the frames still to hold; limited, the frames whose gain was under 1
   (saturating); one spare word, always 0.
   One frame of an advancing stream with c > 0, o = its 480-sample row:
     g0, h:      the stored gain and hold count.       p = max |o[j]| from +0.0f with fmaxf, so a NaN sample is ignored.
     non-finite: !(p <= FLT_MAX) (NONFINITE): row and state are not touched.
     needed:     p > c: q = c / p; if p*q > c, q becomes the float one bit below it; gl = q.  Otherwise gl = 1.0f.
     attack:     gl < g0 (ATTACK | ACTIVE): k = the first j with |o[j]|*g0 > c, or 480; out[j] = o[j] * (g0 + ((float)j / (float)k) *
                 (gl - g0)) for j < k and o[j]*gl for j >= k; g1 = gl, h' = H.  The gain steps only when k == 0.
     otherwise:  h > 0 (HOLDING): g1 = g0, h' = h - 1.  h == 0: g1 = fminf(fminf(g0*R, 1.0f), gl), RELEASING when g1 > g0.  ACTIVE when
                 g0 < 1 or g1 < 1.  The row is scaled by the level control's ramp between g0 and g1 (out[j] = o[j] * (g0 + w_j*(g1 - g0)),
                 w_j = (float)(2j+1) / 960.0f); with g0 == g1 == 1.0f the row is NOT written and keeps its bits.
     state:      gain = g1, hold = h', limited += ACTIVE.
   Guarantee: for every finite row, |out[j]| <= c as floats for every sample that is not NaN (rounding is monotone; pn_lim_rules.h).

   pn_rate_set_stream_limiter(r, ids, n, ceilings) / pn_rate_get_stream_limiter / pn_rate_limiter_ceilings_check(ceilings, n): the id
     list rules of pn_rate_set_stream_agc_targets (distinct ids in range, the first offender named, n == 0 a no-op); every ceiling 0
     or in [1/1024, 1], NaN refused; a refused call changes and launches nothing.  Asynchronous on the context's stream and ordered
     against frames exactly like the AGC targets, on the pipelined path too.  It changes the ceiling only; the state stays.
   pn_rate_set_limiter_params(r, params[2]) / pn_rate_get_limiter_params: one set for the converter, from the next frame submitted on
     (an argument of every launch).  Refused with -1, nothing changed: NaN, a value outside its range, a hold that is no whole
     number, pn_last_error naming the FIRST bad index.  Host only: pn_lim_default_params(params[2]), pn_lim_params_check(params[2]).
   pn_rate_lim_f32(r, d_o48, ids, n_ids): the kernel on its own, in place on [n_streams][480] float rows at a 16-byte aligned device
     address, ids as for pn_rate_up_*.
   pn_lim_frame(params, ceiling, state4, row_in480, row_out480, report4) -> flags, or -1 for a bad argument: host only, the rule above
     on one row (row_out may be row_in); state4: the four state words, read and written; report4: the report row, or NULL.
   pn_rate_kernel_time takes "rate_lim".
   Limiter report (optional; pn_rate_set_limiter_report, pn_rate_read_limiter_report synchronising, pn_rate_read_limiter_report_dev
     asynchronous on the context's stream; -1 while off): PN_LIM_REPORT_WORDS = 4 little-endian 32-bit words per stream,
     [n_streams][4], written for every stream that advances in a frame that launches the kernel:
     word 0  f32 g1       the gain at the row's end, the stored one (a non-finite row: g0)
     word 1  f32 p        the row's peak before the gain
     word 2  u32 flags    PN_LIM_ON the stream is limited, PN_LIM_ATTACK the gain came down inside this row, PN_LIM_HOLDING,
                          PN_LIM_RELEASING the gain rose, PN_LIM_ACTIVE the row met a gain under 1, PN_LIM_NONFINITE
     word 3  u32 limited  the frames that were ACTIVE
     A stream whose ceiling is 0: {1.0f, +0.0f, 0, 0}.
   Lifecycle.  pn_rate_reset zeroes the limiter state of every stream; pn_rate_reset_streams, pn_rate_set_stream_rates and both import
   forms that of the listed slots.  A stream that does not advance keeps its state.  Ceilings, parameters and the report switch are
   settings that survive all of those.  The tails records do not carry the limiter state and their format and sizes are untouched;
   the call-state record ("call-state records", below) carries it.
   NOT provided: look-ahead beyond the row (that would add delay); ceilings and parameters in any record (they are settings: a mover
   sets them on the target); a limiter without a converter; any measurement of perceived quality. */
#define PN_LIM_N_PARAMS 2
#define PN_LIM_RELEASE 0
#define PN_LIM_HOLD 1
#define PN_LIM_REPORT_WORDS 4
#define PN_LIM_ON 1
#define PN_LIM_ATTACK 2
#define PN_LIM_HOLDING 4
#define PN_LIM_RELEASING 8
#define PN_LIM_ACTIVE 16
#define PN_LIM_NONFINITE 32
int pn_lim_default_params(float *params2);                /* host only */
int pn_lim_params_check(const float *params2);            /* host only */
int pn_lim_frame(const float *params2, float ceiling, uint32_t *state4, const float *row_in480, float *row_out480, uint32_t *report4);   /* host only */
int pn_rate_limiter_ceilings_check(const float *ceilings, int n);   /* host only */
int pn_rate_set_stream_limiter(pn_rate *r, const int32_t *ids, int n, const float *ceilings);
int pn_rate_get_stream_limiter(const pn_rate *r, float *h_ceilings);
int pn_rate_set_limiter_params(pn_rate *r, const float *params2);
int pn_rate_get_limiter_params(const pn_rate *r, float *params2);
int pn_rate_lim_f32(pn_rate *r, float *d_o48, const int32_t *ids, int n_ids);
int pn_rate_set_limiter_report(pn_rate *r, int enable);
int pn_rate_read_limiter_report(pn_rate *r, void *h_report);
int pn_rate_read_limiter_report_dev(pn_rate *r, void *d_report);

/* ---- call-state records: a live call moves whole ------------------------------------------------------------------------------- */
/* The tails record above carries the two filters' tails.  The concealer's history, the level control's gain, the limiter's gain and
   hold and the level the loudest-N hold keeps live on the converter too, and pn_rate_import_streams[_host] zero them on purpose
   (the slot is another stream's now).  A SECOND record with entry points of its own carries them, so that a stream moved between
   slots, contexts, devices and processes continues bit for bit: the frame after the move is the frame an unbroken run gives,
   also in the middle of a loss, of a limiter hold or of an AGC slew.  The record does not depend on the stream's rate: one size for
   every rate, and a 48000 stream of a mixed converter — which has no tails record — has this one.
   The layout and the verdict are stated once in csrc/pn_call_rules.h (HIP-free); tests/call_state_model.py restates both.

   Record (little-endian, PN_RATE_CALL_STATE_BYTES = 10640, every section 16-byte aligned):
     header 16 B: uint32 magic PN_RATE_CALL_MAGIC | uint32 version PN_RATE_CALL_VERSION | uint32 record bytes | uint32 section mask
     body, words:    0 PN_CALL_W_HIST  1920 f32  the concealer's history in its LINEAR view, oldest sample first
                  1920 PN_CALL_W_Q      720 f32  its period buffer
                  2640 PN_CALL_W_META     4 u32  P | r | lost | 0   (the ring's head is normalised away: the record is phase-free)
                  2644 PN_CALL_W_AGC      4 u32  the level control's state: lev | gain | adapted | spare
                  2648 PN_CALL_W_LIM      4 u32  the limiter's state: gain | hold | limited | spare
                  2652 PN_CALL_W_MIX      4      the held level f32 | 3 zero words
   Section mask: PN_CALL_PLC | PN_CALL_AGC | PN_CALL_LIM | PN_CALL_MIX, the states the exporting converter HELD — PLC while its switch
   is on, AGC once it was ever enabled, the limiter once a ceiling was ever set, MIX once a mix setting ever left its default
   (pn_rate_call_state_sections gives the mask).  A section whose bit is clear is all zero.
   pn_rate_call_state_check (host only): PN_SS_OK, or PN_SS_BAD_ARG (NULL), PN_SS_BAD_MAGIC, PN_SS_BAD_VERSION, PN_SS_BAD_SIZE (the
   buffer or the size word is not 10640), or PN_SS_BAD_STATE: a mask with an unknown bit; a present section that breaks an invariant
   its kernel relies on — PLC: P == 0 or 240 <= P <= 720, r > 0 only with P != 0, word 3 zero; AGC: lev >= 0 and no NaN, gain bits 0
   or a value in [1/1024, 1024], spare 0; limiter: gain bits 0 or a value in (0, 1], spare 0; MIX: level finite and >= 0, padding 0
   — or an absent section that is not all zero.

   Export (duplicates allowed): record i gets the header with the converter's mask, the held sections of stream ids[i] — the PLC
   ring in age order — and zeros everywhere else.
   Import (distinct ids): each record is judged on its own.  Section by section, an accepted record's section that the target holds
   is written (the ring at head 0); a section the target holds and the record lacks is ZEROED (a fresh state); a section the record
   has and the target does not hold is dropped.  A refused record leaves its stream exactly as it was.
   Device forms: asynchronous on the context's stream and ordered like pn_rate_export_streams, on the pipelined path too; records at a
   16-byte aligned device address, PN_RATE_CALL_STATE_BYTES apart; d_status[i] (required) receives exactly
   pn_rate_call_state_check(record_i, PN_RATE_CALL_STATE_BYTES), and the other records of the call are still imported.  Refused on the
   host with -1, nothing written or launched: a bad or (import) duplicate id, a misaligned or NULL pointer.  n == 0 is a no-op.
   Host forms: synchronous like pn_rate_export_streams_host (frames in flight complete first); the import checks EVERY record before
   anything is launched and is all-or-nothing.
   No call allocates state: a converter that holds nothing exports records with mask 0, and an import into it writes nothing and
   still reports PN_SS_OK.  Both converter kinds, every rate.

   The order a mover follows on the target:
     1. the settings: rates, laws, conferences, send gains, caps and hold, AGC switch, parameters and targets, ceilings and limiter
        parameters, the PLC switch (several of them reset the state they govern, which is why they come first);
     2. pn_ctx_import_streams — the engine's state;
     3. pn_rate_import_streams — the tails (not for a 48000 stream); it still zeroes the four states;
     4. pn_rate_import_call_state — the four states.
   NOT state, and not carried by any record: lost marks set for the next frame (pn_rate_set_lost; the mover sets them again), every
   setting, every report row. */
#define PN_RATE_CALL_MAGIC 0x53434e50u         /* "PNCS" */
#define PN_RATE_CALL_VERSION 1
#define PN_RATE_CALL_STATE_BYTES 10640
#define PN_CALL_PLC 1
#define PN_CALL_AGC 2
#define PN_CALL_LIM 4
#define PN_CALL_MIX 8
#define PN_CALL_W_HIST 0
#define PN_CALL_W_Q 1920
#define PN_CALL_W_META 2640
#define PN_CALL_W_AGC 2644
#define PN_CALL_W_LIM 2648
#define PN_CALL_W_MIX 2652
#define PN_CALL_BODY_WORDS 2656
size_t pn_rate_call_state_bytes(void);                                    /* host only */
int pn_rate_call_state_check(const void *record, size_t bytes);           /* host only */
int pn_rate_call_state_sections(const pn_rate *r);                        /* the held mask; -1 for NULL */
int pn_rate_export_call_state(pn_rate *r, const int32_t *ids, int n, void *d_records);
int pn_rate_import_call_state(pn_rate *r, const int32_t *ids, int n, const void *d_records, int32_t *d_status);
int pn_rate_export_call_state_host(pn_rate *r, const int32_t *ids, int n, void *h_records);
int pn_rate_import_call_state_host(pn_rate *r, const int32_t *ids, int n, const void *h_records);

/* ---- DTMF detection: a pressed key is read on the GPU ------------------------------------------------------------------------------ */
/* "Press 1 to mute", PINs and menu choices arrive as in-band dual tones (DTMF).  The detector reads each ENABLED stream's 48 kHz fp32
   row behind the up-conversion and the concealer and IN FRONT of the engine — the network keeps speech and drops everything else, and
   what it does to a dual tone is unmeasured — in one kernel (csrc/pn_rate_dtmf.hip), on a pn_rate of any kind, whatever the stream's
   rate or coding.  It only reads the rows: the audio is bit for bit what it is without detection, the tone included.
   OFF by default for every stream: a converter on which no stream is enabled launches exactly what it launches without this section
   (the host keeps the count of enabled streams).

   The rule, with every rounding and summation order, is csrc/pn_dtmf_rules.h (HIP-free); tests/dtmf_model.py restates it in numpy
   float32 and the kernel matches both bit for bit.  Every fp32 operation is singly rounded, no product is contracted into an add.
   Frequencies f[0..3] = 697, 770, 852, 941 Hz (rows), f[4..7] = 1209, 1336, 1477, 1633 Hz (columns); the digit code of row r and column c
   is the ASCII of "123A456B789C*0#D"[4r + c].  Tables in double, narrowed once: m = (f[k]*j) % 48000 in integers,
   a = 6.283185307179586*m/48000.0, ct[k][j] = (float)cos(a), st[k][j] = (float)sin(a), j = 0..479; the frame's rotation cr[k], ci[k]
   from m = (f[k]*480) % 48000.  pn_dtmf_tables(ct[8][480], st[8][480], rot16 = cr then ci) copies them out (host only).
   Parameters, one set per converter, PN_DTMF_N_PARAMS = 7 floats:
     0 PN_DTMF_MIN_RMS   [0, 1] 0.005     1 PN_DTMF_PURITY (0, 1] 0.5      2 PN_DTMF_TWIST_FWD [1, 100] 6.3   3 PN_DTMF_TWIST_REV [1, 100] 6.3
     4 PN_DTMF_REL       [1, 100] 6.3     5 PN_DTMF_ON_FRAMES, 6 PN_DTMF_OFF_FRAMES: whole numbers in [1, 100], 3 and 2
   State per stream (96 bytes = 24 words, allocated by the first enabling, never inside a frame; all zero is fresh): 0..7 Cp, 8..15 Sp,
   16 Ep — the previous row's half sums — 17 cand | run << 16, 18 cur | gap << 16, 19 dur, 20 count, 21 last4, 22 and 23 zero.
   One frame of an advancing, enabled stream, x = its 480-sample row:
     half sums: C[k] = sum x[j]*ct[k][j], S[k] = sum x[j]*st[k][j], Ec = sum x[j]*x[j]; all 17 in the order of pn_mix_level: products
                rounded separately, 120 groups of four from +0.0f in index order, padded to 128, two halves of 64 folded by the xor
                butterfly 32..1, the sum = half0[0] + half1[0].
     window:    the 20 ms of the previous row and this one: A = Cp + (C*cr - S*ci), B = Sp + (S*cr + C*ci), every product and sum rounded
                separately in that bracketing; P[k] = A*A + B*B; E = Ep + Ec; then Cp, Sp, Ep = C, S, Ec.
     peaks:     Pr = -1.0f, r = 0; k = 0..3 in order: P[k] > Pr -> Pr = P[k], r = k; Pc and c likewise over k = 4..7.  Ties go to the lower
                index, a NaN never wins.
     hit:       E <= FLT_MAX && E >= (min_rms*min_rms)*960.0f && Pr + Pc >= (purity*480.0f)*E && Pc <= Pr*twist_fwd && Pr <= Pc*twist_rev
                && P[k]*rel <= its group's peak for every other k of either group; any NaN makes it false.  (A pure dual tone has
                P[r] + P[c] = 480 E.)      d = the digit code on a hit, else 0.
     debounce:  1. d != 0 && d == cand: run += 1 (saturating at 65535); otherwise cand = d, run = d ? 1 : 0.
                2. cur != 0 && d == cur: gap = 0, dur += 1.
                3. cur != 0 && d != cur: gap += 1; gap >= off_frames: END, the ended digit and its dur go to the report, cur = 0 (gap and
                   dur too); otherwise dur += 1.
                4. cur == 0 && d != 0 && run >= on_frames: cur = d, gap = 0, dur = run, count += 1 (saturating), BEGIN,
                   last4 = (last4 << 8) | d.   (With on_frames = off_frames = 1 a changed digit ENDs and BEGINs in one frame.)
     concealed (PLC filled this frame for the stream): the whole state stays, the row is not read; the report repeats cur with HELD_LOST.
     not enabled: neither the row nor the state is read; the report row is four zero words.

   pn_rate_set_stream_dtmf(r, ids, n, on) / pn_rate_get_stream_dtmf(r, h_on[n_streams]): the id list rules of
     pn_rate_set_stream_limiter (distinct ids in range, the first offender named, n == 0 a no-op); on[i] != 0 enables.  A setting,
     asynchronous on the context's stream and ordered against frames like the limiter's ceilings, on the pipelined path too.  The first
     enabling allocates the state, the switch words and the tables; a frame never allocates.  Enabling a stream that was off zeroes its
     state; enabling one that is on, or disabling, leaves it.
   pn_rate_set_dtmf_params(r, params[7]) / pn_rate_get_dtmf_params: one set for the converter, from the next frame submitted on (they
     travel as an argument of every launch, so they are ordered like one).  Refused with -1, nothing changed: NaN, a value outside its
     range or a frame count that is no whole number, pn_last_error naming the FIRST bad index.  Host only: pn_dtmf_default_params,
     pn_dtmf_params_check.
   pn_rate_dtmf_f32(r, d_x48, ids, n_ids): the kernel on its own over [n_streams][480] float rows at a 16-byte aligned device address,
     ids as for pn_rate_up_*; nobody counts as concealed.
   pn_dtmf_frame(params, state24, row480, concealed, report4) -> the report's flags, or -1 for a bad argument: host only, the rule above
     on one row of an enabled stream; state24 is read and written, report4 may be NULL.
   pn_rate_kernel_time takes "rate_dtmf".
   DTMF report (optional; pn_rate_set_dtmf_report, pn_rate_read_dtmf_report synchronising, pn_rate_read_dtmf_report_dev asynchronous on
     the context's stream; -1 while off): PN_DTMF_REPORT_WORDS = 4 little-endian 32-bit words per stream, [n_streams][4], written for
     every stream that advances in a frame that launches the kernel:
     word 0  flags | cur << 8 | ended << 16: PN_DTMF_ON the stream is enabled, PN_DTMF_HIT this frame's window is a digit's,
             PN_DTMF_BEGIN cur began in this frame, PN_DTMF_END `ended` ended in it, PN_DTMF_HELD_LOST the frame was concealed
     word 1  the dur of cur in frames — or, with cur == 0 in a frame that ENDs, of the digit that ended
     word 2  count, the digits begun since the state was fresh
     word 3  last4, the four digits begun last, newest in the low byte: a caller that reads less often than every frame loses none
   It is NOT part of pn_host_next_report.
   Lifecycle.  pn_rate_reset zeroes the detector state of every stream; pn_rate_reset_streams, pn_rate_set_stream_rates and both import
   forms (pn_rate_import_streams, pn_rate_import_streams_host) that of the listed slots.  A stream that does not advance keeps its
   state.  Switches and parameters are settings that survive all of those.  NO record carries the detector state — the three record
   formats are untouched — so a digit in flight when a call moves is reported AGAIN with BEGIN on the target (count and last4 start
   from zero there).  With PLC on, a stream is concealed in the frame whose marks the concealer consumed.
   Removing the tone from the audio and RFC 4733 events: the next section.
   NOT provided: second-harmonic talk-off tests; any claim of Q.24
   conformance; detection without a converter; detector state in a record; the report on pn_host_next_report. */
#define PN_DTMF_N_PARAMS 7
#define PN_DTMF_MIN_RMS 0
#define PN_DTMF_PURITY 1
#define PN_DTMF_TWIST_FWD 2
#define PN_DTMF_TWIST_REV 3
#define PN_DTMF_REL 4
#define PN_DTMF_ON_FRAMES 5
#define PN_DTMF_OFF_FRAMES 6
#define PN_DTMF_REPORT_WORDS 4
#define PN_DTMF_ON 1
#define PN_DTMF_HIT 2
#define PN_DTMF_BEGIN 4
#define PN_DTMF_END 8
#define PN_DTMF_HELD_LOST 16
int pn_dtmf_default_params(float *params7);               /* host only */
int pn_dtmf_params_check(const float *params7);           /* host only */
int pn_dtmf_frame(const float *params7, uint32_t *state24, const float *row480, int concealed, uint32_t *report4);   /* host only */
int pn_dtmf_tables(float *ct, float *st, float *rot16);   /* host only */
int pn_rate_set_stream_dtmf(pn_rate *r, const int32_t *ids, int n, const uint8_t *on);
int pn_rate_get_stream_dtmf(const pn_rate *r, uint8_t *h_on);
int pn_rate_set_dtmf_params(pn_rate *r, const float *params7);
int pn_rate_get_dtmf_params(const pn_rate *r, float *params7);
int pn_rate_dtmf_f32(pn_rate *r, const float *d_x48, const int32_t *ids, int n_ids);
int pn_rate_set_dtmf_report(pn_rate *r, int enable);
int pn_rate_read_dtmf_report(pn_rate *r, void *h_report);
int pn_rate_read_dtmf_report_dev(pn_rate *r, void *d_report);
int pn_rate_debug_dtmf_state(pn_rate *r, void *h_state);   /* tests and debugging: [n_streams][24] state words to the host, synchronising; zeros while no stream was ever enabled */

/* ---- DTMF removal: a pressed key is muted ahead of the mix, and handed on as an RFC 4733 event -------------------------------------- */
/* A member who types a PIN is heard by the whole conference, the tone competes in loudest-N and drives the level control, and a gateway
   behind the bridge detects the digit a second time.  With removal ON for a stream, detected DTMF is taken out of its enhanced 48 kHz
   row (y48) by one kernel (csrc/pn_rate_dtmf_clamp.hip) BEHIND the engine and IN FRONT of the level control, the mix, the limiter and
   the down-conversion.  It costs no delay: output row t of pn_process_* is input row t - 6 (60 ms, whole rows), the detector sits in
   front of the engine, so this stage knows the verdict on a row five frames before the row comes out and removes a digit from its first
   sample, with a fade in front of it.  OFF by default for every stream: a converter on which removal is on for nobody launches exactly
   what it launches without this section and produces the same bytes (the host keeps the count).  Removal needs detection (DTMF
   detection, above) on the same stream; a stream with removal on and detection off is left alone.

   The rule is csrc/pn_dtmf_clamp_rules.h (HIP-free); tests/dtmf_clamp_model.py restates it in numpy and the kernel matches both bit for
   bit.  The stage reads the detector's REPORT row of this frame (flags | cur << 8 | ended << 16, dur, ..) and nothing else of it; while
   removal is on for some stream the detector's kernel writes its report whether or not pn_rate_set_dtmf_report is on (reading it
   stays refused while that is off).  The detector, its state, its rule and its report are unchanged.
   Parameters, one set per converter, PN_DTMF_CLAMP_N_PARAMS = 4 int32:
     0 PN_DTMF_CLAMP_PRE   rows removed in front of a marked row [0, 4] 1      1 PN_DTMF_CLAMP_POST  rows removed behind one [0, 8] 0
     2 PN_DTMF_CLAMP_VOLUME  the volume field of a payload [0, 63] 10          3 PN_DTMF_CLAMP_TS_PER_FRAME  RTP units per frame [1, 65535] 80
   In time: a mark of input row p is final by frame p + on_frames (PN_DTMF_ON_FRAMES), so nothing is late exactly when
   on_frames + pre <= 5.  Calls that would break this are refused as a whole, naming the values: pn_rate_set_dtmf_clamp_params,
   pn_rate_set_stream_dtmf_clamp (switching somebody on) and, while removal is on for some stream, pn_rate_set_dtmf_params.
   State per stream (16 bytes = 4 words, in an array of its own, allocated by the first enabling, never inside a frame; all zero is
   fresh): w0 marks, a 32-bit shift register, bit i the mark of input row t - i; w1 bit 0 cut: the previous output row ended at gain 0;
   w2 rows muted so far (saturating); w3 the dur of the previous frame's ongoing event.
   One frame of an advancing stream with removal on, det = the detector's report row of this frame:
     marks:    marks <<= 1.  det four zero words (detection off): nothing is set.  Otherwise BEGIN with duration dur (the run of hits):
               bits 0..min(dur, 31) are set (a hit window spans two rows, dur hits cover dur + 1 rows).  Otherwise cur != 0: bit 0 is
               set, gap frames and concealed frames (HELD_LOST) of a digit included.
     decision: M(k) = any mark bit in [k - pre, k + post] clipped to 0..31; the output row is input row t - 6: m = M(6), m_next = M(5);
               the gain at the row's end e = (m || m_next) ? 0 : 1, at its start s = cut ? 0 : 1.
     the row:  m: all 480 samples become +0.0f, written without being read (a NaN in a removed row is gone), MUTED; with s == 1 the cut
               is hard: LATE.  !m, s 1, e 0: fade out, x[j] * ((float)(479 - j) / 480.0f), FADE_OUT.  !m, s 0, e 1: fade in,
               x[j] * ((float)(j + 1) / 480.0f), FADE_IN.  !m, s 0, e 0: zeros, FADE_OUT | FADE_IN.  s 1, e 1: the row is neither read
               nor written.  Each ramp value is one correctly rounded fp32 quotient, each product rounded once.  Then cut = (e == 0).
     events (RFC 4733 section 2.3): a payload is the 32-bit value event << 24 | E << 23 | volume << 16 | duration, to be sent big-endian;
               event 0..9 for '0'..'9', 10 '*', 11 '#', 12..15 'A'..'D'; duration = min(dur * ts_per_frame, 65535).  While cur != 0: the
               ongoing event, E = 0 (a concealed frame repeats it).  In a frame with END: the ended digit, E = 1, with the dur of the
               previous frame's ongoing event (w3; one frame's where the state never saw the digit ongoing).  0 means no event; a real
               payload is never 0.  Events are about the INPUT: they run 60 ms AHEAD of the audio they describe.
   Removal report (optional; pn_rate_set_dtmf_clamp_report, pn_rate_read_dtmf_clamp_report synchronising,
     pn_rate_read_dtmf_clamp_report_dev asynchronous on the context's stream; -1 while off): PN_DTMF_CLAMP_REPORT_WORDS = 4 little-endian
     32-bit words per stream, [n_streams][4], written for every stream that advances in a frame that launches the kernel; four zero words
     for a stream that is not on:
     word 0  flags: PN_DTMF_CLAMP_ON | MUTED | FADE_OUT | FADE_IN | LATE | EVENT (word 1 holds one) | EVENT_END (word 2 holds one)
     word 1  the ongoing payload      word 2  the ended payload      word 3  rows muted so far
   It is NOT part of pn_host_next_report.

   pn_rate_set_stream_dtmf_clamp(r, ids, n, on) / pn_rate_get_stream_dtmf_clamp(r, h_on[n_streams]): the id list rules of
     pn_rate_set_stream_dtmf; asynchronous on the context's stream and ordered against frames like it, on the pipelined path too.  The
     first enabling allocates the state, the switch words and the detector's report rows; a frame never allocates.  Enabling a stream
     that was off zeroes its removal state; enabling one that is on, or disabling, leaves it.
   pn_rate_set_dtmf_clamp_params(r, params[4]) / pn_rate_get_dtmf_clamp_params: from the next frame submitted on (an argument of every
     launch).  Refused with -1, nothing changed: a value outside its range, pn_last_error naming the FIRST bad index, or a guard that
     is not in time.  Host only: pn_dtmf_clamp_default_params; pn_dtmf_clamp_params_check(params, dtmf_params7) — dtmf_params7 may be
     NULL, otherwise the in-time condition is checked against its PN_DTMF_ON_FRAMES.
   pn_rate_dtmf_clamp_f32(r, d_y48, ids, n_ids): the kernel on its own over [n_streams][480] float rows at a 16-byte aligned device
     address, ids as for pn_rate_up_*, reading the detector's report rows as the last detector launch (or
     pn_rate_debug_set_dtmf_report) left them.
   pn_dtmf_clamp_frame(params, state4, det_report4, row480, report4) -> the report's flags, or -1 for a bad argument: host only, the
     rule above on one row of a stream with removal on; state4 and row480 are read and written, det_report4 NULL means detection off,
     report4 may be NULL.  It does not check the in-time condition: a guard that is too long reports LATE.
   pn_dtmf_event_payload(digit, end, volume, dur, ts_per_frame) -> the payload, 0 for a digit that is none or arguments out of range.
   pn_rate_kernel_time takes "rate_clamp".
   Lifecycle.  pn_rate_reset zeroes the removal state of every stream; pn_rate_reset_streams, pn_rate_set_stream_rates and both import
   forms that of the listed slots, wherever the detector's state goes to zero.  A stream that does not advance keeps its state.
   Switches and parameters are settings that survive all of those.  NO record carries the removal state; the call-state record and its
   10 640 bytes are unchanged.
   Known limit: concealed frames among a digit's first on_frames hits are not counted in dur, so up to that many rows of its head stay.
   What the engine smears past the marked rows (its comb filter reaches 16 ms back) is measured in DESIGN.md section 4.8, not fixed.
   NOT provided: generating tones from received events; a volume measured from the tone; segmenting events longer than 65535 units;
   removal without a converter or without detection; removal or detector state in a record; either report on pn_host_next_report; notch
   filtering instead of muting; comfort noise in the gap. */
#define PN_DTMF_CLAMP_N_PARAMS 4
#define PN_DTMF_CLAMP_PRE 0
#define PN_DTMF_CLAMP_POST 1
#define PN_DTMF_CLAMP_VOLUME 2
#define PN_DTMF_CLAMP_TS_PER_FRAME 3
#define PN_DTMF_CLAMP_REPORT_WORDS 4
#define PN_DTMF_CLAMP_ON 1
#define PN_DTMF_CLAMP_MUTED 2
#define PN_DTMF_CLAMP_FADE_OUT 4
#define PN_DTMF_CLAMP_FADE_IN 8
#define PN_DTMF_CLAMP_LATE 16
#define PN_DTMF_CLAMP_EVENT 32
#define PN_DTMF_CLAMP_EVENT_END 64
int pn_dtmf_clamp_default_params(int32_t *params4);                                  /* host only */
int pn_dtmf_clamp_params_check(const int32_t *params4, const float *dtmf_params7);   /* host only */
int pn_dtmf_clamp_frame(const int32_t *params4, uint32_t *state4, const uint32_t *det_report4, float *row480, uint32_t *report4);   /* host only */
uint32_t pn_dtmf_event_payload(int digit, int end, int volume, uint32_t dur, int ts_per_frame);   /* host only */
int pn_rate_set_stream_dtmf_clamp(pn_rate *r, const int32_t *ids, int n, const uint8_t *on);
int pn_rate_get_stream_dtmf_clamp(const pn_rate *r, uint8_t *h_on);
int pn_rate_set_dtmf_clamp_params(pn_rate *r, const int32_t *params4);
int pn_rate_get_dtmf_clamp_params(const pn_rate *r, int32_t *params4);
int pn_rate_dtmf_clamp_f32(pn_rate *r, float *d_y48, const int32_t *ids, int n_ids);
int pn_rate_set_dtmf_clamp_report(pn_rate *r, int enable);
int pn_rate_read_dtmf_clamp_report(pn_rate *r, void *h_report);
int pn_rate_read_dtmf_clamp_report_dev(pn_rate *r, void *d_report);
int pn_rate_debug_dtmf_clamp_state(pn_rate *r, void *h_state);   /* tests and debugging: [n_streams][4] state words to the host, synchronising; zeros while no stream was ever enabled */
int pn_rate_debug_set_dtmf_report(pn_rate *r, const void *h_report);   /* TESTS ONLY, never in a product: [n_streams][4] words OVERWRITE the detector's report rows — the buffer pn_rate_read_dtmf_report reads too — so that pn_rate_dtmf_clamp_f32 can be run over hand-made rows; synchronising; as a side effect it allocates what removal needs.  The next detector launch overwrites them again */

const char *pn_last_error(void);
const char *pn_version(void);
int pn_device_count(void);                   /* usable HIP devices (0 when there is none) */

/* ---- reference frame-engine interface, extern "C" spelling -------------------------------- */
/* (the C++-mangled rnnoise_* symbols with the reference's exact prototypes are exported too) */
typedef struct DenoiseState DenoiseState;
int rnnoise_get_size_c(void);
int rnnoise_init_c(DenoiseState *st, RNNModel *model);
DenoiseState *rnnoise_create_c(RNNModel *model);
void rnnoise_destroy_c(DenoiseState *st);
float rnnoise_process_frame_c(DenoiseState *st, float *out, const float *in, FILE *f_feature);
int rnnoise_train_c(int argc, char **argv);            /* train(), rnnoise.h:66 */
RNNModel *rnnoise_model_from_file_c(FILE *f);
void rnnoise_model_free_c(RNNModel *model);
/* compute_rnn (rnnoise.h:68, rnn.cpp:42-81), also exported under its C++-mangled name
   _Z11compute_rnnP8RNNStatePfS1_PKf: one network step on a caller-owned RNNState (host arrays); gains[34],
   strengths[34], input[70].  The state is uploaded to a cached batch-of-one context, advanced on the GPU (network mode
   PERCEPNET_STRICT=1|0, device PERCEPNET_DEVICE) and written back, so the caller sees the reference's semantics. */
void rnnoise_compute_rnn_c(RNNState *rnn, float *gains, float *strengths, const float *input);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
