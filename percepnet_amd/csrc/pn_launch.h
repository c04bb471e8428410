// Kernel launchers shared by the host files (pn_context.cpp and the units split from it, pn_network.cpp, pn_featgen.cpp, pn_rate.cpp).  The DSP ones take the
// descriptions of pn_dsp_layout.h (a side, the slots of a frame, its input), the network ones one record of a layer's launch
// (PnLayerLaunch, below) and begin with the rule of their kernel kind (pn_network.h).
#pragma once
#include "pn_common.h"
#include "pn_network.h"       // PnSegs, and through it pn_dsp_layout.h and pn_state_layout.h

// ---- the DSP launchers (pn_dsp_fe*.hip, pn_dsp.hip) ------------------------------------------------------------------------
// A front-end launch takes a side, the frame's slots and the frame's input (pn_dsp_layout.h); a launch that needs no tables or
// no input ignores them, so that all five have one signature.  pn_launch_fe (pn_context.cpp) is launch k of family fe: a context
// and the feature generator both loop over pn_kFe[fe]'s launches.
// grid_cap: test hook of the create-time DSP self-test (pn_selftest.cpp: dsp_selftest).  When > 0 the launcher caps its grid at
// this many blocks, so that a 40-stream batch walks several grid-stride rounds of ONE block (the regime in which a mis-scheduled
// persistent loop once corrupted later rounds).  It is state of the temporary self-test context only
// (pn_ctx::dsp_grid_cap): no other context, thread or device ever sees it.  0 = off.
typedef void PnFeLaunch(hipStream_t st, const PnTables *T, int n_streams, const PnDspSide &s, const PnDspSlots &k, const PnDspIn &in, int grid_cap);
PnFeLaunch pn_launch_frontend;        // four streams per wavefront (pn_dsp_fe.hip)
PnFeLaunch pn_launch_frontend_g2;     // the same kernel with two (pn_dsp_fe_g2.hip): lower latency per stream, lower throughput
PnFeLaunch pn_launch_fe_spec_in, pn_launch_fe_pitch, pn_launch_fe_spec_out;   // the phase kernels, each with its own lane mapping and register / LDS budget
void pn_launch_fe(hipStream_t st, const PnTables *T, int n_streams, int fe, int k, const PnDspSide &s, const PnDspSlots &sl, const PnDspIn &in, int grid_cap);
// per-stream re-initialisation (pn_state.hip): rows ids[] of a [n_slots][rows][row_floats] array / of a fragment-order shadow
void pn_launch_zero_rows(hipStream_t st, void *base, int row_floats, long long row_stride, int n_slots, long long slot_stride,
                         const int *d_ids, int n);
void pn_launch_zero_shadow_rows(hipStream_t st, void *S, int width, int np, int n_slots, long long slot_stride_halfs,
                                const int *d_ids, int n);
// dst[ids[i]] = vals[i] for i < n (distinct ids): the per-stream (lam, mu) pairs of the attenuation limit
void pn_launch_scatter_pairs(hipStream_t st, float2 *dst, const int *d_ids, const float2 *d_vals, int n);
// One section of a context's per-stream state at given counters (pn_context.h state_sections, from pn_state_layout.h): a
// ring or an in-place buffer, its live entries oldest first in slots first, first + 1, ... (mod slots); base + row * row_stride
// + slot * slot_stride = an entry of `cols` floats (all multiples of 4), stored at body word rec_off of a stream-state record.
// shadow: the entry's fragment-order operand shadow of np planes (pn_nn_x3.hip), slot for slot; NULL = none
struct PnSsSection { float *base; uint4 *shadow; long long row_stride, slot_stride; int slots, first, live, cols, rec_off, np; };
// per-call active set (pn_active.hip): the rows ids[0..n) are the streams a call does NOT advance
struct PnActiveArgs {
  const int *ids;                                    // inactive stream ids (device)
  float *synth; int *last_period; float *last_gain;  // in-place state
  void *out; int out_row_words; float *d_gr;         // the caller's output rows (480 int16 = 240 words, or 480 floats); d_gr may be NULL
  float *save_synth; uint32_t *save_out; float *save_gr; int *save_period; float *save_gain;   // save area, row i = ids[i]
  PnSsSection sec[PN_SS_NSEC];                       // the rings at the counters of the tick the fix-up follows
  int restore_only;                                  // the frame FAILED (a refused launch): put the in-place state and the caller's rows of the
                                                     // skipped streams back, shift nothing (the context's counters did not advance)
};
void pn_launch_inactive_save(hipStream_t st, const PnActiveArgs &a, int n);
int pn_launch_spin(hipStream_t st, long long ticks);     // one wave asleep for `ticks` of the 100 MHz wall clock (queue probe)
void pn_launch_inactive_fixup(hipStream_t st, const PnActiveArgs &a, int n);
// per-stream state records (pn_stream_state.hip): the sections at the context's current counters
struct PnStreamStateArgs {
  PnSsSection sec[PN_SS_NSEC];
  float *last_gain; int *last_period;
  const int *ids;                  // row of record i (device)
  void *rec;                       // records [n][PN_STREAM_STATE_BYTES] (device, 16-byte aligned)
  int *status;                     // scatter: verdict per record (device)
  uint32_t hdr[16];                // gather: the header to write; scatter: the header to expect (word 3, nn_mode, unchecked)
};
void pn_launch_ss_gather(hipStream_t st, const PnStreamStateArgs &a, int n);
void pn_launch_ss_scatter(hipStream_t st, const PnStreamStateArgs &a, int n);
// operand shadows of the rows ids[i] whose status[i] == 0 (status may be NULL: every listed row) re-derived from their fp32
// values: the row-list forms of pn_launch_split_x3 / pn_launch_split_d (same fragment indexing)
int pn_launch_split_x3_rows(hipStream_t st, const float *src, int ld, int width, void *S, const int *d_ids, const int *d_status, int n, int np);
int pn_launch_split_d_rows(hipStream_t st, const float *src, int ld, int width, void *S, const int *d_ids, const int *d_status, int n);
// training-feature path (pn_targets.hip)
void pn_launch_targets(hipStream_t st, const PnTables *T, int n_pairs, const float *ex_clean, const float *ex_noisy,
                       const float *ey_look_noisy, const float *aux_clean, const float *aux_noisy,
                       const int *period_noisy, float *records, long long rec_stride, float *gr);
void pn_launch_saturate_i16(hipStream_t st, int n_pairs, const float *in, int16_t *out, long long out_stride);
// the back end takes its operands one by one: the feature generator mixes sides (Xs, Ps, silence of the noisy side; the speech
// state's synthesis memory).  Xs / ex_postfilter: pn_dsp_spec / pn_dsp_bands of a side at the frame's slot_r
void pn_launch_backend(hipStream_t st, const PnTables *T, int n_streams, const float2 *Xs, const float2 *Ps,
                       const float *gr, const float *ex_postfilter /* NULL = off */, const int *silence, float *synth_mem,
                       void *out, int out_is_i16, int grid_cap,
                       const float2 *lam_mu /* [n_streams] (lam, mu) of the attenuation limit; NULL = no stream limited */);
// the output stage (pn_outstage.hip), after the back end while the frame report or the saturating cast is on: o [n_streams][480]
// are the frame's fp32 output samples; pcm (NULL: a float entry point) receives their int16 cast, wrapping like the back end's
// fused one or saturating; report (NULL: off) [n_streams][PN_REPORT_WORDS] the records, whose input figures come from slot
// hist_slot of the side's history ring.  One wavefront per stream, no grid cap.
void pn_launch_outstage(hipStream_t st, int n_streams, const float *o, const PnDspSide &s, int hist_slot, const float *gr,
                        int16_t *pcm, int saturate, void *report);
// the rate converter (pn_rate.hip; factor: a rate's code of pn_rate_design.h, L = 48000 / rate = 6 | 3 | 2, or PN_RATE_F_3_2 for 32000, whose sizes
// pn_rate_factor_frame, pn_rate_down_tail and pn_rate_factor_L give): one wavefront per row, rows d_ids[0..n_rows) or,
// with d_ids == NULL, streams 0..n_rows.  up: in [.][pn_rate_factor_frame(factor)] samples of format fmt -> out48 [.][480], tail [.][32]; down: in48 [.][480] ->
// out [.][pn_rate_factor_frame(factor)] samples of format fmt (int16 and G.711: the wrapping or saturating cast), tail [.][pn_rate_down_tail(factor)]; taps: the
// 2 * 16 * pn_rate_factor_L(factor) + 1 fp32 taps on the device.  fmt: the sample format of the low-rate rows — float, int16, or 8-bit G.711 with the law of
// stream s in d_laws[s] (pn_g711.h; d_laws may be NULL for the other two).  -1 (pn_set_error) without launching for another L or format.
// records: state record i <-> the tails of stream d_ids[i]
enum { PN_FMT_F32 = 0, PN_FMT_I16 = 1, PN_FMT_G711 = 2 };
static inline size_t pn_fmt_bytes(int fmt) { return fmt == PN_FMT_G711 ? 1 : fmt == PN_FMT_I16 ? 2 : 4; }
int pn_launch_rate_up(hipStream_t st, int factor, int fmt, int n_rows, const int *d_ids, const int *d_laws, const void *in, float *out48, float *tail, const float *taps);
int pn_launch_rate_down(hipStream_t st, int factor, int fmt, int n_rows, const int *d_ids, const int *d_laws, const float *in48, void *out, int saturate, float *tail, const float *taps);
// td_stride: words between the down tails of two streams (pn_rate_down_tail(factor) in a single-rate converter, 192 in a mixed one)
void pn_launch_rate_records(hipStream_t st, int factor, int rate_hz, const int *d_ids, int n, float *tail_up, float *tail_down, int td_stride, void *rec, int scatter);
// the mixed converter's kernels: rows of PN_RATE_MIXED_ROW = 480 samples at the low rate too, stream s runs at d_factors[s] in {6, 3, 2, 1, PN_RATE_F_3_2}
// (1: a copy, no tail); tail rows [.][32] and [.][192]; taps: the tables of factor 6, 3, 2 one behind the other (193 + 97 + 65 words), going down the 97 of 32000 behind them.
// set_factors: d_factors[d_ids[i]] = d_vals[i] for i < n (distinct ids); the law table is written by the same launch
int pn_launch_rate_up_mixed(hipStream_t st, int fmt, int n_rows, const int *d_ids, const int *d_factors, const int *d_laws, const void *in, float *out48, float *tail, const float *taps);
int pn_launch_rate_down_mixed(hipStream_t st, int fmt, int n_rows, const int *d_ids, const int *d_factors, const int *d_laws, const float *in48, void *out, int saturate, float *tail, const float *taps);
// device-side records, stride_words apart: each slot's factor from d_factors (mixed) or `factor` (single-rate, d_factors NULL);
// scatter: d_status[i] receives record i's verdict, a refused record moves nothing
void pn_launch_rate_records_dev(hipStream_t st, const int *d_ids, int n, const int *d_factors, int factor, float *tail_up, float *tail_down, int td_stride,
                                void *rec, int stride_words, int *d_status, int scatter);
void pn_launch_rate_set_factors(hipStream_t st, const int *d_ids, const int *d_vals, int n, int *d_factors);
// the conference mix (pn_rate_mix.hip; rules in pn_conf.h): rows d_ids[0..n_rows) or, with d_ids == NULL, streams 0..n_rows of in48
// [.][480] -> out48 [.][480], which must not overlap.  d_conf [n_streams]: the conference of every stream (NULL: nobody is in one,
// every row is copied); d_members [n_streams][32]: the members of conference c in row c, ascending, -1 behind them.  With a list the
// members that advance are those whose d_stamp word equals tick (conf_stamp, launched in front: d_stamp[d_ids[i]] = tick).
// conf_rows: row d_touched[i] of d_members = d_rows[i][0..32), i < k
void pn_launch_rate_mix(hipStream_t st, int n_rows, const int *d_ids, const int *d_conf, const int *d_members, const uint32_t *d_stamp, uint32_t tick,
                        const float *in48, float *out48);
// the same with loudest-N selection, send gains and the mix report (pn_mix_rules.h): d_gains [n_streams], d_caps [n_streams] by
// conference number, d_level [n_streams] read and written, d_report [n_streams][4] words or NULL.  d_conf is not NULL here
void pn_launch_rate_mix_sel(hipStream_t st, int n_rows, const int *d_ids, const int *d_conf, const int *d_members, const uint32_t *d_stamp, uint32_t tick,
                            const float *in48, float *out48, const float *d_gains, const int *d_caps, float *d_level, float hold, void *d_report);
void pn_launch_rate_conf_stamp(hipStream_t st, const int *d_ids, int n, uint32_t *d_stamp, uint32_t tick);
void pn_launch_rate_conf_rows(hipStream_t st, const int *d_touched, const int *d_rows, int k, int *d_members);
// packet-loss concealment (pn_rate_plc.hip; the rule pn_plc_rules.h): rows d_ids[0..n_rows) or, with d_ids == NULL, streams 0..n_rows of
// x48 [.][480], in place.  A stream whose d_lost word equals tick is lost this frame (conf_stamp writes the marks).  State: hist
// [n_streams][1920], q [n_streams][720], meta [n_streams][4] words; d_report [n_streams][4] words or NULL
void pn_launch_rate_plc(hipStream_t st, int n_rows, const int *d_ids, const uint32_t *d_lost, uint32_t tick, float *x48, float *hist, float *q,
                        void *meta, void *d_report);
// comfort noise (pn_rate_cng.hip; the rule pn_cng_rules.h): the rows of the DISTINCT streams d_ids[0..n_rows), never NULL, each of its
// stream's own n_s samples (d_factors [n_streams], or NULL and ns for everybody), into out [n_streams][stride], stride >= n_s.  d_cont
// [n_rows] words: != 0 = the row continues a run.  d_sid [n_streams][16] words: the decoded SIDs (k[12], g, M, 0, 0).  State
// [n_streams][16] words; d_report [n_streams][4] words or NULL.  cng_sids: row i of d_rows [n][16] becomes the SID of stream d_ids[i]
void pn_launch_rate_cng(hipStream_t st, int n_rows, const int *d_ids, const int *d_cont, const int *d_factors, int ns, uint32_t seed, const void *d_sid, void *state,
                        float *out, int stride, void *d_report);
void pn_launch_rate_cng_sids(hipStream_t st, const int *d_ids, const int *d_rows, int n, void *d_sid);
// automatic level control (pn_rate_agc.hip; the rule pn_agc_rules.h): rows d_ids[0..n_rows) or, with d_ids == NULL, streams 0..n_rows of
// y48 [.][480], in place.  d_targets [n_streams]: +0.0 = the stream is not levelled; a stream whose d_lost word equals tick was concealed
// this frame (d_lost == NULL: nobody); params: the converter's PN_AGC_N_PARAMS floats on the HOST, passed by value.  State [n_streams][4]
// words; d_report [n_streams][4] words or NULL
void pn_launch_rate_agc(hipStream_t st, int n_rows, const int *d_ids, const float *d_targets, const uint32_t *d_lost, uint32_t tick, const float *params,
                        float *y48, void *state, void *d_report);
// the output limiter (pn_rate_lim.hip; the rule pn_lim_rules.h): rows d_ids[0..n_rows) or, with d_ids == NULL, streams 0..n_rows of o48
// [.][480], in place.  d_ceilings [n_streams]: +0.0 = the stream is not limited; params: the converter's PN_LIM_N_PARAMS floats on the
// HOST, passed by value.  State [n_streams][4] words; d_report [n_streams][4] words or NULL
void pn_launch_rate_lim(hipStream_t st, int n_rows, const int *d_ids, const float *d_ceilings, const float *params, float *o48, void *state, void *d_report);
// in-band DTMF detection (pn_rate_dtmf.hip; the rule pn_dtmf_rules.h): rows d_ids[0..n_rows) or, with d_ids == NULL, streams 0..n_rows of
// x48 [.][480], which it only reads.  d_on [n_streams] words: 0 = detection is off for the stream; a stream whose d_lost word equals tick
// was concealed this frame (d_lost == NULL: nobody); params, rot16: the converter's PN_DTMF_N_PARAMS floats and the frame rotation on
// the HOST, passed by value; d_tab: ct [8][480] then st [8][480], 16-byte aligned.  State [n_streams][24] words; d_report [n_streams][4]
// words or NULL.  The grid has at most PN_DTMF_MAX_BLOCKS blocks of four rows: beyond 4 * PN_DTMF_MAX_BLOCKS rows a block makes further passes
#define PN_DTMF_MAX_BLOCKS 512
void pn_launch_rate_dtmf(hipStream_t st, int n_rows, const int *d_ids, const int *d_on, const uint32_t *d_lost, uint32_t tick, const float *params, const float *rot16,
                         const float *d_tab, const float *x48, void *state, void *d_report);
// DTMF removal (pn_rate_dtmf_clamp.hip; the rule pn_dtmf_clamp_rules.h): rows d_ids[0..n_rows) or, with d_ids == NULL, streams 0..n_rows
// of y48 [.][480], in place.  d_on [n_streams] words: 0 = removal is off for the stream; params: the converter's PN_DTMF_CLAMP_N_PARAMS
// int32 on the HOST, passed by value; d_det_report [n_streams][4] words: the detector's report rows of this frame, or NULL: detection is
// off for everybody.  State [n_streams][4] words; d_report [n_streams][4] words or NULL
void pn_launch_rate_dtmf_clamp(hipStream_t st, int n_rows, const int *d_ids, const int *d_on, const int32_t *params, const void *d_det_report, float *y48,
                               void *state, void *d_report);
// the DTX send side (pn_rate_dtx.hip; the rule pn_dtx_rules.h): rows d_ids[0..n_rows) or, with d_ids == NULL, streams 0..n_rows of the
// OUTPUT rows [n_streams][stride] samples of format fmt (PN_FMT_*), which it only reads, each of its stream's own n_s samples (d_factors
// [n_streams], or NULL and ns for everybody; stride >= n_s, a multiple of 16).  d_on [n_streams] words: 0 = the stage is off for the
// stream; d_laws [n_streams]: the G.711 laws (read for PN_FMT_G711 only); params: the converter's PN_DTX_N_PARAMS floats on the HOST,
// passed by value.  State [n_streams][24] words; d_report [n_streams][8] words or NULL.  -1 (pn_set_error) without launching for a
// format or geometry it has no kernel for
int pn_launch_rate_dtx(hipStream_t st, int fmt, int n_rows, const int *d_ids, const int *d_on, const int *d_factors, int ns, const int *d_laws, const float *params,
                       const void *rows, int stride, void *state, void *d_report);
// call-state records (pn_rate_call.hip; layout and verdict pn_call_rules.h): record i of rec [n][PN_RATE_CALL_STATE_BYTES] (16-byte aligned)
// <-> the PLC, AGC, limiter and level state of stream d_ids[i].  held: the PN_CALL_* states the converter holds — a state's pointers
// are read only under its bit and may be NULL otherwise.  scatter: d_status[i] receives record i's verdict, a refused record moves nothing
void pn_launch_rate_call_state(hipStream_t st, const int *d_ids, int n, uint32_t held, float *hist, float *q, void *meta, void *agc_state, void *lim_state,
                               float *level, void *rec, int *d_status, int scatter);
// ---- the network launchers (pn_nn*.hip) -----------------------------------------------------------------------------------------
// Device pointers of a layer's biases and weights in the formats of pn_network.h: raw (w, rw), packed fp32 or fp16 planes (wp,
// rwp), the 16x16x4 packing of a narrow layer (wq)
struct DevLayer { float *bias, *w, *rw, *wp, *rwp, *wq; };
// One launch of one layer over n_rows rows, as launch_rnn_rows (pn_network.cpp) assembles it; every launcher takes this record
// and reads the fields its kernel has a use for.
struct PnLayerLaunch {
  PnSegs A, S;                       // input panels: fp32 rows, and their fragment-order operand shadows (uint4* carried as float*; NULL
                                     // where the entry keeps none) for the kinds that read those (pn_kernel_reads_shadows)
  const float *bias;
  const void *w, *rw;                // input / recurrent weights in the format of the kind (pn_kernel_weight_format)
  int N, act; const float *tansig;   // neurons, activation, the activation table
  float *out; int ldo;               // output rows (a GRU: the new state, ldo = N)
  void *outS; int nts_out;           // shadow of the output, a buffer nts_out column tiles wide; NULL: the kind writes none
  const float *h_old; const void *h_oldS;   // GRU: the state it reads and that state's shadow; NULL for dense layers
  int n_rows, rg, np;                // rg: row groups of 32 per wave (pn_plan.h; 3 = 2 with the GRUs on the paired-phase kernel); np: weight planes
};
// A launcher begins with the rule of its kind (pn_kernel_geometry_ok, pn_network.h) and returns 0, or -1 (pn_set_error) WITHOUT
// launching when it refuses the geometry: the caller fails the frame (launch_rnn -> pn_process_*), it must never report a frame
// whose layer outputs are stale.  One launcher per (kind, dense | GRU); pn_launch_dense also serves batch_sh: handed outS it runs
// the kernel that writes it.  The table kind -> launchers is pn_network.cpp's.
typedef int PnLayerLauncher(hipStream_t, const PnLayerLaunch &);
PnLayerLauncher pn_launch_dense_strict, pn_launch_gru_strict, pn_launch_dense, pn_launch_gru;         // pn_nn.hip
PnLayerLauncher pn_launch_dense_small, pn_launch_gru_small, pn_launch_dense_n16, pn_launch_dense_n48; // pn_nn_small.hip, pn_nn_n48.hip
PnLayerLauncher pn_launch_dense_x3, pn_launch_gru_x3, pn_launch_gru_d;   // pn_nn_x3.hip, pn_nn_d.hip (bit-identical to pn_launch_gru)
// split-precision packing (pn_nn_x3.hip): fp16 hi / lo planes in fragment order
size_t pn_packed_halfs_x3(int k_alloc, int ncols, int ct_round, int np /* planes: 2 = hi+lo (split precision), 1 = fp16 operands */);
int pn_pack_weights_x3(const float *W, int K, int k_alloc, int ncols, int ct_round, int np, void *Wp);   // -1: weight outside fp16 range
int pn_x3_sat_set(int enable);          // debug counter of operand values clamped to +-65504 (current device): reset + switch
long long pn_x3_sat_read();             // ... and its value, or -1
// operand shadows re-derived from fp32 rows: fp16 planes (pn_nn_x3.hip), fp32 fragments of the direct-operand family (pn_nn_d.hip)
int pn_launch_split_x3(hipStream_t st, const float *src, int ld, int width, void *S, int n_rows_padded, int np);
int pn_launch_split_d(hipStream_t st, const float *src, int ld, int width, void *S, int n_rows);
