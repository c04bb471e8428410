// Host side of the batched rate converter (include/percepnet_hip.h "batched rate converter" and "mixed rates"): an object BESIDE a context, built
// like the feature generator — it borrows the context's device, batch size and HIP stream, and owns everything else: the two
// tap tables on the device, the per-stream state (the tails of the two kernels of pn_rate.hip and the state of every stage behind them), the 48 kHz rows between the conversions and
// the staging rows of the host-buffer paths.  The pipelined path (pn_rate_submit_host_*) runs its frames through the CONTEXT's
// pipeline (pn_host_pipe.cpp pipe_submit) with the converter's own two staging pairs.  Nothing of it lives in pn_ctx, its state table or its records.  Every launch goes
// to the context's stream, so a converter call is ordered against the context's calls like they are against each other.
//
// What is stated once, and where: the per-stream STATE — its buffers, their widths, the events that clear them, their sections of the
// call-state record — is the table of pn_rate_layout.h, held as pn_rate::st[] and walked by state_clear_all / state_clear_rows /
// state_alloc below; a new stage's state is one entry there.  A STAGE — its timed family, its report — is a row of kRateStage, served by
// rate_set_report / rate_report_copy.  A per-stream SETTING goes through rate_set_words and comes back through rate_get.
#include "pn_context.h"      // the context it borrows, the launchers, dev_alloc_into, stage_ids, the id rule, host_records_sync
#include "pn_rate_layout.h"  // the per-stream state, and through it every stage's rules: pn_rate_design.h, pn_call_rules.h (pn_plc_rules.h,
                             // pn_agc_rules.h, pn_lim_rules.h, pn_mix_rules.h), pn_dtmf_rules.h, pn_dtmf_clamp_rules.h, pn_cng_rules.h, pn_dtx_rules.h
#include "pn_rate_mixed.h"   // the mixed converter's host rules: the five rates, a rate change, one rate per record call
#include "pn_g711.h"         // the 8-bit sample format: the companding and what a list of laws must be
#include "pn_conf.h"         // conferences: what an id must be, the table after a change, the members in ascending order
#include <string>
#include <vector>

// the stages: the timed kernels (pn_rate_kernel_time) and their reports
enum { RF_UP, RF_DOWN, RF_MIX, RF_PLC, RF_AGC, RF_LIM, RF_DTMF, RF_CLAMP, RF_CNG, RF_DTX, RF_COUNT };
struct RateStage { const char *family; int report_words; const char *report_off; };   // report_words per stream, 0: the stage has no report
static const RateStage kRateStage[RF_COUNT] = {
    {"rate_up", 0, NULL},
    {"rate_down", 0, NULL},
    {"rate_mix", PN_MIX_REPORT_WORDS, "the mix report is off (pn_rate_set_mix_report)"},
    {"rate_plc", PN_PLC_REPORT_WORDS, "the PLC report is off (pn_rate_set_plc_report)"},
    {"rate_agc", PN_AGC_REPORT_WORDS, "the AGC report is off (pn_rate_set_agc_report)"},
    {"rate_lim", PN_LIM_REPORT_WORDS, "the limiter report is off (pn_rate_set_limiter_report)"},
    {"rate_dtmf", PN_DTMF_REPORT_WORDS, "the DTMF report is off (pn_rate_set_dtmf_report)"},
    {"rate_clamp", PN_DTMF_CLAMP_REPORT_WORDS, "the DTMF removal report is off (pn_rate_set_dtmf_clamp_report)"},
    {"rate_cng", PN_CNG_REPORT_WORDS, "the comfort-noise report is off (pn_rate_set_cng_report)"},
    {"rate_dtx", PN_DTX_REPORT_WORDS, "the DTX report is off (pn_rate_set_dtx_report)"},
};
enum { RATE_PIECE = 16384 };    // ids a setting stages through the id ring at a time

struct pn_rate {
  pn_ctx *c;                    // borrowed: device, B, stream, the id ring, the saturate setting
  int rate, f, n, td;           // rate_hz, its factor (pn_rate_design.h: L, or PN_RATE_F_3_2 for 32000), samples per row, words per down tail row (2D / M).  Mixed: 0, 0, 480, 192
  size_t bytes;
  float *taps_up, *taps_down;   // [2D + 1] h, g.  Mixed: the tables of L = 6, 3, 2 one behind the other, and behind them the g of 32000
  void *st[PN_RS_COUNT] = {};   // the per-stream state, [B][pn_rate_state_words] each (pn_rate_layout.h): NULL until the owning stage is first used
  void *st2[PN_RS2_COUNT] = {}; // ... and that of the second table: the stages at the edges, at the streams' own rates
  void *d_report[RF_COUNT] = {};   // [B][kRateStage[].report_words] words: allocated by the first enabling of the report
  bool report[RF_COUNT] = {};      // the report switches
  float *x48, *y48;             // [B][480]: the engine's input and output rows of a whole frame
  void *io_in, *io_out;         // [B][n] 4-byte words: staging rows of the host-buffer paths (slot 0 of the pipelined one)
  void *io_in1 = NULL, *io_out1 = NULL;   // slot 1 of the pipelined path: allocated by pn_rate_host_pipeline_prepare or the first submit
  float *io_gr;                 // [B][68]
  // the rate of every stream as last set (host; a single-rate converter: its rate everywhere).  A mixed converter
  // (pn_rate_create_mixed) has its factor on the device — written in stream order, so a frame submitted before a rate change still
  // runs at the old rate — and a pinned landing place of the host-buffer path's output rows, of which only the streams' own samples
  // go on to the caller
  bool mixed;
  std::vector<int32_t> rates;   // [B]
  int *factors;                 // [B] device
  void *h_rows;                 // [B][480] 4-byte words, pinned
  // G.711 rows (pn_rate_*_g711): the law of every stream as last set (host) and on the device, written in stream order like the
  // factors.  A setting, not state: every reset, rate change and record call leaves it alone.  Default: mu-law everywhere
  std::vector<int32_t> laws;    // [B]
  int *d_laws = NULL;           // [B] device
  // conferences (pn_rate_set_stream_confs): the conference of every stream as last set (host) and on the device, the member
  // rows and the second 48 kHz row set the mix writes and the down-conversion then reads.  A setting like the law; the device
  // side exists from the first call that puts a stream into a conference.  in_conf == 0: a frame launches nothing of it
  std::vector<int32_t> confs;   // [B]
  int in_conf = 0;              // streams in a conference
  float *o48 = NULL;            // [B][480]
  int *d_conf = NULL, *d_members = NULL;   // [B], [B][32]
  uint32_t *d_stamp = NULL, tick = 0;      // [B]: == tick where the stream is on this frame's id list
  // loudest-N selection, send gains, hold and the mix report (pn_mix_rules.h): SETTINGS as last set (host) and on the device, and the
  // one new state, a level per stream (st[PN_RS_LEVEL]).  While every setting is at its default (mix_plain) rate_mix launches the plain kernel and
  // none of the device side is read; it is allocated by the first setting call that leaves the defaults, never inside a frame
  std::vector<float> gains;     // [B], 1.0f
  std::vector<int32_t> caps;    // [B] N_c by conference number, 0: everybody
  int gains_off = 0, caps_on = 0;          // how many gains are not 1.0f, how many caps not 0
  float hold = 0.0f;            // d
  float *d_gains = NULL;        // [B]
  int *d_caps = NULL;           // [B]
  // packet-loss concealment (pn_rate_set_plc; the rule pn_plc_rules.h): the state — history ring, period buffer and four meta words per
  // stream — exists from the first enable on, never allocated inside a frame.  Marks (pn_rate_set_lost): a stamp word per stream on
  // the device, == plc_tick where the stream is lost in the NEXT frame, written in stream order through the id ring; the host keeps
  // the same marks, which is how a frame knows whom to leave out of the up-conversion.  A frame consumes them: plc_tick moves on
  bool plc = false;
  uint32_t *d_plc_lost = NULL, plc_tick = 1;          // [B]
  std::vector<uint8_t> lost_mark;                     // [B]
  std::vector<int32_t> lost_ids, up_ids;              // the marked streams; a frame's "advancing minus lost"
  // automatic level control (pn_rate_set_agc; the rule pn_agc_rules.h): SETTINGS — the switch, the converter's parameters, a target per
  // stream as last set (host) and on the device, written in stream order through the id ring like the send gains — and the state, four
  // words per stream.  The device side exists from the first enable on.  agc_on == 0: a frame launches nothing of it
  bool agc = false;
  float agc_params[PN_AGC_N_PARAMS];
  std::vector<float> agc_targets;                     // [B], 0
  int agc_on = 0;                                     // streams whose target is not 0
  float *d_agc_targets = NULL;                        // [B]
  // the output limiter (pn_rate_set_stream_limiter; the rule pn_lim_rules.h): SETTINGS — the converter's parameters, a ceiling per stream
  // as last set (host) and on the device, written in stream order through the id ring like the AGC targets — and the
  // state, four words per stream.  The device side exists from the first call that sets a ceiling on.  lim_on == 0: a frame launches nothing of it
  float lim_params[PN_LIM_N_PARAMS];
  std::vector<float> lim_ceilings;                    // [B], 0
  int lim_on = 0;                                     // streams whose ceiling is not 0
  float *d_lim_ceilings = NULL;                       // [B]
  // DTMF detection (pn_rate_set_stream_dtmf; the rule pn_dtmf_rules.h): SETTINGS — the converter's parameters, a switch per stream as last
  // set (host) and as a word on the device, written in stream order through the id ring like the ceilings — and the state, 24 words per
  // stream.  The device side (with the twiddle tables) exists from the first enabling on.  dtmf_on == 0: a frame launches nothing of it
  float dtmf_params[PN_DTMF_N_PARAMS];
  std::vector<uint8_t> dtmf_sw;                       // [B], 0
  int dtmf_on = 0;                                    // streams whose switch is on
  int *d_dtmf_on = NULL;                              // [B] words
  float *d_dtmf_tab = NULL;                           // ct [8][480], st [8][480]
  // DTMF removal (pn_rate_set_stream_dtmf_clamp; the rule pn_dtmf_clamp_rules.h): SETTINGS — the converter's parameters, a switch per stream as
  // last set (host) and as a word on the device, written in stream order through the id ring like the detector's — and the state, four words
  // per stream.  The device side exists from the first enabling on, and with it d_report[RF_DTMF]: while clamp_on > 0 the detector writes its
  // report rows whether or not the user reads them (report[RF_DTMF]).  clamp_on == 0: a frame launches nothing of it
  int32_t clamp_params[PN_DTMF_CLAMP_N_PARAMS];
  std::vector<uint8_t> clamp_sw;                      // [B], 0
  int clamp_on = 0;                                   // streams whose switch is on
  int *d_clamp_on = NULL;                             // [B] words
  // comfort noise (pn_rate_set_cng; the rule pn_cng_rules.h): SETTINGS — the switch, the seed (an argument of every launch), a SID per
  // stream as last set (host, PN_CNG_SID_BYTES each, from creation on) and decoded on the device, written in stream order through the id
  // ring — the state, 16 words per stream (st2[PN_RS2_CNG]), and the rows the kernel writes at the streams' own rates, strided like an
  // input row.  The device side exists from the first enable on.  Marks (pn_rate_set_silent) live on the HOST alone: a frame compacts
  // them into the list the kernel runs over, and consumes them.  cng_last: the tick of the frame that last generated a stream's row, 0:
  // none — a row CONTINUES a run when that is the tick before this frame's.  Nobody marked: a frame launches nothing of it
  bool cng = false;
  uint32_t cng_seed = PN_CNG_DEFAULT_SEED, cng_tick = 1;
  std::vector<uint8_t> sids;                          // [B][PN_CNG_SID_BYTES]
  uint32_t *d_cng_sid = NULL;                         // [B][PN_CNG_PARAM_WORDS]
  float *cng_rows = NULL;                             // [B][n]
  std::vector<uint8_t> silent_mark;                   // [B]
  std::vector<int32_t> silent_ids, gen_ids, gen_cont; // the marked streams; a frame's generated streams and their "continues" words
  std::vector<uint32_t> cng_last;                     // [B]
  // the DTX send side (pn_rate_set_stream_dtx; the rule pn_dtx_rules.h): SETTINGS — the converter's parameters, a switch per stream as last
  // set (host) and as a word on the device, written in stream order through the id ring like the detector's — and the state, 24 words per
  // stream (st2[PN_RS2_DTX]).  The device side exists from the first enabling on.  dtx_on == 0: a frame launches nothing of it
  float dtx_params[PN_DTX_N_PARAMS];
  std::vector<uint8_t> dtx_sw;                        // [B], 0
  int dtx_on = 0;                                     // streams whose switch is on
  int *d_dtx_on = NULL;                               // [B] words
  std::vector<void *> allocs;
  // timing of the kernels (pn_rate_set_profiling): HIP events around their launches, like the context's families but owned
  // here; while it is off no event exists and none is recorded
  bool profiling = false;
  struct Ev { int fam; hipEvent_t a, b; };
  std::vector<Ev> events;
  std::vector<hipEvent_t> event_pool;
  double fam_ms[RF_COUNT] = {}; int64_t fam_n[RF_COUNT] = {};
};
struct RateScope {
  pn_rate *r; int fam; hipEvent_t a, b; bool on;
  RateScope(pn_rate *r_, int fam_) : r(r_), fam(fam_), on(r_->profiling) {
    if (on) {
      auto take = [&](hipEvent_t &e) { if (r->event_pool.empty()) hipEventCreate(&e); else { e = r->event_pool.back(); r->event_pool.pop_back(); } };
      take(a); take(b); hipEventRecord(a, r->c->stream);
    }
  }
  ~RateScope() { if (on) { hipEventRecord(b, r->c->stream); r->events.push_back({fam, a, b}); } }
};
static int rate_flush_events(pn_rate *r) {
  PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  for (auto &e : r->events) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { r->fam_ms[e.fam] += ms; r->fam_n[e.fam]++; }
    r->event_pool.push_back(e.a); r->event_pool.push_back(e.b);
  }
  r->events.clear();
  return 0;
}

// ---- host only ---------------------------------------------------------------------------------------------------------------
static int rate_factor_or_error(int rate_hz) {       // the factor of a single-rate converter's rate, or 0 with the error set
  const int f = pn_rate_factor(rate_hz);
  if (!f) pn_set_error("rate %d Hz: a converter takes " PN_RATE_TEXT, rate_hz);
  return f;
}
extern "C" int pn_rate_frame_samples(int rate_hz) { const int f = rate_factor_or_error(rate_hz); return f ? pn_rate_factor_frame(f) : -1; }
// the engine's 2880 samples at the low rate, T up and T down
extern "C" int pn_rate_delay_samples(int rate_hz) { const int f = rate_factor_or_error(rate_hz); return f ? pn_rate_factor_delay(f) : -1; }
extern "C" int pn_rate_taps(int rate_hz, int down, float *taps, int cap) { const int f = rate_factor_or_error(rate_hz); return f ? pn_rate_design(f, down, taps, cap) : -1; }
extern "C" size_t pn_rate_state_bytes(int rate_hz) { const int f = rate_factor_or_error(rate_hz); return f ? 4 * pn_rate_record_words(f) : 0; }
extern "C" int pn_rate_state_check(const void *record, size_t bytes, int rate_hz) { return pn_rate_record_check(record, bytes, rate_hz); }
extern "C" int pn_rate_mixed_frame_samples(int rate_hz) { return pn_rate_mixed_frame(rate_hz); }
extern "C" int pn_rate_mixed_delay_samples(int rate_hz) { return pn_rate_mixed_delay(rate_hz); }
extern "C" int pn_rate_mixed_rates_check(const int32_t *rates_hz, int n) { return pn_rate_mixed_rates_list_check(rates_hz, n); }
extern "C" int pn_g711_decode(int law, const uint8_t *in, int16_t *out, size_t n) { return pn_g711_decode_host(law, in, out, n); }
extern "C" int pn_g711_encode(int law, const int16_t *in, uint8_t *out, size_t n) { return pn_g711_encode_host(law, in, out, n); }
extern "C" int pn_rate_laws_check(const int32_t *laws, int n) { return pn_g711_laws_list_check(laws, n); }
extern "C" int pn_rate_confs_check(const int32_t *confs, int n, int n_streams) { return pn_conf_list_check(confs, n, n_streams); }
extern "C" int pn_rate_mix_gains_check(const float *gains, int n) { return pn_mix_gains_list_check(gains, n); }
extern "C" float pn_mix_level(const float *row480) { if (!row480) { pn_set_error("NULL argument"); return NAN; } return pn_mix_level_host(row480); }
extern "C" int pn_mix_select(const float *levels, int k, int n_max, uint8_t *selected) { return pn_mix_select_host(levels, k, n_max, selected); }
extern "C" int pn_plc_pitch(const float *hist1920) { if (!hist1920) { pn_set_error("NULL argument"); return -1; } return pn_plc_pitch_host(hist1920); }
extern "C" int pn_plc_period(const float *hist1920, int P, float *q) { return pn_plc_period_host(hist1920, P, q); }
extern "C" float pn_plc_gain(int64_t m) { return pn_plc_gain_host(m); }
extern "C" int pn_agc_default_params(float *params8) { if (!params8) { pn_set_error("NULL argument"); return -1; } pn_agc_default_params_host(params8); return 0; }
extern "C" int pn_agc_params_check(const float *params8) { return pn_agc_params_check_host(params8); }
extern "C" int pn_agc_frame(const float *params8, float target, uint32_t *state4, const float *row_in480, float *row_out480, int concealed) {
  return pn_agc_frame_host(params8, target, state4, row_in480, row_out480, concealed);
}
extern "C" int pn_rate_agc_targets_check(const float *targets, int n) { return pn_agc_targets_list_check(targets, n); }
extern "C" int pn_lim_default_params(float *params2) { if (!params2) { pn_set_error("NULL argument"); return -1; } pn_lim_default_params_host(params2); return 0; }
extern "C" int pn_lim_params_check(const float *params2) { return pn_lim_params_check_host(params2); }
extern "C" int pn_lim_frame(const float *params2, float ceiling, uint32_t *state4, const float *row_in480, float *row_out480, uint32_t *report4) {
  return pn_lim_frame_host(params2, ceiling, state4, row_in480, row_out480, report4);
}
extern "C" int pn_dtmf_default_params(float *params7) { if (!params7) { pn_set_error("NULL argument"); return -1; } pn_dtmf_default_params_host(params7); return 0; }
extern "C" int pn_dtmf_params_check(const float *params7) { return pn_dtmf_params_check_host(params7); }
extern "C" int pn_dtmf_frame(const float *params7, uint32_t *state24, const float *row480, int concealed, uint32_t *report4) {
  return pn_dtmf_frame_host(params7, state24, row480, concealed, report4);
}
extern "C" int pn_dtmf_tables(float *ct, float *st, float *rot16) { return pn_dtmf_tables_host(ct, st, rot16); }
extern "C" int pn_dtmf_clamp_default_params(int32_t *params4) { if (!params4) { pn_set_error("NULL argument"); return -1; } pn_dtmf_clamp_default_params_host(params4); return 0; }
extern "C" int pn_dtmf_clamp_params_check(const int32_t *params4, const float *dtmf_params7) {
  if (dtmf_params7 && pn_dtmf_params_check_host(dtmf_params7)) return -1;
  return pn_dtmf_clamp_params_check_host(params4, dtmf_params7 ? (int)dtmf_params7[PN_DTMF_ON_FRAMES] : 0);
}
extern "C" int pn_dtmf_clamp_frame(const int32_t *params4, uint32_t *state4, const uint32_t *det_report4, float *row480, uint32_t *report4) {
  return pn_dtmf_clamp_frame_host(params4, state4, det_report4, row480, report4);
}
extern "C" uint32_t pn_dtmf_event_payload(int digit, int end, int volume, uint32_t dur, int ts_per_frame) {
  if (digit < 0 || volume < 0 || volume > 63 || ts_per_frame < 1 || ts_per_frame > 65535) return 0u;
  return pn_dtmf_event_payload_hd((uint32_t)digit, end != 0, (uint32_t)volume, dur, (uint32_t)ts_per_frame);
}
extern "C" int pn_rate_limiter_ceilings_check(const float *ceilings, int n) { return pn_lim_ceilings_list_check(ceilings, n); }
extern "C" int pn_cng_sid_decode(const uint8_t *sid14, float *g, float *k12, int32_t *M) {
  PnCngSid d;
  if (!g || !k12 || !M) { pn_set_error("NULL argument"); return -1; }
  if (pn_cng_sid_decode_host(sid14, &d)) return -1;
  *g = d.g; *M = d.M; memcpy(k12, d.k, sizeof d.k);
  return 0;
}
extern "C" float pn_cng_level(int L) { if (L < 0 || L > 127) { pn_set_error("SID level %d: a level in [0, 127] -dBov", L); return NAN; } return pn_kCngLevel[L]; }
extern "C" int pn_dtx_default_params(float *params9) { if (!params9) { pn_set_error("NULL argument"); return -1; } pn_dtx_default_params_host(params9); return 0; }
extern "C" int pn_dtx_params_check(const float *params9) { return pn_dtx_params_check_host(params9); }
extern "C" int pn_dtx_frame(const float *params9, uint32_t *state24, const float *row, int n, uint32_t *report8) { return pn_dtx_frame_host(params9, state24, row, n, report8); }
extern "C" int pn_dtx_sid_from_acorr(const float *R13, int order, uint8_t *sid14) { return pn_dtx_sid_from_acorr_host(R13, order, sid14); }
extern "C" int pn_dtx_level(float mean_square) { return pn_dtx_level_hd(mean_square); }
extern "C" int pn_cng_frame(const uint8_t *sid14, uint32_t *state16, uint32_t seed, int slot, int cont, int n, float *row, uint32_t *report4) {
  PnCngSid d;
  if (slot < 0) { pn_set_error("stream slot %d", slot); return -1; }
  if (pn_cng_sid_decode_host(sid14, &d)) return -1;
  return pn_cng_frame_host(&d, state16, pn_cng_key(seed, (uint32_t)slot), cont, n, row, report4);
}

// ---- the shared routines: allocation, the state table's walks, reports, per-stream settings ----------------------------------------
// (callers are on the context's device.)  Device memory of the converter; p is written on success only, which is what lets a stage
// allocate into locals and store its pointers in pn_rate once ALL of them are there: a failed enable leaves the stage "never enabled"
template <class T>
static int rate_alloc(pn_rate *r, T *&p, size_t bytes, bool zero) {
  void *v = NULL;
  if (dev_alloc_into(r->allocs, r->bytes, r->c->stream, &v, bytes, zero)) return -1;
  p = static_cast<T *>(v);
  return 0;
}
static float *stf(const pn_rate *r, int e) { return static_cast<float *>(r->st[e]); }
static size_t state_bytes(const pn_rate *r, int e) { return (size_t)r->c->B * pn_rate_state_words(e, r->td) * 4; }
// the state buffers of `stage`, zeroed, into p[] — r->st itself, or a stage's locals that state_commit stores behind its other allocations
static int state_alloc(pn_rate *r, int stage, void *p[PN_RS_COUNT]) {
  for (int e = 0; e < PN_RS_COUNT; e++)
    if (pn_kRateState[e].stage == stage && rate_alloc(r, p[e], state_bytes(r, e), true)) return -1;
  return 0;
}
static void state_commit(pn_rate *r, int stage, void *const p[PN_RS_COUNT]) {
  for (int e = 0; e < PN_RS_COUNT; e++) if (pn_kRateState[e].stage == stage) r->st[e] = p[e];
}
// the host's side of a cleared comfort-noise state: the streams (ids == NULL: all) have generated no row, so their next one starts a run
static void cng_forget(pn_rate *r, const int32_t *ids, int n) {
  if (r->cng_last.empty()) return;
  if (!ids) std::fill(r->cng_last.begin(), r->cng_last.end(), 0u);
  else for (int i = 0; i < n; i++) r->cng_last[ids[i]] = 0u;
}
// The two zeroing rules.  What `event` (of `stage`, where it is a stage's event) clears goes to zero for every stream ...
static int state_clear_all(pn_rate *r, unsigned event, int stage = -1) {
  for (int e = 0; e < PN_RS_COUNT; e++)
    if (pn_rate_state_cleared(e, event, stage) && r->st[e]) PN_HIP_CHECK(hipMemsetAsync(r->st[e], 0, state_bytes(r, e), r->c->stream));
  for (int e = 0; e < PN_RS2_COUNT; e++)
    if (pn_rate_state2_cleared(e, event, stage) && r->st2[e]) PN_HIP_CHECK(hipMemsetAsync(r->st2[e], 0, (size_t)r->c->B * pn_kRateState2[e].words * 4, r->c->stream));
  if (pn_rate_state2_cleared(PN_RS2_CNG, event, stage)) cng_forget(r, NULL, 0);
  return 0;
}
// ... or for the staged streams d[0..n) (nothing where the buffer does not exist: pn_launch_zero_rows)
static void state_clear_rows(pn_rate *r, unsigned event, const int *d, int n, int stage = -1) {
  for (int e = 0; e < PN_RS_COUNT; e++) {
    const int w = pn_rate_state_words(e, r->td);
    if (pn_rate_state_cleared(e, event, stage)) pn_launch_zero_rows(r->c->stream, r->st[e], w, w, 1, 0, d, n);
  }
  for (int e = 0; e < PN_RS2_COUNT; e++) {
    const int w = pn_kRateState2[e].words;
    if (pn_rate_state2_cleared(e, event, stage)) pn_launch_zero_rows(r->c->stream, r->st2[e], w, w, 1, 0, d, n);
  }
}
// a stage switched on for streams that were off: they start from the fresh state.  Staged in pieces, in front of the switch write
static int state_switch_on(pn_rate *r, int stage, const std::vector<int32_t> &fresh) {
  for (size_t at = 0; at < fresh.size(); at += RATE_PIECE) {
    const int m = (int)(fresh.size() - at < RATE_PIECE ? fresh.size() - at : RATE_PIECE);
    const int *d = stage_ids(r->c, fresh.data() + at, m);
    if (!d) return -1;
    state_clear_rows(r, PN_RE_SWITCH_ON, d, m, stage);
  }
  return 0;
}
// the state of entry e of every stream to the host, synchronising (tests and debugging); zeros while the buffer does not exist
static int state_debug_copy(pn_rate *r, int e, void *h_state) {
  if (!r || !h_state) { pn_set_error("NULL argument"); return -1; }
  if (!r->st[e]) { memset(h_state, 0, state_bytes(r, e)); return 0; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(h_state, r->st[e], state_bytes(r, e), hipMemcpyDeviceToHost, r->c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}

// a stage's report: the switch — the rows are allocated by the first enabling — what a launch is handed, and the two reads
static int mix_buffers(pn_rate *r);
static size_t report_bytes(const pn_rate *r, int fam) { return (size_t)r->c->B * kRateStage[fam].report_words * 4; }
static int rate_set_report(pn_rate *r, int fam, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (enable && !r->d_report[fam]) {
    PN_ON_DEVICE(r->c);
    if (fam == RF_MIX && mix_buffers(r)) return -1;  // (the mix report is written by the selecting kernel, which reads the settings' device side)
    if (rate_alloc(r, r->d_report[fam], report_bytes(r, fam), true)) return -1;
  }
  r->report[fam] = enable != 0;
  return 0;
}
static void *rate_report(const pn_rate *r, int fam) { return r->report[fam] ? r->d_report[fam] : NULL; }
static int rate_report_copy(pn_rate *r, int fam, void *dst, hipMemcpyKind kind) {
  if (!r || !dst) { pn_set_error("NULL argument"); return -1; }
  if (!r->report[fam]) { pn_set_error("%s", kRateStage[fam].report_off); return -1; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(dst, r->d_report[fam], report_bytes(r, fam), kind, r->c->stream));
  if (kind == hipMemcpyDeviceToHost) PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}

// A per-stream word setting (the caller has checked the list): dst[ids[i]] = v[i] in stream order through the context's id ring, so a frame
// submitted before the call runs under the old values.  Nothing while the stage's device side does not exist and no value leaves
// `neutral` ("nothing has ever left the defaults, and nothing does"); otherwise `buffers` allocates it on first use — here, never inside
// a frame — `before` runs the stage's own launches that must precede the write, the words go through the ring in bounded pieces, each
// followed by the launch that reads it, and the host's copy follows with `on`, its count of values that are not neutral.
template <class T, class D, class H, class Before>
static int rate_set_words(pn_rate *r, const int32_t *ids, int n, const T *v, T neutral, D *&dst, int (*buffers)(pn_rate *), std::vector<H> &host, int &on, Before before) {
  static_assert(sizeof(T) == 4 && sizeof(D) == 4, "a word");
  bool all_neutral = true;
  for (int i = 0; i < n; i++) all_neutral &= v[i] == neutral;
  if (n == 0 || (!dst && all_neutral)) return 0;
  PN_ON_DEVICE(r->c);
  if ((buffers && buffers(r)) || before()) return -1;
  for (int at = 0; at < n; at += RATE_PIECE) {
    const int m = n - at < RATE_PIECE ? n - at : RATE_PIECE;
    const int *d = stage_ids(r->c, ids + at, m, v + at, m);
    if (!d) return -1;
    pn_launch_rate_set_factors(r->c->stream, d, d + ((m + 3) & ~3), m, reinterpret_cast<int *>(dst));
  }
  PN_HIP_CHECK(hipGetLastError());
  for (int i = 0; i < n; i++) { on += (v[i] != neutral) - (host[ids[i]] != (H)neutral); host[ids[i]] = (H)v[i]; }
  return 0;
}
template <class T, class D, class H>
static int rate_set_words(pn_rate *r, const int32_t *ids, int n, const T *v, T neutral, D *&dst, int (*buffers)(pn_rate *), std::vector<H> &host, int &on) {
  return rate_set_words(r, ids, n, v, neutral, dst, buffers, host, on, [] { return 0; });
}
static std::vector<float> plus_zero(const float *v, int n) {   // (-0.0f is 0)
  std::vector<float> o(v, v + n);
  for (float &x : o) if (x == 0.0f) x = 0.0f;
  return o;
}
// a whole table of settings to the caller
template <class H, class O>
static int rate_get(const pn_rate *r, std::vector<H> pn_rate::*host, O *out) {
  if (!r || !out) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) out[s] = (r->*host)[s];
  return 0;
}

// a stage's parameters to the caller
template <class T, size_t N>
static int rate_get_params(const pn_rate *r, T (pn_rate::*params)[N], T *out) {
  if (!r || !out) { pn_set_error("NULL argument"); return -1; }
  memcpy(out, r->*params, sizeof(T) * N);
  return 0;
}

// ---- lifecycle ---------------------------------------------------------------------------------------------------------------
extern "C" void pn_rate_destroy(pn_rate *r) {
  if (!r) return;
  DeviceGuard _dg(r->c->device);
  (void)pipe_drain(r->c);                            // frames in flight on the pipelined path read and write the staging rows
  hipStreamSynchronize(r->c->stream);
  for (auto &e : r->events) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
  for (hipEvent_t e : r->event_pool) hipEventDestroy(e);
  for (void *p : r->allocs) hipFree(p);
  if (r->h_rows) hipHostFree(r->h_rows);
  delete r;
}

// f: the factor of rate_hz, or 0 for a converter with a rate per stream (rates_hz, NULL: 48000 everywhere): the tap tables of all four
// filters, tails of the largest size for every stream (a rate change never reallocates), rows of 480 samples, zeroed so that the part
// of a row no kernel writes is never stale memory.  The caller has checked the rates.
static pn_rate *rate_create(pn_ctx *c, int rate_hz, int f, const int32_t *rates_hz) {
  DeviceGuard _dg(c->device);
  if (!_dg.ok) { pn_set_error("hipSetDevice(%d) failed", c->device); return NULL; }
  const bool mixed = f == 0;
  const size_t B = (size_t)c->B;
  pn_rate *r = new pn_rate();
  r->c = c; r->rate = rate_hz; r->f = f; r->mixed = mixed; r->bytes = 0; r->factors = NULL; r->h_rows = NULL;
  r->n = mixed ? PN_RATE_MIXED_ROW : pn_rate_factor_frame(f); r->td = pn_rate_down_tail(mixed ? PN_RATE_MAX_L : f);
  if (rates_hz) r->rates.assign(rates_hz, rates_hz + B); else r->rates.assign(B, mixed ? 48000 : rate_hz);
  r->laws.assign(B, PN_G711_ULAW); r->confs.assign(B, PN_CONF_NONE);
  r->gains.assign(B, 1.0f); r->caps.assign(B, 0);
  r->agc_targets.assign(B, 0.0f); pn_agc_default_params_host(r->agc_params);
  r->lim_ceilings.assign(B, 0.0f); pn_lim_default_params_host(r->lim_params);
  r->dtmf_sw.assign(B, 0); pn_dtmf_default_params_host(r->dtmf_params);
  r->clamp_sw.assign(B, 0); pn_dtmf_clamp_default_params_host(r->clamp_params);
  r->dtx_sw.assign(B, 0); pn_dtx_default_params_host(r->dtx_params);
  r->sids.assign(B * PN_CNG_SID_BYTES, 0);
  for (size_t s = 0; s < B; s++) pn_cng_default_sid(&r->sids[s * PN_CNG_SID_BYTES]);
  static const int kF[4] = {6, 3, 2, PN_RATE_F_3_2};   // (the order of pn_rate.hip rt_taps_offset; the h of 32000 is the table of 3 and is not staged twice)
  std::vector<float> h[2];
  std::vector<int> fs(B);
  for (size_t s = 0; s < B; s++) fs[s] = pn_rate_mixed_factor(r->rates[s]);
  for (int down = 0; down < 2; down++)
    for (int g : kF) {
      if (mixed ? !down && g == PN_RATE_F_3_2 : g != f) continue;
      float t[PN_RATE_MAX_TAPS];
      const int nt = pn_rate_design(g, down, t, PN_RATE_MAX_TAPS);
      if (nt < 0) goto fail;
      h[down].insert(h[down].end(), t, t + nt);
    }
  if (rate_alloc(r, r->taps_up, h[0].size() * 4, false) || rate_alloc(r, r->taps_down, h[1].size() * 4, false) || state_alloc(r, PN_RST_CORE, r->st) ||
      rate_alloc(r, r->x48, B * PN_FRAME * 4, true) || rate_alloc(r, r->y48, B * PN_FRAME * 4, true) ||
      rate_alloc(r, r->io_in, B * r->n * 4, mixed) || rate_alloc(r, r->io_out, B * r->n * 4, mixed) || rate_alloc(r, r->io_gr, B * 68 * 4, false) ||
      rate_alloc(r, r->d_laws, B * sizeof(int), true) || (mixed && rate_alloc(r, r->factors, B * sizeof(int), false))) goto fail;
  if (mixed && hipHostMalloc(&r->h_rows, B * r->n * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); r->h_rows = NULL; pn_set_error("rate converter: no pinned memory for %zu bytes", B * r->n * 4); goto fail; }
  // (synchronous copies: the sources are locals)
  if (hipMemcpyAsync(r->taps_up, h[0].data(), h[0].size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(r->taps_down, h[1].data(), h[1].size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      (mixed && hipMemcpyAsync(r->factors, fs.data(), B * sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
      hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); pn_set_error("rate converter init failed"); goto fail; }
  return r;
fail:
  pn_rate_destroy(r);
  return NULL;
}
extern "C" pn_rate *pn_rate_create(pn_ctx *c, int rate_hz) {
  if (!c) { pn_set_error("NULL argument"); return NULL; }
  const int f = rate_factor_or_error(rate_hz);
  return f ? rate_create(c, rate_hz, f, NULL) : NULL;
}
extern "C" pn_rate *pn_rate_create_mixed(pn_ctx *c, const int32_t *rates_hz) {
  if (!c) { pn_set_error("NULL argument"); return NULL; }
  if (rates_hz && pn_rate_mixed_rates_list_check(rates_hz, c->B)) return NULL;
  return rate_create(c, 0, 0, rates_hz);
}
extern "C" int pn_rate_is_mixed(const pn_rate *r) { if (!r) { pn_set_error("NULL argument"); return -1; } return r->mixed ? 1 : 0; }
extern "C" int pn_rate_row_samples(const pn_rate *r) { if (!r) { pn_set_error("NULL argument"); return -1; } return r->n; }
extern "C" int pn_rate_get_stream_rates(const pn_rate *r, int32_t *h_rates) { return rate_get(r, &pn_rate::rates, h_rates); }

// A rate change of the listed streams, asynchronous and ordered like pn_rate_reset_streams: the ids and the new factors go
// through the context's id ring in one copy, one launch writes the factors, the state table's walk zeroes the streams' state.
extern "C" int pn_rate_set_stream_rates(pn_rate *r, const int32_t *ids, int n, const int32_t *rates_hz) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (!r->mixed) { pn_set_error("a single-rate converter (%d Hz) keeps its rate: per-stream rates need pn_rate_create_mixed", r->rate); return -1; }
  if (pn_rate_mixed_set_check(r->c->B, ids, n, rates_hz)) return -1;
  if (n == 0) return 0;
  PN_ON_DEVICE(r->c);
  std::vector<int> f(n);
  for (int i = 0; i < n; i++) f[i] = pn_rate_mixed_factor(rates_hz[i]);
  const int *d = stage_ids(r->c, ids, n, f.data(), n);
  if (!d) return -1;
  pn_launch_rate_set_factors(r->c->stream, d, d + ((n + 3) & ~3), n, r->factors);
  state_clear_rows(r, PN_RE_RATE, d, n); cng_forget(r, ids, n);
  PN_HIP_CHECK(hipGetLastError());
  for (int i = 0; i < n; i++) r->rates[ids[i]] = rates_hz[i];
  return 0;
}

// A law change of the listed streams (G.711 rows), asynchronous and ordered like a rate change: the ids and the new laws go through
// the context's id ring in one copy, one launch writes the table.  No state is touched: the law is a setting of the edges.
extern "C" int pn_rate_set_stream_laws(pn_rate *r, const int32_t *ids, int n, const int32_t *laws) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_g711_laws_set_check(r->c->B, ids, n, laws)) return -1;
  if (n == 0) return 0;
  PN_ON_DEVICE(r->c);
  const int *d = stage_ids(r->c, ids, n, laws, n);
  if (!d) return -1;
  pn_launch_rate_set_factors(r->c->stream, d, d + ((n + 3) & ~3), n, r->d_laws);
  PN_HIP_CHECK(hipGetLastError());
  for (int i = 0; i < n; i++) r->laws[ids[i]] = laws[i];
  return 0;
}
extern "C" int pn_rate_get_stream_laws(const pn_rate *r, int32_t *h_laws) { return rate_get(r, &pn_rate::laws, h_laws); }

// A conference change of the listed streams, ordered like a law change.  Everything is decided on the host first (pn_conf.h
// pn_conf_change: the table after the change, the conferences it touches and their member rows); then the ids with their new
// conferences and the touched rows go through the context's id ring, in bounded pieces, each followed by the launch that reads it.
// Of the state only a listed stream's level starts again.  The device side is allocated by the first call that needs it — here, never inside a frame.
static int conf_buffers(pn_rate *r) {                // (the caller is on the context's device)
  if (r->d_conf) return 0;
  pn_ctx *c = r->c;
  const size_t B = (size_t)c->B;
  float *o48 = NULL; int *conf = NULL, *members = NULL; uint32_t *stamp = NULL;
  if (rate_alloc(r, o48, B * PN_FRAME * 4, true) || rate_alloc(r, conf, B * sizeof(int), false) ||
      rate_alloc(r, members, B * PN_CONF_MAX_MEMBERS * sizeof(int), false) || rate_alloc(r, stamp, B * sizeof(uint32_t), true)) return -1;
  PN_HIP_CHECK(hipMemsetAsync(conf, 0xFF, B * sizeof(int), c->stream));                               // PN_CONF_NONE
  PN_HIP_CHECK(hipMemsetAsync(members, 0xFF, B * PN_CONF_MAX_MEMBERS * sizeof(int), c->stream));     // -1: no member
  r->o48 = o48; r->d_members = members; r->d_stamp = stamp; r->tick = 0; r->d_conf = conf;
  return 0;
}
extern "C" int pn_rate_set_stream_confs(pn_rate *r, const int32_t *ids, int n, const int32_t *confs) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  PnConfChange ch;
  if (pn_conf_change(r->confs, ids, n, confs, &ch)) return -1;
  if (n == 0 || (!r->d_conf && ch.in_conf == 0)) return 0;          // (nobody has ever been in a conference, and nobody is now)
  PN_ON_DEVICE(r->c);
  if (conf_buffers(r)) return -1;
  for (int at = 0; at < n; at += RATE_PIECE) {
    const int m = n - at < RATE_PIECE ? n - at : RATE_PIECE;
    const int *d = stage_ids(r->c, ids + at, m, confs + at, m);
    if (!d) return -1;
    pn_launch_rate_set_factors(r->c->stream, d, d + ((m + 3) & ~3), m, r->d_conf);
    state_clear_rows(r, PN_RE_CONF, d, m);
  }
  const int k = (int)ch.touched.size();
  for (int at = 0; at < k; at += 512) {
    const int m = k - at < 512 ? k - at : 512;
    const int *d = stage_ids(r->c, ch.touched.data() + at, m, ch.rows.data() + (size_t)at * PN_CONF_MAX_MEMBERS, m * PN_CONF_MAX_MEMBERS);
    if (!d) return -1;
    pn_launch_rate_conf_rows(r->c->stream, d, d + ((m + 3) & ~3), m, r->d_members);
  }
  PN_HIP_CHECK(hipGetLastError());
  r->confs.swap(ch.next); r->in_conf = ch.in_conf;
  return 0;
}
extern "C" int pn_rate_get_stream_confs(const pn_rate *r, int32_t *h_confs) { return rate_get(r, &pn_rate::confs, h_confs); }

// ---- loudest-N talkers, send gains, hold, mix report (include/percepnet_hip.h; rules pn_mix_rules.h) ---------------------------
// Settings, written in stream order through the context's id ring like the conference table, so a frame submitted before a call
// runs under the old values.  "plain": every setting at its default — rate_mix then launches what it always launched.
static bool mix_plain(const pn_rate *r) { return r->gains_off == 0 && r->caps_on == 0 && r->hold == 0.0f && !r->report[RF_MIX]; }
static int mix_buffers(pn_rate *r) {                 // (the caller is on the context's device)
  if (conf_buffers(r)) return -1;
  if (r->d_gains) return 0;
  float *gains = NULL; int *caps = NULL; void *st[PN_RS_COUNT] = {};
  if (rate_alloc(r, gains, (size_t)r->c->B * 4, false) || rate_alloc(r, caps, (size_t)r->c->B * sizeof(int), true) || state_alloc(r, PN_RST_MIX, st)) return -1;
  PN_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)gains, 0x3f800000, (size_t)r->c->B, r->c->stream));                  // 1.0f
  r->d_caps = caps; state_commit(r, PN_RST_MIX, st); r->d_gains = gains;
  return 0;
}
extern "C" int pn_rate_set_stream_mix_gains(pn_rate *r, const int32_t *ids, int n, const float *gains) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_mix_gains_set_check(r->c->B, ids, n, gains)) return -1;
  return rate_set_words(r, ids, n, plus_zero(gains, n).data(), 1.0f, r->d_gains, mix_buffers, r->gains, r->gains_off);
}
extern "C" int pn_rate_get_stream_mix_gains(const pn_rate *r, float *h_gains) { return rate_get(r, &pn_rate::gains, h_gains); }
extern "C" int pn_rate_set_conf_speakers(pn_rate *r, const int32_t *confs, int n, const int32_t *max_speakers) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_mix_speakers_set_check(r->c->B, confs, n, max_speakers)) return -1;
  return rate_set_words(r, confs, n, max_speakers, (int32_t)0, r->d_caps, mix_buffers, r->caps, r->caps_on);
}
extern "C" int pn_rate_get_conf_speakers(const pn_rate *r, int32_t *h_n) { return rate_get(r, &pn_rate::caps, h_n); }
// the hold factor travels as an argument of every launch, so it is ordered like one; the levels go to zero in stream order
extern "C" int pn_rate_set_mix_hold(pn_rate *r, float d) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_mix_hold_check(d)) return -1;
  if (d == 0.0f) d = 0.0f;
  PN_ON_DEVICE(r->c);
  if (d != 0.0f && mix_buffers(r)) return -1;
  if (state_clear_all(r, PN_RE_HOLD)) return -1;
  r->hold = d;
  return 0;
}
extern "C" float pn_rate_get_mix_hold(const pn_rate *r) { if (!r) { pn_set_error("NULL argument"); return NAN; } return r->hold; }
extern "C" int pn_rate_set_mix_report(pn_rate *r, int enable) { return rate_set_report(r, RF_MIX, enable); }
extern "C" int pn_rate_read_mix_report(pn_rate *r, void *h_report) { return rate_report_copy(r, RF_MIX, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_mix_report_dev(pn_rate *r, void *d_report) { return rate_report_copy(r, RF_MIX, d_report, hipMemcpyDeviceToDevice); }

// ---- packet-loss concealment (include/percepnet_hip.h; the rule pn_plc_rules.h; the kernel pn_rate_plc.hip) ----------------------
static int plc_drop_marks(pn_rate *r) {              // (the caller is on the context's device)
  for (int32_t s : r->lost_ids) r->lost_mark[s] = 0;
  r->lost_ids.clear();
  if (++r->plc_tick == 0) {                          // (2^32 frames on: no stale stamp may meet the new tick)
    PN_HIP_CHECK(hipMemsetAsync(r->d_plc_lost, 0, (size_t)r->c->B * sizeof(uint32_t), r->c->stream));
    r->plc_tick = 1;
  }
  return 0;
}
extern "C" int pn_rate_set_plc(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  if (enable && !r->d_plc_lost) {
    pn_ctx *c = r->c;
    const size_t B = (size_t)c->B;
    void *st[PN_RS_COUNT] = {}; uint32_t *lost = NULL;
    if (state_alloc(r, PN_RST_PLC, st) || rate_alloc(r, lost, B * sizeof(uint32_t), true)) return -1;
    r->lost_mark.assign(B, 0); r->lost_ids.reserve(B);
    state_commit(r, PN_RST_PLC, st); r->plc_tick = 1; r->d_plc_lost = lost;
    // room in the id ring for the longest list a frame stages, "every stream but the lost ones", so that no frame grows the ring:
    // the identity list goes through it once, read by nobody
    r->up_ids.resize(B);
    for (size_t s = 0; s < B; s++) r->up_ids[s] = (int32_t)s;
    if (!stage_ids(c, r->up_ids.data(), (int)B)) return -1;
    r->up_ids.clear();
  } else if (enable && !r->plc) {
    // on again after a pause: the frames in between are missing from the histories, so every stream starts with an empty one
    if (state_clear_all(r, PN_RE_AGAIN, PN_RST_PLC)) return -1;
  }
  if (!enable && r->plc && plc_drop_marks(r)) return -1;
  r->plc = enable != 0;
  return 0;
}
extern "C" int pn_rate_set_lost(pn_rate *r, const int32_t *ids, int n) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (!r->plc) { pn_set_error("packet-loss concealment is off (pn_rate_set_plc)"); return -1; }
  if (pn_ids_check(r->c->B, ids, n, true)) return -1;
  if (n == 0) return 0;
  PN_ON_DEVICE(r->c);
  for (int at = 0; at < n; at += RATE_PIECE) {
    const int m = n - at < RATE_PIECE ? n - at : RATE_PIECE;
    const int *d = stage_ids(r->c, ids + at, m);
    if (!d) return -1;
    pn_launch_rate_conf_stamp(r->c->stream, d, m, r->d_plc_lost, r->plc_tick);
    PN_HIP_CHECK(hipGetLastError());
    // the host's marks chunk by chunk, right behind the device's: a device failure at a later chunk leaves the two in step
    for (int i = at; i < at + m; i++)
      if (!r->lost_mark[ids[i]]) { r->lost_mark[ids[i]] = 1; r->lost_ids.push_back(ids[i]); }
  }
  return 0;
}
extern "C" int pn_rate_set_plc_report(pn_rate *r, int enable) { return rate_set_report(r, RF_PLC, enable); }
extern "C" int pn_rate_read_plc_report(pn_rate *r, void *h_report) { return rate_report_copy(r, RF_PLC, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_plc_report_dev(pn_rate *r, void *d_report) { return rate_report_copy(r, RF_PLC, d_report, hipMemcpyDeviceToDevice); }

// ---- comfort noise (include/percepnet_hip.h; the rule pn_cng_rules.h; the kernel pn_rate_cng.hip) ----------------------------------
static void cng_drop_marks(pn_rate *r) {
  for (int32_t s : r->silent_ids) r->silent_mark[s] = 0;
  r->silent_ids.clear();
  if (++r->cng_tick == 0) { cng_forget(r, NULL, 0); r->cng_tick = 1; }   // (2^32 frames on: no stale tick may meet the new one; every run starts again)
}
static void cng_param_row(const PnCngSid &d, uint32_t *row) {   // a decoded SID as the kernel reads it
  memset(row, 0, PN_CNG_PARAM_WORDS * 4);
  memcpy(row, d.k, sizeof d.k); memcpy(row + PN_CNG_P_G, &d.g, 4); row[PN_CNG_P_M] = (uint32_t)d.M;
}
extern "C" int pn_rate_set_cng(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  if (enable && !r->d_cng_sid) {
    pn_ctx *c = r->c;
    const size_t B = (size_t)c->B;
    void *st = NULL; uint32_t *sid = NULL; float *rows = NULL;
    if (rate_alloc(r, st, B * PN_CNG_STATE_WORDS * 4, true) || rate_alloc(r, sid, B * PN_CNG_PARAM_WORDS * 4, false) || rate_alloc(r, rows, B * r->n * 4, true)) return -1;
    // the SIDs as set so far (the defaults, or what pn_rate_set_stream_sid has kept on the host), decoded; a synchronous copy: the source is a local
    std::vector<uint32_t> tab(B * PN_CNG_PARAM_WORDS);
    for (size_t s = 0; s < B; s++) {
      PnCngSid d;
      if (pn_cng_sid_decode_host(&r->sids[s * PN_CNG_SID_BYTES], &d)) return -1;
      cng_param_row(d, &tab[s * PN_CNG_PARAM_WORDS]);
    }
    PN_HIP_CHECK(hipMemcpyAsync(sid, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    PN_HIP_CHECK(hipStreamSynchronize(c->stream));
    // room in the id ring for the longest lists a frame stages — "every stream but the silent ones", and every stream with its
    // "continues" word — so that no frame grows the ring: the identity list goes through it once, read by nobody
    r->gen_ids.resize(B); r->gen_cont.assign(B, 0);
    for (size_t s = 0; s < B; s++) r->gen_ids[s] = (int32_t)s;
    if (!stage_ids(c, r->gen_ids.data(), (int)B, r->gen_cont.data(), (int)B)) return -1;
    r->gen_ids.clear(); r->gen_cont.clear(); r->up_ids.reserve(B);
    r->silent_mark.assign(B, 0); r->silent_ids.reserve(B); r->cng_last.assign(B, 0u);
    r->st2[PN_RS2_CNG] = st; r->cng_rows = rows; r->cng_tick = 1; r->d_cng_sid = sid;
  } else if (enable && !r->cng) {
    // on again after a pause: every stream's noise starts again, counts included, like pn_rate_reset
    if (state_clear_all(r, PN_RE_AGAIN, PN_RST_CNG)) return -1;
  }
  if (!enable && r->cng) cng_drop_marks(r);
  r->cng = enable != 0;
  return 0;
}
// the seed travels as an argument of every launch, so a change is ordered like one
extern "C" int pn_rate_set_cng_seed(pn_rate *r, uint32_t seed) { if (!r) { pn_set_error("NULL argument"); return -1; } r->cng_seed = seed; return 0; }
extern "C" int pn_rate_get_cng_seed(const pn_rate *r, uint32_t *seed) { if (!r || !seed) { pn_set_error("NULL argument"); return -1; } *seed = r->cng_seed; return 0; }
// The SIDs of the listed streams, a per-stream setting ordered like the law: decoded on the host, the ids and the decoded rows go through
// the context's id ring in bounded pieces, each followed by the launch that reads it.  While the device side does not exist the host's
// copy is all there is; the first enable decodes it.  No state is touched: a run goes on under the new SID, its gain ramping to the new g
extern "C" int pn_rate_set_stream_sid(pn_rate *r, const int32_t *ids, int n, const uint8_t *sids, int stride) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_cng_sids_set_check(r->c->B, ids, n, sids, stride)) return -1;
  if (n == 0) return 0;
  if (r->d_cng_sid) {
    PN_ON_DEVICE(r->c);
    enum { PIECE = RATE_PIECE / PN_CNG_PARAM_WORDS };
    std::vector<uint32_t> rows((size_t)(n < PIECE ? n : PIECE) * PN_CNG_PARAM_WORDS);
    for (int at = 0; at < n; at += PIECE) {
      const int m = n - at < PIECE ? n - at : PIECE;
      for (int i = 0; i < m; i++) {
        PnCngSid d;
        if (pn_cng_sid_decode_host(sids + (size_t)(at + i) * stride, &d)) return -1;
        cng_param_row(d, &rows[(size_t)i * PN_CNG_PARAM_WORDS]);
      }
      const int *d = stage_ids(r->c, ids + at, m, rows.data(), m * PN_CNG_PARAM_WORDS);
      if (!d) return -1;
      pn_launch_rate_cng_sids(r->c->stream, d, d + ((m + 3) & ~3), m, r->d_cng_sid);
      PN_HIP_CHECK(hipGetLastError());
    }
  }
  // the host's copy behind the last piece.  Every refusal stands in front of the first, so only a failure of the device itself gets
  // between two pieces: the call then returns -1 with the earlier pieces written on the device and the host's copy as it was
  for (int i = 0; i < n; i++) pn_cng_sid_store(sids + (size_t)i * stride, &r->sids[(size_t)ids[i] * PN_CNG_SID_BYTES]);
  return 0;
}
extern "C" int pn_rate_get_stream_sid(const pn_rate *r, uint8_t *h_sids) {
  if (!r || !h_sids) { pn_set_error("NULL argument"); return -1; }
  memcpy(h_sids, r->sids.data(), r->sids.size());
  return 0;
}
// Marks for the next frame, with the lifetime of pn_rate_set_lost's.  They live on the host alone — a frame compacts them into the list
// its kernel runs over — so the call launches nothing and is ordered, like every call, by where it stands between two submits
extern "C" int pn_rate_set_silent(pn_rate *r, const int32_t *ids, int n) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (!r->cng) { pn_set_error("comfort noise is off (pn_rate_set_cng)"); return -1; }
  if (pn_ids_check(r->c->B, ids, n, true)) return -1;
  for (int i = 0; i < n; i++)
    if (!r->silent_mark[ids[i]]) { r->silent_mark[ids[i]] = 1; r->silent_ids.push_back(ids[i]); }
  return 0;
}
extern "C" int pn_rate_set_cng_report(pn_rate *r, int enable) { return rate_set_report(r, RF_CNG, enable); }
extern "C" int pn_rate_read_cng_report(pn_rate *r, void *h_report) { return rate_report_copy(r, RF_CNG, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_cng_report_dev(pn_rate *r, void *d_report) { return rate_report_copy(r, RF_CNG, d_report, hipMemcpyDeviceToDevice); }
extern "C" int pn_rate_debug_cng_state(pn_rate *r, void *h_state) {
  if (!r || !h_state) { pn_set_error("NULL argument"); return -1; }
  const size_t bytes = (size_t)r->c->B * PN_CNG_STATE_WORDS * 4;
  if (!r->st2[PN_RS2_CNG]) { memset(h_state, 0, bytes); return 0; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(h_state, r->st2[PN_RS2_CNG], bytes, hipMemcpyDeviceToHost, r->c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}

// ---- automatic level control (include/percepnet_hip.h; the rule pn_agc_rules.h; the kernel pn_rate_agc.hip) -----------------------
extern "C" int pn_rate_set_agc(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  if (enable && !r->d_agc_targets) {
    float *targets = NULL; void *st[PN_RS_COUNT] = {};
    if (rate_alloc(r, targets, (size_t)r->c->B * 4, true) || state_alloc(r, PN_RST_AGC, st)) return -1;
    state_commit(r, PN_RST_AGC, st); r->d_agc_targets = targets;
  } else if (enable && !r->agc) {
    // on again after a pause: the frames in between are missing from the levels, so every stream starts fresh
    if (state_clear_all(r, PN_RE_AGAIN, PN_RST_AGC)) return -1;
  }
  r->agc = enable != 0;
  return 0;
}
// the parameters travel as an argument of every launch, so a change is ordered like one
extern "C" int pn_rate_set_agc_params(pn_rate *r, const float *params8) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_agc_params_check_host(params8)) return -1;
  memcpy(r->agc_params, params8, sizeof(r->agc_params));
  return 0;
}
extern "C" int pn_rate_get_agc_params(const pn_rate *r, float *params8) { return rate_get_params(r, &pn_rate::agc_params, params8); }
extern "C" int pn_rate_set_stream_agc_targets(pn_rate *r, const int32_t *ids, int n, const float *targets) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (!r->agc) { pn_set_error("automatic level control is off (pn_rate_set_agc)"); return -1; }
  if (pn_agc_targets_set_check(r->c->B, ids, n, targets)) return -1;
  return rate_set_words(r, ids, n, plus_zero(targets, n).data(), 0.0f, r->d_agc_targets, NULL, r->agc_targets, r->agc_on);   // (on: the device side exists)
}
extern "C" int pn_rate_get_stream_agc_targets(const pn_rate *r, float *h_targets) { return rate_get(r, &pn_rate::agc_targets, h_targets); }
extern "C" int pn_rate_set_agc_report(pn_rate *r, int enable) { return rate_set_report(r, RF_AGC, enable); }
extern "C" int pn_rate_read_agc_report(pn_rate *r, void *h_report) { return rate_report_copy(r, RF_AGC, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_agc_report_dev(pn_rate *r, void *d_report) { return rate_report_copy(r, RF_AGC, d_report, hipMemcpyDeviceToDevice); }

// ---- the output limiter (include/percepnet_hip.h; the rule pn_lim_rules.h; the kernel pn_rate_lim.hip) ----------------------------
static int lim_buffers(pn_rate *r) {                 // (the caller is on the context's device)
  if (r->d_lim_ceilings) return 0;
  float *ceilings = NULL; void *st[PN_RS_COUNT] = {};
  if (rate_alloc(r, ceilings, (size_t)r->c->B * 4, true) || state_alloc(r, PN_RST_LIM, st)) return -1;
  state_commit(r, PN_RST_LIM, st); r->d_lim_ceilings = ceilings;
  return 0;
}
extern "C" int pn_rate_set_stream_limiter(pn_rate *r, const int32_t *ids, int n, const float *ceilings) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_lim_ceilings_set_check(r->c->B, ids, n, ceilings)) return -1;
  return rate_set_words(r, ids, n, plus_zero(ceilings, n).data(), 0.0f, r->d_lim_ceilings, lim_buffers, r->lim_ceilings, r->lim_on);
}
extern "C" int pn_rate_get_stream_limiter(const pn_rate *r, float *h_ceilings) { return rate_get(r, &pn_rate::lim_ceilings, h_ceilings); }
// the parameters travel as an argument of every launch, so a change is ordered like one
extern "C" int pn_rate_set_limiter_params(pn_rate *r, const float *params2) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_lim_params_check_host(params2)) return -1;
  memcpy(r->lim_params, params2, sizeof(r->lim_params));
  return 0;
}
extern "C" int pn_rate_get_limiter_params(const pn_rate *r, float *params2) { return rate_get_params(r, &pn_rate::lim_params, params2); }
extern "C" int pn_rate_set_limiter_report(pn_rate *r, int enable) { return rate_set_report(r, RF_LIM, enable); }
extern "C" int pn_rate_read_limiter_report(pn_rate *r, void *h_report) { return rate_report_copy(r, RF_LIM, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_limiter_report_dev(pn_rate *r, void *d_report) { return rate_report_copy(r, RF_LIM, d_report, hipMemcpyDeviceToDevice); }

// ---- DTMF detection and removal (include/percepnet_hip.h; the rules pn_dtmf_rules.h, pn_dtmf_clamp_rules.h; the kernels pn_rate_dtmf.hip, pn_rate_dtmf_clamp.hip)
static int dtmf_buffers(pn_rate *r) {                // (the caller is on the context's device)
  if (r->d_dtmf_on) return 0;
  const PnDtmfTables &T = pn_dtmf_tables_ref();
  int *on = NULL; float *tab = NULL; void *st[PN_RS_COUNT] = {};
  if (rate_alloc(r, on, (size_t)r->c->B * 4, true) || rate_alloc(r, tab, sizeof(T.ct) + sizeof(T.st), false) || state_alloc(r, PN_RST_DTMF, st)) return -1;
  static_assert(offsetof(PnDtmfTables, st) == sizeof(T.ct), "ct and st are one block");
  PN_HIP_CHECK(hipMemcpyAsync(tab, T.ct, sizeof(T.ct) + sizeof(T.st), hipMemcpyHostToDevice, r->c->stream));   // (from a static table: the source outlives the copy)
  r->d_dtmf_tab = tab; state_commit(r, PN_RST_DTMF, st); r->d_dtmf_on = on;
  return 0;
}
// This stage's own rule: it reads the detector's report rows, so it allocates them — the user's buffer if there is one, otherwise one
// of the same kind — and while clamp_on > 0 the detector writes them whatever report[RF_DTMF] says (rate_dtmf)
static int clamp_buffers(pn_rate *r) {               // (the caller is on the context's device)
  if (r->d_clamp_on) return 0;
  int *on = NULL; void *st[PN_RS_COUNT] = {};
  if (!r->d_report[RF_DTMF] && rate_alloc(r, r->d_report[RF_DTMF], report_bytes(r, RF_DTMF), true)) return -1;
  if (rate_alloc(r, on, (size_t)r->c->B * 4, true) || state_alloc(r, PN_RST_CLAMP, st)) return -1;
  state_commit(r, PN_RST_CLAMP, st); r->d_clamp_on = on;
  return 0;
}
// switches as words, and the listed streams that come on from off
static void switch_words(const std::vector<uint8_t> &sw, const int32_t *ids, int n, const uint8_t *on, std::vector<int32_t> &v, std::vector<int32_t> &fresh) {
  v.resize(n);
  for (int i = 0; i < n; i++) { v[i] = on[i] ? 1 : 0; if (on[i] && !sw[ids[i]]) fresh.push_back(ids[i]); }
}
extern "C" int pn_rate_set_stream_dtmf(pn_rate *r, const int32_t *ids, int n, const uint8_t *on) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_on_set_check(r->c->B, ids, n, on)) return -1;
  std::vector<int32_t> v, fresh;
  switch_words(r->dtmf_sw, ids, n, on, v, fresh);
  return rate_set_words(r, ids, n, v.data(), (int32_t)0, r->d_dtmf_on, dtmf_buffers, r->dtmf_sw, r->dtmf_on, [&] { return state_switch_on(r, PN_RST_DTMF, fresh); });
}
extern "C" int pn_rate_get_stream_dtmf(const pn_rate *r, uint8_t *h_on) { return rate_get(r, &pn_rate::dtmf_sw, h_on); }
// the parameters travel as an argument of every launch, so a change is ordered like one
extern "C" int pn_rate_set_dtmf_params(pn_rate *r, const float *params7) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_params_check_host(params7)) return -1;
  // while removal is on for somebody its guard in front must stay in time
  if (r->clamp_on > 0 && pn_dtmf_clamp_params_check_host(r->clamp_params, (int)params7[PN_DTMF_ON_FRAMES])) return -1;
  memcpy(r->dtmf_params, params7, sizeof(r->dtmf_params));
  return 0;
}
extern "C" int pn_rate_get_dtmf_params(const pn_rate *r, float *params7) { return rate_get_params(r, &pn_rate::dtmf_params, params7); }
extern "C" int pn_rate_set_dtmf_report(pn_rate *r, int enable) { return rate_set_report(r, RF_DTMF, enable); }
extern "C" int pn_rate_read_dtmf_report(pn_rate *r, void *h_report) { return rate_report_copy(r, RF_DTMF, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_dtmf_report_dev(pn_rate *r, void *d_report) { return rate_report_copy(r, RF_DTMF, d_report, hipMemcpyDeviceToDevice); }
extern "C" int pn_rate_debug_dtmf_state(pn_rate *r, void *h_state) { return state_debug_copy(r, PN_RS_DTMF, h_state); }

extern "C" int pn_rate_set_stream_dtmf_clamp(pn_rate *r, const int32_t *ids, int n, const uint8_t *on) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_clamp_on_set_check(r->c->B, ids, n, on)) return -1;
  std::vector<int32_t> v, fresh;
  switch_words(r->clamp_sw, ids, n, on, v, fresh);
  bool any_on = false;
  for (int32_t w : v) any_on |= w != 0;
  if (any_on && pn_dtmf_clamp_params_check_host(r->clamp_params, (int)r->dtmf_params[PN_DTMF_ON_FRAMES])) return -1;
  return rate_set_words(r, ids, n, v.data(), (int32_t)0, r->d_clamp_on, clamp_buffers, r->clamp_sw, r->clamp_on, [&] { return state_switch_on(r, PN_RST_CLAMP, fresh); });
}
extern "C" int pn_rate_get_stream_dtmf_clamp(const pn_rate *r, uint8_t *h_on) { return rate_get(r, &pn_rate::clamp_sw, h_on); }
// the parameters travel as an argument of every launch, so a change is ordered like one
extern "C" int pn_rate_set_dtmf_clamp_params(pn_rate *r, const int32_t *params4) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_clamp_params_check_host(params4, (int)r->dtmf_params[PN_DTMF_ON_FRAMES])) return -1;
  memcpy(r->clamp_params, params4, sizeof(r->clamp_params));
  return 0;
}
extern "C" int pn_rate_get_dtmf_clamp_params(const pn_rate *r, int32_t *params4) { return rate_get_params(r, &pn_rate::clamp_params, params4); }
extern "C" int pn_rate_set_dtmf_clamp_report(pn_rate *r, int enable) { return rate_set_report(r, RF_CLAMP, enable); }
extern "C" int pn_rate_read_dtmf_clamp_report(pn_rate *r, void *h_report) { return rate_report_copy(r, RF_CLAMP, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_dtmf_clamp_report_dev(pn_rate *r, void *d_report) { return rate_report_copy(r, RF_CLAMP, d_report, hipMemcpyDeviceToDevice); }
extern "C" int pn_rate_debug_dtmf_clamp_state(pn_rate *r, void *h_state) { return state_debug_copy(r, PN_RS_CLAMP, h_state); }
// TESTS ONLY: the detector's report rows — the user's buffer too — overwritten from the host, synchronising, so that the stand-alone stage
// can be run over hand-made rows; the next detector launch overwrites them again
extern "C" int pn_rate_debug_set_dtmf_report(pn_rate *r, const void *h_report) {
  if (!r || !h_report) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  if (clamp_buffers(r)) return -1;
  PN_HIP_CHECK(hipMemcpyAsync(r->d_report[RF_DTMF], h_report, report_bytes(r, RF_DTMF), hipMemcpyHostToDevice, r->c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}

// ---- the DTX send side (include/percepnet_hip.h; the rule pn_dtx_rules.h; the kernel pn_rate_dtx.hip) ------------------------------------
static int dtx_buffers(pn_rate *r) {                 // (the caller is on the context's device)
  if (r->d_dtx_on) return 0;
  int *on = NULL; void *st = NULL;
  if (rate_alloc(r, on, (size_t)r->c->B * 4, true) || rate_alloc(r, st, (size_t)r->c->B * PN_DTX_STATE_WORDS * 4, true)) return -1;
  r->st2[PN_RS2_DTX] = st; r->d_dtx_on = on;
  return 0;
}
extern "C" int pn_rate_set_stream_dtx(pn_rate *r, const int32_t *ids, int n, const uint8_t *on) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtx_on_set_check(r->c->B, ids, n, on)) return -1;
  std::vector<int32_t> v, fresh;
  switch_words(r->dtx_sw, ids, n, on, v, fresh);
  return rate_set_words(r, ids, n, v.data(), (int32_t)0, r->d_dtx_on, dtx_buffers, r->dtx_sw, r->dtx_on, [&] { return state_switch_on(r, PN_RST_DTX, fresh); });
}
extern "C" int pn_rate_get_stream_dtx(const pn_rate *r, uint8_t *h_on) { return rate_get(r, &pn_rate::dtx_sw, h_on); }
// the parameters travel as an argument of every launch, so a change is ordered like one
extern "C" int pn_rate_set_dtx_params(pn_rate *r, const float *params9) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtx_params_check_host(params9)) return -1;
  memcpy(r->dtx_params, params9, sizeof(r->dtx_params));
  return 0;
}
extern "C" int pn_rate_get_dtx_params(const pn_rate *r, float *params9) { return rate_get_params(r, &pn_rate::dtx_params, params9); }
extern "C" int pn_rate_set_dtx_report(pn_rate *r, int enable) { return rate_set_report(r, RF_DTX, enable); }
extern "C" int pn_rate_read_dtx_report(pn_rate *r, void *h_report) { return rate_report_copy(r, RF_DTX, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_dtx_report_dev(pn_rate *r, void *d_report) { return rate_report_copy(r, RF_DTX, d_report, hipMemcpyDeviceToDevice); }
extern "C" int pn_rate_debug_dtx_state(pn_rate *r, void *h_state) {
  if (!r || !h_state) { pn_set_error("NULL argument"); return -1; }
  const size_t bytes = (size_t)r->c->B * PN_DTX_STATE_WORDS * 4;
  if (!r->st2[PN_RS2_DTX]) { memset(h_state, 0, bytes); return 0; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(h_state, r->st2[PN_RS2_DTX], bytes, hipMemcpyDeviceToHost, r->c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}

// ---- the two resets: what they clear is the state table's ------------------------------------------------------------------------
extern "C" int pn_rate_reset(pn_rate *r) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  return state_clear_all(r, PN_RE_RESET);
}
extern "C" int pn_rate_reset_streams(pn_rate *r, const int32_t *ids, int n) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_ids_check(r->c->B, ids, n, false)) return -1;
  if (n == 0) return 0;
  PN_ON_DEVICE(r->c);
  const int *d = stage_ids(r->c, ids, n);
  if (!d) return -1;
  state_clear_rows(r, PN_RE_RESET_STREAMS, d, n); cng_forget(r, ids, n);
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- the two kernels -----------------------------------------------------------------------------------------------------------
// The rows of one call: every stream (ids == NULL), or the listed ones staged ONCE through the context's id ring; both kernels of a
// whole frame read the same staged list.
struct RateRows { const int *d_ids; int n; };
static int rate_rows(pn_rate *r, const int32_t *ids, int n, RateRows *rows) {
  rows->d_ids = NULL; rows->n = r->c->B;
  if (!ids) return 0;
  if (pn_ids_check(r->c->B, ids, n, true)) return -1;
  rows->n = n;
  if (n > 0 && !(rows->d_ids = stage_ids(r->c, ids, n))) return -1;
  return 0;
}
static int rate_aligned(const void *a, const void *b) {
  if (!a || !b) { pn_set_error("NULL argument"); return -1; }
  if (((uintptr_t)a | (uintptr_t)b) & 15) { pn_set_error("rate converter rows must be 16-byte aligned"); return -1; }
  return 0;
}
static int rate_up(pn_rate *r, const void *d_in, int fmt, float *d_out48, const RateRows &rows) {
  RateScope sc(r, RF_UP);
  if (r->mixed ? pn_launch_rate_up_mixed(r->c->stream, fmt, rows.n, rows.d_ids, r->factors, r->d_laws, d_in, d_out48, stf(r, PN_RS_TAIL_UP), r->taps_up)
               : pn_launch_rate_up(r->c->stream, r->f, fmt, rows.n, rows.d_ids, r->d_laws, d_in, d_out48, stf(r, PN_RS_TAIL_UP), r->taps_up)) return -1;
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
static int rate_down(pn_rate *r, const float *d_in48, void *d_out, int fmt, const RateRows &rows) {
  const int sat = r->c->saturate ? 1 : 0;
  RateScope sc(r, RF_DOWN);
  if (r->mixed ? pn_launch_rate_down_mixed(r->c->stream, fmt, rows.n, rows.d_ids, r->factors, r->d_laws, d_in48, d_out, sat, stf(r, PN_RS_TAIL_DOWN), r->taps_down)
               : pn_launch_rate_down(r->c->stream, r->f, fmt, rows.n, rows.d_ids, r->d_laws, d_in48, d_out, sat, stf(r, PN_RS_TAIL_DOWN), r->taps_down)) return -1;
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
// the mix: with a list, the listed streams' stamps first (which members advance is then known on the device), then one launch over the rows
static int rate_mix(pn_rate *r, const float *d_in48, float *d_out48, const RateRows &rows) {
  if (rows.n <= 0) return 0;
  if (rows.d_ids && r->d_conf) {
    if (++r->tick == 0) { PN_HIP_CHECK(hipMemsetAsync(r->d_stamp, 0, (size_t)r->c->B * sizeof(uint32_t), r->c->stream)); r->tick = 1; }   // (2^32 frames on)
    pn_launch_rate_conf_stamp(r->c->stream, rows.d_ids, rows.n, r->d_stamp, r->tick);
  }
  RateScope sc(r, RF_MIX);
  if (mix_plain(r)) pn_launch_rate_mix(r->c->stream, rows.n, rows.d_ids, r->d_conf, r->d_members, r->d_stamp, r->tick, d_in48, d_out48);
  else pn_launch_rate_mix_sel(r->c->stream, rows.n, rows.d_ids, r->d_conf, r->d_members, r->d_stamp, r->tick, d_in48, d_out48, r->d_gains, r->d_caps,
                              stf(r, PN_RS_LEVEL), r->hold, rate_report(r, RF_MIX));
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
// a stage's launch inside its timed scope, then the launch's verdict
template <class Launch>
static int rate_timed(pn_rate *r, int fam, Launch launch) {
  { RateScope sc(r, fam); launch(); }
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
// the concealer over the rows, in place; it consumes the marks: the tick moves on, and the host's copy of them is cleared
static int rate_plc(pn_rate *r, float *d_x48, const RateRows &rows) {
  if (rate_timed(r, RF_PLC, [&] { pn_launch_rate_plc(r->c->stream, rows.n, rows.d_ids, r->d_plc_lost, r->plc_tick, d_x48, stf(r, PN_RS_PLC_HIST), stf(r, PN_RS_PLC_Q),
                                                     r->st[PN_RS_PLC_META], rate_report(r, RF_PLC)); })) return -1;
  return plc_drop_marks(r);
}
// the level control over the rows, in place; d_lost / tick: the concealer's stamps and the tick it used for this frame (NULL: nobody is concealed)
static int rate_agc(pn_rate *r, float *d_y48, const RateRows &rows, const uint32_t *d_lost, uint32_t tick) {
  return rate_timed(r, RF_AGC, [&] { pn_launch_rate_agc(r->c->stream, rows.n, rows.d_ids, r->d_agc_targets, d_lost, tick, r->agc_params, d_y48, r->st[PN_RS_AGC], rate_report(r, RF_AGC)); });
}
// the output limiter over the rows, in place on the rows the down-conversion reads next
static int rate_lim(pn_rate *r, float *d_o48, const RateRows &rows) {
  return rate_timed(r, RF_LIM, [&] { pn_launch_rate_lim(r->c->stream, rows.n, rows.d_ids, r->d_lim_ceilings, r->lim_params, d_o48, r->st[PN_RS_LIM], rate_report(r, RF_LIM)); });
}
// the DTMF detector over the rows, which it only reads; d_lost / tick as for the level control.  Its report rows are written for the
// user, or for the removal stage while that is on for somebody
static int rate_dtmf(pn_rate *r, const float *d_x48, const RateRows &rows, const uint32_t *d_lost, uint32_t tick) {
  return rate_timed(r, RF_DTMF, [&] { pn_launch_rate_dtmf(r->c->stream, rows.n, rows.d_ids, r->d_dtmf_on, d_lost, tick, r->dtmf_params, pn_dtmf_tables_ref().rot, r->d_dtmf_tab, d_x48,
                                                          r->st[PN_RS_DTMF], r->report[RF_DTMF] || r->clamp_on > 0 ? r->d_report[RF_DTMF] : NULL); });
}
// DTMF removal over the rows, in place on y48; det: the detector ran in this frame (or the caller vouches for its report rows), otherwise
// every stream counts as "detection off"
static int rate_clamp(pn_rate *r, float *d_y48, const RateRows &rows, bool det) {
  return rate_timed(r, RF_CLAMP, [&] { pn_launch_rate_dtmf_clamp(r->c->stream, rows.n, rows.d_ids, r->d_clamp_on, r->clamp_params, det ? r->d_report[RF_DTMF] : NULL, d_y48,
                                                                 r->st[PN_RS_CLAMP], rate_report(r, RF_CLAMP)); });
}
// comfort noise for the streams gen (host, distinct): their rows at their own rates into cng_rows, then the unchanged up-conversion, float,
// from there into d_x48 — both over ONE staged list, which carries every stream's "continues" word behind the ids
static int rate_cng(pn_rate *r, float *d_x48, const std::vector<int32_t> &gen) {
  const int n = (int)gen.size();
  r->gen_cont.resize(n);
  for (int i = 0; i < n; i++) {
    uint32_t &last = r->cng_last[gen[i]];
    r->gen_cont[i] = last != 0u && last == r->cng_tick - 1u;
    last = r->cng_tick;
  }
  const int *d = stage_ids(r->c, gen.data(), n, r->gen_cont.data(), n);
  if (!d) return -1;
  if (rate_timed(r, RF_CNG, [&] { pn_launch_rate_cng(r->c->stream, n, d, d + ((n + 3) & ~3), r->mixed ? r->factors : NULL, r->n, r->cng_seed, r->d_cng_sid, r->st2[PN_RS2_CNG],
                                                     r->cng_rows, r->n, rate_report(r, RF_CNG)); })) return -1;
  const RateRows rows = {d, n};
  return rate_up(r, r->cng_rows, PN_FMT_F32, d_x48, rows);
}
// the DTX send side over the OUTPUT rows (fmt: their format), which it only reads: rows strided like an output row
static int rate_dtx(pn_rate *r, const void *d_out, int fmt, const RateRows &rows) {
  if (rows.n <= 0) return 0;                         // (an empty list: nothing to launch, nothing to time)
  int rc = 0;
  if (rate_timed(r, RF_DTX, [&] { rc = pn_launch_rate_dtx(r->c->stream, fmt, rows.n, rows.d_ids, r->d_dtx_on, r->mixed ? r->factors : NULL, r->n, r->d_laws, r->dtx_params, d_out, r->n,
                                                         r->st2[PN_RS2_DTX], rate_report(r, RF_DTX)); })) return -1;
  return rc;
}
// The stand-alone stage calls.  Their prologue: the converter, `off` (the stage's switch is off: its message), the rows' alignment —
// then RATE_STAGE_ROWS: the context's device for the rest of the call, and the rows
static int rate_stage_check(const pn_rate *r, const void *a, const void *b, const char *off = NULL) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (off) { pn_set_error("%s", off); return -1; }
  return rate_aligned(a, b);
}
#define RATE_STAGE_ROWS(r, ids, n) PN_ON_DEVICE((r)->c); RateRows rows; if (rate_rows(r, ids, n, &rows)) return -1
static int rate_up_call(pn_rate *r, const void *d_in, int fmt, float *d_out48, const int32_t *ids, int n) {
  if (rate_stage_check(r, d_in, d_out48)) return -1;
  RATE_STAGE_ROWS(r, ids, n);
  return rate_up(r, d_in, fmt, d_out48, rows);
}
static int rate_down_call(pn_rate *r, const float *d_in48, void *d_out, int fmt, const int32_t *ids, int n) {
  if (rate_stage_check(r, d_in48, d_out)) return -1;
  RATE_STAGE_ROWS(r, ids, n);
  return rate_down(r, d_in48, d_out, fmt, rows);
}
extern "C" int pn_rate_up_f32(pn_rate *r, const float *d_in, float *d_out48, const int32_t *ids, int n_ids) { return rate_up_call(r, d_in, PN_FMT_F32, d_out48, ids, n_ids); }
extern "C" int pn_rate_up_i16(pn_rate *r, const int16_t *d_in, float *d_out48, const int32_t *ids, int n_ids) { return rate_up_call(r, d_in, PN_FMT_I16, d_out48, ids, n_ids); }
extern "C" int pn_rate_up_g711(pn_rate *r, const uint8_t *d_in, float *d_out48, const int32_t *ids, int n_ids) { return rate_up_call(r, d_in, PN_FMT_G711, d_out48, ids, n_ids); }
extern "C" int pn_rate_down_f32(pn_rate *r, const float *d_in48, float *d_out, const int32_t *ids, int n_ids) { return rate_down_call(r, d_in48, d_out, PN_FMT_F32, ids, n_ids); }
extern "C" int pn_rate_down_i16(pn_rate *r, const float *d_in48, int16_t *d_out, const int32_t *ids, int n_ids) { return rate_down_call(r, d_in48, d_out, PN_FMT_I16, ids, n_ids); }
extern "C" int pn_rate_down_g711(pn_rate *r, const float *d_in48, uint8_t *d_out, const int32_t *ids, int n_ids) { return rate_down_call(r, d_in48, d_out, PN_FMT_G711, ids, n_ids); }
extern "C" int pn_rate_mix_f32(pn_rate *r, const float *d_in48, float *d_out48, const int32_t *ids, int n_ids) {
  if (rate_stage_check(r, d_in48, d_out48)) return -1;
  const uintptr_t a = (uintptr_t)d_in48, b = (uintptr_t)d_out48, span = (uintptr_t)r->c->B * PN_FRAME * 4;
  if (a < b + span && b < a + span) { pn_set_error("the mix reads every member's row for every listener: its input and output rows must not overlap"); return -1; }
  RATE_STAGE_ROWS(r, ids, n_ids);
  return rate_mix(r, d_in48, d_out48, rows);
}
extern "C" int pn_rate_plc_f32(pn_rate *r, float *d_x48, const int32_t *ids, int n_ids) {
  if (rate_stage_check(r, d_x48, d_x48, r && !r->plc ? "packet-loss concealment is off (pn_rate_set_plc)" : NULL)) return -1;
  RATE_STAGE_ROWS(r, ids, n_ids);
  return rate_plc(r, d_x48, rows);
}
extern "C" int pn_rate_agc_f32(pn_rate *r, float *d_y48, const int32_t *ids, int n_ids) {
  if (rate_stage_check(r, d_y48, d_y48, r && !r->agc ? "automatic level control is off (pn_rate_set_agc)" : NULL)) return -1;
  RATE_STAGE_ROWS(r, ids, n_ids);
  return rate_agc(r, d_y48, rows, NULL, 0);
}
// (the next three: where the stage was never used every stream is off, and its device side exists from here on)
extern "C" int pn_rate_lim_f32(pn_rate *r, float *d_o48, const int32_t *ids, int n_ids) {
  if (rate_stage_check(r, d_o48, d_o48)) return -1;
  RATE_STAGE_ROWS(r, ids, n_ids);
  return lim_buffers(r) ? -1 : rate_lim(r, d_o48, rows);
}
extern "C" int pn_rate_dtmf_f32(pn_rate *r, const float *d_x48, const int32_t *ids, int n_ids) {
  if (rate_stage_check(r, d_x48, d_x48)) return -1;
  RATE_STAGE_ROWS(r, ids, n_ids);
  return dtmf_buffers(r) ? -1 : rate_dtmf(r, d_x48, rows, NULL, 0);
}
extern "C" int pn_rate_dtmf_clamp_f32(pn_rate *r, float *d_y48, const int32_t *ids, int n_ids) {
  if (rate_stage_check(r, d_y48, d_y48)) return -1;
  RATE_STAGE_ROWS(r, ids, n_ids);
  return clamp_buffers(r) ? -1 : rate_clamp(r, d_y48, rows, true);
}
// (where the stage was never used every stream is off, and its device side exists from here on)
static int rate_dtx_call(pn_rate *r, const void *d_out, int fmt, const int32_t *ids, int n) {
  if (rate_stage_check(r, d_out, d_out)) return -1;
  RATE_STAGE_ROWS(r, ids, n);
  return dtx_buffers(r) ? -1 : rate_dtx(r, d_out, fmt, rows);
}
extern "C" int pn_rate_dtx_f32(pn_rate *r, const float *d_out_rows, const int32_t *ids, int n_ids) { return rate_dtx_call(r, d_out_rows, PN_FMT_F32, ids, n_ids); }
extern "C" int pn_rate_dtx_i16(pn_rate *r, const int16_t *d_out_rows, const int32_t *ids, int n_ids) { return rate_dtx_call(r, d_out_rows, PN_FMT_I16, ids, n_ids); }
extern "C" int pn_rate_dtx_g711(pn_rate *r, const uint8_t *d_out_rows, const int32_t *ids, int n_ids) { return rate_dtx_call(r, d_out_rows, PN_FMT_G711, ids, n_ids); }
// comfort noise on its own: every listed stream's row is generated and up-converted into d_x48, marked or not; like a frame it moves the
// tick on and drops the marks
extern "C" int pn_rate_cng_f32(pn_rate *r, float *d_x48, const int32_t *ids, int n_ids) {
  if (rate_stage_check(r, d_x48, d_x48, r && !r->cng ? "comfort noise is off (pn_rate_set_cng)" : NULL)) return -1;
  PN_ON_DEVICE(r->c);
  if (ids && pn_ids_check(r->c->B, ids, n_ids, true)) return -1;
  r->gen_ids.clear();
  if (ids) r->gen_ids.assign(ids, ids + n_ids); else for (int s = 0; s < r->c->B; s++) r->gen_ids.push_back(s);
  const int rc = r->gen_ids.empty() ? 0 : rate_cng(r, d_x48, r->gen_ids);
  cng_drop_marks(r);
  return rc;
}

// ---- one whole frame -----------------------------------------------------------------------------------------------------------
// up into x48 — for the streams marked silent while comfort noise is on, from the rows its kernel writes —, while packet-loss concealment is on the concealer in place on x48, the engine's float frame from x48 into y48 (all streams, or the listed ones through the context's own active
// set), while automatic level control is on and a stream has a target the level control in place on y48, down from y48 — or, while a stream is in a conference, the mix from y48 into o48 and down from o48 — and in front of the down-conversion, while a stream has a ceiling, the output limiter in place on the rows it reads; behind it, while a stream has the DTX send side on, that stage reading the output rows.  A frame the engine refuses returns -1 with its error kept; the up kernel has then advanced its tails
// and the down kernel has not, which is why the header asks for a reset of both objects before reuse.
// rate_frame: the launches alone — the caller is on the context's device and has checked the rows and, when active, the list
// (pn_ids_check, distinct), which is what lets the pipelined path refuse a list BEFORE the frame takes a pipeline slot.
static int rate_frame(pn_rate *r, const void *d_in, void *d_out, float *d_gr, int fmt, bool active, const int32_t *ids, int n) {
  pn_ctx *c = r->c;
  RateRows rows = {NULL, c->B};
  // marked streams: the up-conversion runs over "advancing minus lost minus silent" — its own staged list, in front of the frame's — so a
  // lost or silent stream's input row is never read, and a lost stream's tail stays.  The advancing silent streams that are not lost
  // (lost wins) get their rows from the comfort-noise kernel and their own up-conversion, float, behind the others'.  Nobody marked, or
  // no marked stream advancing: the launch of always
  bool up_done = false;
  const bool any_lost = r->plc && !r->lost_ids.empty(), any_silent = r->cng && !r->silent_ids.empty();
  if (any_lost || any_silent) {
    r->up_ids.clear(); r->gen_ids.clear();
    auto sort = [&](int32_t s) {
      if (any_lost && r->lost_mark[s]) return;
      if (any_silent && r->silent_mark[s]) r->gen_ids.push_back(s); else r->up_ids.push_back(s);
    };
    if (active) for (int i = 0; i < n; i++) sort(ids[i]);
    else for (int s = 0; s < c->B; s++) sort(s);
    const int nu = (int)r->up_ids.size();
    if (nu != (active ? n : c->B)) {
      RateRows up = {NULL, nu};
      if (nu > 0 && !(up.d_ids = stage_ids(c, r->up_ids.data(), nu))) return -1;
      if (nu > 0 && rate_up(r, d_in, fmt, r->x48, up)) return -1;
      if (!r->gen_ids.empty() && rate_cng(r, r->x48, r->gen_ids)) return -1;
      up_done = true;
    }
  }
  if (r->cng) cng_drop_marks(r);                      // the frame consumes the silent marks: the tick moves on
  if (active) {                                      // (an empty list is legal, as for pn_process_*_active: nobody advances)
    rows.n = n;
    if (n > 0 && !(rows.d_ids = stage_ids(c, ids, n))) return -1;
  }
  if (!up_done && rate_up(r, d_in, fmt, r->x48, rows)) return -1;
  const uint32_t plc_tick_used = r->plc_tick;        // the tick the concealer stamps this frame's lost streams with: rate_plc moves it on
  const bool concealing = r->plc;
  if (r->plc && rate_plc(r, r->x48, rows)) return -1;
  // the DTMF detector, while somebody is enabled: behind the concealer and in front of the engine, reading x48 only
  if (r->dtmf_on > 0 && rate_dtmf(r, r->x48, rows, concealing ? r->d_plc_lost : NULL, plc_tick_used)) return -1;
  if (active ? pn_process_f32_active(c, r->x48, r->y48, d_gr, ids, n) : pn_process_f32(c, r->x48, r->y48, d_gr)) return -1;
  // DTMF removal, while somebody has it on: in place on y48, so the level control, the mix, the limiter and the down-conversion never see the
  // tone.  The detector's report rows are this frame's only if it ran (somebody has detection on); otherwise nobody has a digit
  if (r->clamp_on > 0 && rate_clamp(r, r->y48, rows, r->dtmf_on > 0)) return -1;
  // the level control, while on and somebody has a target: in place on y48, so the mix, its levels and the down-conversion see levelled rows
  if (r->agc && r->agc_on > 0 && rate_agc(r, r->y48, rows, concealing ? r->d_plc_lost : NULL, plc_tick_used)) return -1;
  float *o = r->y48;
  if (r->in_conf > 0 || !mix_plain(r)) {             // somebody is in a conference (or a mix setting is on): the mix writes every advancing stream's row of o48
    if (rate_mix(r, r->y48, r->o48, rows)) return -1;
    o = r->o48;
  }
  // the output limiter, while somebody has a ceiling: in place on the rows the down-conversion reads — mix rows, or the streams' own
  if (r->lim_on > 0 && rate_lim(r, o, rows)) return -1;
  if (rate_down(r, o, d_out, fmt, rows)) return -1;
  // the DTX send side, while somebody is switched on: behind the down-conversion, reading the rows the caller is about to send
  if (r->dtx_on > 0 && rate_dtx(r, d_out, fmt, rows)) return -1;
  if (r->events.size() >= 4096 && rate_flush_events(r)) return -1;   // profiling left on: bound the pending events
  return 0;
}
static int rate_process(pn_rate *r, const void *d_in, void *d_out, float *d_gr, int fmt, bool active, const int32_t *ids, int n) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (rate_aligned(d_in, d_out)) return -1;
  PN_ON_DEVICE(r->c);
  if (active && pn_ids_check(r->c->B, ids, n, true)) return -1;
  return rate_frame(r, d_in, d_out, d_gr, fmt, active, ids, n);
}
extern "C" int pn_rate_process_f32(pn_rate *r, const float *d_in, float *d_out, float *d_gr) { return rate_process(r, d_in, d_out, d_gr, PN_FMT_F32, false, NULL, 0); }
extern "C" int pn_rate_process_i16(pn_rate *r, const int16_t *d_in, int16_t *d_out, float *d_gr) { return rate_process(r, d_in, d_out, d_gr, PN_FMT_I16, false, NULL, 0); }
extern "C" int pn_rate_process_g711(pn_rate *r, const uint8_t *d_in, uint8_t *d_out, float *d_gr) { return rate_process(r, d_in, d_out, d_gr, PN_FMT_G711, false, NULL, 0); }
extern "C" int pn_rate_process_f32_active(pn_rate *r, const float *d_in, float *d_out, float *d_gr, const int32_t *ids, int n) { return rate_process(r, d_in, d_out, d_gr, PN_FMT_F32, true, ids, n); }
extern "C" int pn_rate_process_i16_active(pn_rate *r, const int16_t *d_in, int16_t *d_out, float *d_gr, const int32_t *ids, int n) { return rate_process(r, d_in, d_out, d_gr, PN_FMT_I16, true, ids, n); }
extern "C" int pn_rate_process_g711_active(pn_rate *r, const uint8_t *d_in, uint8_t *d_out, float *d_gr, const int32_t *ids, int n) { return rate_process(r, d_in, d_out, d_gr, PN_FMT_G711, true, ids, n); }

static int rate_process_host(pn_rate *r, const void *h_in, void *h_out, float *h_gr, int fmt) {
  if (!r || !h_in || !h_out) { pn_set_error("NULL argument"); return -1; }
  pn_ctx *c = r->c;
  PN_ON_DEVICE(c);
  if (pn_host_wait(c)) return -1;                    // frames in flight on the context's pipelined path complete first
  const size_t nbytes = (size_t)c->B * r->n * pn_fmt_bytes(fmt);
  PN_HIP_CHECK(hipMemcpyAsync(r->io_in, h_in, nbytes, hipMemcpyHostToDevice, c->stream));
  if (rate_process(r, r->io_in, r->io_out, h_gr ? r->io_gr : NULL, fmt, false, NULL, 0)) return -1;
  // (mixed: the rows land in the converter's pinned buffer, and only each stream's own samples go on to the caller's row)
  PN_HIP_CHECK(hipMemcpyAsync(r->mixed ? r->h_rows : h_out, r->io_out, nbytes, hipMemcpyDeviceToHost, c->stream));
  if (h_gr) PN_HIP_CHECK(hipMemcpyAsync(h_gr, r->io_gr, (size_t)c->B * 68 * 4, hipMemcpyDeviceToHost, c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (r->mixed) {
    const size_t w = pn_fmt_bytes(fmt);
    for (int s = 0; s < c->B; s++)
      memcpy(static_cast<char *>(h_out) + (size_t)s * r->n * w, static_cast<const char *>(r->h_rows) + (size_t)s * r->n * w,
             (size_t)pn_rate_factor_frame(pn_rate_mixed_factor(r->rates[s])) * w);
  }
  return 0;
}
extern "C" int pn_rate_process_host_f32(pn_rate *r, const float *h_in, float *h_out, float *h_gr) { return rate_process_host(r, h_in, h_out, h_gr, PN_FMT_F32); }
extern "C" int pn_rate_process_host_i16(pn_rate *r, const int16_t *h_in, int16_t *h_out, float *h_gr) { return rate_process_host(r, h_in, h_out, h_gr, PN_FMT_I16); }
extern "C" int pn_rate_process_host_g711(pn_rate *r, const uint8_t *h_in, uint8_t *h_out, float *h_gr) { return rate_process_host(r, h_in, h_out, h_gr, PN_FMT_G711); }

// ---- the pipelined host path ---------------------------------------------------------------------------------------------------
// A converter's frame through the CONTEXT's pipeline (pn_host_pipe.cpp pipe_submit): the context's copy streams, slot counter,
// events, g|r and report slots and its two-frames-in-flight bound, so pn_host_wait, pn_host_frames_delivered and
// pn_host_next_report count frames of either kind in submission order.  The converter adds its own staging rows — slot 0 is
// io_in / io_out, slot 1 is allocated once — and the frame body rate_frame.  x48 / y48 stay single: the compute stream
// serialises the frames.  Whole rows travel both ways; on a mixed converter that is 480 samples per stream, of which the
// kernels read and write each stream's own n_s, with no landing buffer and no host copy.
static int rate_pipe_prepare(pn_rate *r) {           // (the caller is on the context's device)
  const size_t bytes = (size_t)r->c->B * r->n * 4;
  // (a mixed converter's rows are zeroed like slot 0's, so that the part of an output row no kernel writes is never stale memory)
  if (!r->io_in1 && rate_alloc(r, r->io_in1, bytes, r->mixed)) return -1;
  if (!r->io_out1 && rate_alloc(r, r->io_out1, bytes, r->mixed)) return -1;
  return pn_host_pipeline_prepare(r->c);
}
extern "C" int pn_rate_host_pipeline_prepare(pn_rate *r) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  return rate_pipe_prepare(r);
}
struct RateFrame { pn_rate *r; int fmt; bool active; const int32_t *ids; int n; };
static int rate_frame_body(void *arg, void *d_in, void *d_out, float *d_gr) {
  const RateFrame &f = *static_cast<const RateFrame *>(arg);
  return rate_frame(f.r, d_in, d_out, d_gr, f.fmt, f.active, f.ids, f.n);
}
static int rate_submit_host(pn_rate *r, const void *h_in, void *h_out, float *h_gr, int fmt, bool active, const int32_t *ids, int n) {
  if (!r || !h_in || !h_out) { pn_set_error("NULL argument"); return -1; }
  pn_ctx *c = r->c;
  if (active && pn_ids_check(c->B, ids, n, true)) return -1;          // refused before the frame takes a pipeline slot
  PN_ON_DEVICE(c);
  if (rate_pipe_prepare(r)) return -1;
  const PipeStaging st = {{r->io_in, r->io_in1}, {r->io_out, r->io_out1}, (size_t)c->B * r->n * pn_fmt_bytes(fmt)};
  RateFrame f = {r, fmt, active, ids, n};
  return pipe_submit(c, st, h_in, h_out, h_gr, rate_frame_body, &f);
}
extern "C" int pn_rate_submit_host_f32(pn_rate *r, const float *h_in, float *h_out, float *h_gr) { return rate_submit_host(r, h_in, h_out, h_gr, PN_FMT_F32, false, NULL, 0); }
extern "C" int pn_rate_submit_host_i16(pn_rate *r, const int16_t *h_in, int16_t *h_out, float *h_gr) { return rate_submit_host(r, h_in, h_out, h_gr, PN_FMT_I16, false, NULL, 0); }
extern "C" int pn_rate_submit_host_g711(pn_rate *r, const uint8_t *h_in, uint8_t *h_out, float *h_gr) { return rate_submit_host(r, h_in, h_out, h_gr, PN_FMT_G711, false, NULL, 0); }
extern "C" int pn_rate_submit_host_f32_active(pn_rate *r, const float *h_in, float *h_out, float *h_gr, const int32_t *ids, int n) { return rate_submit_host(r, h_in, h_out, h_gr, PN_FMT_F32, true, ids, n); }
extern "C" int pn_rate_submit_host_i16_active(pn_rate *r, const int16_t *h_in, int16_t *h_out, float *h_gr, const int32_t *ids, int n) { return rate_submit_host(r, h_in, h_out, h_gr, PN_FMT_I16, true, ids, n); }
extern "C" int pn_rate_submit_host_g711_active(pn_rate *r, const uint8_t *h_in, uint8_t *h_out, float *h_gr, const int32_t *ids, int n) { return rate_submit_host(r, h_in, h_out, h_gr, PN_FMT_G711, true, ids, n); }

// ---- timing the kernels --------------------------------------------------------------------------------------------------------
extern "C" int pn_rate_set_profiling(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (enable && r->event_pool.size() < 1408) {        // up to eleven scopes a frame (up, cng, up, plc, dtmf, clamp, agc, mix, lim, down, dtx): enough for 64 frames between two reads; created outside any timed region
    PN_ON_DEVICE(r->c);
    while (r->event_pool.size() < 1408) { hipEvent_t e; PN_HIP_CHECK(hipEventCreate(&e)); r->event_pool.push_back(e); }
  }
  r->profiling = enable != 0;
  return 0;
}
extern "C" int pn_rate_kernel_time(pn_rate *r, const char *name, double *total_ms, int64_t *launches) {
  if (!r || !name) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  if (rate_flush_events(r)) return -1;
  for (int i = 0; i < RF_COUNT; i++)
    if (!strcmp(name, kRateStage[i].family)) { if (total_ms) *total_ms = r->fam_ms[i]; if (launches) *launches = r->fam_n[i]; return 0; }
  pn_set_error("unknown converter kernel '%s' (rate_up, rate_down, rate_mix, rate_plc, rate_agc, rate_lim, rate_dtmf, rate_clamp, rate_cng, rate_dtx)", name);
  return -1;
}
extern "C" int pn_rate_reset_profile(pn_rate *r) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  if (rate_flush_events(r)) return -1;
  for (int i = 0; i < RF_COUNT; i++) { r->fam_ms[i] = 0; r->fam_n[i] = 0; }
  return 0;
}

// ---- state records -----------------------------------------------------------------------------------------------------------
// What the four host record calls ask of their arguments: -1 refused, 1 nothing to do (n == 0), 0 go on
static int host_records_args(const pn_rate *r, const int32_t *ids, int n, const void *h_records, bool distinct) {
  if (!r || n < 0 || (n > 0 && (!ids || !h_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 1;
  return pn_ids_check(r->c->B, ids, n, distinct) ? -1 : 0;
}
// ... and the four device ones, ahead of their list check
static int dev_records_args(const pn_rate *r, bool import, const int32_t *ids, int n, const void *d_records, const int32_t *d_status) {
  if (!r || n < 0 || (n > 0 && (!ids || !d_records || (import && !d_status)))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 1;
  if ((uintptr_t)d_records & 15) { pn_set_error("records must be 16-byte aligned"); return -1; }
  return 0;
}
// Host forms only: synchronous, through the context's host form of a record transfer (host_records_sync).
// rate: the records' rate — the converter's, or on a mixed one the rate the listed streams share (record_rate).
// An imported slot is now another stream: behind the scatter, what the state table clears on PN_RE_IMPORT starts fresh
static int rate_records_host(pn_rate *r, bool import, const int32_t *ids, int n, void *h_records) {
  if (int rc = host_records_args(r, ids, n, h_records, import)) return rc < 0 ? -1 : 0;
  pn_ctx *c = r->c;
  const int rate = r->mixed ? pn_rate_mixed_record_rate(r->rates.data(), ids, n) : r->rate;
  if (rate < 0) return -1;
  const int f = pn_rate_factor(rate);
  if (import && pn_records_check(h_records, n, 4 * pn_rate_record_words(f), [&](const void *rec, size_t b) { return pn_rate_record_check(rec, b, rate); })) return -1;
  return host_records_sync(c, import, h_records, (size_t)n * 4 * pn_rate_record_words(f), [&](void *d) {
    const int *d_ids = stage_ids(c, ids, n);
    if (!d_ids) return -1;
    pn_launch_rate_records(c->stream, f, rate, d_ids, n, stf(r, PN_RS_TAIL_UP), stf(r, PN_RS_TAIL_DOWN), r->td, d, import ? 1 : 0);
    if (import) { state_clear_rows(r, PN_RE_IMPORT, d_ids, n); cng_forget(r, ids, n); }
    if (hipGetLastError() != hipSuccess) { pn_set_error(import ? "record scatter launch failed" : "record gather launch failed"); return -1; }
    return 0;
  });
}
extern "C" int pn_rate_export_streams_host(pn_rate *r, const int32_t *ids, int n, void *h_records) { return rate_records_host(r, false, ids, n, h_records); }
extern "C" int pn_rate_import_streams_host(pn_rate *r, const int32_t *ids, int n, const void *h_records) { return rate_records_host(r, true, ids, n, const_cast<void *>(h_records)); }

// Device forms: asynchronous on the context's stream and ordered like pn_ctx_export_streams / pn_ctx_import_streams.  Records are
// pn_rate_record_stride(r) apart — on a mixed converter the largest record's size, which is what lets one call move streams of
// different rates: each record carries its own stream's rate, and the kernel takes rate and tail length per slot from the factor
// table.  Everything the host can judge is refused before anything is launched (pn_rate_mixed.h pn_rate_records_list_check).
static_assert(PN_RATE_STATE_MAX_BYTES == PN_RATE_STATE_HEADER_BYTES + 4 * (PN_RATE_UP_TAIL + 2 * PN_RATE_TAPS * PN_RATE_MAX_L) && PN_RATE_STATE_MAX_BYTES % 16 == 0,
              "the fixed stride is the 8000 Hz record, a whole number of 16-byte groups");
extern "C" size_t pn_rate_state_max_bytes(void) { return PN_RATE_STATE_MAX_BYTES; }
extern "C" size_t pn_rate_record_stride(const pn_rate *r) {
  if (!r) { pn_set_error("NULL argument"); return 0; }
  return r->mixed ? (size_t)PN_RATE_STATE_MAX_BYTES : 4 * pn_rate_record_words(r->f);
}
static int rate_records_dev(pn_rate *r, bool import, const int32_t *ids, int n, void *d_records, int32_t *d_status) {
  if (int rc = dev_records_args(r, import, ids, n, d_records, d_status)) return rc < 0 ? -1 : 0;
  pn_ctx *c = r->c;
  if (pn_rate_records_list_check(c->B, r->mixed ? r->rates.data() : NULL, ids, n, import)) return -1;
  PN_ON_DEVICE(c);
  const int *d = stage_ids(c, ids, n);
  if (!d) return -1;
  pn_launch_rate_records_dev(c->stream, d, n, r->mixed ? r->factors : NULL, r->f, stf(r, PN_RS_TAIL_UP), stf(r, PN_RS_TAIL_DOWN), r->td, d_records,
                             (int)(pn_rate_record_stride(r) / 4), d_status, import ? 1 : 0);
  if (import) { state_clear_rows(r, PN_RE_IMPORT, d, n); cng_forget(r, ids, n); }   // (whatever the record's status: the slot is another stream's now)
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
extern "C" int pn_rate_export_streams(pn_rate *r, const int32_t *ids, int n, void *d_records) { return rate_records_dev(r, false, ids, n, d_records, NULL); }
extern "C" int pn_rate_import_streams(pn_rate *r, const int32_t *ids, int n, const void *d_records, int32_t *d_status) {
  return rate_records_dev(r, true, ids, n, const_cast<void *>(d_records), d_status);
}

// ---- call-state records (include/percepnet_hip.h; layout and verdict pn_call_rules.h; the kernel pn_rate_call.hip) ----------------
// The second record of a stream: the PLC, AGC, limiter and level state, whatever its rate — the entries of the state table that have a
// section.  Nothing here allocates state: a section the converter does not hold is zero on export and dropped on import.  A section
// is held while its buffers exist; the concealer's, while the concealer is ON
static uint32_t call_held(const pn_rate *r) {
  uint32_t held = 0;
  for (int e = 0; e < PN_RS_COUNT; e++) if (r->st[e]) held |= pn_kRateState[e].call_bit;
  return r->plc ? held : held & ~(uint32_t)PN_CALL_PLC;
}
extern "C" size_t pn_rate_call_state_bytes(void) { return PN_RATE_CALL_STATE_BYTES; }
extern "C" int pn_rate_call_state_check(const void *record, size_t bytes) { return pn_call_record_check(record, bytes); }
extern "C" int pn_rate_call_state_sections(const pn_rate *r) { if (!r) { pn_set_error("NULL argument"); return -1; } return (int)call_held(r); }
// the launch alone: the caller is on the context's device and has checked ids, pointers and alignment
static int call_state_launch(pn_rate *r, bool import, const int32_t *ids, int n, void *d_records, int32_t *d_status) {
  const int *d = stage_ids(r->c, ids, n);
  if (!d) return -1;
  pn_launch_rate_call_state(r->c->stream, d, n, call_held(r), stf(r, PN_RS_PLC_HIST), stf(r, PN_RS_PLC_Q), r->st[PN_RS_PLC_META], r->st[PN_RS_AGC], r->st[PN_RS_LIM],
                            stf(r, PN_RS_LEVEL), d_records, d_status, import ? 1 : 0);
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
static int call_state_dev(pn_rate *r, bool import, const int32_t *ids, int n, void *d_records, int32_t *d_status) {
  if (int rc = dev_records_args(r, import, ids, n, d_records, d_status)) return rc < 0 ? -1 : 0;
  if (pn_ids_check(r->c->B, ids, n, import)) return -1;
  PN_ON_DEVICE(r->c);
  return call_state_launch(r, import, ids, n, d_records, d_status);
}
extern "C" int pn_rate_export_call_state(pn_rate *r, const int32_t *ids, int n, void *d_records) { return call_state_dev(r, false, ids, n, d_records, NULL); }
extern "C" int pn_rate_import_call_state(pn_rate *r, const int32_t *ids, int n, const void *d_records, int32_t *d_status) {
  return call_state_dev(r, true, ids, n, const_cast<void *>(d_records), d_status);
}
// Host forms: synchronous through host_records_sync, like the tails records'.  The import judges every record with the kernel's own
// verdict before anything is launched; the statuses the kernel then writes come back with the transfer and must all be PN_SS_OK.
extern "C" int pn_rate_export_call_state_host(pn_rate *r, const int32_t *ids, int n, void *h_records) {
  if (int rc = host_records_args(r, ids, n, h_records, false)) return rc < 0 ? -1 : 0;
  return host_records_sync(r->c, false, h_records, (size_t)n * PN_RATE_CALL_STATE_BYTES, [&](void *d) { return call_state_launch(r, false, ids, n, d, NULL); });
}
extern "C" int pn_rate_import_call_state_host(pn_rate *r, const int32_t *ids, int n, const void *h_records) {
  if (int rc = host_records_args(r, ids, n, h_records, true)) return rc < 0 ? -1 : 0;
  if (pn_records_check(h_records, n, PN_RATE_CALL_STATE_BYTES, [&](const void *rec, size_t b) { return pn_call_record_check(rec, b); })) return -1;
  const size_t bytes = (size_t)n * PN_RATE_CALL_STATE_BYTES;
  std::vector<int32_t> status(n, 0);
  int rc = host_records_sync(r->c, true, const_cast<void *>(h_records), bytes, [&](void *d) {
    return call_state_launch(r, true, ids, n, d, reinterpret_cast<int32_t *>(static_cast<char *>(d) + bytes)); }, status.data(), (size_t)n * sizeof(int32_t));
  for (int i = 0; i < n && !rc; i++)
    if (status[i]) { pn_set_error("record %d refused on the device (%d) after passing the host check", i, status[i]); rc = -1; }
  return rc;
}
