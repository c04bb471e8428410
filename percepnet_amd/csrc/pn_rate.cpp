// Host side of the batched rate converter (include/percepnet_hip.h "batched rate converter" and "mixed rates"): an object BESIDE a context, built
// like the feature generator — it borrows the context's device, batch size and HIP stream, and owns everything else: the two
// tap tables on the device, the per-stream tails of the two kernels (pn_rate.hip), the 48 kHz rows between the conversions and
// the staging rows of the host-buffer paths.  The pipelined path (pn_rate_submit_host_*) runs its frames through the CONTEXT's
// pipeline (pn_host_pipe.cpp pipe_submit) with the converter's own two staging pairs.  Nothing of it lives in pn_ctx, its state table or its records.  Every launch goes
// to the context's stream, so a converter call is ordered against the context's calls like they are against each other.
#include "pn_context.h"      // the context it borrows, the launchers, dev_alloc_into, stage_ids, the id rule, host_records_sync
#include "pn_rate_design.h"
#include "pn_rate_mixed.h"   // the mixed converter's host rules: the five rates, a rate change, one rate per record call
#include "pn_g711.h"         // the 8-bit sample format: the companding and what a list of laws must be
#include "pn_conf.h"         // conferences: what an id must be, the table after a change, the members in ascending order
#include "pn_mix_rules.h"    // loudest-N, send gains, hold: what the settings must be; the level and the selection for the host
#include "pn_plc_rules.h"    // packet-loss concealment: the signal rule for the host, the sizes of the state
#include "pn_agc_rules.h"    // automatic level control: the rule for the host, what parameters and targets must be
#include "pn_lim_rules.h"    // the output limiter: the rule for the host, what parameters and ceilings must be
#include "pn_call_rules.h"   // call-state records: the layout and the verdict
#include "pn_dtmf_rules.h"   // DTMF detection: the rule for the host, what parameters must be, the tables
#include "pn_dtmf_clamp_rules.h"   // DTMF removal: the rule for the host, what parameters must be, when a guard is in time
#include <string>
#include <vector>

enum { RF_UP, RF_DOWN, RF_MIX, RF_PLC, RF_AGC, RF_LIM, RF_DTMF, RF_CLAMP, RF_COUNT };   // the timed kernels (pn_rate_kernel_time), named by kRateFamily below
struct pn_rate {
  pn_ctx *c;                    // borrowed: device, B, stream, the id ring, the saturate setting
  int rate, f, n, td;           // rate_hz, its factor (pn_rate_design.h: L, or PN_RATE_F_3_2 for 32000), samples per row, words per down tail row (2D / M).  Mixed: 0, 0, 480, 192
  size_t bytes;
  float *taps_up, *taps_down;   // [2D + 1] h, g.  Mixed: the tables of L = 6, 3, 2 one behind the other, and behind them the g of 32000
  float *tail_up, *tail_down;   // [B][32], [B][td]: the state
  float *x48, *y48;             // [B][480]: the engine's input and output rows of a whole frame
  void *io_in, *io_out;         // [B][n] 4-byte words: staging rows of the host-buffer paths (slot 0 of the pipelined one)
  void *io_in1 = NULL, *io_out1 = NULL;   // slot 1 of the pipelined path: allocated by pn_rate_host_pipeline_prepare or the first submit
  float *io_gr;                 // [B][68]
  // a mixed converter (pn_rate_create_mixed): the rate of every stream as last set (host), its factor on the device — written
  // in stream order, so a frame submitted before a rate change still runs at the old rate — and a pinned landing place of the
  // host-buffer path's output rows, of which only the streams' own samples go on to the caller
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
  // one new state, a level per stream.  While every setting is at its default (mix_plain) rate_mix launches the plain kernel and
  // none of the device side is read; it is allocated by the first setting call that leaves the defaults, never inside a frame
  std::vector<float> gains;     // [B], 1.0f
  std::vector<int32_t> caps;    // [B] N_c by conference number, 0: everybody
  int gains_off = 0, caps_on = 0;          // how many gains are not 1.0f, how many caps not 0
  float hold = 0.0f;            // d
  bool mix_report = false;
  float *d_gains = NULL, *d_level = NULL;  // [B], [B]
  int *d_caps = NULL;                      // [B]
  void *d_mix_report = NULL;               // [B][PN_MIX_REPORT_WORDS] words
  // packet-loss concealment (pn_rate_set_plc; the rule pn_plc_rules.h): the state — history ring, period buffer and four meta words per
  // stream — exists from the first enable on, never allocated inside a frame.  Marks (pn_rate_set_lost): a stamp word per stream on
  // the device, == plc_tick where the stream is lost in the NEXT frame, written in stream order through the id ring; the host keeps
  // the same marks, which is how a frame knows whom to leave out of the up-conversion.  A frame consumes them: plc_tick moves on
  bool plc = false, plc_report = false;
  float *d_plc_hist = NULL, *d_plc_q = NULL;           // [B][1920], [B][720]
  void *d_plc_meta = NULL, *d_plc_report = NULL;      // [B][4] words each
  uint32_t *d_plc_lost = NULL, plc_tick = 1;          // [B]
  std::vector<uint8_t> lost_mark;                     // [B]
  std::vector<int32_t> lost_ids, up_ids;              // the marked streams; a frame's "advancing minus lost"
  // automatic level control (pn_rate_set_agc; the rule pn_agc_rules.h): SETTINGS — the switch, the converter's parameters, a target per
  // stream as last set (host) and on the device, written in stream order through the id ring like the send gains — and the state, four
  // words per stream.  The device side exists from the first enable on.  agc_on == 0: a frame launches nothing of it
  bool agc = false, agc_report = false;
  float agc_params[PN_AGC_N_PARAMS];
  std::vector<float> agc_targets;                     // [B], 0
  int agc_on = 0;                                     // streams whose target is not 0
  float *d_agc_targets = NULL;                        // [B]
  void *d_agc_state = NULL, *d_agc_report = NULL;     // [B][4] words each
  // the output limiter (pn_rate_set_stream_limiter; the rule pn_lim_rules.h): SETTINGS — the converter's parameters, a ceiling per stream
  // as last set (host) and on the device, written in stream order through the id ring like the AGC targets, the report switch — and the
  // state, four words per stream.  The device side exists from the first call that sets a ceiling on.  lim_on == 0: a frame launches nothing of it
  bool lim_report = false;
  float lim_params[PN_LIM_N_PARAMS];
  std::vector<float> lim_ceilings;                    // [B], 0
  int lim_on = 0;                                     // streams whose ceiling is not 0
  float *d_lim_ceilings = NULL;                       // [B]
  void *d_lim_state = NULL, *d_lim_report = NULL;     // [B][4] words each
  // DTMF detection (pn_rate_set_stream_dtmf; the rule pn_dtmf_rules.h): SETTINGS — the converter's parameters, a switch per stream as last
  // set (host) and as a word on the device, written in stream order through the id ring like the ceilings — and the state, 24 words per
  // stream.  The device side (with the twiddle tables) exists from the first enabling on.  dtmf_on == 0: a frame launches nothing of it
  bool dtmf_report = false;
  float dtmf_params[PN_DTMF_N_PARAMS];
  std::vector<uint8_t> dtmf_sw;                       // [B], 0
  int dtmf_on = 0;                                    // streams whose switch is on
  int *d_dtmf_on = NULL;                              // [B] words
  float *d_dtmf_tab = NULL;                           // ct [8][480], st [8][480]
  void *d_dtmf_state = NULL, *d_dtmf_report = NULL;   // [B][24] and [B][4] words
  // DTMF removal (pn_rate_set_stream_dtmf_clamp; the rule pn_dtmf_clamp_rules.h): SETTINGS — the converter's parameters, a switch per stream as
  // last set (host) and as a word on the device, written in stream order through the id ring like the detector's — and the state, four words
  // per stream.  The device side exists from the first enabling on, and with it d_dtmf_report: while clamp_on > 0 the detector writes its
  // report rows whether or not the user reads them (dtmf_report).  clamp_on == 0: a frame launches nothing of it
  bool clamp_report = false;
  int32_t clamp_params[PN_DTMF_CLAMP_N_PARAMS];
  std::vector<uint8_t> clamp_sw;                      // [B], 0
  int clamp_on = 0;                                   // streams whose switch is on
  int *d_clamp_on = NULL;                             // [B] words
  void *d_clamp_state = NULL, *d_clamp_report = NULL; // [B][4] words each
  std::vector<void *> allocs;
  // timing of the kernels (pn_rate_set_profiling): HIP events around their launches, like the context's families but owned
  // here; while it is off no event exists and none is recorded
  bool profiling = false;
  struct Ev { int fam; hipEvent_t a, b; };
  std::vector<Ev> events;
  std::vector<hipEvent_t> event_pool;
  double fam_ms[RF_COUNT] = {}; int64_t fam_n[RF_COUNT] = {};
};
static const char *const kRateFamily[RF_COUNT] = {"rate_up", "rate_down", "rate_mix", "rate_plc", "rate_agc", "rate_lim", "rate_dtmf", "rate_clamp"};
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
extern "C" int pn_rate_frame_samples(int rate_hz) {
  const int f = pn_rate_factor(rate_hz);
  if (!f) { pn_set_error("rate %d Hz: a converter takes " PN_RATE_TEXT, rate_hz); return -1; }
  return pn_rate_factor_frame(f);
}
extern "C" int pn_rate_delay_samples(int rate_hz) {
  const int f = pn_rate_factor(rate_hz);
  if (!f) { pn_set_error("rate %d Hz: a converter takes " PN_RATE_TEXT, rate_hz); return -1; }
  return pn_rate_factor_delay(f);                      // the engine's 2880 samples at the low rate, T up and T down
}
extern "C" int pn_rate_taps(int rate_hz, int down, float *taps, int cap) {
  const int f = pn_rate_factor(rate_hz);
  if (!f) { pn_set_error("rate %d Hz: a converter takes " PN_RATE_TEXT, rate_hz); return -1; }
  return pn_rate_design(f, down, taps, cap);
}
extern "C" size_t pn_rate_state_bytes(int rate_hz) {
  const int f = pn_rate_factor(rate_hz);
  if (!f) { pn_set_error("rate %d Hz: a converter takes " PN_RATE_TEXT, rate_hz); return 0; }
  return 4 * pn_rate_record_words(f);
}
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

extern "C" pn_rate *pn_rate_create(pn_ctx *c, int rate_hz) {
  if (!c) { pn_set_error("NULL argument"); return NULL; }
  const int f = pn_rate_factor(rate_hz);
  if (!f) { pn_set_error("rate %d Hz: a converter takes " PN_RATE_TEXT, rate_hz); return NULL; }
  DeviceGuard _dg(c->device);
  if (!_dg.ok) { pn_set_error("hipSetDevice(%d) failed", c->device); return NULL; }
  pn_rate *r = new pn_rate();
  r->c = c; r->rate = rate_hz; r->f = f; r->n = pn_rate_factor_frame(f); r->td = pn_rate_down_tail(f); r->bytes = 0;
  r->mixed = false; r->factors = NULL; r->h_rows = NULL; r->laws.assign((size_t)c->B, PN_G711_ULAW); r->confs.assign((size_t)c->B, PN_CONF_NONE);
  r->gains.assign((size_t)c->B, 1.0f); r->caps.assign((size_t)c->B, 0);
  r->agc_targets.assign((size_t)c->B, 0.0f); pn_agc_default_params_host(r->agc_params);
  r->lim_ceilings.assign((size_t)c->B, 0.0f); pn_lim_default_params_host(r->lim_params);
  r->dtmf_sw.assign((size_t)c->B, 0); pn_dtmf_default_params_host(r->dtmf_params);
  r->clamp_sw.assign((size_t)c->B, 0); pn_dtmf_clamp_default_params_host(r->clamp_params);
  const size_t B = (size_t)c->B, nt = 2 * (size_t)PN_RATE_TAPS * pn_rate_factor_L(f) + 1;
  float h[2][PN_RATE_MAX_TAPS];
  auto alloc = [&](void **p, size_t bytes, bool zero) { return dev_alloc_into(r->allocs, r->bytes, c->stream, p, bytes, zero); };
  if (pn_rate_design(f, 0, h[0], PN_RATE_MAX_TAPS) < 0 || pn_rate_design(f, 1, h[1], PN_RATE_MAX_TAPS) < 0) goto fail;
  if (alloc((void **)&r->taps_up, nt * 4, false) || alloc((void **)&r->taps_down, nt * 4, false) ||
      alloc((void **)&r->tail_up, B * PN_RATE_UP_TAIL * 4, true) || alloc((void **)&r->tail_down, B * r->td * 4, true) ||
      alloc((void **)&r->x48, B * PN_FRAME * 4, true) || alloc((void **)&r->y48, B * PN_FRAME * 4, true) ||
      alloc(&r->io_in, B * r->n * 4, false) || alloc(&r->io_out, B * r->n * 4, false) || alloc((void **)&r->io_gr, B * 68 * 4, false) ||
      alloc((void **)&r->d_laws, B * sizeof(int), true)) goto fail;
  // (synchronous copies: h is on this stack)
  if (hipMemcpyAsync(r->taps_up, h[0], nt * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(r->taps_down, h[1], nt * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); pn_set_error("rate converter init failed"); goto fail; }
  return r;
fail:
  pn_rate_destroy(r);
  return NULL;
}

// A converter with a rate per stream: the tap tables of all four filters, tails of the largest size for every stream (a rate
// change never reallocates), rows of 480 samples.
extern "C" pn_rate *pn_rate_create_mixed(pn_ctx *c, const int32_t *rates_hz) {
  if (!c) { pn_set_error("NULL argument"); return NULL; }
  if (rates_hz && pn_rate_mixed_rates_list_check(rates_hz, c->B)) return NULL;
  DeviceGuard _dg(c->device);
  if (!_dg.ok) { pn_set_error("hipSetDevice(%d) failed", c->device); return NULL; }
  pn_rate *r = new pn_rate();
  r->c = c; r->rate = 0; r->f = 0; r->n = PN_RATE_MIXED_ROW; r->td = pn_rate_down_tail(PN_RATE_MAX_L); r->bytes = 0;
  r->mixed = true; r->factors = NULL; r->h_rows = NULL; r->laws.assign((size_t)c->B, PN_G711_ULAW); r->confs.assign((size_t)c->B, PN_CONF_NONE);
  r->gains.assign((size_t)c->B, 1.0f); r->caps.assign((size_t)c->B, 0);
  r->agc_targets.assign((size_t)c->B, 0.0f); pn_agc_default_params_host(r->agc_params);
  r->lim_ceilings.assign((size_t)c->B, 0.0f); pn_lim_default_params_host(r->lim_params);
  r->dtmf_sw.assign((size_t)c->B, 0); pn_dtmf_default_params_host(r->dtmf_params);
  r->clamp_sw.assign((size_t)c->B, 0); pn_dtmf_clamp_default_params_host(r->clamp_params);
  const size_t B = (size_t)c->B;
  if (rates_hz) r->rates.assign(rates_hz, rates_hz + B); else r->rates.assign(B, 48000);
  static const int kF[4] = {6, 3, 2, PN_RATE_F_3_2};   // (the order of pn_rate.hip rt_taps_offset; the h of 32000 is the table of 3 and is not staged twice)
  std::vector<float> h[2];
  std::vector<int> f(B);
  for (size_t s = 0; s < B; s++) f[s] = pn_rate_mixed_factor(r->rates[s]);
  auto alloc = [&](void **p, size_t bytes, bool zero) { return dev_alloc_into(r->allocs, r->bytes, c->stream, p, bytes, zero); };
  for (int down = 0; down < 2; down++)
    for (int f : kF) {
      if (!down && f == PN_RATE_F_3_2) continue;
      float t[PN_RATE_MAX_TAPS];
      const int nt = pn_rate_design(f, down, t, PN_RATE_MAX_TAPS);
      if (nt < 0) goto fail;
      h[down].insert(h[down].end(), t, t + nt);
    }
  if (alloc((void **)&r->taps_up, h[0].size() * 4, false) || alloc((void **)&r->taps_down, h[1].size() * 4, false) ||
      alloc((void **)&r->tail_up, B * PN_RATE_UP_TAIL * 4, true) || alloc((void **)&r->tail_down, B * r->td * 4, true) ||
      alloc((void **)&r->x48, B * PN_FRAME * 4, true) || alloc((void **)&r->y48, B * PN_FRAME * 4, true) ||
      alloc(&r->io_in, B * r->n * 4, true) || alloc(&r->io_out, B * r->n * 4, true) || alloc((void **)&r->io_gr, B * 68 * 4, false) ||
      alloc((void **)&r->factors, B * sizeof(int), false) || alloc((void **)&r->d_laws, B * sizeof(int), true)) goto fail;
  if (hipHostMalloc(&r->h_rows, B * r->n * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); r->h_rows = NULL; pn_set_error("rate converter: no pinned memory for %zu bytes", B * r->n * 4); goto fail; }
  // (synchronous copies: the sources are locals)
  if (hipMemcpyAsync(r->taps_up, h[0].data(), h[0].size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(r->taps_down, h[1].data(), h[1].size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(r->factors, f.data(), B * sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); pn_set_error("rate converter init failed"); goto fail; }
  return r;
fail:
  pn_rate_destroy(r);
  return NULL;
}
extern "C" int pn_rate_is_mixed(const pn_rate *r) { if (!r) { pn_set_error("NULL argument"); return -1; } return r->mixed ? 1 : 0; }
extern "C" int pn_rate_row_samples(const pn_rate *r) { if (!r) { pn_set_error("NULL argument"); return -1; } return r->n; }
extern "C" int pn_rate_get_stream_rates(const pn_rate *r, int32_t *h_rates) {
  if (!r || !h_rates) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) h_rates[s] = r->mixed ? r->rates[s] : r->rate;
  return 0;
}
// the PLC state of the staged streams d[0..n) goes to zero: an empty history, no lag, no run (nothing while PLC was never enabled)
static void plc_zero_rows(pn_rate *r, const int *d, int n) {
  pn_launch_zero_rows(r->c->stream, r->d_plc_hist, PN_PLC_HIST, PN_PLC_HIST, 1, 0, d, n);
  pn_launch_zero_rows(r->c->stream, r->d_plc_q, PN_PLC_P_MAX, PN_PLC_P_MAX, 1, 0, d, n);
  pn_launch_zero_rows(r->c->stream, r->d_plc_meta, 4, 4, 1, 0, d, n);
}
// the AGC state of the staged streams d[0..n) goes to zero: no level, a fresh gain (nothing while AGC was never enabled)
static void agc_zero_rows(pn_rate *r, const int *d, int n) { pn_launch_zero_rows(r->c->stream, r->d_agc_state, 4, 4, 1, 0, d, n); }
// the limiter state of the staged streams d[0..n) goes to zero: a fresh gain, no hold (nothing while no ceiling was ever set)
static void lim_zero_rows(pn_rate *r, const int *d, int n) { pn_launch_zero_rows(r->c->stream, r->d_lim_state, 4, 4, 1, 0, d, n); }
// the detector state of the staged streams d[0..n) goes to zero: no half sums, no digit (nothing while no stream was ever enabled)
// ... and with it the removal state: no marks, no cut, no event (nothing while removal was never enabled)
static void dtmf_zero_rows(pn_rate *r, const int *d, int n) {
  pn_launch_zero_rows(r->c->stream, r->d_dtmf_state, PN_DTMF_STATE_WORDS, PN_DTMF_STATE_WORDS, 1, 0, d, n);
  pn_launch_zero_rows(r->c->stream, r->d_clamp_state, PN_DTMF_CLAMP_STATE_WORDS, PN_DTMF_CLAMP_STATE_WORDS, 1, 0, d, n);
}
// A rate change of the listed streams, asynchronous and ordered like pn_rate_reset_streams: the ids and the new factors go
// through the context's id ring in one copy, one launch writes the factors, two zero the tails.
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
  pn_launch_zero_rows(r->c->stream, r->tail_up, PN_RATE_UP_TAIL, PN_RATE_UP_TAIL, 1, 0, d, n);
  pn_launch_zero_rows(r->c->stream, r->tail_down, r->td, r->td, 1, 0, d, n);
  pn_launch_zero_rows(r->c->stream, r->d_level, 1, 1, 1, 0, d, n);       // (nothing while no level exists)
  plc_zero_rows(r, d, n);
  agc_zero_rows(r, d, n);
  lim_zero_rows(r, d, n);
  dtmf_zero_rows(r, d, n);
  PN_HIP_CHECK(hipGetLastError());
  for (int i = 0; i < n; i++) r->rates[ids[i]] = rates_hz[i];
  return 0;
}

// A law change of the listed streams (G.711 rows), asynchronous and ordered like a rate change: the ids and the new laws go through
// the context's id ring in one copy, one launch writes the table.  No tail is touched: the law is a setting of the edges.
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
extern "C" int pn_rate_get_stream_laws(const pn_rate *r, int32_t *h_laws) {
  if (!r || !h_laws) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) h_laws[s] = r->laws[s];
  return 0;
}

// A conference change of the listed streams, ordered like a law change.  Everything is decided on the host first (pn_conf.h
// pn_conf_change: the table after the change, the conferences it touches and their member rows); then the ids with their new
// conferences and the touched rows go through the context's id ring, in bounded pieces, each followed by the launch that reads it.
// No tail is touched.  The device side is allocated by the first call that needs it — here, never inside a frame.
static int conf_buffers(pn_rate *r) {                // (the caller is on the context's device)
  if (r->d_conf) return 0;
  pn_ctx *c = r->c;
  const size_t B = (size_t)c->B;
  float *o48 = NULL; int *conf = NULL, *members = NULL; uint32_t *stamp = NULL;
  auto alloc = [&](void **p, size_t bytes, bool zero) { return dev_alloc_into(r->allocs, r->bytes, c->stream, p, bytes, zero); };
  if (alloc((void **)&o48, B * PN_FRAME * 4, true) || alloc((void **)&conf, B * sizeof(int), false) ||
      alloc((void **)&members, B * PN_CONF_MAX_MEMBERS * sizeof(int), false) || alloc((void **)&stamp, B * sizeof(uint32_t), true)) return -1;
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
  for (int at = 0; at < n; at += 16384) {
    const int m = n - at < 16384 ? n - at : 16384;
    const int *d = stage_ids(r->c, ids + at, m, confs + at, m);
    if (!d) return -1;
    pn_launch_rate_set_factors(r->c->stream, d, d + ((m + 3) & ~3), m, r->d_conf);
    pn_launch_zero_rows(r->c->stream, r->d_level, 1, 1, 1, 0, d, m);     // a listed stream's level starts again
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
extern "C" int pn_rate_get_stream_confs(const pn_rate *r, int32_t *h_confs) {
  if (!r || !h_confs) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) h_confs[s] = r->confs[s];
  return 0;
}

// ---- loudest-N talkers, send gains, hold, mix report (include/percepnet_hip.h; rules pn_mix_rules.h) ---------------------------
// Settings, written in stream order through the context's id ring like the conference table, so a frame submitted before a call
// runs under the old values.  "plain": every setting at its default — rate_mix then launches what it always launched.
static bool mix_plain(const pn_rate *r) { return r->gains_off == 0 && r->caps_on == 0 && r->hold == 0.0f && !r->mix_report; }
static int mix_buffers(pn_rate *r) {                 // (the caller is on the context's device)
  if (conf_buffers(r)) return -1;
  if (r->d_level) return 0;
  pn_ctx *c = r->c;
  const size_t B = (size_t)c->B;
  float *gains = NULL, *level = NULL; int *caps = NULL;
  auto alloc = [&](void **p, size_t bytes, bool zero) { return dev_alloc_into(r->allocs, r->bytes, c->stream, p, bytes, zero); };
  if (alloc((void **)&gains, B * 4, false) || alloc((void **)&caps, B * sizeof(int), true) || alloc((void **)&level, B * 4, true)) return -1;
  PN_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)gains, 0x3f800000, B, c->stream));                  // 1.0f
  r->d_gains = gains; r->d_caps = caps; r->d_level = level;
  return 0;
}
// dst[ids[i]] = words[i] through the id ring, in bounded pieces, each followed by the launch that reads it
static int mix_set_words(pn_rate *r, const int32_t *ids, int n, const void *words, int *dst) {
  for (int at = 0; at < n; at += 16384) {
    const int m = n - at < 16384 ? n - at : 16384;
    const int *d = stage_ids(r->c, ids + at, m, static_cast<const int32_t *>(words) + at, m);
    if (!d) return -1;
    pn_launch_rate_set_factors(r->c->stream, d, d + ((m + 3) & ~3), m, dst);
  }
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
extern "C" int pn_rate_set_stream_mix_gains(pn_rate *r, const int32_t *ids, int n, const float *gains) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_mix_gains_set_check(r->c->B, ids, n, gains)) return -1;
  if (n == 0) return 0;
  std::vector<float> g(gains, gains + n);
  bool all_one = true;
  for (float &v : g) { if (v == 0.0f) v = 0.0f; all_one &= v == 1.0f; }     // (-0.0f is 0)
  if (!r->d_level && all_one) return 0;                                        // (nothing has ever left the defaults, and nothing does)
  PN_ON_DEVICE(r->c);
  if (mix_buffers(r) || mix_set_words(r, ids, n, g.data(), reinterpret_cast<int *>(r->d_gains))) return -1;
  for (int i = 0; i < n; i++) { r->gains_off += (g[i] != 1.0f) - (r->gains[ids[i]] != 1.0f); r->gains[ids[i]] = g[i]; }
  return 0;
}
extern "C" int pn_rate_get_stream_mix_gains(const pn_rate *r, float *h_gains) {
  if (!r || !h_gains) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) h_gains[s] = r->gains[s];
  return 0;
}
extern "C" int pn_rate_set_conf_speakers(pn_rate *r, const int32_t *confs, int n, const int32_t *max_speakers) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_mix_speakers_set_check(r->c->B, confs, n, max_speakers)) return -1;
  if (n == 0) return 0;
  bool all_zero = true;
  for (int i = 0; i < n; i++) all_zero &= max_speakers[i] == 0;
  if (!r->d_level && all_zero) return 0;
  PN_ON_DEVICE(r->c);
  if (mix_buffers(r) || mix_set_words(r, confs, n, max_speakers, r->d_caps)) return -1;
  for (int i = 0; i < n; i++) { r->caps_on += (max_speakers[i] != 0) - (r->caps[confs[i]] != 0); r->caps[confs[i]] = max_speakers[i]; }
  return 0;
}
extern "C" int pn_rate_get_conf_speakers(const pn_rate *r, int32_t *h_n) {
  if (!r || !h_n) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) h_n[s] = r->caps[s];
  return 0;
}
// the hold factor travels as an argument of every launch, so it is ordered like one; the levels go to zero in stream order
extern "C" int pn_rate_set_mix_hold(pn_rate *r, float d) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_mix_hold_check(d)) return -1;
  if (d == 0.0f) d = 0.0f;
  PN_ON_DEVICE(r->c);
  if (d != 0.0f && mix_buffers(r)) return -1;
  if (r->d_level) PN_HIP_CHECK(hipMemsetAsync(r->d_level, 0, (size_t)r->c->B * 4, r->c->stream));
  r->hold = d;
  return 0;
}
extern "C" float pn_rate_get_mix_hold(const pn_rate *r) { if (!r) { pn_set_error("NULL argument"); return NAN; } return r->hold; }
extern "C" int pn_rate_set_mix_report(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (enable && !r->d_mix_report) {
    PN_ON_DEVICE(r->c);
    if (mix_buffers(r) || dev_alloc_into(r->allocs, r->bytes, r->c->stream, &r->d_mix_report, (size_t)r->c->B * PN_MIX_REPORT_WORDS * 4, true)) return -1;
  }
  r->mix_report = enable != 0;
  return 0;
}
static int mix_report_copy(pn_rate *r, void *dst, hipMemcpyKind kind) {
  if (!r || !dst) { pn_set_error("NULL argument"); return -1; }
  if (!r->mix_report) { pn_set_error("the mix report is off (pn_rate_set_mix_report)"); return -1; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(dst, r->d_mix_report, (size_t)r->c->B * PN_MIX_REPORT_WORDS * 4, kind, r->c->stream));
  if (kind == hipMemcpyDeviceToHost) PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}
extern "C" int pn_rate_read_mix_report(pn_rate *r, void *h_report) { return mix_report_copy(r, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_mix_report_dev(pn_rate *r, void *d_report) { return mix_report_copy(r, d_report, hipMemcpyDeviceToDevice); }

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
  if (enable && !r->d_plc_meta) {
    pn_ctx *c = r->c;
    const size_t B = (size_t)c->B;
    float *hist = NULL, *q = NULL; void *meta = NULL; uint32_t *lost = NULL;
    auto alloc = [&](void **p, size_t bytes, bool zero) { return dev_alloc_into(r->allocs, r->bytes, c->stream, p, bytes, zero); };
    if (alloc((void **)&hist, B * PN_PLC_HIST * 4, true) || alloc((void **)&q, B * PN_PLC_P_MAX * 4, true) || alloc(&meta, B * 16, true) ||
        alloc((void **)&lost, B * sizeof(uint32_t), true)) return -1;
    r->lost_mark.assign(B, 0); r->lost_ids.reserve(B);
    r->d_plc_hist = hist; r->d_plc_q = q; r->d_plc_lost = lost; r->plc_tick = 1; r->d_plc_meta = meta;
    // room in the id ring for the longest list a frame stages, "every stream but the lost ones", so that no frame grows the ring:
    // the identity list goes through it once, read by nobody
    r->up_ids.resize(B);
    for (size_t s = 0; s < B; s++) r->up_ids[s] = (int32_t)s;
    if (!stage_ids(c, r->up_ids.data(), (int)B)) return -1;
    r->up_ids.clear();
  } else if (enable && !r->plc) {
    // on again after a pause: the frames in between are missing from the histories, so every stream starts with an empty one
    PN_HIP_CHECK(hipMemsetAsync(r->d_plc_hist, 0, (size_t)r->c->B * PN_PLC_HIST * 4, r->c->stream));
    PN_HIP_CHECK(hipMemsetAsync(r->d_plc_q, 0, (size_t)r->c->B * PN_PLC_P_MAX * 4, r->c->stream));
    PN_HIP_CHECK(hipMemsetAsync(r->d_plc_meta, 0, (size_t)r->c->B * 16, r->c->stream));
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
  for (int at = 0; at < n; at += 16384) {
    const int m = n - at < 16384 ? n - at : 16384;
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
extern "C" int pn_rate_set_plc_report(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (enable && !r->d_plc_report) {
    PN_ON_DEVICE(r->c);
    if (dev_alloc_into(r->allocs, r->bytes, r->c->stream, &r->d_plc_report, (size_t)r->c->B * PN_PLC_REPORT_WORDS * 4, true)) return -1;
  }
  r->plc_report = enable != 0;
  return 0;
}
static int plc_report_copy(pn_rate *r, void *dst, hipMemcpyKind kind) {
  if (!r || !dst) { pn_set_error("NULL argument"); return -1; }
  if (!r->plc_report) { pn_set_error("the PLC report is off (pn_rate_set_plc_report)"); return -1; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(dst, r->d_plc_report, (size_t)r->c->B * PN_PLC_REPORT_WORDS * 4, kind, r->c->stream));
  if (kind == hipMemcpyDeviceToHost) PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}
extern "C" int pn_rate_read_plc_report(pn_rate *r, void *h_report) { return plc_report_copy(r, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_plc_report_dev(pn_rate *r, void *d_report) { return plc_report_copy(r, d_report, hipMemcpyDeviceToDevice); }

// ---- automatic level control (include/percepnet_hip.h; the rule pn_agc_rules.h; the kernel pn_rate_agc.hip) -----------------------
extern "C" int pn_rate_set_agc(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  if (enable && !r->d_agc_state) {
    pn_ctx *c = r->c;
    const size_t B = (size_t)c->B;
    float *targets = NULL; void *state = NULL;
    auto alloc = [&](void **p, size_t bytes, bool zero) { return dev_alloc_into(r->allocs, r->bytes, c->stream, p, bytes, zero); };
    if (alloc((void **)&targets, B * 4, true) || alloc(&state, B * PN_AGC_STATE_BYTES, true)) return -1;
    r->d_agc_targets = targets; r->d_agc_state = state;
  } else if (enable && !r->agc) {
    // on again after a pause: the frames in between are missing from the levels, so every stream starts fresh
    PN_HIP_CHECK(hipMemsetAsync(r->d_agc_state, 0, (size_t)r->c->B * PN_AGC_STATE_BYTES, r->c->stream));
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
extern "C" int pn_rate_get_agc_params(const pn_rate *r, float *params8) {
  if (!r || !params8) { pn_set_error("NULL argument"); return -1; }
  memcpy(params8, r->agc_params, sizeof(r->agc_params));
  return 0;
}
extern "C" int pn_rate_set_stream_agc_targets(pn_rate *r, const int32_t *ids, int n, const float *targets) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (!r->agc) { pn_set_error("automatic level control is off (pn_rate_set_agc)"); return -1; }
  if (pn_agc_targets_set_check(r->c->B, ids, n, targets)) return -1;
  if (n == 0) return 0;
  std::vector<float> t(targets, targets + n);
  for (float &v : t) if (v == 0.0f) v = 0.0f;                                   // (-0.0f is 0)
  PN_ON_DEVICE(r->c);
  if (mix_set_words(r, ids, n, t.data(), reinterpret_cast<int *>(r->d_agc_targets))) return -1;
  for (int i = 0; i < n; i++) { r->agc_on += (t[i] != 0.0f) - (r->agc_targets[ids[i]] != 0.0f); r->agc_targets[ids[i]] = t[i]; }
  return 0;
}
extern "C" int pn_rate_get_stream_agc_targets(const pn_rate *r, float *h_targets) {
  if (!r || !h_targets) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) h_targets[s] = r->agc_targets[s];
  return 0;
}
extern "C" int pn_rate_set_agc_report(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (enable && !r->d_agc_report) {
    PN_ON_DEVICE(r->c);
    if (dev_alloc_into(r->allocs, r->bytes, r->c->stream, &r->d_agc_report, (size_t)r->c->B * PN_AGC_REPORT_WORDS * 4, true)) return -1;
  }
  r->agc_report = enable != 0;
  return 0;
}
static int agc_report_copy(pn_rate *r, void *dst, hipMemcpyKind kind) {
  if (!r || !dst) { pn_set_error("NULL argument"); return -1; }
  if (!r->agc_report) { pn_set_error("the AGC report is off (pn_rate_set_agc_report)"); return -1; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(dst, r->d_agc_report, (size_t)r->c->B * PN_AGC_REPORT_WORDS * 4, kind, r->c->stream));
  if (kind == hipMemcpyDeviceToHost) PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}
extern "C" int pn_rate_read_agc_report(pn_rate *r, void *h_report) { return agc_report_copy(r, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_agc_report_dev(pn_rate *r, void *d_report) { return agc_report_copy(r, d_report, hipMemcpyDeviceToDevice); }

// ---- the output limiter (include/percepnet_hip.h; the rule pn_lim_rules.h; the kernel pn_rate_lim.hip) ----------------------------
static int lim_buffers(pn_rate *r) {                 // (the caller is on the context's device)
  if (r->d_lim_state) return 0;
  pn_ctx *c = r->c;
  const size_t B = (size_t)c->B;
  float *ceilings = NULL; void *state = NULL;
  auto alloc = [&](void **p, size_t bytes, bool zero) { return dev_alloc_into(r->allocs, r->bytes, c->stream, p, bytes, zero); };
  if (alloc((void **)&ceilings, B * 4, true) || alloc(&state, B * PN_LIM_STATE_BYTES, true)) return -1;
  r->d_lim_ceilings = ceilings; r->d_lim_state = state;
  return 0;
}
extern "C" int pn_rate_set_stream_limiter(pn_rate *r, const int32_t *ids, int n, const float *ceilings) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_lim_ceilings_set_check(r->c->B, ids, n, ceilings)) return -1;
  if (n == 0) return 0;
  std::vector<float> v(ceilings, ceilings + n);
  bool all_zero = true;
  for (float &x : v) { if (x == 0.0f) x = 0.0f; all_zero &= x == 0.0f; }       // (-0.0f is 0)
  if (!r->d_lim_state && all_zero) return 0;                                     // (no ceiling has ever been set, and none is)
  PN_ON_DEVICE(r->c);
  if (lim_buffers(r) || mix_set_words(r, ids, n, v.data(), reinterpret_cast<int *>(r->d_lim_ceilings))) return -1;
  for (int i = 0; i < n; i++) { r->lim_on += (v[i] != 0.0f) - (r->lim_ceilings[ids[i]] != 0.0f); r->lim_ceilings[ids[i]] = v[i]; }
  return 0;
}
extern "C" int pn_rate_get_stream_limiter(const pn_rate *r, float *h_ceilings) {
  if (!r || !h_ceilings) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) h_ceilings[s] = r->lim_ceilings[s];
  return 0;
}
// the parameters travel as an argument of every launch, so a change is ordered like one
extern "C" int pn_rate_set_limiter_params(pn_rate *r, const float *params2) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_lim_params_check_host(params2)) return -1;
  memcpy(r->lim_params, params2, sizeof(r->lim_params));
  return 0;
}
extern "C" int pn_rate_get_limiter_params(const pn_rate *r, float *params2) {
  if (!r || !params2) { pn_set_error("NULL argument"); return -1; }
  memcpy(params2, r->lim_params, sizeof(r->lim_params));
  return 0;
}
extern "C" int pn_rate_set_limiter_report(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (enable && !r->d_lim_report) {
    PN_ON_DEVICE(r->c);
    if (dev_alloc_into(r->allocs, r->bytes, r->c->stream, &r->d_lim_report, (size_t)r->c->B * PN_LIM_REPORT_WORDS * 4, true)) return -1;
  }
  r->lim_report = enable != 0;
  return 0;
}
static int lim_report_copy(pn_rate *r, void *dst, hipMemcpyKind kind) {
  if (!r || !dst) { pn_set_error("NULL argument"); return -1; }
  if (!r->lim_report) { pn_set_error("the limiter report is off (pn_rate_set_limiter_report)"); return -1; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(dst, r->d_lim_report, (size_t)r->c->B * PN_LIM_REPORT_WORDS * 4, kind, r->c->stream));
  if (kind == hipMemcpyDeviceToHost) PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}
extern "C" int pn_rate_read_limiter_report(pn_rate *r, void *h_report) { return lim_report_copy(r, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_limiter_report_dev(pn_rate *r, void *d_report) { return lim_report_copy(r, d_report, hipMemcpyDeviceToDevice); }

// ---- DTMF detection (include/percepnet_hip.h; the rule pn_dtmf_rules.h; the kernel pn_rate_dtmf.hip) ------------------------------
static int dtmf_buffers(pn_rate *r) {                // (the caller is on the context's device)
  if (r->d_dtmf_state) return 0;
  pn_ctx *c = r->c;
  const size_t B = (size_t)c->B;
  const PnDtmfTables &T = pn_dtmf_tables_ref();
  int *on = NULL; float *tab = NULL; void *state = NULL;
  auto alloc = [&](void **p, size_t bytes, bool zero) { return dev_alloc_into(r->allocs, r->bytes, c->stream, p, bytes, zero); };
  if (alloc((void **)&on, B * 4, true) || alloc((void **)&tab, sizeof(T.ct) + sizeof(T.st), false) || alloc(&state, B * PN_DTMF_STATE_BYTES, true)) return -1;
  static_assert(offsetof(PnDtmfTables, st) == sizeof(T.ct), "ct and st are one block");
  PN_HIP_CHECK(hipMemcpyAsync(tab, T.ct, sizeof(T.ct) + sizeof(T.st), hipMemcpyHostToDevice, c->stream));   // (from a static table: the source outlives the copy)
  r->d_dtmf_on = on; r->d_dtmf_tab = tab; r->d_dtmf_state = state;
  return 0;
}
extern "C" int pn_rate_set_stream_dtmf(pn_rate *r, const int32_t *ids, int n, const uint8_t *on) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_on_set_check(r->c->B, ids, n, on)) return -1;
  if (n == 0) return 0;
  std::vector<int32_t> v(n), fresh;
  bool all_off = true;
  for (int i = 0; i < n; i++) { v[i] = on[i] ? 1 : 0; all_off &= !on[i]; if (on[i] && !r->dtmf_sw[ids[i]]) fresh.push_back(ids[i]); }
  if (!r->d_dtmf_state && all_off) return 0;                                     // (no stream has ever been enabled, and none is)
  PN_ON_DEVICE(r->c);
  if (dtmf_buffers(r)) return -1;
  for (size_t at = 0; at < fresh.size(); at += 16384) {                            // a stream that was off starts from the fresh state
    const int m = (int)(fresh.size() - at < 16384 ? fresh.size() - at : 16384);
    const int *d = stage_ids(r->c, fresh.data() + at, m);
    if (!d) return -1;
    pn_launch_zero_rows(r->c->stream, r->d_dtmf_state, PN_DTMF_STATE_WORDS, PN_DTMF_STATE_WORDS, 1, 0, d, m);
  }
  if (mix_set_words(r, ids, n, v.data(), r->d_dtmf_on)) return -1;
  for (int i = 0; i < n; i++) { r->dtmf_on += v[i] - (r->dtmf_sw[ids[i]] ? 1 : 0); r->dtmf_sw[ids[i]] = (uint8_t)v[i]; }
  return 0;
}
extern "C" int pn_rate_get_stream_dtmf(const pn_rate *r, uint8_t *h_on) {
  if (!r || !h_on) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) h_on[s] = r->dtmf_sw[s];
  return 0;
}
// the parameters travel as an argument of every launch, so a change is ordered like one
extern "C" int pn_rate_set_dtmf_params(pn_rate *r, const float *params7) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_params_check_host(params7)) return -1;
  // while removal is on for somebody its guard in front must stay in time
  if (r->clamp_on > 0 && pn_dtmf_clamp_params_check_host(r->clamp_params, (int)params7[PN_DTMF_ON_FRAMES])) return -1;
  memcpy(r->dtmf_params, params7, sizeof(r->dtmf_params));
  return 0;
}
extern "C" int pn_rate_get_dtmf_params(const pn_rate *r, float *params7) {
  if (!r || !params7) { pn_set_error("NULL argument"); return -1; }
  memcpy(params7, r->dtmf_params, sizeof(r->dtmf_params));
  return 0;
}
extern "C" int pn_rate_set_dtmf_report(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (enable && !r->d_dtmf_report) {
    PN_ON_DEVICE(r->c);
    if (dev_alloc_into(r->allocs, r->bytes, r->c->stream, &r->d_dtmf_report, (size_t)r->c->B * PN_DTMF_REPORT_WORDS * 4, true)) return -1;
  }
  r->dtmf_report = enable != 0;
  return 0;
}
static int dtmf_report_copy(pn_rate *r, void *dst, hipMemcpyKind kind) {
  if (!r || !dst) { pn_set_error("NULL argument"); return -1; }
  if (!r->dtmf_report) { pn_set_error("the DTMF report is off (pn_rate_set_dtmf_report)"); return -1; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(dst, r->d_dtmf_report, (size_t)r->c->B * PN_DTMF_REPORT_WORDS * 4, kind, r->c->stream));
  if (kind == hipMemcpyDeviceToHost) PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}
// the detector state of every stream to the host, synchronising (tests and debugging); zeros while no stream was ever enabled
extern "C" int pn_rate_debug_dtmf_state(pn_rate *r, void *h_state) {
  if (!r || !h_state) { pn_set_error("NULL argument"); return -1; }
  const size_t bytes = (size_t)r->c->B * PN_DTMF_STATE_BYTES;
  if (!r->d_dtmf_state) { memset(h_state, 0, bytes); return 0; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(h_state, r->d_dtmf_state, bytes, hipMemcpyDeviceToHost, r->c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}
extern "C" int pn_rate_read_dtmf_report(pn_rate *r, void *h_report) { return dtmf_report_copy(r, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_dtmf_report_dev(pn_rate *r, void *d_report) { return dtmf_report_copy(r, d_report, hipMemcpyDeviceToDevice); }

// ---- DTMF removal (include/percepnet_hip.h; the rule pn_dtmf_clamp_rules.h; the kernel pn_rate_dtmf_clamp.hip) ---------------------
static int clamp_buffers(pn_rate *r) {               // (the caller is on the context's device)
  if (r->d_clamp_state) return 0;
  pn_ctx *c = r->c;
  const size_t B = (size_t)c->B;
  int *on = NULL; void *state = NULL;
  auto alloc = [&](void **p, size_t bytes, bool zero) { return dev_alloc_into(r->allocs, r->bytes, c->stream, p, bytes, zero); };
  // the detector's report rows, which this stage reads: the user's buffer if there is one, otherwise one of the same kind
  if (!r->d_dtmf_report && alloc(&r->d_dtmf_report, B * PN_DTMF_REPORT_WORDS * 4, true)) return -1;
  if (alloc((void **)&on, B * 4, true) || alloc(&state, B * PN_DTMF_CLAMP_STATE_BYTES, true)) return -1;
  r->d_clamp_on = on; r->d_clamp_state = state;
  return 0;
}
extern "C" int pn_rate_set_stream_dtmf_clamp(pn_rate *r, const int32_t *ids, int n, const uint8_t *on) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_clamp_on_set_check(r->c->B, ids, n, on)) return -1;
  if (n == 0) return 0;
  std::vector<int32_t> v(n), fresh;
  bool all_off = true;
  for (int i = 0; i < n; i++) { v[i] = on[i] ? 1 : 0; all_off &= !on[i]; if (on[i] && !r->clamp_sw[ids[i]]) fresh.push_back(ids[i]); }
  if (!all_off && pn_dtmf_clamp_params_check_host(r->clamp_params, (int)r->dtmf_params[PN_DTMF_ON_FRAMES])) return -1;
  if (!r->d_clamp_state && all_off) return 0;                                    // (no stream has ever been enabled, and none is)
  PN_ON_DEVICE(r->c);
  if (clamp_buffers(r)) return -1;
  for (size_t at = 0; at < fresh.size(); at += 16384) {                            // a stream that was off starts from the fresh state
    const int m = (int)(fresh.size() - at < 16384 ? fresh.size() - at : 16384);
    const int *d = stage_ids(r->c, fresh.data() + at, m);
    if (!d) return -1;
    pn_launch_zero_rows(r->c->stream, r->d_clamp_state, PN_DTMF_CLAMP_STATE_WORDS, PN_DTMF_CLAMP_STATE_WORDS, 1, 0, d, m);
  }
  if (mix_set_words(r, ids, n, v.data(), r->d_clamp_on)) return -1;
  for (int i = 0; i < n; i++) { r->clamp_on += v[i] - (r->clamp_sw[ids[i]] ? 1 : 0); r->clamp_sw[ids[i]] = (uint8_t)v[i]; }
  return 0;
}
extern "C" int pn_rate_get_stream_dtmf_clamp(const pn_rate *r, uint8_t *h_on) {
  if (!r || !h_on) { pn_set_error("NULL argument"); return -1; }
  for (int s = 0; s < r->c->B; s++) h_on[s] = r->clamp_sw[s];
  return 0;
}
// the parameters travel as an argument of every launch, so a change is ordered like one
extern "C" int pn_rate_set_dtmf_clamp_params(pn_rate *r, const int32_t *params4) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_dtmf_clamp_params_check_host(params4, (int)r->dtmf_params[PN_DTMF_ON_FRAMES])) return -1;
  memcpy(r->clamp_params, params4, sizeof(r->clamp_params));
  return 0;
}
extern "C" int pn_rate_get_dtmf_clamp_params(const pn_rate *r, int32_t *params4) {
  if (!r || !params4) { pn_set_error("NULL argument"); return -1; }
  memcpy(params4, r->clamp_params, sizeof(r->clamp_params));
  return 0;
}
extern "C" int pn_rate_set_dtmf_clamp_report(pn_rate *r, int enable) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (enable && !r->d_clamp_report) {
    PN_ON_DEVICE(r->c);
    if (dev_alloc_into(r->allocs, r->bytes, r->c->stream, &r->d_clamp_report, (size_t)r->c->B * PN_DTMF_CLAMP_REPORT_WORDS * 4, true)) return -1;
  }
  r->clamp_report = enable != 0;
  return 0;
}
static int clamp_report_copy(pn_rate *r, void *dst, hipMemcpyKind kind) {
  if (!r || !dst) { pn_set_error("NULL argument"); return -1; }
  if (!r->clamp_report) { pn_set_error("the DTMF removal report is off (pn_rate_set_dtmf_clamp_report)"); return -1; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(dst, r->d_clamp_report, (size_t)r->c->B * PN_DTMF_CLAMP_REPORT_WORDS * 4, kind, r->c->stream));
  if (kind == hipMemcpyDeviceToHost) PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}
extern "C" int pn_rate_read_dtmf_clamp_report(pn_rate *r, void *h_report) { return clamp_report_copy(r, h_report, hipMemcpyDeviceToHost); }
extern "C" int pn_rate_read_dtmf_clamp_report_dev(pn_rate *r, void *d_report) { return clamp_report_copy(r, d_report, hipMemcpyDeviceToDevice); }
// the removal state of every stream to the host, synchronising (tests and debugging); zeros while no stream was ever enabled
extern "C" int pn_rate_debug_dtmf_clamp_state(pn_rate *r, void *h_state) {
  if (!r || !h_state) { pn_set_error("NULL argument"); return -1; }
  const size_t bytes = (size_t)r->c->B * PN_DTMF_CLAMP_STATE_BYTES;
  if (!r->d_clamp_state) { memset(h_state, 0, bytes); return 0; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemcpyAsync(h_state, r->d_clamp_state, bytes, hipMemcpyDeviceToHost, r->c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}
// TESTS ONLY: the detector's report rows — the user's buffer too — overwritten from the host, synchronising, so that the stand-alone stage
// can be run over hand-made rows; the next detector launch overwrites them again
extern "C" int pn_rate_debug_set_dtmf_report(pn_rate *r, const void *h_report) {
  if (!r || !h_report) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  if (clamp_buffers(r)) return -1;
  PN_HIP_CHECK(hipMemcpyAsync(r->d_dtmf_report, h_report, (size_t)r->c->B * PN_DTMF_REPORT_WORDS * 4, hipMemcpyHostToDevice, r->c->stream));
  PN_HIP_CHECK(hipStreamSynchronize(r->c->stream));
  return 0;
}

extern "C" int pn_rate_reset(pn_rate *r) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  PN_HIP_CHECK(hipMemsetAsync(r->tail_up, 0, (size_t)r->c->B * PN_RATE_UP_TAIL * 4, r->c->stream));
  PN_HIP_CHECK(hipMemsetAsync(r->tail_down, 0, (size_t)r->c->B * r->td * 4, r->c->stream));
  if (r->d_level) PN_HIP_CHECK(hipMemsetAsync(r->d_level, 0, (size_t)r->c->B * 4, r->c->stream));
  if (r->d_plc_meta) {
    PN_HIP_CHECK(hipMemsetAsync(r->d_plc_hist, 0, (size_t)r->c->B * PN_PLC_HIST * 4, r->c->stream));
    PN_HIP_CHECK(hipMemsetAsync(r->d_plc_q, 0, (size_t)r->c->B * PN_PLC_P_MAX * 4, r->c->stream));
    PN_HIP_CHECK(hipMemsetAsync(r->d_plc_meta, 0, (size_t)r->c->B * 16, r->c->stream));
  }
  if (r->d_agc_state) PN_HIP_CHECK(hipMemsetAsync(r->d_agc_state, 0, (size_t)r->c->B * PN_AGC_STATE_BYTES, r->c->stream));
  if (r->d_lim_state) PN_HIP_CHECK(hipMemsetAsync(r->d_lim_state, 0, (size_t)r->c->B * PN_LIM_STATE_BYTES, r->c->stream));
  if (r->d_dtmf_state) PN_HIP_CHECK(hipMemsetAsync(r->d_dtmf_state, 0, (size_t)r->c->B * PN_DTMF_STATE_BYTES, r->c->stream));
  if (r->d_clamp_state) PN_HIP_CHECK(hipMemsetAsync(r->d_clamp_state, 0, (size_t)r->c->B * PN_DTMF_CLAMP_STATE_BYTES, r->c->stream));
  return 0;
}

extern "C" int pn_rate_reset_streams(pn_rate *r, const int32_t *ids, int n) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (pn_ids_check(r->c->B, ids, n, false)) return -1;
  if (n == 0) return 0;
  PN_ON_DEVICE(r->c);
  const int *d = stage_ids(r->c, ids, n);
  if (!d) return -1;
  pn_launch_zero_rows(r->c->stream, r->tail_up, PN_RATE_UP_TAIL, PN_RATE_UP_TAIL, 1, 0, d, n);
  pn_launch_zero_rows(r->c->stream, r->tail_down, r->td, r->td, 1, 0, d, n);
  pn_launch_zero_rows(r->c->stream, r->d_level, 1, 1, 1, 0, d, n);
  plc_zero_rows(r, d, n);
  agc_zero_rows(r, d, n);
  lim_zero_rows(r, d, n);
  dtmf_zero_rows(r, d, n);
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
  if (r->mixed ? pn_launch_rate_up_mixed(r->c->stream, fmt, rows.n, rows.d_ids, r->factors, r->d_laws, d_in, d_out48, r->tail_up, r->taps_up)
               : pn_launch_rate_up(r->c->stream, r->f, fmt, rows.n, rows.d_ids, r->d_laws, d_in, d_out48, r->tail_up, r->taps_up)) return -1;
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
static int rate_down(pn_rate *r, const float *d_in48, void *d_out, int fmt, const RateRows &rows) {
  const int sat = r->c->saturate ? 1 : 0;
  RateScope sc(r, RF_DOWN);
  if (r->mixed ? pn_launch_rate_down_mixed(r->c->stream, fmt, rows.n, rows.d_ids, r->factors, r->d_laws, d_in48, d_out, sat, r->tail_down, r->taps_down)
               : pn_launch_rate_down(r->c->stream, r->f, fmt, rows.n, rows.d_ids, r->d_laws, d_in48, d_out, sat, r->tail_down, r->taps_down)) return -1;
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
                              r->d_level, r->hold, r->mix_report ? r->d_mix_report : NULL);
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
// the concealer over the rows, in place; it consumes the marks: the tick moves on, and the host's copy of them is cleared
static int rate_plc(pn_rate *r, float *d_x48, const RateRows &rows) {
  {
    RateScope sc(r, RF_PLC);
    pn_launch_rate_plc(r->c->stream, rows.n, rows.d_ids, r->d_plc_lost, r->plc_tick, d_x48, r->d_plc_hist, r->d_plc_q, r->d_plc_meta,
                       r->plc_report ? r->d_plc_report : NULL);
  }
  PN_HIP_CHECK(hipGetLastError());
  return plc_drop_marks(r);
}
// the level control over the rows, in place; d_lost / tick: the concealer's stamps and the tick it used for this frame (NULL: nobody is concealed)
static int rate_agc(pn_rate *r, float *d_y48, const RateRows &rows, const uint32_t *d_lost, uint32_t tick) {
  {
    RateScope sc(r, RF_AGC);
    pn_launch_rate_agc(r->c->stream, rows.n, rows.d_ids, r->d_agc_targets, d_lost, tick, r->agc_params, d_y48, r->d_agc_state,
                       r->agc_report ? r->d_agc_report : NULL);
  }
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
// the output limiter over the rows, in place on the rows the down-conversion reads next
static int rate_lim(pn_rate *r, float *d_o48, const RateRows &rows) {
  {
    RateScope sc(r, RF_LIM);
    pn_launch_rate_lim(r->c->stream, rows.n, rows.d_ids, r->d_lim_ceilings, r->lim_params, d_o48, r->d_lim_state, r->lim_report ? r->d_lim_report : NULL);
  }
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
// the DTMF detector over the rows, which it only reads; d_lost / tick as for the level control
static int rate_dtmf(pn_rate *r, const float *d_x48, const RateRows &rows, const uint32_t *d_lost, uint32_t tick) {
  {
    RateScope sc(r, RF_DTMF);
    pn_launch_rate_dtmf(r->c->stream, rows.n, rows.d_ids, r->d_dtmf_on, d_lost, tick, r->dtmf_params, pn_dtmf_tables_ref().rot, r->d_dtmf_tab, d_x48,
                        r->d_dtmf_state, r->dtmf_report || r->clamp_on > 0 ? r->d_dtmf_report : NULL);
  }
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
// DTMF removal over the rows, in place on y48; det: the detector ran in this frame (or the caller vouches for its report rows), otherwise
// every stream counts as "detection off"
static int rate_clamp(pn_rate *r, float *d_y48, const RateRows &rows, bool det) {
  {
    RateScope sc(r, RF_CLAMP);
    pn_launch_rate_dtmf_clamp(r->c->stream, rows.n, rows.d_ids, r->d_clamp_on, r->clamp_params, det ? r->d_dtmf_report : NULL, d_y48, r->d_clamp_state,
                              r->clamp_report ? r->d_clamp_report : NULL);
  }
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
static int rate_up_call(pn_rate *r, const void *d_in, int fmt, float *d_out48, const int32_t *ids, int n) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (rate_aligned(d_in, d_out48)) return -1;
  PN_ON_DEVICE(r->c);
  RateRows rows;
  if (rate_rows(r, ids, n, &rows)) return -1;
  return rate_up(r, d_in, fmt, d_out48, rows);
}
static int rate_down_call(pn_rate *r, const float *d_in48, void *d_out, int fmt, const int32_t *ids, int n) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (rate_aligned(d_in48, d_out)) return -1;
  PN_ON_DEVICE(r->c);
  RateRows rows;
  if (rate_rows(r, ids, n, &rows)) return -1;
  return rate_down(r, d_in48, d_out, fmt, rows);
}
extern "C" int pn_rate_up_f32(pn_rate *r, const float *d_in, float *d_out48, const int32_t *ids, int n_ids) { return rate_up_call(r, d_in, PN_FMT_F32, d_out48, ids, n_ids); }
extern "C" int pn_rate_up_i16(pn_rate *r, const int16_t *d_in, float *d_out48, const int32_t *ids, int n_ids) { return rate_up_call(r, d_in, PN_FMT_I16, d_out48, ids, n_ids); }
extern "C" int pn_rate_up_g711(pn_rate *r, const uint8_t *d_in, float *d_out48, const int32_t *ids, int n_ids) { return rate_up_call(r, d_in, PN_FMT_G711, d_out48, ids, n_ids); }
extern "C" int pn_rate_down_f32(pn_rate *r, const float *d_in48, float *d_out, const int32_t *ids, int n_ids) { return rate_down_call(r, d_in48, d_out, PN_FMT_F32, ids, n_ids); }
extern "C" int pn_rate_down_i16(pn_rate *r, const float *d_in48, int16_t *d_out, const int32_t *ids, int n_ids) { return rate_down_call(r, d_in48, d_out, PN_FMT_I16, ids, n_ids); }
extern "C" int pn_rate_down_g711(pn_rate *r, const float *d_in48, uint8_t *d_out, const int32_t *ids, int n_ids) { return rate_down_call(r, d_in48, d_out, PN_FMT_G711, ids, n_ids); }
extern "C" int pn_rate_mix_f32(pn_rate *r, const float *d_in48, float *d_out48, const int32_t *ids, int n_ids) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (rate_aligned(d_in48, d_out48)) return -1;
  const uintptr_t a = (uintptr_t)d_in48, b = (uintptr_t)d_out48, span = (uintptr_t)r->c->B * PN_FRAME * 4;
  if (a < b + span && b < a + span) { pn_set_error("the mix reads every member's row for every listener: its input and output rows must not overlap"); return -1; }
  PN_ON_DEVICE(r->c);
  RateRows rows;
  if (rate_rows(r, ids, n_ids, &rows)) return -1;
  return rate_mix(r, d_in48, d_out48, rows);
}
extern "C" int pn_rate_plc_f32(pn_rate *r, float *d_x48, const int32_t *ids, int n_ids) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (!r->plc) { pn_set_error("packet-loss concealment is off (pn_rate_set_plc)"); return -1; }
  if (rate_aligned(d_x48, d_x48)) return -1;
  PN_ON_DEVICE(r->c);
  RateRows rows;
  if (rate_rows(r, ids, n_ids, &rows)) return -1;
  return rate_plc(r, d_x48, rows);
}
extern "C" int pn_rate_agc_f32(pn_rate *r, float *d_y48, const int32_t *ids, int n_ids) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (!r->agc) { pn_set_error("automatic level control is off (pn_rate_set_agc)"); return -1; }
  if (rate_aligned(d_y48, d_y48)) return -1;
  PN_ON_DEVICE(r->c);
  RateRows rows;
  if (rate_rows(r, ids, n_ids, &rows)) return -1;
  return rate_agc(r, d_y48, rows, NULL, 0);
}
extern "C" int pn_rate_lim_f32(pn_rate *r, float *d_o48, const int32_t *ids, int n_ids) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (rate_aligned(d_o48, d_o48)) return -1;
  PN_ON_DEVICE(r->c);
  RateRows rows;
  if (rate_rows(r, ids, n_ids, &rows)) return -1;
  if (lim_buffers(r)) return -1;                     // (no ceiling was ever set: every stream is off, the state exists from here on)
  return rate_lim(r, d_o48, rows);
}
extern "C" int pn_rate_dtmf_f32(pn_rate *r, const float *d_x48, const int32_t *ids, int n_ids) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (rate_aligned(d_x48, d_x48)) return -1;
  PN_ON_DEVICE(r->c);
  RateRows rows;
  if (rate_rows(r, ids, n_ids, &rows)) return -1;
  if (dtmf_buffers(r)) return -1;                    // (no stream was ever enabled: every stream is off, the state exists from here on)
  return rate_dtmf(r, d_x48, rows, NULL, 0);
}

extern "C" int pn_rate_dtmf_clamp_f32(pn_rate *r, float *d_y48, const int32_t *ids, int n_ids) {
  if (!r) { pn_set_error("NULL argument"); return -1; }
  if (rate_aligned(d_y48, d_y48)) return -1;
  PN_ON_DEVICE(r->c);
  RateRows rows;
  if (rate_rows(r, ids, n_ids, &rows)) return -1;
  if (clamp_buffers(r)) return -1;                   // (no stream was ever enabled: every stream is off, the state exists from here on)
  return rate_clamp(r, d_y48, rows, true);
}

// ---- one whole frame -----------------------------------------------------------------------------------------------------------
// up into x48, while packet-loss concealment is on the concealer in place on x48, the engine's float frame from x48 into y48 (all streams, or the listed ones through the context's own active
// set), while automatic level control is on and a stream has a target the level control in place on y48, down from y48 — or, while a stream is in a conference, the mix from y48 into o48 and down from o48 — and in front of the down-conversion, while a stream has a ceiling, the output limiter in place on the rows it reads.  A frame the engine refuses returns -1 with its error kept; the up kernel has then advanced its tails
// and the down kernel has not, which is why the header asks for a reset of both objects before reuse.
// rate_frame: the launches alone — the caller is on the context's device and has checked the rows and, when active, the list
// (pn_ids_check, distinct), which is what lets the pipelined path refuse a list BEFORE the frame takes a pipeline slot.
static int rate_frame(pn_rate *r, const void *d_in, void *d_out, float *d_gr, int fmt, bool active, const int32_t *ids, int n) {
  pn_ctx *c = r->c;
  RateRows rows = {NULL, c->B};
  // marked streams: the up-conversion runs over "advancing minus lost" — its own staged list, in front of the frame's — so a lost
  // stream's input row is never read and its tail stays.  Nobody marked, or no marked stream advancing: the launch of always
  bool up_done = false;
  if (r->plc && !r->lost_ids.empty()) {
    r->up_ids.clear();
    if (active) { for (int i = 0; i < n; i++) if (!r->lost_mark[ids[i]]) r->up_ids.push_back(ids[i]); }
    else for (int s = 0; s < c->B; s++) if (!r->lost_mark[s]) r->up_ids.push_back(s);
    const int nu = (int)r->up_ids.size();
    if (nu != (active ? n : c->B)) {
      RateRows up = {NULL, nu};
      if (nu > 0 && !(up.d_ids = stage_ids(c, r->up_ids.data(), nu))) return -1;
      if (nu > 0 && rate_up(r, d_in, fmt, r->x48, up)) return -1;
      up_done = true;
    }
  }
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
  pn_ctx *c = r->c;
  const size_t bytes = (size_t)c->B * r->n * 4;
  // (a mixed converter's rows are zeroed like slot 0's, so that the part of an output row no kernel writes is never stale memory)
  if (!r->io_in1 && dev_alloc_into(r->allocs, r->bytes, c->stream, &r->io_in1, bytes, r->mixed)) return -1;
  if (!r->io_out1 && dev_alloc_into(r->allocs, r->bytes, c->stream, &r->io_out1, bytes, r->mixed)) return -1;
  return pn_host_pipeline_prepare(c);
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
  if (enable && r->event_pool.size() < 1024) {        // up to eight scopes a frame (up, plc, dtmf, clamp, agc, mix, lim, down): enough for 64 frames between two reads; created outside any timed region
    PN_ON_DEVICE(r->c);
    while (r->event_pool.size() < 1024) { hipEvent_t e; PN_HIP_CHECK(hipEventCreate(&e)); r->event_pool.push_back(e); }
  }
  r->profiling = enable != 0;
  return 0;
}
extern "C" int pn_rate_kernel_time(pn_rate *r, const char *name, double *total_ms, int64_t *launches) {
  if (!r || !name) { pn_set_error("NULL argument"); return -1; }
  PN_ON_DEVICE(r->c);
  if (rate_flush_events(r)) return -1;
  for (int i = 0; i < RF_COUNT; i++)
    if (!strcmp(name, kRateFamily[i])) { if (total_ms) *total_ms = r->fam_ms[i]; if (launches) *launches = r->fam_n[i]; return 0; }
  pn_set_error("unknown converter kernel '%s' (rate_up, rate_down, rate_mix, rate_plc, rate_agc, rate_lim, rate_dtmf, rate_clamp)", name);
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
// Host forms only: synchronous, through the context's host form of a record transfer (host_records_sync).
// rate: the records' rate — the converter's, or on a mixed one the rate the listed streams share (record_rate)
static int rate_records_host(pn_rate *r, int rate, bool import, const int32_t *ids, int n, void *h_records) {
  pn_ctx *c = r->c;
  const int f = pn_rate_factor(rate);
  return host_records_sync(c, import, h_records, (size_t)n * 4 * pn_rate_record_words(f), [&](void *d) {
    const int *d_ids = stage_ids(c, ids, n);
    if (!d_ids) return -1;
    pn_launch_rate_records(c->stream, f, rate, d_ids, n, r->tail_up, r->tail_down, r->td, d, import ? 1 : 0);
    if (import) { plc_zero_rows(r, d_ids, n); agc_zero_rows(r, d_ids, n); lim_zero_rows(r, d_ids, n); dtmf_zero_rows(r, d_ids, n); }   // the slot is now another stream: it starts with an empty history and fresh gains
    if (hipGetLastError() != hipSuccess) { pn_set_error(import ? "record scatter launch failed" : "record gather launch failed"); return -1; }
    return 0;
  });
}
static int record_rate(const pn_rate *r, const int32_t *ids, int n) { return r->mixed ? pn_rate_mixed_record_rate(r->rates.data(), ids, n) : r->rate; }
extern "C" int pn_rate_export_streams_host(pn_rate *r, const int32_t *ids, int n, void *h_records) {
  if (!r || n < 0 || (n > 0 && (!ids || !h_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if (pn_ids_check(r->c->B, ids, n, false)) return -1;
  const int rate = record_rate(r, ids, n);
  if (rate < 0) return -1;
  return rate_records_host(r, rate, false, ids, n, h_records);
}
extern "C" int pn_rate_import_streams_host(pn_rate *r, const int32_t *ids, int n, const void *h_records) {
  if (!r || n < 0 || (n > 0 && (!ids || !h_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if (pn_ids_check(r->c->B, ids, n, true)) return -1;
  const int rate = record_rate(r, ids, n);
  if (rate < 0) return -1;
  if (pn_records_check(h_records, n, 4 * pn_rate_record_words(pn_rate_factor(rate)), [&](const void *rec, size_t b) { return pn_rate_record_check(rec, b, rate); })) return -1;
  return rate_records_host(r, rate, true, ids, n, const_cast<void *>(h_records));
}

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
  if (!r || n < 0 || (n > 0 && (!ids || !d_records || (import && !d_status)))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if ((uintptr_t)d_records & 15) { pn_set_error("records must be 16-byte aligned"); return -1; }
  pn_ctx *c = r->c;
  if (pn_rate_records_list_check(c->B, r->mixed ? r->rates.data() : NULL, ids, n, import)) return -1;
  PN_ON_DEVICE(c);
  const int *d = stage_ids(c, ids, n);
  if (!d) return -1;
  pn_launch_rate_records_dev(c->stream, d, n, r->mixed ? r->factors : NULL, r->f, r->tail_up, r->tail_down, r->td, d_records,
                             (int)(pn_rate_record_stride(r) / 4), d_status, import ? 1 : 0);
  if (import) { plc_zero_rows(r, d, n); agc_zero_rows(r, d, n); lim_zero_rows(r, d, n); dtmf_zero_rows(r, d, n); }   // the slot is now another stream: it starts with an empty history and fresh gains, whatever its record's status
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
extern "C" int pn_rate_export_streams(pn_rate *r, const int32_t *ids, int n, void *d_records) { return rate_records_dev(r, false, ids, n, d_records, NULL); }
extern "C" int pn_rate_import_streams(pn_rate *r, const int32_t *ids, int n, const void *d_records, int32_t *d_status) {
  return rate_records_dev(r, true, ids, n, const_cast<void *>(d_records), d_status);
}

// ---- call-state records (include/percepnet_hip.h; layout and verdict pn_call_rules.h; the kernel pn_rate_call.hip) ----------------
// The second record of a stream: the PLC, AGC, limiter and level state, whatever its rate.  Nothing here allocates state: a section
// the converter does not hold is zero on export and dropped on import.
static uint32_t call_held(const pn_rate *r) {
  return (r->plc ? PN_CALL_PLC : 0u) | (r->d_agc_state ? PN_CALL_AGC : 0u) | (r->d_lim_state ? PN_CALL_LIM : 0u) | (r->d_level ? PN_CALL_MIX : 0u);
}
extern "C" size_t pn_rate_call_state_bytes(void) { return PN_RATE_CALL_STATE_BYTES; }
extern "C" int pn_rate_call_state_check(const void *record, size_t bytes) { return pn_call_record_check(record, bytes); }
extern "C" int pn_rate_call_state_sections(const pn_rate *r) { if (!r) { pn_set_error("NULL argument"); return -1; } return (int)call_held(r); }
// the launch alone: the caller is on the context's device and has checked ids, pointers and alignment
static int call_state_launch(pn_rate *r, bool import, const int32_t *ids, int n, void *d_records, int32_t *d_status) {
  const int *d = stage_ids(r->c, ids, n);
  if (!d) return -1;
  pn_launch_rate_call_state(r->c->stream, d, n, call_held(r), r->d_plc_hist, r->d_plc_q, r->d_plc_meta, r->d_agc_state, r->d_lim_state, r->d_level, d_records,
                            d_status, import ? 1 : 0);
  PN_HIP_CHECK(hipGetLastError());
  return 0;
}
static int call_state_dev(pn_rate *r, bool import, const int32_t *ids, int n, void *d_records, int32_t *d_status) {
  if (!r || n < 0 || (n > 0 && (!ids || !d_records || (import && !d_status)))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if ((uintptr_t)d_records & 15) { pn_set_error("records must be 16-byte aligned"); return -1; }
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
  if (!r || n < 0 || (n > 0 && (!ids || !h_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if (pn_ids_check(r->c->B, ids, n, false)) return -1;
  return host_records_sync(r->c, false, h_records, (size_t)n * PN_RATE_CALL_STATE_BYTES, [&](void *d) { return call_state_launch(r, false, ids, n, d, NULL); });
}
extern "C" int pn_rate_import_call_state_host(pn_rate *r, const int32_t *ids, int n, const void *h_records) {
  if (!r || n < 0 || (n > 0 && (!ids || !h_records))) { pn_set_error("bad argument"); return -1; }
  if (n == 0) return 0;
  if (pn_ids_check(r->c->B, ids, n, true)) return -1;
  if (pn_records_check(h_records, n, PN_RATE_CALL_STATE_BYTES, [&](const void *rec, size_t b) { return pn_call_record_check(rec, b); })) return -1;
  const size_t bytes = (size_t)n * PN_RATE_CALL_STATE_BYTES;
  std::vector<int32_t> status(n, 0);
  int rc = host_records_sync(r->c, true, const_cast<void *>(h_records), bytes, [&](void *d) {
    return call_state_launch(r, true, ids, n, d, reinterpret_cast<int32_t *>(static_cast<char *>(d) + bytes)); }, status.data(), (size_t)n * sizeof(int32_t));
  for (int i = 0; i < n && !rc; i++)
    if (status[i]) { pn_set_error("record %d refused on the device (%d) after passing the host check", i, status[i]); rc = -1; }
  return rc;
}
