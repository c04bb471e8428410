// percepnet_run — the reference's `percepNet_run <noisy.pcm> <out.pcm>` CLI (src/main.cpp:11-44) on
// top of libpercepnet_hip's batched C-ABI, extended to N file pairs processed as N concurrent
// streams on one or several GPUs.  Same I/O contract per stream: raw little-endian int16
// mono 48 kHz in; (frames-1)*480 samples out (first output frame dropped, main.cpp:37; partial tail frame
// dropped, main.cpp:32-33); with a single pair ./feature_test.raw gets 68 floats per frame.
//
//   percepnet_run [--model model.pnw] [--strict | --x3] [--postfilter] [--atten-lim DB] [--saturate] [--report] [--slots N]
//                 [--rate 8000|16000|24000|32000 | --rates R0,R1,..] [--g711 ulaw|alaw] [--conference C0,C1,.. [--conf-speakers N] [--mix-gains G0,G1,..]] [--plc [--lose P:F0-F1,P:F,..]] [--dtx P:F0-F1,P:F,.. [--sid L[:N1:..:NM]]] [--agc RMS [--agc-max-gain G]] [--limiter CEIL [--limiter-hold H]] [--dtmf [--dtmf-on-frames N]] [--dtmf-clamp [--dtmf-guard PRE,POST]] [--dtx-send [--dtx-send-hangover H]] [--migrate-at F] [--device N | --devices 0,1,..|all] [--no-numa] [--verbose]
//                 in0.pcm out0.pcm [in1.pcm out1.pcm ...]
//
// --rate R: the files are raw int16 at R Hz instead of 48 kHz, in frames of n = 480 * R / 48000 samples (80 | 160 | 240 | 320): a rate
// converter beside each context (pn_rate) takes every frame up to 48 kHz in front of the engine and back down behind it.  The
// per-stream contract is unchanged: (frames-1)*n samples out, first output frame and partial tail dropped.  The frames go through
// the converter's pipelined path (pn_rate_submit_host_i16: the context's pipeline with the converter's frame in the middle) with
// the same rotation of three pinned buffer sets as the 48 kHz path, --report gets each frame's records through
// pn_host_next_report — its figures stay those of the 48 kHz signal inside the engine — and the converter's slots are reset
// with the context's.  Without --rate nothing of this runs.
//
// --rates R0,R1,..: one rate per pair out of 8000, 16000, 24000, 32000 and 48000 (exclusive with --rate): a MIXED converter beside each
// context (pn_rate_create_mixed), whose shard's slice of the list goes to its device.  Pair i is read and written in frames of
// its own n = 480 * Ri / 48000 samples; the pinned rows are 480 samples whatever the rate (only a pair's own n samples of an
// output row are written to its file: the rest of the row is unspecified on the pipelined path); the per-pair contract is the one
// above.  With --slots a slot taken over by a pair of another rate continues at that rate (pn_rate_set_stream_rates for the
// restart list, where --rate calls pn_rate_reset_streams), followed by the context's reset as always.
//
// --g711 ulaw|alaw (needs --rate or --rates; on its own it is refused with the usage text): the files are raw G.711 bytes, one per
// sample, mu-law or A-law, read and written in frames of the pair's own size; the frames go through pn_rate_submit_host_g711 (the
// converter's 8-bit rows: decode in front of the up-conversion, encode behind the down-conversion's int16 cast).  One law covers
// all pairs; it is a setting of the converter's slots, set once, which slot resets and rate changes keep.  The rest of the
// contract is unchanged: first output frame and partial tail dropped, --slots, --saturate (which a G.711 caller wants: a clipped
// sample otherwise wraps before it is encoded), --report.
//
// --conference C0,C1,..: one entry per pair, a conference number in [0, pairs) or `-` for none: output file i holds what participant
// i HEARS — the sum of the other members' enhanced signals (pn_rate_set_stream_confs: the mix between the engine and the
// down-conversion, at 48 kHz, whatever the members' rates and codings) — and a pair marked `-` gets its own enhanced signal as
// always.  It needs a converter: with --rate or --rates it uses theirs, alone it makes a mixed converter of all 48000 (the files
// are then int16 at 48 kHz).  It combines with --g711 and --saturate (which a conference wants: a sum of voices clips where one
// voice does not).  The frames go through pn_rate_submit_host_*_active with the list of the pairs that still have input: a pair
// whose input has ended is no longer listed, so it contributes nothing instead of silence-through-the-engine, and its file is
// complete.  Refused with --slots (a conference's members play from the start, side by side) and with more than one device (a
// conference lives in one context).  --report stays about each pair's OWN output before the mix.
// --conf-speakers N: every conference mixes its N loudest talkers only (pn_rate_set_conf_speakers; 0 = everybody, up to 32);
// --mix-gains G0,G1,..: one send gain per pair (pn_rate_set_stream_mix_gains; 0 mutes the pair, which still hears).  Both need
// --conference and are refused without it.
// --plc: packet-loss concealment on the converter (pn_rate_set_plc): with --rate or --rates it uses theirs, alone it makes a mixed
// converter of all 48000, as --conference does.  --lose P:F0-F1,P:F,..: pair P (counted over the whole command line, from 0) loses its
// frames F0..F1 (or the one frame F; a pair's frames count from 0): the frame is still READ from the pair's input and discarded, so the
// files stay aligned, and pn_rate_set_lost marks the pair's slot in front of that frame's submit.  --lose without --plc is refused.
// --dtx P:F0-F1,P:F,..: comfort noise on the converter (pn_rate_set_cng), with the syntax of --lose: pair P is SILENT on its frames F0..F1 — the
// frame is still read from the pair's input and discarded, pn_rate_set_silent marks the pair's slot in front of that frame's submit, and the
// row the engine sees is the noise of the pair's silence descriptor.  --sid L[:N1:..:NM]: that descriptor for every pair, the level L in
// -dBov (0..127) and up to 12 quantised reflection coefficients (0..254) (pn_rate_set_stream_sid; default: level only, 60); it needs --dtx.
// With --rate or --rates it uses their converter, alone it makes a mixed converter of all 48000, as --plc does; with --plc a frame that is
// both lost and silent is concealed; with --migrate-at the noise starts again behind the move: no record carries its state.
// --agc RMS: automatic level control on the converter (pn_rate_set_agc): every pair's enhanced signal is levelled towards the linear RMS
// target RMS in (0, 1] (parsed with strtof; pn_rate_set_stream_agc_targets for every slot, once: a slot reset starts the slot's level
// again and keeps its target), in front of the mix where there is one.  With --rate or --rates it uses their converter, alone it makes a
// mixed converter of all 48000, as --plc does.  --agc-max-gain G: the largest gain, in [1, 1024] (parameter PN_AGC_MAX_GAIN; default 16);
// it needs --agc.
// --limiter CEIL: the output limiter on the converter (pn_rate_set_stream_limiter): every pair's output — its conference's mix where it is
// in one — stays under the linear ceiling CEIL in [1/1024, 1] (parsed with strtof; set for every slot, once: a slot reset starts the
// slot's gain again and keeps its ceiling).  With --rate or --rates it uses their converter, alone it makes a mixed converter of all
// 48000, as --agc does.  --limiter-hold H: the frames the gain is held after an attack, a whole number in [0, 1000] (parameter
// PN_LIM_HOLD; default 2); it needs --limiter.
// --dtmf: in-band DTMF detection on the converter (pn_rate_set_stream_dtmf for every slot, once: a slot reset starts the slot's detector
// again and keeps its switch): one line "dtmf: pair P frame F digit D" on stdout for every digit that BEGINs, P counted over the whole
// command line and F over the pair's frames, both from 0.  The audio is untouched.  The DTMF report is not part of the pipelined
// path's report, so the run reads it (pn_rate_read_dtmf_report, synchronising) behind every submit: with --dtmf a frame's GPU work no
// longer overlaps the next frame's file reads.  With --rate or --rates it uses their converter, alone it makes a mixed converter of all
// 48000, as --agc does.  --dtmf-on-frames N: the hits in a row that begin a digit, a whole number in [1, 100] (parameter
// PN_DTMF_ON_FRAMES; default 3); it needs --dtmf.  With --migrate-at a digit in flight at the move is reported again: no record carries
// the detector's state.
// --dtmf-clamp (needs --dtmf): DTMF removal on every slot (pn_rate_set_stream_dtmf_clamp, once, like --dtmf): a detected digit is muted in
// the pair's enhanced audio, with a fade in front and behind, at no added delay; one line "dtmf-event: pair P frame F event N end E
// duration D" on stdout for every frame that carries an ENDED RFC 4733 event (N the event code 0..15, E its end bit, D its duration in
// units of an 8 kHz RTP clock), read behind every submit like the digits.  F is the frame of the INPUT: the audio it describes leaves six
// frames later.  --dtmf-guard PRE,POST: the rows removed in front of and behind a digit's marked rows, whole numbers in [0, 4] and
// [0, 8] (parameters PN_DTMF_CLAMP_PRE and PN_DTMF_CLAMP_POST; default 1,0); it needs --dtmf-clamp, and on_frames + PRE must be <= 5.
// --dtx-send: the DTX send side on the converter (pn_rate_set_stream_dtx for every slot, once: a slot reset starts the slot's detector
// again and keeps its switch): behind the run one line "dtx-send: pair P frame F sid S none N last-sid M:L:N1:..:NM" on stdout for every
// pair — how many of its frames the stage decided to send, to replace by a SID, to leave out, and the last SID it emitted ("-": none).
// The audio is untouched and every frame is still written to the output file: the decisions are what a sender would act on.  Like the
// DTMF report, the DTX report is not part of the pipelined path's report, so the run reads it (pn_rate_read_dtx_report, synchronising)
// behind every submit: with --dtx-send a frame's GPU work no longer overlaps the next frame's file reads.  With --rate or --rates it
// uses their converter, alone it makes a mixed converter of all 48000, as --agc does.  --dtx-send-hangover H: the frames sent behind the
// last active one, a whole number in [0, 255] (parameter PN_DTX_HANGOVER; default 20); it needs --dtx-send.  With --migrate-at every
// pair starts again in VOICE on the target and relearns its floor: no record carries the stage's state.
// --migrate-at F (needs a converter — --rate, --rates or an option that makes one — and one device): when frame F (the shard's frames
// count from 0) has been delivered, the run builds a SECOND context and converter with the same settings, moves every slot there with
// all three record kinds in the mover's order of include/percepnet_hip.h "call-state records" (the engine's, the converter's tails,
// the call state), destroys the first pair and goes on: what a caller does who rebalances live calls.  The output files are byte for
// byte those of the run without the option.
//
// --atten-lim DB: every stream takes out at most DB dB of noise (pn_ctx_set_atten_limit; 0 = the input, delayed; default: no
// limit).  A slot reset clears a stream's limit (a reset slot is a new call), so the limit is set again on every reset slot.
//
// --saturate: the int16 output saturates at +-full scale instead of wrapping like main.cpp:36 (pn_ctx_set_output_saturate).
// --report: one line per pair on stdout when its output file is complete (pn_ctx_set_report): the frames written, how many of
// their samples left the int16 range, the largest |sample| before the cast, and 10 log10(output energy / input energy) over
// those frames (the input delayed like the output).  Both are settings of the context: a slot reset leaves them on, so unlike
// --atten-lim they need no setting again on a reused slot; the per-pair sums start over with every pair.
//
// --slots N: at most N concurrent streams per device; further pairs wait and take over the slot of a pair that has ended
// (per-stream re-initialisation on the device, pn_ctx_reset_streams) — a directory of recordings of different lengths goes
// through a fixed-size context without padding the short ones with silence.
//
// Multi-GPU: streams are independent, so the pairs are cut into contiguous balanced shards, one per
// device; every device gets its own host thread, its own context (a replica of the weights and tables) and its own
// pinned buffers, and the threads never talk to each other — the one-process counterpart of the reference's shell
// fan-out (utils/run.sh:49,65,99).  No collective is involved.  Each device's thread binds itself to the CPUs of that GPU's NUMA
// node before it creates its context and pinned buffers (pn_bind_thread_to_device_numa; --no-numa leaves the affinity alone,
// --verbose prints the binding).
#include "../../include/percepnet_hip.h"
#include "pn_cli_util.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>

extern const RNNModel percepnet_model_orig __attribute__((weak));

struct Shard { int device, first, count, rc; std::string err; };

// Everything a shard holds; released on every exit path of run_shard.
struct ShardRes {
  pn_ctx *cx = NULL;
  pn_rate *rt = NULL;                   // --rate: the converter beside cx (destroyed before it)
  std::vector<FILE *> fin, fout;        // per SLOT: the pair currently playing there
  FILE *ftap = NULL;
  // one of three rotating pinned buffer sets; file[s] = the output file the frame of slot s belongs to (NULL: slot idle),
  // skip[s] = that frame is the pair's first output frame, which main.cpp:37 drops
  // (--report) rep: the frame's report records, pair[s]: the pair the frame of slot s belongs to
  // fs[s]: samples of that frame (the pair's own frame size; differs between slots only with --rates)
  struct Slot { char *in = NULL, *out = NULL; float *gr = NULL; uint32_t *rep = NULL; std::vector<FILE *> file; std::vector<char> skip, last; std::vector<int> pair; std::vector<size_t> fs; } slot[3];
  ~ShardRes() {
    for (auto &sl : slot) { pn_host_free(sl.in); pn_host_free(sl.out); pn_host_free(sl.gr); pn_host_free(sl.rep); }
    for (FILE *f : fin) if (f) fclose(f);
    for (FILE *f : fout) if (f) fclose(f);
    if (ftap) fclose(ftap);
    pn_rate_destroy(rt);
    pn_ctx_destroy(cx);
  }
};

// One device: pairs [first, first+count) of argv-style (in, out) paths through `n_slots` concurrent streams (n_slots =
// count: every pair has its own stream from the start, the round-1 behaviour).  With fewer slots than pairs the shard is a
// queue: when the pair playing in a slot runs out of input, the slot is re-initialised on the device
// (pn_ctx_reset_streams = rnnoise_destroy + rnnoise_create of the reference, denoise.cpp:252-280,326-331) and the next
// waiting pair starts there on the following frame, while the other slots keep running.
static bool g_numa = true, g_verbose = false;
static float g_atten_lim = INFINITY;                  // --atten-lim: dB for every stream (inf: not set)
static bool g_saturate = false, g_report = false;     // --saturate, --report
static int g_rate = 0;                                // --rate: the files' sample rate (0: 48 kHz, no converter)
static std::vector<int32_t> g_rates;                  // --rates: one rate per pair (empty: not given), a mixed converter
static int g_g711 = -1;                               // --g711: the law of every pair's files (PN_G711_*; -1: linear int16)
static std::vector<int32_t> g_confs;                  // --conference: one conference per pair (empty: not given; PN_CONF_NONE for `-`)
static int g_conf_speakers = -1;                      // --conf-speakers: N of every conference (-1: not given)
static std::vector<float> g_mix_gains;                // --mix-gains: one send gain per pair (empty: not given)
static bool g_plc = false;                            // --plc: packet-loss concealment on the converter
struct LoseRange { long pair, f0, f1; };
static std::vector<LoseRange> g_lose;                 // --lose: pair, first and last lost frame of the pair
static std::vector<LoseRange> g_dtx;                  // --dtx: pair, first and last silent frame of the pair; not empty: comfort noise is on
static uint8_t g_sid[PN_CNG_SID_BYTES];               // --sid: every pair's silence descriptor
static bool g_sid_given = false;
static float g_agc = 0.0f, g_agc_max_gain = 0.0f;     // --agc: every pair's target RMS (0: not given); --agc-max-gain (0: not given)
static bool g_dtmf = false;                            // --dtmf: detection on every pair
static float g_dtmf_on_frames = 0.0f;                  // --dtmf-on-frames (0: not given)
static bool g_dtx_send = false;                        // --dtx-send: the DTX send side on every pair
static float g_dtx_hangover = -1.0f;                   // --dtx-send-hangover (-1: not given)
static bool g_dtmf_clamp = false;                      // --dtmf-clamp: removal on every pair
static int g_dtmf_guard[2] = {-1, -1};                 // --dtmf-guard PRE,POST (-1: not given)
static float g_limiter = 0.0f, g_limiter_hold = -1.0f; // --limiter: every pair's ceiling (0: not given); --limiter-hold (-1: not given)
static long g_migrate_at = -1;                        // --migrate-at: the frame behind which every slot moves to a second context and converter (-1: not given)
// --report: what a pair's written frames add up to (one report record = PN_REPORT_WORDS words, include/percepnet_hip.h)
struct PairStat { long frames = 0; long long clipped = 0; float peak = 0.f; double e_in = 0, e_out = 0; };
static void run_shard(Shard *sh, const pn_model *m, char **paths, int nn_mode, int postfilter, bool tap, int n_slots) {
  const int P = sh->count, B = n_slots > 0 && n_slots < P ? n_slots : P;
  const bool mixed = !g_rates.empty();
  const int32_t *pair_rate = mixed ? g_rates.data() + sh->first : NULL;                // --rates: this shard's slice
  const size_t FS = mixed ? PN_RATE_MIXED_ROW : g_rate ? (size_t)pn_rate_frame_samples(g_rate) : PN_FRAME_SIZE;     // samples per pinned row
  const size_t SW = g_g711 >= 0 ? 1 : sizeof(int16_t);                                  // bytes per sample in the files and the pinned rows
  const int idle = g_g711 == PN_G711_ALAW ? 0xD5 : g_g711 == PN_G711_ULAW ? 0xFF : 0;   // a sample of silence
  auto pair_fs = [&](int pair) { return mixed ? (size_t)pn_rate_mixed_frame_samples(pair_rate[pair]) : FS; };       // ... per frame in a pair's files
  auto fail = [&](int rc, const std::string &msg) { sh->rc = rc; sh->err = msg; };
  ShardRes R;
  // this thread owns the device from here on: run on the CPUs of the GPU's NUMA node BEFORE the context and the pinned
  // buffers exist (first touch places them), so that N threads feeding N GPUs do not all pull through one socket
  if (g_numa) {
    char msg[256];
    pn_bind_thread_to_device_numa(sh->device, msg, sizeof(msg));
    if (g_verbose) fprintf(stderr, "percepnet_run: %s\n", msg);
  }
  const bool conf = !g_confs.empty();
  auto set_limit = [&](pn_ctx *c, const int32_t *ids, int n) {     // --atten-lim on these slots (after creation and after every slot reset)
    if (isinf(g_atten_lim) || n == 0) return 0;
    std::vector<float> db(n, g_atten_lim);
    return pn_ctx_set_atten_limit(c, ids, n, db.data());
  };
  // A context, the converter beside it and every setting of the command line: at the start (slot s starts with pair s, rates =
  // pair_rate), and once more for --migrate-at (rates = the slots' rates at that frame).  false: the error is in sh, and the
  // caller owns whatever cx and rt hold by then
  auto make = [&](pn_ctx *&cx, pn_rate *&rt, const int32_t *rates) -> bool {
    auto bad = [&](const std::string &msg) { fail(3, msg); return false; };
    cx = pn_ctx_create(m, sh->device, B, nn_mode, NULL);
    if (!cx) return bad(std::string("pn_ctx_create: ") + pn_last_error());
    if (g_rate && !(rt = pn_rate_create(cx, g_rate))) return bad(std::string("pn_rate_create: ") + pn_last_error());
    if (mixed && !(rt = pn_rate_create_mixed(cx, rates))) return bad(std::string("pn_rate_create_mixed: ") + pn_last_error());
    if (g_g711 > 0) {                                     // every slot's law, once (a new converter's is mu-law)
      std::vector<int32_t> all(B), laws(B, g_g711);
      for (int s = 0; s < B; s++) all[s] = s;
      if (pn_rate_set_stream_laws(rt, all.data(), B, laws.data())) return bad(std::string("pn_rate_set_stream_laws: ") + pn_last_error());
    }
    if (conf) {                                           // every slot's conference, once (one device, no --slots: slot s plays pair s)
      std::vector<int32_t> all(B);
      for (int s = 0; s < B; s++) all[s] = s;
      if (pn_rate_set_stream_confs(rt, all.data(), B, g_confs.data() + sh->first)) return bad(std::string("pn_rate_set_stream_confs: ") + pn_last_error());
      if (g_conf_speakers >= 0) {                         // one cap for every conference number
        std::vector<int32_t> caps(B, g_conf_speakers);
        if (pn_rate_set_conf_speakers(rt, all.data(), B, caps.data())) return bad(std::string("pn_rate_set_conf_speakers: ") + pn_last_error());
      }
      if (!g_mix_gains.empty() && pn_rate_set_stream_mix_gains(rt, all.data(), B, g_mix_gains.data() + sh->first))
        return bad(std::string("pn_rate_set_stream_mix_gains: ") + pn_last_error());
    }
    if (g_plc && pn_rate_set_plc(rt, 1)) return bad(std::string("pn_rate_set_plc: ") + pn_last_error());
    if (!g_dtx.empty()) {                                 // comfort noise, and every slot's SID, once (a setting: slot resets and rate changes keep it)
      if (pn_rate_set_cng(rt, 1)) return bad(std::string("pn_rate_set_cng: ") + pn_last_error());
      std::vector<int32_t> all(B);
      std::vector<uint8_t> sids((size_t)B * PN_CNG_SID_BYTES);
      for (int s = 0; s < B; s++) { all[s] = s; memcpy(&sids[(size_t)s * PN_CNG_SID_BYTES], g_sid, PN_CNG_SID_BYTES); }
      if (g_sid_given && pn_rate_set_stream_sid(rt, all.data(), B, sids.data(), PN_CNG_SID_BYTES)) return bad(std::string("pn_rate_set_stream_sid: ") + pn_last_error());
    }
    if (g_agc > 0.0f) {                                   // every slot's target, once (a setting: slot resets and rate changes keep it)
      std::vector<int32_t> all(B);
      std::vector<float> targets(B, g_agc);
      float params[PN_AGC_N_PARAMS];
      for (int s = 0; s < B; s++) all[s] = s;
      pn_agc_default_params(params);
      if (g_agc_max_gain > 0.0f) params[PN_AGC_MAX_GAIN] = g_agc_max_gain;
      if (pn_rate_set_agc(rt, 1) || pn_rate_set_agc_params(rt, params) || pn_rate_set_stream_agc_targets(rt, all.data(), B, targets.data()))
        return bad(std::string("--agc: ") + pn_last_error());
    }
    if (g_limiter > 0.0f) {                               // every slot's ceiling, once (a setting: slot resets and rate changes keep it)
      std::vector<int32_t> all(B);
      std::vector<float> ceilings(B, g_limiter);
      float params[PN_LIM_N_PARAMS];
      for (int s = 0; s < B; s++) all[s] = s;
      pn_lim_default_params(params);
      if (g_limiter_hold >= 0.0f) params[PN_LIM_HOLD] = g_limiter_hold;
      if (pn_rate_set_limiter_params(rt, params) || pn_rate_set_stream_limiter(rt, all.data(), B, ceilings.data()))
        return bad(std::string("--limiter: ") + pn_last_error());
    }
    if (g_dtmf) {                                         // every slot's switch, once (a setting: slot resets and rate changes keep it)
      std::vector<int32_t> all(B);
      std::vector<uint8_t> on(B, 1);
      float params[PN_DTMF_N_PARAMS];
      for (int s = 0; s < B; s++) all[s] = s;
      pn_dtmf_default_params(params);
      if (g_dtmf_on_frames > 0.0f) params[PN_DTMF_ON_FRAMES] = g_dtmf_on_frames;
      if (pn_rate_set_dtmf_params(rt, params) || pn_rate_set_stream_dtmf(rt, all.data(), B, on.data()) || pn_rate_set_dtmf_report(rt, 1))
        return bad(std::string("--dtmf: ") + pn_last_error());
    }
    if (g_dtmf_clamp) {                                   // every slot's switch, once, behind the detector's parameters
      std::vector<int32_t> all(B);
      std::vector<uint8_t> on(B, 1);
      int32_t params[PN_DTMF_CLAMP_N_PARAMS];
      for (int s = 0; s < B; s++) all[s] = s;
      pn_dtmf_clamp_default_params(params);
      if (g_dtmf_guard[0] >= 0) { params[PN_DTMF_CLAMP_PRE] = g_dtmf_guard[0]; params[PN_DTMF_CLAMP_POST] = g_dtmf_guard[1]; }
      if (pn_rate_set_dtmf_clamp_params(rt, params) || pn_rate_set_stream_dtmf_clamp(rt, all.data(), B, on.data()) || pn_rate_set_dtmf_clamp_report(rt, 1))
        return bad(std::string("--dtmf-clamp: ") + pn_last_error());
    }
    if (g_dtx_send) {                                     // every slot's switch, once (a setting: slot resets and rate changes keep it)
      std::vector<int32_t> all(B);
      std::vector<uint8_t> on(B, 1);
      float params[PN_DTX_N_PARAMS];
      for (int s = 0; s < B; s++) all[s] = s;
      pn_dtx_default_params(params);
      if (g_dtx_hangover >= 0.0f) params[PN_DTX_HANGOVER] = g_dtx_hangover;
      if (pn_rate_set_dtx_params(rt, params) || pn_rate_set_stream_dtx(rt, all.data(), B, on.data()) || pn_rate_set_dtx_report(rt, 1))
        return bad(std::string("--dtx-send: ") + pn_last_error());
    }
    if (postfilter) pn_ctx_set_postfilter(cx, 1);
    if ((g_saturate && pn_ctx_set_output_saturate(cx, 1)) || (g_report && pn_ctx_set_report(cx, 1))) return bad(pn_last_error());
    {
      std::vector<int32_t> all(B);
      for (int s = 0; s < B; s++) all[s] = s;
      if (set_limit(cx, all.data(), B)) return bad(std::string("pn_ctx_set_atten_limit: ") + pn_last_error());
    }
    return true;
  };
  if (!make(R.cx, R.rt, pair_rate)) return;
  pn_ctx *cx = R.cx;
  pn_rate *rt = R.rt;
  std::vector<FILE *> &fin = R.fin, &fout = R.fout;
  fin.assign(B, NULL); fout.assign(B, NULL);
  int next_pair = 0;
  std::vector<int> cur_pair(B, 0);
  std::vector<long> pair_frame(B, 0);                   // --lose: the frames the pair playing in a slot has supplied so far
  std::vector<PairStat> stat(g_report ? P : 0);
  std::vector<uint32_t> dtmf_rep(g_dtmf ? (size_t)B * PN_DTMF_REPORT_WORDS : 0), clamp_rep(g_dtmf_clamp ? (size_t)B * PN_DTMF_CLAMP_REPORT_WORDS : 0);
  std::vector<uint32_t> dtx_rep(g_dtx_send ? (size_t)B * PN_DTX_REPORT_WORDS : 0);
  struct DtxStat { long n[3] = {0, 0, 0}; uint32_t sid[4] = {0, 0, 0, 0}; bool any = false; };
  std::vector<DtxStat> dtx_stat(g_dtx_send ? P : 0);  // --dtx-send: the decisions of every pair of the shard
  auto open_pair = [&](int s) -> bool {                 // the next waiting pair starts playing in slot s
    const char *pi = paths[2 * (sh->first + next_pair)], *po = paths[2 * (sh->first + next_pair) + 1];
    cur_pair[s] = next_pair++; pair_frame[s] = 0;
    fin[s] = fopen(pi, "rb"); fout[s] = fopen(po, "wb");
    if (!fin[s] || !fout[s]) { fail(4, std::string("cannot open ") + pi + " / " + po); return false; }
    return true;
  };
  for (int s = 0; s < B; s++) if (!open_pair(s)) return;
  R.ftap = tap ? fopen("feature_test.raw", "wb") : NULL;
  FILE *ftap = R.ftap;
  // Three rotating pinned buffer sets on the pipelined entry point (the context's, or with --rate / --rates the converter's): the files of frame t+1 are read while the GPU
  // works on frame t, and frame t-2's output is on the host once pn_submit_host_i16(t) has returned.
  typedef ShardRes::Slot Slot;
  Slot *slot = R.slot;
  for (int k = 0; k < 3; k++) {
    Slot &sl = slot[k];
    sl.in = (char *)pn_host_alloc((size_t)B * FS * SW);
    sl.out = (char *)pn_host_alloc((size_t)B * FS * SW);
    sl.gr = (float *)pn_host_alloc((size_t)B * 68 * sizeof(float));
    if (g_report) sl.rep = (uint32_t *)pn_host_alloc((size_t)B * PN_REPORT_WORDS * sizeof(uint32_t));
    if (!sl.in || !sl.out || !sl.gr || (g_report && !sl.rep)) return fail(5, pn_last_error());
    sl.file.assign(B, NULL); sl.skip.assign(B, 0); sl.last.assign(B, 0); sl.pair.assign(B, 0); sl.fs.assign(B, FS);
  }
  std::vector<char> first(B, 1);
  auto flush = [&](Slot &sl) {                       // main.cpp:36-38 for every stream that supplied this frame
    for (int s = 0; s < B; s++) {
      if (!sl.file[s]) continue;
      if (ftap) fwrite(&sl.gr[(size_t)s * 68], sizeof(float), 68, ftap);
      if (!sl.skip[s]) fwrite(&sl.out[(size_t)s * FS * SW], SW, sl.fs[s], sl.file[s]);
      if (g_report) {
        PairStat &ps = stat[sl.pair[s]];
        if (!sl.skip[s]) {
          const uint32_t *w = sl.rep + (size_t)s * PN_REPORT_WORDS;
          float f[4];
          memcpy(f, w, sizeof(f));                    // in_peak, in_energy, out_peak, out_energy
          ps.frames++; ps.clipped += (int32_t)w[6]; ps.e_in += f[1]; ps.e_out += f[3];
          if (f[2] > ps.peak) ps.peak = f[2];
        }
        if (sl.last[s]) {
          char level[32] = "n/a";
          if (ps.e_in > 0 && ps.e_out > 0) snprintf(level, sizeof(level), "%.2f dB", 10 * log10(ps.e_out / ps.e_in));
          printf("%s: frames %ld clipped %lld peak %.6f level %s\n", paths[2 * (sh->first + sl.pair[s]) + 1], ps.frames, ps.clipped, (double)ps.peak, level);
        }
      }
      if (sl.last[s]) { fclose(sl.file[s]); }        // the pair's last frame has been written: its output file is complete
    }
  };
  // --migrate-at: a second context and converter with the same settings, every slot's three records across, the first pair destroyed.
  // The order is the mover's (include/percepnet_hip.h "call-state records"): settings, the engine's record, the tails — one call per
  // rate, none for a 48000 slot — and the call state, which the tails' import has just zeroed.  1: failed, the error is in sh
  auto migrate = [&]() -> int {
    if (pn_host_wait(cx)) { fail(5, pn_last_error()); return 1; }
    std::vector<int32_t> all(B), rates(B);
    for (int s = 0; s < B; s++) all[s] = s;
    if (pn_rate_get_stream_rates(rt, rates.data())) { fail(5, pn_last_error()); return 1; }
    pn_ctx *cx2 = NULL;
    pn_rate *rt2 = NULL;
    auto moved = [&]() -> bool {
      if (!make(cx2, rt2, rates.data())) return false;
      std::vector<char> rec((size_t)B * pn_stream_state_bytes());
      if (pn_ctx_export_streams_host(cx, all.data(), B, rec.data()) || pn_ctx_import_streams_host(cx2, all.data(), B, rec.data())) return false;
      for (int rate : {8000, 16000, 24000, 32000}) {
        std::vector<int32_t> ids;
        for (int s = 0; s < B; s++) if (rates[s] == rate) ids.push_back(s);
        if (ids.empty()) continue;
        rec.resize(ids.size() * pn_rate_state_bytes(rate));
        if (pn_rate_export_streams_host(rt, ids.data(), (int)ids.size(), rec.data()) || pn_rate_import_streams_host(rt2, ids.data(), (int)ids.size(), rec.data())) return false;
      }
      rec.resize((size_t)B * pn_rate_call_state_bytes());
      return !(pn_rate_export_call_state_host(rt, all.data(), B, rec.data()) || pn_rate_import_call_state_host(rt2, all.data(), B, rec.data()));
    };
    if (!moved()) {
      if (!sh->rc) fail(5, std::string("--migrate-at: ") + pn_last_error());
      pn_rate_destroy(rt2); pn_ctx_destroy(cx2);
      return 1;
    }
    pn_rate_destroy(rt); pn_ctx_destroy(cx);
    R.cx = cx = cx2; R.rt = rt = rt2;
    if (g_verbose) fprintf(stderr, "percepnet_run: %d slots moved to a second context behind frame %ld\n", B, g_migrate_at);
    return 0;
  };
  std::vector<int32_t> restart, restart_rates, live;   // live (--conference): the slots whose pair still has input, this frame's id list
  std::vector<int32_t> lost;                           // --lose: the slots whose pair loses this frame
  std::vector<int32_t> silent;                         // --dtx: the slots whose pair is silent this frame
  int n_alive = B;
  long t = 0;
  for (;; t++) {
    Slot &sl = slot[t % 3];
    restart.clear(); restart_rates.clear(); live.clear(); lost.clear(); silent.clear();
    for (int s = 0; s < B; s++) {
      char *x = sl.in + (size_t)s * FS * SW;
      sl.file[s] = NULL; sl.skip[s] = 0; sl.last[s] = 0;
      if (fin[s] && fread(x, SW, pair_fs(cur_pair[s]), fin[s]) != pair_fs(cur_pair[s])) {
        // this pair is finished (partial tail dropped, main.cpp:32-33): mark the frame it supplied last as its final one
        fclose(fin[s]); fin[s] = NULL;
        Slot &prev = slot[(t + 2) % 3];                // = frame t - 1
        if (t >= 1 && prev.file[s] == fout[s]) prev.last[s] = 1; else if (fout[s]) fclose(fout[s]);
        fout[s] = NULL;
        while (next_pair < P) {                        // the slot starts over with the next waiting pair, from this frame on
          if (!open_pair(s)) return;
          if (fread(x, SW, pair_fs(cur_pair[s]), fin[s]) == pair_fs(cur_pair[s])) {
            restart.push_back(s); first[s] = 1;
            if (mixed) restart_rates.push_back(pair_rate[cur_pair[s]]);
            break;
          }
          fclose(fin[s]); fin[s] = NULL; fclose(fout[s]); fout[s] = NULL;       // shorter than one frame: an empty output, next pair
        }
        if (!fin[s]) n_alive--;
      }
      if (fin[s]) { sl.file[s] = fout[s]; sl.skip[s] = first[s]; first[s] = 0; sl.pair[s] = cur_pair[s]; sl.fs[s] = pair_fs(cur_pair[s]); }
      else memset(x, idle, FS * SW);
      if (fin[s]) live.push_back(s);
      if (fin[s]) {                                    // the frame was read, so the files stay aligned; lost: its samples never reach the device's kernels
        for (const LoseRange &lr : g_lose)
          if (lr.pair == sh->first + cur_pair[s] && pair_frame[s] >= lr.f0 && pair_frame[s] <= lr.f1) { lost.push_back(s); break; }
        for (const LoseRange &lr : g_dtx)              // silent: likewise read and discarded; its row is comfort noise
          if (lr.pair == sh->first + cur_pair[s] && pair_frame[s] >= lr.f0 && pair_frame[s] <= lr.f1) { silent.push_back(s); break; }
        pair_frame[s]++;
      }
    }
    if (n_alive == 0) break;
    if (t == g_migrate_at + 1 && g_migrate_at >= 0) {   // frame F is submitted: deliver it, then every slot moves
      if (migrate()) return;
    }
    if (!restart.empty() && (pn_ctx_reset_streams(cx, restart.data(), (int)restart.size()) ||
                             (rt && (mixed ? pn_rate_set_stream_rates(rt, restart.data(), (int)restart.size(), restart_rates.data())
                                           : pn_rate_reset_streams(rt, restart.data(), (int)restart.size()))) ||
                             set_limit(cx, restart.data(), (int)restart.size()))) return fail(5, pn_last_error());
    if (!lost.empty() && pn_rate_set_lost(rt, lost.data(), (int)lost.size())) return fail(5, pn_last_error());
    if (!silent.empty() && pn_rate_set_silent(rt, silent.data(), (int)silent.size())) return fail(5, pn_last_error());
    if (g_report && pn_host_next_report(cx, sl.rep)) return fail(5, pn_last_error());
    // --rate, --rates: the converter's frame through the same pipeline
    // --conference: only the pairs that still have input advance, so an ended one is no member of this frame's mix
    if (conf ? (g_g711 >= 0 ? pn_rate_submit_host_g711_active(rt, (const uint8_t *)sl.in, (uint8_t *)sl.out, sl.gr, live.data(), (int)live.size())
                            : pn_rate_submit_host_i16_active(rt, (const int16_t *)sl.in, (int16_t *)sl.out, sl.gr, live.data(), (int)live.size()))
        : g_g711 >= 0 ? pn_rate_submit_host_g711(rt, (const uint8_t *)sl.in, (uint8_t *)sl.out, sl.gr)
                    : rt ? pn_rate_submit_host_i16(rt, (const int16_t *)sl.in, (int16_t *)sl.out, sl.gr)
                         : pn_submit_host_i16(cx, (const int16_t *)sl.in, (int16_t *)sl.out, sl.gr)) return fail(5, pn_last_error());
    if (g_dtmf) {                                      // this frame's digits: the read waits for the frame just submitted
      if (pn_rate_read_dtmf_report(rt, dtmf_rep.data())) return fail(5, pn_last_error());
      for (int s = 0; s < B; s++) {
        const uint32_t w0 = dtmf_rep[(size_t)s * PN_DTMF_REPORT_WORDS];
        if (sl.file[s] && (w0 & PN_DTMF_BEGIN)) printf("dtmf: pair %d frame %ld digit %c\n", sh->first + cur_pair[s], pair_frame[s] - 1, (char)((w0 >> 8) & 0xff));
      }
    }
    if (g_dtmf_clamp) {                                // this frame's ended events
      if (pn_rate_read_dtmf_clamp_report(rt, clamp_rep.data())) return fail(5, pn_last_error());
      for (int s = 0; s < B; s++) {
        const uint32_t *w = &clamp_rep[(size_t)s * PN_DTMF_CLAMP_REPORT_WORDS];
        if (sl.file[s] && (w[0] & PN_DTMF_CLAMP_EVENT_END))
          printf("dtmf-event: pair %d frame %ld event %u end %u duration %u\n", sh->first + cur_pair[s], pair_frame[s] - 1, w[2] >> 24, (w[2] >> 23) & 1u, w[2] & 0xffffu);
      }
    }
    if (g_dtx_send) {                                  // this frame's decisions: the read waits for the frame just submitted
      if (pn_rate_read_dtx_report(rt, dtx_rep.data())) return fail(5, pn_last_error());
      for (int s = 0; s < B; s++) {
        const uint32_t *w = &dtx_rep[(size_t)s * PN_DTX_REPORT_WORDS];
        if (!sl.file[s] || w[0] > PN_DTX_NONE) continue;
        DtxStat &ds = dtx_stat[cur_pair[s]];
        ds.n[w[0]]++;
        if (w[0] == PN_DTX_SID) { memcpy(ds.sid, w + 4, sizeof ds.sid); ds.any = true; }
      }
    }
    if (t >= 2) flush(slot[(t - 2) % 3]);
  }
  if (pn_host_wait(cx)) return fail(5, pn_last_error());
  for (long u = (t >= 2 ? t - 2 : 0); u < t; u++) flush(slot[u % 3]);     // the last two frames in flight
  for (int s = 0; s < B; s++) fout[s] = NULL;        // every output file was closed with its last frame
  for (size_t q = 0; q < dtx_stat.size(); q++) {      // --dtx-send: one line a pair
    const DtxStat &ds = dtx_stat[q];
    std::string sid = "-";
    if (ds.any) {
      const int M = (int)(ds.sid[0] & 0xffu);
      sid = std::to_string(M);
      for (int b = 1; b < 2 + M && b < PN_CNG_SID_BYTES; b++) sid += ":" + std::to_string((ds.sid[b >> 2] >> (8 * (b & 3))) & 0xffu);
    }
    printf("dtx-send: pair %d frame %ld sid %ld none %ld last-sid %s\n", sh->first + (int)q, ds.n[PN_DTX_FRAME], ds.n[PN_DTX_SID], ds.n[PN_DTX_NONE], sid.c_str());
  }
}

// the usage text, for a command line without pairs and for a rate no converter takes.  Returns the exit status, 1.
static int usage(const char *argv0) {
  fprintf(stderr, "usage: %s [--model model.pnw] [--strict | --x3] [--postfilter] [--atten-lim DB] [--saturate] [--report] [--slots N] [--rate 8000|16000|24000|32000 | --rates R0,R1,..] [--g711 ulaw|alaw] [--conference C0,C1,.. [--conf-speakers N] [--mix-gains G0,G1,..]] [--plc [--lose P:F0-F1,P:F,..]] [--dtx P:F0-F1,P:F,.. [--sid L[:N1:..:NM]]] [--agc RMS [--agc-max-gain G]] [--limiter CEIL [--limiter-hold H]] [--dtmf [--dtmf-on-frames N]] [--dtmf-clamp [--dtmf-guard PRE,POST]] [--dtx-send [--dtx-send-hangover H]] [--migrate-at F] [--device N | --devices 0,1,..|all] <noisy speech> <output denoised> [...more pairs]\n", argv0);
  return 1;
}

int main(int argc, char **argv) {
  const char *model_path = getenv("PERCEPNET_MODEL");
  int nn_mode = PN_NN_MFMA, postfilter = 0, ai = 1, n_slots = 0;
  std::vector<int> devices;
  for (; ai < argc; ai++) {
    if (!strcmp(argv[ai], "--model") && ai + 1 < argc) model_path = argv[++ai];
    else if (!strcmp(argv[ai], "--strict")) nn_mode = PN_NN_STRICT;      // reference-order network, bit-exact to the CPU path
    else if (!strcmp(argv[ai], "--x3")) nn_mode = PN_NN_MFMA_X3;         // split-precision network (same +-1 LSB bound, ~2x the rate)
    else if (!strcmp(argv[ai], "--postfilter")) postfilter = 1;      // optional envelope post-filter (denoise.cpp:216-250)
    else if (!strcmp(argv[ai], "--atten-lim") && ai + 1 < argc) {   // per-stream attenuation limit in dB (pn_ctx_set_atten_limit)
      char *end = NULL;
      const char *v = argv[++ai];
      g_atten_lim = strtof(v, &end);
      if (end == v || *end || !(g_atten_lim >= 0.f)) { fprintf(stderr, "--atten-lim: expected a number of dB >= 0 (inf = off), got '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[ai], "--saturate")) g_saturate = true;     // int16 output saturates instead of wrapping (pn_ctx_set_output_saturate)
    else if (!strcmp(argv[ai], "--report")) g_report = true;         // one line of levels and clipping per pair (pn_ctx_set_report)
    else if (!strcmp(argv[ai], "--rate") && ai + 1 < argc) {        // the files' sample rate: a rate converter beside each context (pn_rate)
      g_rate = atoi(argv[++ai]);
      if (pn_rate_frame_samples(g_rate) < 0) { fprintf(stderr, "--rate: expected 8000, 16000, 24000 or 32000, got '%s'\n", argv[ai]); return usage(argv[0]); }
    }
    else if (!strcmp(argv[ai], "--rates") && ai + 1 < argc) {       // one rate per pair, 48000 allowed: a mixed converter beside each context
      const char *v = argv[++ai];
      for (const char *q = v; ; ) {
        char *end = NULL;
        const long r = strtol(q, &end, 10);
        if (end == q || (*end && *end != ',') || pn_rate_mixed_frame_samples((int)r) < 0) { fprintf(stderr, "--rates: expected a comma-separated list of 8000, 16000, 24000, 32000 or 48000, got '%s'\n", v); return usage(argv[0]); }
        g_rates.push_back((int32_t)r);
        if (!*end) break;
        q = end + 1;
      }
    }
    else if (!strcmp(argv[ai], "--g711") && ai + 1 < argc) {        // the files are G.711 bytes of this law (needs --rate or --rates)
      const char *v = argv[++ai];
      g_g711 = !strcmp(v, "ulaw") ? PN_G711_ULAW : !strcmp(v, "alaw") ? PN_G711_ALAW : -1;
      if (g_g711 < 0) { fprintf(stderr, "--g711: expected ulaw or alaw, got '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[ai], "--conference") && ai + 1 < argc) {  // one conference per pair, `-` for none (pn_rate_set_stream_confs)
      const char *v = argv[++ai];
      for (const char *q = v; ; ) {
        char *end = NULL;
        long c = PN_CONF_NONE;
        if (*q == '-' && (q[1] == ',' || !q[1])) end = const_cast<char *>(q) + 1;
        else c = strtol(q, &end, 10);
        if (end == q || (*end && *end != ',') || c < PN_CONF_NONE || c > 0x7fffffff) { fprintf(stderr, "--conference: expected a comma-separated list of conference numbers or '-', got '%s'\n", v); return 1; }
        g_confs.push_back((int32_t)c);
        if (!*end) break;
        q = end + 1;
      }
    }
    else if (!strcmp(argv[ai], "--conf-speakers") && ai + 1 < argc) {   // the loudest N talkers of every conference (pn_rate_set_conf_speakers)
      const char *v = argv[++ai];
      char *end = NULL;
      const long n = strtol(v, &end, 10);
      if (end == v || *end || n < 0 || n > PN_CONF_MAX_MEMBERS) { fprintf(stderr, "--conf-speakers: expected a number in [0, %d], got '%s'\n", PN_CONF_MAX_MEMBERS, v); return 1; }
      g_conf_speakers = (int)n;
    }
    else if (!strcmp(argv[ai], "--mix-gains") && ai + 1 < argc) {   // one send gain per pair (pn_rate_set_stream_mix_gains)
      const char *v = argv[++ai];
      for (const char *q = v; ; ) {
        char *end = NULL;
        const float g = strtof(q, &end);
        if (end == q || (*end && *end != ',')) { fprintf(stderr, "--mix-gains: expected a comma-separated list of gains, got '%s'\n", v); return 1; }
        g_mix_gains.push_back(g);
        if (!*end) break;
        q = end + 1;
      }
    }
    else if (!strcmp(argv[ai], "--plc")) g_plc = true;               // packet-loss concealment on the converter (pn_rate_set_plc)
    else if ((!strcmp(argv[ai], "--lose") || !strcmp(argv[ai], "--dtx")) && ai + 1 < argc) {   // pair:frame or pair:first-last: lost frames (pn_rate_set_lost), silent frames (pn_rate_set_silent)
      const char *opt = argv[ai], *v = argv[++ai];
      std::vector<LoseRange> &list = !strcmp(opt, "--lose") ? g_lose : g_dtx;
      for (const char *q = v; ; ) {
        char *end = NULL;
        LoseRange lr;
        lr.pair = strtol(q, &end, 10);
        bool ok = end != q && *end == ':' && lr.pair >= 0;
        if (ok) { q = end + 1; lr.f0 = lr.f1 = strtol(q, &end, 10); ok = end != q && lr.f0 >= 0; }
        if (ok && *end == '-') { q = end + 1; lr.f1 = strtol(q, &end, 10); ok = end != q && lr.f1 >= lr.f0; }
        if (!ok || (*end && *end != ',')) { fprintf(stderr, "%s: expected a comma-separated list of pair:frame or pair:first-last, got '%s'\n", opt, v); return 1; }
        list.push_back(lr);
        if (!*end) break;
        q = end + 1;
      }
    }
    else if (!strcmp(argv[ai], "--sid") && ai + 1 < argc) {         // L[:N1:..:NM]: every pair's silence descriptor (pn_rate_set_stream_sid)
      const char *v = argv[++ai];
      std::vector<long> f;
      for (const char *q = v; ; ) {
        char *end = NULL;
        const long x = strtol(q, &end, 10);
        if (end == q || (*end && *end != ':') || x < 0 || x > 255) { fprintf(stderr, "--sid: expected L[:N1:..:NM], whole numbers in [0, 255], got '%s'\n", v); return 1; }
        f.push_back(x);
        if (!*end) break;
        q = end + 1;
      }
      if (f.size() > 1 + PN_CNG_MAX_ORDER) { fprintf(stderr, "--sid: %d reflection coefficients, at most %d\n", (int)f.size() - 1, PN_CNG_MAX_ORDER); return 1; }
      memset(g_sid, 0, sizeof g_sid);
      g_sid[0] = (uint8_t)(f.size() - 1);
      for (size_t i = 0; i < f.size(); i++) g_sid[1 + i] = (uint8_t)f[i];
      float g, k[PN_CNG_MAX_ORDER]; int32_t M;
      if (pn_cng_sid_decode(g_sid, &g, k, &M)) { fprintf(stderr, "--sid: %s\n", pn_last_error()); return 1; }
      g_sid_given = true;
    }
    else if (!strcmp(argv[ai], "--agc") && ai + 1 < argc) {         // every pair's target RMS, linear (pn_rate_set_stream_agc_targets)
      const char *v = argv[++ai];
      char *end = NULL;
      g_agc = strtof(v, &end);
      if (end == v || *end || !(g_agc > 0.0f && g_agc <= 1.0f)) { fprintf(stderr, "--agc: expected a linear RMS target in (0, 1], got '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[ai], "--agc-max-gain") && ai + 1 < argc) {   // the level control's largest gain (PN_AGC_MAX_GAIN)
      const char *v = argv[++ai];
      char *end = NULL;
      g_agc_max_gain = strtof(v, &end);
      if (end == v || *end || !(g_agc_max_gain >= 1.0f && g_agc_max_gain <= 1024.0f)) { fprintf(stderr, "--agc-max-gain: expected a gain in [1, 1024], got '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[ai], "--limiter") && ai + 1 < argc) {     // every pair's ceiling, linear (pn_rate_set_stream_limiter)
      const char *v = argv[++ai];
      char *end = NULL;
      g_limiter = strtof(v, &end);
      if (end == v || *end || !(g_limiter >= 1.0f / 1024.0f && g_limiter <= 1.0f)) { fprintf(stderr, "--limiter: expected a linear ceiling in [1/1024, 1], got '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[ai], "--limiter-hold") && ai + 1 < argc) {   // the frames the limiter holds its gain after an attack (PN_LIM_HOLD)
      const char *v = argv[++ai];
      char *end = NULL;
      g_limiter_hold = strtof(v, &end);
      float params[PN_LIM_N_PARAMS];
      pn_lim_default_params(params);
      params[PN_LIM_HOLD] = g_limiter_hold;
      if (end == v || *end || pn_lim_params_check(params)) { fprintf(stderr, "--limiter-hold: expected a whole number of frames in [0, 1000], got '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[ai], "--dtmf")) g_dtmf = true;            // DTMF detection on every pair (pn_rate_set_stream_dtmf)
    else if (!strcmp(argv[ai], "--dtmf-on-frames") && ai + 1 < argc) {   // the hits in a row that begin a digit (PN_DTMF_ON_FRAMES)
      const char *v = argv[++ai];
      char *end = NULL;
      g_dtmf_on_frames = strtof(v, &end);
      float params[PN_DTMF_N_PARAMS];
      pn_dtmf_default_params(params);
      params[PN_DTMF_ON_FRAMES] = g_dtmf_on_frames;
      if (end == v || *end || pn_dtmf_params_check(params)) { fprintf(stderr, "--dtmf-on-frames: expected a whole number of frames in [1, 100], got '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[ai], "--dtx-send")) g_dtx_send = true;    // the DTX send side on every pair (pn_rate_set_stream_dtx)
    else if (!strcmp(argv[ai], "--dtx-send-hangover") && ai + 1 < argc) {   // the frames sent behind the last active one (PN_DTX_HANGOVER)
      const char *v = argv[++ai];
      char *end = NULL;
      g_dtx_hangover = strtof(v, &end);
      float params[PN_DTX_N_PARAMS];
      pn_dtx_default_params(params);
      params[PN_DTX_HANGOVER] = g_dtx_hangover;
      if (end == v || *end || pn_dtx_params_check(params)) { fprintf(stderr, "--dtx-send-hangover: expected a whole number of frames in [0, 255], got '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[ai], "--dtmf-clamp")) g_dtmf_clamp = true;   // DTMF removal on every pair (pn_rate_set_stream_dtmf_clamp)
    else if (!strcmp(argv[ai], "--dtmf-guard") && ai + 1 < argc) {    // rows removed in front of and behind a digit (PN_DTMF_CLAMP_PRE, PN_DTMF_CLAMP_POST)
      const char *v = argv[++ai];
      char *end = NULL;
      int32_t params[PN_DTMF_CLAMP_N_PARAMS];
      pn_dtmf_clamp_default_params(params);
      const long pre = strtol(v, &end, 10);
      bool ok = end != v && *end == ',';
      const char *v2 = ok ? end + 1 : v;
      const long post = ok ? strtol(v2, &end, 10) : 0;
      ok = ok && end != v2 && !*end && pre >= 0 && pre <= 100 && post >= 0 && post <= 100;
      if (ok) { params[PN_DTMF_CLAMP_PRE] = (int32_t)pre; params[PN_DTMF_CLAMP_POST] = (int32_t)post; }
      if (!ok || pn_dtmf_clamp_params_check(params, NULL)) { fprintf(stderr, "--dtmf-guard: expected PRE,POST, whole numbers in [0, 4] and [0, 8], got '%s'\n", v); return 1; }
      g_dtmf_guard[0] = (int)pre; g_dtmf_guard[1] = (int)post;
    }
    else if (!strcmp(argv[ai], "--migrate-at") && ai + 1 < argc) {    // move every slot to a second context and converter behind this frame
      const char *v = argv[++ai];
      char *end = NULL;
      g_migrate_at = strtol(v, &end, 10);
      if (end == v || *end || g_migrate_at < 0) { fprintf(stderr, "--migrate-at: expected a frame number >= 0, got '%s'\n", v); return 1; }
    }
    else if (!strcmp(argv[ai], "--no-numa")) g_numa = false;        // leave the host threads' CPU affinity alone
    else if (!strcmp(argv[ai], "--verbose")) g_verbose = true;       // one line per device: its NUMA binding
    else if (!strcmp(argv[ai], "--slots") && ai + 1 < argc) n_slots = atoi(argv[++ai]);   // concurrent streams per device: pairs queue for them
    else if (!strcmp(argv[ai], "--device") && ai + 1 < argc) devices.assign(1, atoi(argv[++ai]));
    else if (!strcmp(argv[ai], "--devices") && ai + 1 < argc) {
      if (!pn_cli_parse_devices(argv[++ai], pn_device_count(), devices)) {
        fprintf(stderr, "--devices: expected a comma-separated list of device ordinals in [0,%d) or 'all', got '%s'\n", pn_device_count(), argv[ai]);
        return 1;
      }
    }
    else break;
  }
  if (devices.empty()) devices.push_back(0);
  const int nfiles = argc - ai;
  if (nfiles < 2 || (nfiles & 1) || (g_g711 >= 0 && !g_rate && g_rates.empty())) {
    if (g_g711 >= 0 && !g_rate && g_rates.empty()) fprintf(stderr, "--g711 needs --rate or --rates: G.711 rows go through a rate converter\n");
    return usage(argv[0]);
  }
  const int B = nfiles / 2;
  if (g_rate && !g_rates.empty()) { fprintf(stderr, "--rate and --rates exclude each other\n"); return 1; }
  if (!g_rates.empty() && (int)g_rates.size() != B) { fprintf(stderr, "--rates: %d rates for %d pairs (one per pair)\n", (int)g_rates.size(), B); return 1; }
  if (g_confs.empty() && (g_conf_speakers >= 0 || !g_mix_gains.empty())) {
    fprintf(stderr, "%s needs --conference: it is a setting of the conference mix\n", g_conf_speakers >= 0 ? "--conf-speakers" : "--mix-gains");
    return 1;
  }
  if (!g_mix_gains.empty()) {
    if ((int)g_mix_gains.size() != B) { fprintf(stderr, "--mix-gains: %d gains for %d pairs (one per pair)\n", (int)g_mix_gains.size(), B); return 1; }
    if (pn_rate_mix_gains_check(g_mix_gains.data(), B)) { fprintf(stderr, "--mix-gains: %s\n", pn_last_error()); return 1; }
  }
  if (!g_confs.empty()) {
    if ((int)g_confs.size() != B) { fprintf(stderr, "--conference: %d entries for %d pairs (one per pair)\n", (int)g_confs.size(), B); return 1; }
    if (n_slots > 0) { fprintf(stderr, "--conference and --slots exclude each other: the members of a conference play side by side from the start\n"); return 1; }
    if (devices.size() > 1) { fprintf(stderr, "--conference takes one device: a conference lives in one context\n"); return 1; }
    if (pn_rate_confs_check(g_confs.data(), B, B)) { fprintf(stderr, "--conference: %s\n", pn_last_error()); return 1; }
    if (!g_rate && g_rates.empty()) g_rates.assign(B, 48000);        // on its own: a mixed converter of all 48000
  }
  if (!g_lose.empty() && !g_plc) { fprintf(stderr, "--lose needs --plc: a lost frame is filled by the packet-loss concealment\n"); return 1; }
  for (const LoseRange &lr : g_lose)
    if (lr.pair >= B) { fprintf(stderr, "--lose: pair %ld of %d pairs (pairs count from 0)\n", lr.pair, B); return 1; }
  if (g_sid_given && g_dtx.empty()) { fprintf(stderr, "--sid needs --dtx: it describes the comfort noise of the silent frames\n"); return 1; }
  for (const LoseRange &lr : g_dtx)
    if (lr.pair >= B) { fprintf(stderr, "--dtx: pair %ld of %d pairs (pairs count from 0)\n", lr.pair, B); return 1; }
  if (g_agc_max_gain > 0.0f && !(g_agc > 0.0f)) { fprintf(stderr, "--agc-max-gain needs --agc: it is a parameter of the level control\n"); return 1; }
  if (g_limiter_hold >= 0.0f && !(g_limiter > 0.0f)) { fprintf(stderr, "--limiter-hold needs --limiter: it is a parameter of the output limiter\n"); return 1; }
  if (g_dtmf_on_frames > 0.0f && !g_dtmf) { fprintf(stderr, "--dtmf-on-frames needs --dtmf: it is a parameter of the DTMF detector\n"); return 1; }
  if (g_dtx_hangover >= 0.0f && !g_dtx_send) { fprintf(stderr, "--dtx-send-hangover needs --dtx-send: it is a parameter of the DTX send side\n"); return 1; }
  if (g_dtmf_clamp && !g_dtmf) { fprintf(stderr, "--dtmf-clamp needs --dtmf: a digit is removed where the detector finds it\n"); return 1; }
  if (g_dtmf_guard[0] >= 0 && !g_dtmf_clamp) { fprintf(stderr, "--dtmf-guard needs --dtmf-clamp: it is a parameter of DTMF removal\n"); return 1; }
  if (g_dtmf_clamp) {                                  // the guard in front must be in time for the detector's on_frames
    float dp[PN_DTMF_N_PARAMS];
    int32_t cp[PN_DTMF_CLAMP_N_PARAMS];
    pn_dtmf_default_params(dp); pn_dtmf_clamp_default_params(cp);
    if (g_dtmf_on_frames > 0.0f) dp[PN_DTMF_ON_FRAMES] = g_dtmf_on_frames;
    if (g_dtmf_guard[0] >= 0) { cp[PN_DTMF_CLAMP_PRE] = g_dtmf_guard[0]; cp[PN_DTMF_CLAMP_POST] = g_dtmf_guard[1]; }
    if (pn_dtmf_clamp_params_check(cp, dp)) { fprintf(stderr, "--dtmf-clamp: %s\n", pn_last_error()); return 1; }
  }
  if ((g_plc || !g_dtx.empty() || g_agc > 0.0f || g_limiter > 0.0f || g_dtmf || g_dtx_send) && !g_rate && g_rates.empty()) g_rates.assign(B, 48000);        // on its own: a mixed converter of all 48000
  if (g_migrate_at >= 0) {
    if (devices.size() > 1) { fprintf(stderr, "--migrate-at takes one device: the slots move between two contexts of one device\n"); return 1; }
    if (!g_rate && g_rates.empty()) { fprintf(stderr, "--migrate-at needs a converter (--rate or --rates): it moves the converter's records with the engine's\n"); return 1; }
  }
  pn_model *m = NULL;
  if (model_path) { FILE *f = fopen(model_path, "rb"); if (f) { m = pn_model_from_file(f); fclose(f); } }
  else if (&percepnet_model_orig) m = pn_model_from_rnnmodel(&percepnet_model_orig);
  if (!m) { fprintf(stderr, "no model: pass --model file.pnw (or link a generated nnet_data.cpp): %s\n", pn_last_error()); return 2; }
  // contiguous balanced shards (the same rule as percepnet_amd/sharding.py: shard_streams); devices beyond the number
  // of pairs stay idle
  const int W = (int)devices.size() < B ? (int)devices.size() : B;
  std::vector<Shard> shards(W);
  for (int r = 0; r < W; r++) {
    int first, count;
    pn_cli_shard(B, W, r, &first, &count);
    shards[r] = {devices[r], first, count, 0, ""};
  }
  const bool tap = B == 1;
  if (W == 1) run_shard(&shards[0], m, argv + ai, nn_mode, postfilter, tap, n_slots);
  else {
    std::vector<std::thread> th;
    for (int r = 0; r < W; r++) th.emplace_back(run_shard, &shards[r], m, argv + ai, nn_mode, postfilter, false, n_slots);
    for (auto &t : th) t.join();
  }
  int rc = 0;
  for (const Shard &sh : shards)
    if (sh.rc) { fprintf(stderr, "device %d (pairs %d..%d): %s\n", sh.device, sh.first, sh.first + sh.count - 1, sh.err.c_str()); if (sh.rc > rc) rc = sh.rc; }
  if (rc && W > 1)         // some shards may have finished: say which outputs are complete and which are not
    for (const Shard &sh : shards)
      fprintf(stderr, "  outputs of pairs %d..%d (device %d): %s\n", sh.first, sh.first + sh.count - 1, sh.device,
              sh.rc ? "INCOMPLETE - discard" : "complete");
  pn_model_free(m);
  return rc;
}
