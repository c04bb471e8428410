// The two create-time self-tests of a batched context (ctx_create, pn_context.cpp) and the synthetic model both run: known-answer
// checks of THE KERNELS of this build, not of the caller's model.  Their verdicts are cached for the process.
#include "pn_context.h"
#include <stdio.h>
#include <math.h>
#include <map>
#include <mutex>
#include <string>

#include "pn_selftest_golden.h"

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

int nn_selftest(pn_ctx *c) {
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
    last_alloc_oom() = false;
    cx[pass] = ctx_create(m, c->device, rows, pass ? PN_NN_STRICT : c->nn_mode, NULL, false, &plan[pass]);
    if (!cx[pass]) { rc = -1; oom = last_alloc_oom(); break; }
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

int dsp_selftest(pn_ctx *c) {
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
  last_alloc_oom() = false;
  PnPlan plan = pn_plan_for(Bt, PN_NN_MFMA);
  plan.fe = c->plan.fe;
  pn_ctx *t = m ? ctx_create(m, c->device, Bt, PN_NN_MFMA, NULL, false, &plan) : NULL;
  if (!t) {
    const bool oom = last_alloc_oom();
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
