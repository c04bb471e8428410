// CPU-only sanitizer harness of the automatic level control's rule (tests/test_agc_host.py builds it with
// g++ -DPN_NO_HIP -ffp-contract=off -fsanitize=address,undefined, like plc_sanitize.cpp): pn_agc_rules.h over exactly-sized heap
// buffers — rows of exactly 480 floats in and out (apart and in place), a state and a report of exactly four words, the parameters at
// exactly eight floats, a target list at its exact length — through the hostile rows (NaN, inf, 3e38, zeros, -0.0, subnormals, a
// full-scale square, a peak at the ceiling), a concealed frame, every parameter's edges, the count's saturation.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_agc_rules.h"
#include <stdio.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "agc_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

typedef std::vector<float> F;
typedef std::vector<uint32_t> U;

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t as_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static F voice(float amp, int frame) {
  F y(PN_FRAME);
  for (int j = 0; j < PN_FRAME; j++) {
    double v = 0;
    for (int h = 1; h <= 6; h++) v += cos(3.14159265358979323846 * (2.0 * h * 130.0 * (frame * PN_FRAME + j) / 48000.0 - h * (h - 1) / 6.0));   // Schroeder's phases: a flat envelope
    y[j] = (float)(amp * v);
  }
  return y;
}

int main() {
  static_assert(PN_AGC_N_PARAMS == 8 && PN_AGC_REPORT_WORDS == 4 && PN_AGC_STATE_BYTES == 16 && PN_AGC_ON == 1 && PN_AGC_ADAPTED == 2 && PN_AGC_LIMITED == 4 &&
                PN_AGC_AT_MAX == 8 && PN_AGC_AT_MIN == 16 && PN_AGC_HELD_LOST == 32 && PN_AGC_CEILING == 7, "the header's constants");
  F P(PN_AGC_N_PARAMS);
  pn_agc_default_params_host(P.data());
  CHECK(P[0] == 16.0f && P[1] == 0.125f && P[2] == 0.001f && P[3] == 0.5f && P[4] == 0.05f && P[5] == 1.0592537f && P[6] == 0.8912509f && P[7] == 32767.0f / 32768.0f);
  CHECK(pn_agc_params_check_host(P.data()) == 0 && pn_agc_params_check_host(NULL) == -1);
  // ---- every parameter at both edges and one step outside
  { const float lo[8] = {1.0f, 1.0f / 1024.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f}, hi[8] = {1024.0f, 1.0f, 1.0f, 1.0f, 1.0f, 2.0f, 1.0f, 1.0f};
    const bool open_lo[8] = {false, false, false, true, true, false, true, true};
    for (int i = 0; i < PN_AGC_N_PARAMS; i++) {
      F q = P;
      q[i] = hi[i]; CHECK(pn_agc_params_check_host(q.data()) == 0);
      q[i] = nextafterf(hi[i], INFINITY); CHECK(pn_agc_params_check_host(q.data()) == -1);
      char want[32];
      snprintf(want, sizeof(want), "index %d ", i);
      CHECK(strstr(pn_last_error(), want));
      q[i] = lo[i]; CHECK(pn_agc_params_check_host(q.data()) == (open_lo[i] ? -1 : 0));
      q[i] = open_lo[i] ? nextafterf(lo[i], INFINITY) : nextafterf(lo[i], -INFINITY); CHECK(pn_agc_params_check_host(q.data()) == (open_lo[i] ? 0 : -1));
      q[i] = NAN; CHECK(pn_agc_params_check_host(q.data()) == -1);
    } }
  // ---- targets: a list at its exact length
  { F t = {0.0f, -0.0f, 1.0f, 1e-45f, 0.5f};
    CHECK(pn_agc_targets_list_check(t.data(), 5) == 0 && pn_agc_targets_list_check(NULL, 0) == 0 && pn_agc_targets_list_check(NULL, 1) == -1);
    t[4] = NAN; CHECK(pn_agc_targets_list_check(t.data(), 5) == -1 && strstr(pn_last_error(), "index 4"));
    t[3] = nextafterf(1.0f, 2.0f); CHECK(pn_agc_targets_list_check(t.data(), 5) == -1 && strstr(pn_last_error(), "index 3"));
    t[0] = -1e-45f; CHECK(pn_agc_targets_list_check(t.data(), 5) == -1 && strstr(pn_last_error(), "index 0"));
    std::vector<int32_t> ids = {2, 0, 1}, dup = {2, 0, 2};
    F ok = {0.1f, 0.0f, 1.0f};
    CHECK(pn_agc_targets_set_check(3, ids.data(), 3, ok.data()) == 0 && pn_agc_targets_set_check(3, dup.data(), 3, ok.data()) == -1 && pn_agc_targets_set_check(2, ids.data(), 3, ok.data()) == -1); }
  // ---- whole frames over exactly-sized buffers
  { U st(4, 0u), rep(PN_AGC_REPORT_WORDS, 0xdeadbeefu);
    F out(PN_FRAME);
    // not levelled: a copy, the state untouched
    F y = voice(0.05f, 0);
    y[3] = NAN; y[9] = -0.0f;
    st[0] = as_bits(3.0f); st[1] = as_bits(2.0f); st[2] = 9u;
    CHECK(pn_agc_frame_host(P.data(), -0.0f, st.data(), y.data(), out.data(), 0, rep.data()) == 0);
    CHECK(!memcmp(out.data(), y.data(), PN_FRAME * 4) && st[0] == as_bits(3.0f) && st[1] == as_bits(2.0f) && st[2] == 9u && st[3] == 0u);
    CHECK(rep[0] == as_bits(1.0f) && rep[1] == 0u && rep[2] == 0u && rep[3] == 0u);
    // bad arguments change nothing
    CHECK(pn_agc_frame_host(NULL, 0.1f, st.data(), y.data(), out.data(), 0) == -1 && pn_agc_frame_host(P.data(), 0.1f, NULL, y.data(), out.data(), 0) == -1);
    CHECK(pn_agc_frame_host(P.data(), NAN, st.data(), y.data(), out.data(), 0) == -1 && pn_agc_frame_host(P.data(), 1.5f, st.data(), y.data(), out.data(), 0) == -1 && st[2] == 9u); }
  { // a voice from a fresh state: the first frame takes its energy as the level; 120 frames settle near the target, slewed frame by frame
    U st(4, 0u), rep(PN_AGC_REPORT_WORDS);
    F out(PN_FRAME);
    float g_prev = 1.0f;
    double rms = 0;
    for (int t = 0; t < 120; t++) {
      F y = voice(0.02f, t);
      const int fl = pn_agc_frame_host(P.data(), 0.1f, st.data(), y.data(), out.data(), 0, rep.data());
      CHECK(fl >= 0 && (fl & PN_AGC_ON) && (fl & PN_AGC_ADAPTED) && (uint32_t)fl == rep[2] && rep[0] == st[1] && rep[1] == st[0] && st[2] == (uint32_t)(t + 1) && st[3] == 0u);
      if (t == 0) CHECK(as_float(st[0]) == pn_mix_level_host(y.data()));
      const float g = as_float(st[1]);
      CHECK(g >= P[1] && g <= P[0] && g >= g_prev * P[6] && g <= g_prev * P[5]);
      CHECK(as_float(rep[3]) == pn_agc_peak_host(y.data()));
      g_prev = g;
      rms = 0;
      for (float v : out) rms += (double)v * v;
      rms = sqrt(rms / PN_FRAME);
    }
    CHECK(rms > 0.1 / 1.122 && rms < 0.1 * 1.122);                  // within 1 dB of the target
    // a pause and a concealed frame hold level and gain; in place
    const U before = st;
    F z(PN_FRAME, 1e-5f);
    CHECK(pn_agc_frame_host(P.data(), 0.1f, st.data(), z.data(), z.data(), 0) == PN_AGC_ON && st == before);
    CHECK(z[0] == 1e-5f * as_float(st[1]));
    F y = voice(0.3f, 7);
    const int fl = pn_agc_frame_host(P.data(), 0.1f, st.data(), y.data(), y.data(), 1, rep.data());
    CHECK(fl >= 0 && (fl & PN_AGC_HELD_LOST) && !(fl & PN_AGC_ADAPTED) && st[0] == before[0] && st[2] == before[2]); }
  { // hostile rows: a live state behind every one of them, the gain in range and not stuck
    const float fills[] = {NAN, INFINITY, -INFINITY, 3e38f, 0.0f, -0.0f, 1e-41f, 1.0f, -1.0f};
    U st(4, 0u);
    F out(PN_FRAME);
    for (float fill : fills) {
      F y(PN_FRAME, fill);
      if (fill == 1.0f) for (int j = 0; j < PN_FRAME; j++) y[j] = (j / 48) % 2 ? -1.0f : 1.0f;      // a full-scale square
      const int fl = pn_agc_frame_host(P.data(), 0.1f, st.data(), y.data(), out.data(), 0);
      const float g = as_float(st[1]), lev = as_float(st[0]);
      CHECK(fl > 0 && st[1] != 0u && g >= P[1] && g <= P[0] && lev >= 0.0f && lev <= FLT_MAX);
      if (fabsf(fill) == 1.0f) for (float v : out) CHECK(fabsf(v * 32768.0f) < 32768.0f);             // the limiter: no sample clips
      if (fill == 0.0f && !signbit(fill)) for (float v : out) CHECK(v == 0.0f);
    }
    // the full-scale rows left a level of 480 behind, which releases by 5 % a frame: within 60 frames of voice the gain moves again
    const float g_before = as_float(st[1]);
    for (int t = 0; t < 60; t++) {
      F y = voice(0.05f, t);
      CHECK(pn_agc_frame_host(P.data(), 0.1f, st.data(), y.data(), out.data(), 0) & PN_AGC_ADAPTED);
    }
    CHECK(as_float(st[1]) > g_before); }
  { // the peak exactly at the ceiling under a fresh gain is not limited; one step above it is.  Unity gains keep the bits
    F q = P;
    q[PN_AGC_MAX_GAIN] = q[PN_AGC_MIN_GAIN] = 1.0f;
    F y = voice(0.1f, 3), out(PN_FRAME);
    y[100] = q[PN_AGC_CEILING]; y[101] = -0.0f;
    U st(4, 0u);
    const int fl = pn_agc_frame_host(q.data(), 0.1f, st.data(), y.data(), out.data(), 0);
    CHECK(fl > 0 && (fl & PN_AGC_ADAPTED) && !(fl & PN_AGC_LIMITED));
    CHECK(!memcmp(out.data(), y.data(), PN_FRAME * 4) && st[1] == as_bits(1.0f));
    y[100] = nextafterf(q[PN_AGC_CEILING], 2.0f);
    st.assign(4, 0u);
    CHECK(pn_agc_frame_host(q.data(), 0.1f, st.data(), y.data(), out.data(), 0) & PN_AGC_LIMITED); }
  { // the count saturates
    U st = {0u, 0u, 0xfffffffeu, 0u};
    F y = voice(0.1f, 0), out(PN_FRAME);
    for (int i = 0; i < 3; i++) CHECK(pn_agc_frame_host(P.data(), 0.1f, st.data(), y.data(), out.data(), 0) > 0);
    CHECK(st[2] == 0xffffffffu); }
  puts("ok");
  return 0;
}
