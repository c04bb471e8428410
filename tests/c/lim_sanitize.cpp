// CPU-only sanitizer harness of the output limiter's rule (tests/test_lim_host.py builds it with
// g++ -DPN_NO_HIP -ffp-contract=off -fsanitize=address,undefined, like agc_sanitize.cpp): pn_lim_rules.h over exactly-sized heap
// buffers — rows of exactly 480 floats in and out (apart and in place), a state and a report of exactly four words, the parameters at
// exactly two floats, a ceiling list at its exact length — through an attack at k = 0, in the middle and at 479, hold, release back to
// unity, the hostile rows (NaN, inf, FLT_MAX, zeros, -0.0, subnormals, a full-scale square), every parameter's edges, the count's
// saturation, and the guarantee |out| <= c on every finite row.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_lim_rules.h"
#include <stdio.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "lim_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

typedef std::vector<float> F;
typedef std::vector<uint32_t> U;

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t as_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool under(const F &out, float c) {
  for (float v : out) if (!(fabsf(v) <= c) && v == v) return false;
  return true;
}

int main() {
  static_assert(PN_LIM_N_PARAMS == 2 && PN_LIM_REPORT_WORDS == 4 && PN_LIM_STATE_BYTES == 16 && PN_LIM_RELEASE == 0 && PN_LIM_HOLD == 1 && PN_LIM_ON == 1 &&
                PN_LIM_ATTACK == 2 && PN_LIM_HOLDING == 4 && PN_LIM_RELEASING == 8 && PN_LIM_ACTIVE == 16 && PN_LIM_NONFINITE == 32, "the header's constants");
  F P(PN_LIM_N_PARAMS);
  pn_lim_default_params_host(P.data());
  CHECK(P[0] == 1.0592537f && P[1] == 2.0f && pn_lim_params_check_host(P.data()) == 0 && pn_lim_params_check_host(NULL) == -1);
  // ---- every parameter at both edges and one step outside
  { const float lo[2] = {1.0f, 0.0f}, hi[2] = {2.0f, 1000.0f};
    for (int i = 0; i < PN_LIM_N_PARAMS; i++) {
      F q = P;
      q[i] = hi[i]; CHECK(pn_lim_params_check_host(q.data()) == 0);
      q[i] = nextafterf(hi[i], INFINITY); CHECK(pn_lim_params_check_host(q.data()) == -1);
      char want[32];
      snprintf(want, sizeof(want), "index %d ", i);
      CHECK(strstr(pn_last_error(), want));
      q[i] = lo[i]; CHECK(pn_lim_params_check_host(q.data()) == 0);
      q[i] = nextafterf(lo[i], -INFINITY); CHECK(pn_lim_params_check_host(q.data()) == -1);
      q[i] = NAN; CHECK(pn_lim_params_check_host(q.data()) == -1);
    }
    F q = P;
    q[PN_LIM_HOLD] = 1.5f; CHECK(pn_lim_params_check_host(q.data()) == -1 && strstr(pn_last_error(), "index 1 "));
    q[PN_LIM_RELEASE] = 0.5f; CHECK(pn_lim_params_check_host(q.data()) == -1 && strstr(pn_last_error(), "index 0 ")); }
  // ---- ceilings: a list at its exact length
  { F c = {0.0f, -0.0f, 1.0f, 1.0f / 1024.0f, 0.5f};
    CHECK(pn_lim_ceilings_list_check(c.data(), 5) == 0 && pn_lim_ceilings_list_check(NULL, 0) == 0 && pn_lim_ceilings_list_check(NULL, 1) == -1);
    c[4] = NAN; CHECK(pn_lim_ceilings_list_check(c.data(), 5) == -1 && strstr(pn_last_error(), "index 4"));
    c[3] = nextafterf(1.0f / 1024.0f, 0.0f); CHECK(pn_lim_ceilings_list_check(c.data(), 5) == -1 && strstr(pn_last_error(), "index 3"));
    c[2] = nextafterf(1.0f, 2.0f); CHECK(pn_lim_ceilings_list_check(c.data(), 5) == -1 && strstr(pn_last_error(), "index 2"));
    std::vector<int32_t> ids = {2, 0, 1}, dup = {2, 0, 2};
    F ok = {0.1f, 0.0f, 1.0f};
    CHECK(pn_lim_ceilings_set_check(3, ids.data(), 3, ok.data()) == 0 && pn_lim_ceilings_set_check(3, dup.data(), 3, ok.data()) == -1 && pn_lim_ceilings_set_check(2, ids.data(), 3, ok.data()) == -1); }
  const float c = 0.5f;
  // ---- not limited: a copy, the state untouched; bad arguments change nothing
  { U st = {as_bits(0.25f), 7u, 9u, 0u}, rep(PN_LIM_REPORT_WORDS, 0xdeadbeefu);
    F y(PN_FRAME, 0.9f), out(PN_FRAME);
    y[3] = NAN; y[9] = -0.0f;
    CHECK(pn_lim_frame_host(P.data(), -0.0f, st.data(), y.data(), out.data(), rep.data()) == 0);
    CHECK(!memcmp(out.data(), y.data(), PN_FRAME * 4) && st[0] == as_bits(0.25f) && st[1] == 7u && st[2] == 9u && st[3] == 0u);
    CHECK(rep[0] == as_bits(1.0f) && rep[1] == 0u && rep[2] == 0u && rep[3] == 0u);
    CHECK(pn_lim_frame_host(NULL, c, st.data(), y.data(), out.data()) == -1 && pn_lim_frame_host(P.data(), c, NULL, y.data(), out.data()) == -1);
    CHECK(pn_lim_frame_host(P.data(), NAN, st.data(), y.data(), out.data()) == -1 && pn_lim_frame_host(P.data(), 1.5f, st.data(), y.data(), out.data()) == -1 && st[2] == 9u); }
  // ---- unity: a row under the ceiling with a fresh state keeps its bits, apart and in place
  { U st(4, 0u), rep(PN_LIM_REPORT_WORDS);
    F y(PN_FRAME, 0.25f), out(PN_FRAME);
    y[0] = c; y[5] = -0.0f; y[6] = as_float(0x7fc12345u);
    const F y0 = y;
    CHECK(pn_lim_frame_host(P.data(), c, st.data(), y.data(), out.data(), rep.data()) == PN_LIM_ON);
    CHECK(!memcmp(out.data(), y0.data(), PN_FRAME * 4) && st[0] == as_bits(1.0f) && st[1] == 0u && st[2] == 0u && st[3] == 0u && rep[1] == as_bits(c));
    CHECK(pn_lim_frame_host(P.data(), c, st.data(), y.data(), y.data()) == PN_LIM_ON && !memcmp(y.data(), y0.data(), PN_FRAME * 4)); }
  // ---- an attack at k = 0, 300 and 479, then hold, then release back to unity; in place; the guarantee on every row
  for (int k : {0, 300, 479}) {
    U st(4, 0u), rep(PN_LIM_REPORT_WORDS);
    F y(PN_FRAME, 0.5f * c), out(PN_FRAME);
    y[k] = -2.0f * c;
    int fl = pn_lim_frame_host(P.data(), c, st.data(), y.data(), out.data(), rep.data());
    CHECK(fl == (PN_LIM_ON | PN_LIM_ATTACK | PN_LIM_ACTIVE) && (uint32_t)fl == rep[2] && as_float(st[0]) == 0.5f && st[1] == 2u && st[2] == 1u && st[3] == 0u && rep[3] == 1u);
    CHECK(under(out, c) && out[k] == -c && out[0] == (k ? y[0] : -c));
    for (int j = 1; j < PN_FRAME; j++) CHECK(j == k || (j < k ? out[j] <= out[j - 1] : out[j] == 0.25f * c));     // the gain falls to index k and is flat behind it
    F z(PN_FRAME, 0.4f * c);
    int frames = 0;
    for (; frames < 40 && as_float(st[0]) < 1.0f; frames++) {
      const float g_before = as_float(st[0]);
      fl = pn_lim_frame_host(P.data(), c, st.data(), z.data(), z.data(), rep.data());
      CHECK(fl > 0 && under(z, c) && as_float(st[0]) <= g_before * P[0] && as_float(st[0]) >= g_before && as_float(st[0]) <= 1.0f);
      CHECK(frames < 2 ? (fl & PN_LIM_HOLDING) && as_float(st[0]) == 0.5f : (fl & PN_LIM_RELEASING) != 0);
      z.assign(PN_FRAME, 0.4f * c);
    }
    CHECK(frames == 2 + 13 && st[0] == as_bits(1.0f));
    const uint32_t limited = st[2];
    CHECK(pn_lim_frame_host(P.data(), c, st.data(), z.data(), out.data()) == PN_LIM_ON && !memcmp(out.data(), z.data(), PN_FRAME * 4) && st[2] == limited);
  }
  { // hostile rows: a live state behind every one of them, the gain in (0, 1]; a non-finite row touches nothing
    const float fills[] = {NAN, INFINITY, -INFINITY, FLT_MAX, 0.0f, -0.0f, 1e-41f, 1.0f, -1.0f};
    U st(4, 0u), rep(PN_LIM_REPORT_WORDS);
    F out(PN_FRAME);
    for (float fill : fills) {
      F y(PN_FRAME, fill);
      if (fill == 1.0f) for (int j = 0; j < PN_FRAME; j++) y[j] = (j / 48) % 2 ? -1.0f : 1.0f;      // a full-scale square
      const U before = st;
      const int fl = pn_lim_frame_host(P.data(), c, st.data(), y.data(), out.data(), rep.data());
      CHECK(fl > 0);
      if (fabsf(fill) == INFINITY) CHECK((fl & PN_LIM_NONFINITE) && st == before && !memcmp(out.data(), y.data(), PN_FRAME * 4));
      else CHECK(!(fl & PN_LIM_NONFINITE) && under(out, c));
      const float g = st[0] ? as_float(st[0]) : 1.0f;
      CHECK(g > 0.0f && g <= 1.0f && st[3] == 0u);
    }
    // one NaN and one inf inside a voice-like row: the NaN is ignored, the inf makes the row non-finite
    F y(PN_FRAME, 0.7f);
    y[5] = NAN;
    CHECK(!(pn_lim_frame_host(P.data(), c, st.data(), y.data(), out.data()) & PN_LIM_NONFINITE) && under(out, c) && out[5] != out[5]);
    y[200] = -INFINITY;
    CHECK(pn_lim_frame_host(P.data(), c, st.data(), y.data(), out.data()) & PN_LIM_NONFINITE); }
  { // the count saturates
    U st = {as_bits(0.5f), 0u, 0xfffffffeu, 0u};
    F y(PN_FRAME, 0.1f), out(PN_FRAME);
    for (int i = 0; i < 3; i++) CHECK(pn_lim_frame_host(P.data(), c, st.data(), y.data(), out.data()) & PN_LIM_ACTIVE);
    CHECK(st[2] == 0xffffffffu); }
  { // the needed gain: p * gl rounds to at most c, over a walk of peaks at the smallest, a middle and the largest ceiling
    const float cs[3] = {1.0f / 1024.0f, 0.3f, 1.0f};
    for (float cc : cs) {
      float p = nextafterf(cc, INFINITY);
      for (int i = 0; i < 200000; i++) {
        const float gl = pn_lim_needed_host(p, cc);
        CHECK(gl > 0.0f && gl < 1.0f && p * gl <= cc);
        p = p * 1.00007f;
        if (!(p <= FLT_MAX)) break;
      }
    } }
  puts("ok");
  return 0;
}
