// The mixed rate converter's rules that need no GPU, each stated once — HIP-free (builds with -DPN_NO_HIP), checked on the CPU by
// tests/c/rate_mixed_sanitize.cpp under the sanitizers and by tests/test_rate_mixed_host.py through the C-ABI
// (include/percepnet_hip.h "mixed rates"): the five per-stream rates and their sizes, what a list of rates and a rate change must
// be, and the one-rate-per-call rule of the state records.  48000 is a rate of a STREAM of a mixed converter (L = 1, a copy); no
// single-rate converter, no filter design and no state record has it (pn_rate_design.h keeps refusing it).
#pragma once
#include "pn_rate_design.h"

#define PN_RATE_MIXED_TEXT "8000, 16000, 24000, 32000 or 48000"

// the factor (pn_rate_design.h) of the five rates a stream of a mixed converter takes, 0 for every other
static inline int pn_rate_mixed_factor(int rate_hz) { return rate_hz == 48000 ? 1 : pn_rate_factor(rate_hz); }
static inline int pn_rate_mixed_frame(int rate_hz) {
  const int f = pn_rate_mixed_factor(rate_hz);
  if (!f) { pn_set_error("rate %d Hz: a stream of a mixed converter takes " PN_RATE_MIXED_TEXT, rate_hz); return -1; }
  return pn_rate_factor_frame(f);
}
// the engine's 2880 samples at the stream's rate, plus T up and T down where there is a filter
static inline int pn_rate_mixed_delay(int rate_hz) {
  const int f = pn_rate_mixed_factor(rate_hz);
  if (!f) { pn_set_error("rate %d Hz: a stream of a mixed converter takes " PN_RATE_MIXED_TEXT, rate_hz); return -1; }
  return pn_rate_factor_delay(f);
}

// rates_hz[0..n): every one of the five.  -1 with pn_last_error naming the FIRST bad index; n == 0 is a legal list.
static inline int pn_rate_mixed_rates_list_check(const int32_t *rates_hz, int n) {
  if (n < 0 || (n > 0 && !rates_hz)) { pn_set_error("bad argument"); return -1; }
  for (int i = 0; i < n; i++)
    if (!pn_rate_mixed_factor(rates_hz[i])) {
      pn_set_error("rate %d Hz at index %d: a stream of a mixed converter takes " PN_RATE_MIXED_TEXT, (int)rates_hz[i], i);
      return -1;
    }
  return 0;
}

// A rate change: ids[0..n) distinct streams of a batch of B (pn_ids_check), rates_hz[i] the new rate of ids[i].
static inline int pn_rate_mixed_set_check(int B, const int32_t *ids, int n, const int32_t *rates_hz) {
  if (pn_ids_check(B, ids, n, true)) return -1;
  return pn_rate_mixed_rates_list_check(rates_hz, n);
}

// One export or import call moves records of ONE rate: the rate R != 48000 that the streams ids[0..n) (checked by the caller
// against cur_rates' length) all have in cur_rates, or -1 with the error set — a list spanning two rates, or a 48000 slot, which
// has no converter state to move.  n == 0 gives -1 too (the callers return before asking).
static inline int pn_rate_mixed_record_rate(const int32_t *cur_rates, const int32_t *ids, int n) {
  if (!cur_rates || !ids || n <= 0) { pn_set_error("bad argument"); return -1; }
  const int R = cur_rates[ids[0]];
  for (int i = 0; i < n; i++) {
    const int r = cur_rates[ids[i]];
    if (r == 48000) { pn_set_error("stream %d runs at 48000 Hz: it has no converter state to move", (int)ids[i]); return -1; }
    if (r != R) {
      pn_set_error("streams %d (%d Hz) and %d (%d Hz): one record call moves streams of one rate", (int)ids[0], R, (int)ids[i], r);
      return -1;
    }
  }
  return R;
}

// The list of a DEVICE-side record call (pn_rate_export_streams / pn_rate_import_streams), host only: ids[0..n) in range —
// distinct where the streams are written (import) — and none of them a 48000 slot, which has no converter state to move.
// cur_rates: the rate of every stream as last set ([B]; NULL = a single-rate converter, which has no 48000 slot).  The fixed
// record stride lifts the one-rate-per-call rule above: the listed streams may run at different rates.  0, or -1 with the error set.
static inline int pn_rate_records_list_check(int B, const int32_t *cur_rates, const int32_t *ids, int n, bool distinct) {
  if (pn_ids_check(B, ids, n, distinct)) return -1;
  for (int i = 0; cur_rates && i < n; i++)
    if (cur_rates[ids[i]] == 48000) { pn_set_error("stream %d runs at 48000 Hz: it has no converter state to move", (int)ids[i]); return -1; }
  return 0;
}
