// The rate converter's arithmetic that needs no GPU, described once — HIP-free (builds with -DPN_NO_HIP), checked on the CPU by
// tests/c/rate_sanitize.cpp under the sanitizers and by tests/test_rate_host.py through the C-ABI (include/percepnet_hip.h says
// what the numbers mean): the four rates and their sizes, the prototype filter, and the per-stream state record.
// The filter is computed like the tables of pn_tables.cpp: in double, each value narrowed to float once.
//   h[k] = sinc(k / L) * I0(beta * sqrt(1 - (k / D)^2)) / I0(beta),  k = -D..D,  D = T * L,  beta = 8
// for k >= 0 and mirrored, so the table is symmetric bit for bit; h[0] = 1 and h[jL] = 0 are set, not computed (sin(pi j) is not
// 0 in double), which is what makes phase 0 of the up-conversion a copy.  The down-converter's taps are (float)(h_double[k] / L).
// 32000 Hz is 48000 * M / L with (L, M) = (3, 2): its prototype is the L = 3 table, bit for bit, and its down taps are
// (float)(h_double[k] * M / L) — up by L, every M-th output kept; down: the 48 kHz samples sit M apart on the L-times grid.
#pragma once
#include "pn_host_rules.h"   // pn_le32, pn_record_header_check
#include <math.h>

#define PN_RATE_BETA 8.0
#define PN_RATE_UP_TAIL (2 * PN_RATE_TAPS)      // low-rate samples an up-converted stream carries: x[q - 2T + 1 .. q] is 32 wide
#define PN_RATE_MAX_L 6
#define PN_RATE_MAX_TAPS (2 * PN_RATE_TAPS * PN_RATE_MAX_L + 1)

#if defined(__HIPCC__)
#define PN_RATE_HD __host__ __device__
#else
#define PN_RATE_HD
#endif
// A rate is 48000 * M / L.  Its FACTOR is what the tables, the launchers and the device's per-stream table carry: L itself where
// M = 1 (6, 3, 2 — and 1, a copy, on a mixed converter only), PN_RATE_F_3_2 = 32 ("3 over 2") for 32000.  This is the one place
// that states (L, M) and what follows from them per rate:
//   rate     factor  (L, M)   n = 480 M / L   down tail 2 T L / M   record 16 + 4 (32 + tail)   delay 2880 M / L + 2 T
//    8000       6    (6, 1)        80               192                      912                       512
//   16000       3    (3, 1)       160                96                      528                       992
//   24000       2    (2, 1)       240                64                      400                      1472
//   32000      32    (3, 2)       320                48                      336                      1952
#define PN_RATE_F_3_2 32
// the factor of the four rates a converter takes, 0 for every other
PN_RATE_HD constexpr static inline int pn_rate_factor(int rate_hz) { return rate_hz == 8000 ? 6 : rate_hz == 16000 ? 3 : rate_hz == 24000 ? 2 : rate_hz == 32000 ? PN_RATE_F_3_2 : 0; }
PN_RATE_HD constexpr static inline int pn_rate_factor_L(int f) { return f == PN_RATE_F_3_2 ? 3 : f; }
PN_RATE_HD constexpr static inline int pn_rate_factor_M(int f) { return f == PN_RATE_F_3_2 ? 2 : 1; }
PN_RATE_HD constexpr static inline int pn_rate_factor_hz(int f) { return 48000 * pn_rate_factor_M(f) / pn_rate_factor_L(f); }
PN_RATE_HD constexpr static inline int pn_rate_factor_frame(int f) { return PN_FRAME * pn_rate_factor_M(f) / pn_rate_factor_L(f); }       // n: samples of a 10 ms row
PN_RATE_HD constexpr static inline int pn_rate_factor_delay(int f) { return 6 * pn_rate_factor_frame(f) + (f == 1 ? 0 : 2 * PN_RATE_TAPS); }   // the engine's 2880 samples at the stream's rate, T up and T down
PN_RATE_HD constexpr static inline int pn_rate_down_tail(int f) { return 2 * PN_RATE_TAPS * pn_rate_factor_L(f) / pn_rate_factor_M(f); }   // 48 kHz samples a down-converted stream carries: 2D / M
PN_RATE_HD constexpr static inline size_t pn_rate_record_words(int f) { return PN_RATE_STATE_HEADER_BYTES / 4 + PN_RATE_UP_TAIL + (size_t)pn_rate_down_tail(f); }
#define PN_RATE_TEXT "8000, 16000, 24000 or 32000"

// modified Bessel function of the first kind, order 0: sum_k ((x / 2)^k / k!)^2, terms are positive and fall monotonically
// once k > x / 2, so stopping below 1e-20 of the sum leaves a relative error far under double's
static inline double pn_rate_i0(double x) {
  double sum = 1.0, term = 1.0;
  const double q = 0.25 * x * x;
  for (int k = 1; k < 500; k++) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-20 * sum) break;
  }
  return sum;
}

// taps[k + D], k = -D..D: h (down == 0) or g = h * M / L (down != 0) for the factors 2, 3, 6 and PN_RATE_F_3_2, whose h is the
// table of 3.  Returns 2D + 1, or -1 (another factor, cap too small).
static inline int pn_rate_design(int f, int down, float *taps, int cap) {
  if (f != 2 && f != 3 && f != 6 && f != PN_RATE_F_3_2) { pn_set_error("rate converter: no design for factor %d", f); return -1; }
  const int L = pn_rate_factor_L(f), M = pn_rate_factor_M(f);
  const int D = PN_RATE_TAPS * L, n = 2 * D + 1;
  if (!taps || cap < n) { pn_set_error("rate converter: %d taps need room for %d, got %d", n, n, taps ? cap : 0); return -1; }
  const double pi = 3.14159265358979323846264338327, i0b = pn_rate_i0(PN_RATE_BETA);
  for (int k = 0; k <= D; k++) {
    double h;
    if (k == 0) h = 1.0;
    else if (k % L == 0) h = 0.0;
    else {
      const double t = (double)k / L, r = (double)k / D;
      h = sin(pi * t) / (pi * t) * pn_rate_i0(PN_RATE_BETA * sqrt(1.0 - r * r)) / i0b;
    }
    const float v = !down ? (float)h : M == 1 ? (float)(h / L) : (float)(h * M / L);
    taps[D + k] = v; taps[D - k] = v;
  }
  return n;
}

static inline void pn_rate_record_header(uint32_t hdr[4], int rate_hz) {
  hdr[0] = PN_RATE_STATE_MAGIC; hdr[1] = PN_RATE_STATE_VERSION;
  hdr[2] = (uint32_t)(4 * pn_rate_record_words(pn_rate_factor(rate_hz))); hdr[3] = (uint32_t)rate_hz;
}
// The verdict of a record HEADER in a slot of rate_hz (one of the four rates), stated once: the four header words as read
// (little-endian), in the order every record check keeps — magic, version, the rate, then the size word.  Side-effect-free (no
// message, no memory access), so that the device import (pn_rate.hip pn_rate_records_dev_kernel) and the host check below give the same
// verdict for the same bytes.
PN_RATE_HD static inline int pn_rate_header_verdict(uint32_t magic, uint32_t version, uint32_t size_word, uint32_t rate_word, int rate_hz) {
  const int f = pn_rate_factor(rate_hz);
  if (!f) return PN_SS_BAD_RATE;
  if (magic != PN_RATE_STATE_MAGIC) return PN_SS_BAD_MAGIC;
  if (version != PN_RATE_STATE_VERSION) return PN_SS_BAD_VERSION;
  if ((int32_t)rate_word != rate_hz) return PN_SS_BAD_RATE;
  if (size_word != (uint32_t)(4 * pn_rate_record_words(f))) return PN_SS_BAD_SIZE;
  return PN_SS_OK;
}
// is `bytes` bytes at `record` one state record of a converter of rate_hz?  Reads the 16 header bytes only, and only when
// they are there.  The header's verdict is pn_rate_header_verdict's; this function adds the length of the buffer and the words.
static inline int pn_rate_record_check(const void *record, size_t bytes, int rate_hz) {
  const int f = pn_rate_factor(rate_hz);
  if (!record) { pn_set_error("NULL argument"); return PN_SS_BAD_ARG; }
  if (!f) { pn_set_error("rate %d Hz: a converter takes " PN_RATE_TEXT, rate_hz); return PN_SS_BAD_RATE; }
  const size_t want = 4 * pn_rate_record_words(f);
  const unsigned char *r = static_cast<const unsigned char *>(record);
  if (bytes < 16) { pn_set_error("rate-state record of %zu bytes: a record at %d Hz has %zu", bytes, rate_hz, want); return PN_SS_BAD_SIZE; }
  const int v = pn_rate_header_verdict(pn_le32(r), pn_le32(r + 4), pn_le32(r + 8), pn_le32(r + 12), rate_hz);
  if (v == PN_SS_BAD_MAGIC || v == PN_SS_BAD_VERSION) return pn_record_header_check(r, bytes, PN_RATE_STATE_MAGIC, PN_RATE_STATE_VERSION, "rate-state");   // (words it)
  if (v == PN_SS_BAD_RATE) { pn_set_error("rate-state record written at %d Hz, this converter runs at %d", (int32_t)pn_le32(r + 12), rate_hz); return v; }
  if (v == PN_SS_BAD_SIZE || bytes != want) {
    pn_set_error("rate-state record of %zu bytes (header: %u), a record at %d Hz has %zu", bytes, pn_le32(r + 8), rate_hz, want);
    return PN_SS_BAD_SIZE;
  }
  return PN_SS_OK;
}
