// The call-state record of the rate converter (include/percepnet_hip.h "call-state records"), the layout and the verdict stated once —
// HIP-free (builds with -DPN_NO_HIP): the host's pn_rate_call_state_check is pn_call_record_check below, the kernel
// (pn_rate_call.hip pn_rate_call_kernel) gives the verdict with the same pn_call_verdict, tests/call_state_model.py restates both in
// numpy, tests/c/call_state_sanitize.cpp runs them under the sanitizers over exactly-sized buffers and hostile records.
//
// What a stream carries on the converter beside its two tails (those travel in the version-1 rate-state record, pn_rate_design.h):
// the concealer's history, period and counters (pn_plc_rules.h), the level control's four words (pn_agc_rules.h), the limiter's four
// words (pn_lim_rules.h) and the level the loudest-N hold keeps (pn_mix_rules.h).  None of it depends on the stream's rate, so one
// record serves every rate, 48000 included.
//
// Record (little-endian, PN_RATE_CALL_STATE_BYTES = 10640, every section a whole number of 16-byte groups):
//   header 16 B : uint32 magic PN_RATE_CALL_MAGIC | uint32 version PN_RATE_CALL_VERSION | uint32 record bytes | uint32 section mask
//   body, words :    0  PN_CALL_W_HIST   1920 f32   the LINEAR view of pn_plc_rules.h, oldest sample first: ring row (head + j) & 3 is record row j
//                 1920  PN_CALL_W_Q       720 f32   the period buffer
//                 2640  PN_CALL_W_META      4 u32   P | r | lost | 0 — the head is normalised away, the record is phase-free
//                 2644  PN_CALL_W_AGC       4 u32   lev | gain | adapted | spare
//                 2648  PN_CALL_W_LIM       4 u32   gain | hold | limited | spare
//                 2652  PN_CALL_W_MIX       4       the held level f32 | 3 zero words
// Section mask: PN_CALL_PLC (hist, q, meta) | PN_CALL_AGC | PN_CALL_LIM | PN_CALL_MIX — the states the exporting converter held.  A
// section whose bit is clear is all zero.
//
// The verdict, in this order: magic (PN_SS_BAD_MAGIC), version (PN_SS_BAD_VERSION), the size word (PN_SS_BAD_SIZE), then
// PN_SS_BAD_STATE for a mask with an unknown bit, for a present section that breaks an invariant its kernel relies on, and for an
// absent section that is not all zero:
//   PLC   P == 0 or PN_PLC_P_MIN <= P <= PN_PLC_P_MAX; r > 0 implies P != 0 (syn() indexes q[m % P]); word 3 is 0
//   AGC   lev is not NaN and >= 0; the gain's bits are 0 (fresh) or a finite value in [1/1024, 1024] — the widest [Gmin, max(Gmax, 1)]
//         pn_agc_params_check accepts; the spare word is 0
//   LIM   the gain's bits are 0 (fresh) or a value in (0, 1] — the premise of the |out| <= ceiling proof of pn_lim_rules.h; the spare
//         word is 0
//   MIX   the level is finite and >= 0; the three padding words are 0
// pn_call_verdict is free of side effects and of memory accesses: it takes the four header words, the sixteen words behind the
// period buffer and ONE bit that says whether any of the 2640 words of hist and q is non-zero — the only part of the check that
// reads the bulk of a record, and the one the kernel's whole block computes together.
#pragma once
#include "pn_lim_rules.h"    // and through it pn_agc_rules.h, pn_mix_rules.h, pn_host_rules.h: pn_le32, pn_set_error, the header's constants
#include "pn_plc_rules.h"

#if defined(__HIPCC__)
#define PN_CALL_HD __host__ __device__
#else
#define PN_CALL_HD
#endif

#define PN_CALL_HEADER_WORDS 4
#define PN_CALL_TAIL_WORDS 16                  // meta, AGC, LIM, MIX: the words the verdict reads one by one
#define PN_CALL_ALL (PN_CALL_PLC | PN_CALL_AGC | PN_CALL_LIM | PN_CALL_MIX)
static_assert(PN_CALL_W_HIST == 0 && PN_CALL_W_Q == PN_PLC_HIST && PN_CALL_W_META == PN_CALL_W_Q + PN_PLC_P_MAX && PN_CALL_W_AGC == PN_CALL_W_META + 4 &&
              PN_CALL_W_LIM == PN_CALL_W_AGC + PN_AGC_STATE_BYTES / 4 && PN_CALL_W_MIX == PN_CALL_W_LIM + PN_LIM_STATE_BYTES / 4 &&
              PN_CALL_BODY_WORDS == PN_CALL_W_MIX + 4 && PN_CALL_BODY_WORDS == PN_CALL_W_META + PN_CALL_TAIL_WORDS &&
              PN_RATE_CALL_STATE_BYTES == 4 * (PN_CALL_HEADER_WORDS + PN_CALL_BODY_WORDS) && PN_RATE_CALL_STATE_BYTES == 10640 &&
              PN_RATE_CALL_STATE_BYTES == 16 + PN_PLC_STATE_BYTES + PN_AGC_STATE_BYTES + PN_LIM_STATE_BYTES + 16 && PN_CALL_W_Q % 4 == 0 && PN_CALL_W_META % 4 == 0,
              "a header, the three states at their own sizes and one group for the level, each 16-byte aligned");

PN_CALL_HD static inline float pn_call_f32(uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(bits);
#else
  float v; memcpy(&v, &bits, 4); return v;
#endif
}
// hdr: the four header words; t: the sixteen words from PN_CALL_W_META on; bulk_nonzero: some word of hist or q is not 0
PN_CALL_HD static inline int pn_call_verdict(const uint32_t hdr[PN_CALL_HEADER_WORDS], const uint32_t t[PN_CALL_TAIL_WORDS], bool bulk_nonzero) {
  if (hdr[0] != PN_RATE_CALL_MAGIC) return PN_SS_BAD_MAGIC;
  if (hdr[1] != PN_RATE_CALL_VERSION) return PN_SS_BAD_VERSION;
  if (hdr[2] != PN_RATE_CALL_STATE_BYTES) return PN_SS_BAD_SIZE;
  const uint32_t mask = hdr[3];
  if (mask & ~(uint32_t)PN_CALL_ALL) return PN_SS_BAD_STATE;
  const uint32_t *m = t, *a = t + 4, *l = t + 8, *x = t + 12;
  if (mask & PN_CALL_PLC) {
    const uint32_t P = m[0], r = m[1];
    if (P != 0u && (P < (uint32_t)PN_PLC_P_MIN || P > (uint32_t)PN_PLC_P_MAX)) return PN_SS_BAD_STATE;
    if (r > 0u && P == 0u) return PN_SS_BAD_STATE;
    if (m[3] != 0u) return PN_SS_BAD_STATE;
  } else if (bulk_nonzero || (m[0] | m[1] | m[2] | m[3])) return PN_SS_BAD_STATE;
  if (mask & PN_CALL_AGC) {
    const float lev = pn_call_f32(a[0]), g = pn_call_f32(a[1]);
    if (!(lev >= 0.0f)) return PN_SS_BAD_STATE;                                     // (false for NaN)
    if (a[1] != 0u && !(g >= 1.0f / 1024.0f && g <= 1024.0f)) return PN_SS_BAD_STATE;
    if (a[3] != 0u) return PN_SS_BAD_STATE;
  } else if (a[0] | a[1] | a[2] | a[3]) return PN_SS_BAD_STATE;
  if (mask & PN_CALL_LIM) {
    const float g = pn_call_f32(l[0]);
    if (l[0] != 0u && !(g > 0.0f && g <= 1.0f)) return PN_SS_BAD_STATE;
    if (l[3] != 0u) return PN_SS_BAD_STATE;
  } else if (l[0] | l[1] | l[2] | l[3]) return PN_SS_BAD_STATE;
  if (mask & PN_CALL_MIX) {
    const float lv = pn_call_f32(x[0]);
    if (!(lv >= 0.0f && lv <= FLT_MAX)) return PN_SS_BAD_STATE;
    if (x[1] | x[2] | x[3]) return PN_SS_BAD_STATE;
  } else if (x[0] | x[1] | x[2] | x[3]) return PN_SS_BAD_STATE;
  return PN_SS_OK;
}

// is `bytes` bytes at `record` one call-state record?  Reads the record only when all of it is there.  The verdict is
// pn_call_verdict's; this function adds the NULL pointer, the length of the buffer and the words.
static inline int pn_call_record_check(const void *record, size_t bytes) {
  if (!record) { pn_set_error("NULL argument"); return PN_SS_BAD_ARG; }
  const unsigned char *r = static_cast<const unsigned char *>(record);
  if (bytes < 16) { pn_set_error("call-state record of %zu bytes: a record has %d", bytes, PN_RATE_CALL_STATE_BYTES); return PN_SS_BAD_SIZE; }
  uint32_t hdr[PN_CALL_HEADER_WORDS], t[PN_CALL_TAIL_WORDS] = {0};
  for (int i = 0; i < PN_CALL_HEADER_WORDS; i++) hdr[i] = pn_le32(r + 4 * i);
  bool bulk = false;
  const bool whole = bytes == PN_RATE_CALL_STATE_BYTES;
  if (whole) {
    const unsigned char *body = r + 4 * PN_CALL_HEADER_WORDS;
    for (int i = 0; i < PN_CALL_TAIL_WORDS; i++) t[i] = pn_le32(body + 4 * (PN_CALL_W_META + i));
    for (size_t i = 0; i < 4 * (size_t)PN_CALL_W_META; i++) bulk |= body[i] != 0;
  }
  // (the header's own verdicts come first, whatever the buffer's length; a short or long buffer never reaches the body's)
  int v = pn_call_verdict(hdr, t, bulk);
  if (v == PN_SS_BAD_MAGIC || v == PN_SS_BAD_VERSION) return pn_record_header_check(r, bytes, PN_RATE_CALL_MAGIC, PN_RATE_CALL_VERSION, "call-state");   // (words it)
  if (v == PN_SS_BAD_SIZE || !whole) {
    pn_set_error("call-state record of %zu bytes (header: %u), a record has %d", bytes, hdr[2], PN_RATE_CALL_STATE_BYTES);
    return PN_SS_BAD_SIZE;
  }
  if (v == PN_SS_BAD_STATE) {
    const uint32_t mask = hdr[3];
    const float ag = pn_call_f32(t[5]), lg = pn_call_f32(t[8]);
    if (mask & ~(uint32_t)PN_CALL_ALL) pn_set_error("call-state record with section mask 0x%x: the sections are 0x%x", mask, PN_CALL_ALL);
    else pn_set_error("call-state record (sections 0x%x) breaks an invariant of its state or carries words in an absent section: PLC P %u r %u word3 %u, "
                      "AGC gain %g spare %u, limiter gain %g spare %u", mask, t[0], t[1], t[3], (double)ag, t[7], (double)lg, t[11]);
  }
  return v;
}
