// G.711 companding, the 8-bit sample format of the rate converter's edges (include/percepnet_hip.h "G.711 streams"), described
// once — HIP-free (builds with -DPN_NO_HIP) and usable from device code: the kernels of pn_rate.hip, the host entry points
// pn_g711_decode / pn_g711_encode (pn_rate.cpp) and the numpy model tests/g711_model.py are the same integer formulas, checked
// on the CPU by tests/c/g711_sanitize.cpp under the sanitizers and by tests/test_g711_host.py through the C-ABI.
// Formulas, not tables: a lane needs no LDS traffic, and floor(log2 x) of the encoders is one count-leading-zeros.
// All values are int32; b is the byte, v the linear value in the int16 range.
//   decode  mu-law  u = ~b & 0xFF, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 132) << e) - 132, v = (u & 0x80) ? -mag : mag
//                   +-32124; 0xFF and 0x7F both give 0
//           A-law   a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15, mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 264) << (e - 1),
//                   v = (a & 0x80) ? mag : -mag      +-32256, never 0
//   encode  the one's-complement magnitude of the ITU software tool library, for both laws: neg = v < 0, mag = neg ? ~v : v
//           mu-law  p = min((mag >> 2) + 33, 8191), e = floor(log2 p) - 5, m = (p >> (e + 1)) & 15, b = ~(sign | e << 4 | m) & 0xFF
//           A-law   e = mag < 256 ? 0 : floor(log2 mag) - 7, m = (e == 0 ? mag >> 4 : mag >> (e + 3)) & 15, b = (sign | e << 4 | m) ^ 0x55
#pragma once
#include "pn_host_rules.h"   // pn_ids_check, pn_set_error, PN_G711_ULAW / PN_G711_ALAW

#ifdef PN_NO_HIP
#define PN_G711_FN static inline
#else
#define PN_G711_FN __host__ __device__ __forceinline__
#endif

PN_G711_FN bool pn_g711_law_ok(int law) { return law == PN_G711_ULAW || law == PN_G711_ALAW; }

PN_G711_FN int32_t pn_g711_dec_ulaw(uint32_t b) {
  const int32_t u = (int32_t)(~b & 0xFFu), e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 132) << e) - 132;
  return (u & 0x80) ? -mag : mag;
}
PN_G711_FN int32_t pn_g711_dec_alaw(uint32_t b) {
  const int32_t a = (int32_t)((b ^ 0x55u) & 0xFFu), e = (a >> 4) & 7, m = a & 15;
  const int32_t mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 264) << (e - 1);
  return (a & 0x80) ? mag : -mag;
}
// floor(log2 x), x > 0
PN_G711_FN int32_t pn_g711_log2(int32_t x) { return 31 - __builtin_clz((uint32_t)x); }
PN_G711_FN uint32_t pn_g711_enc_ulaw(int32_t v) {
  const bool neg = v < 0;
  const int32_t mag = neg ? ~v : v;
  int32_t p = (mag >> 2) + 33;
  if (p > 8191) p = 8191;
  const int32_t e = pn_g711_log2(p) - 5, m = (p >> (e + 1)) & 15;
  return (uint32_t)~((neg ? 0x80 : 0) | e << 4 | m) & 0xFFu;
}
PN_G711_FN uint32_t pn_g711_enc_alaw(int32_t v) {
  const bool neg = v < 0;
  const int32_t mag = neg ? ~v : v;
  const int32_t e = mag < 256 ? 0 : pn_g711_log2(mag) - 7, m = (e == 0 ? mag >> 4 : mag >> (e + 3)) & 15;
  return (uint32_t)(((neg ? 0 : 0x80) | e << 4 | m) ^ 0x55);
}
PN_G711_FN int32_t pn_g711_dec(int law, uint32_t b) { return law == PN_G711_ALAW ? pn_g711_dec_alaw(b) : pn_g711_dec_ulaw(b); }
PN_G711_FN uint32_t pn_g711_enc(int law, int32_t v) { return law == PN_G711_ALAW ? pn_g711_enc_alaw(v) : pn_g711_enc_ulaw(v); }

// ---- host rules ------------------------------------------------------------------------------------------------------------------
// n samples of one law, host memory.  -1 for a law that is neither of the two or a NULL pointer (nothing read or written).
static inline int pn_g711_decode_host(int law, const uint8_t *in, int16_t *out, size_t n) {
  if (!pn_g711_law_ok(law)) { pn_set_error("G.711 law %d: PN_G711_ULAW (0) or PN_G711_ALAW (1)", law); return -1; }
  if (!in || !out) { pn_set_error("NULL argument"); return -1; }
  for (size_t i = 0; i < n; i++) out[i] = (int16_t)pn_g711_dec(law, in[i]);
  return 0;
}
static inline int pn_g711_encode_host(int law, const int16_t *in, uint8_t *out, size_t n) {
  if (!pn_g711_law_ok(law)) { pn_set_error("G.711 law %d: PN_G711_ULAW (0) or PN_G711_ALAW (1)", law); return -1; }
  if (!in || !out) { pn_set_error("NULL argument"); return -1; }
  for (size_t i = 0; i < n; i++) out[i] = (uint8_t)pn_g711_enc(law, in[i]);
  return 0;
}
// laws[0..n): every one of the two.  -1 with pn_last_error naming the FIRST bad index; n == 0 is a legal list.
static inline int pn_g711_laws_list_check(const int32_t *laws, int n) {
  if (n < 0 || (n > 0 && !laws)) { pn_set_error("bad argument"); return -1; }
  for (int i = 0; i < n; i++)
    if (!pn_g711_law_ok(laws[i])) {
      pn_set_error("G.711 law %d at index %d: PN_G711_ULAW (0) or PN_G711_ALAW (1)", (int)laws[i], i);
      return -1;
    }
  return 0;
}
// A law change: ids[0..n) distinct streams of a batch of B (pn_ids_check), laws[i] the new law of ids[i].
static inline int pn_g711_laws_set_check(int B, const int32_t *ids, int n, const int32_t *laws) {
  if (pn_ids_check(B, ids, n, true)) return -1;
  return pn_g711_laws_list_check(laws, n);
}
