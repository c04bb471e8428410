// CPU-only sanitizer harness of the G.711 companding (tests/test_g711_host.py builds it with
// g++ -DPN_NO_HIP -fsanitize=address,undefined, like rate_sanitize.cpp): pn_g711.h's functions over every code and every value
// into exactly-sized heap buffers, so that a read or write past what a caller handed in aborts and a shift or an overflow the
// formulas do not intend is reported; n = 0; and hostile lists of laws and ids.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_g711.h"
#include <stdio.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "g711_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

int main() {
  const int laws[2] = {PN_G711_ULAW, PN_G711_ALAW};
  const int range[2] = {32124, 32256}, max_err[2] = {644, 512};
  for (int li = 0; li < 2; li++) {
    const int law = laws[li];
    // every code, into exactly 256 values
    std::vector<uint8_t> codes(256);
    for (int b = 0; b < 256; b++) codes[b] = (uint8_t)b;
    std::vector<int16_t> lin(256);
    CHECK(pn_g711_decode_host(law, codes.data(), lin.data(), 256) == 0);
    int lo = 0, hi = 0;
    for (int b = 0; b < 256; b++) {
      CHECK(lin[b] == pn_g711_dec(law, (uint32_t)b));
      if (lin[b] < lo) lo = lin[b];
      if (lin[b] > hi) hi = lin[b];
      if (law == PN_G711_ALAW) CHECK(lin[b] != 0);
    }
    CHECK(hi == range[li] && lo == -range[li]);
    // ... and back: every byte is its own code, but for the second mu-law zero
    std::vector<uint8_t> back(256);
    CHECK(pn_g711_encode_host(law, lin.data(), back.data(), 256) == 0);
    for (int b = 0; b < 256; b++) CHECK(back[b] == (law == PN_G711_ULAW && b == 0x7F ? 0xFF : b));
    // every value, into exactly 65 536 bytes; the round trip is monotonic and within the law's largest step
    std::vector<int16_t> all(65536);
    for (int v = -32768; v <= 32767; v++) all[v + 32768] = (int16_t)v;
    std::vector<uint8_t> enc(65536);
    CHECK(pn_g711_encode_host(law, all.data(), enc.data(), 65536) == 0);
    int prev = -40000, worst = 0;
    for (int v = -32768; v <= 32767; v++) {
      CHECK(enc[v + 32768] == pn_g711_enc(law, v));
      const int d = pn_g711_dec(law, enc[v + 32768]);
      CHECK(d >= prev);
      prev = d;
      const int e = d > v ? d - v : v - d;
      if (e > worst) worst = e;
    }
    CHECK(worst == max_err[li]);
    // n = 0: legal, touches nothing (buffers of one element that must keep their values)
    { std::vector<uint8_t> b1(1, 0xAB); std::vector<int16_t> v1(1, 1234);
      CHECK(pn_g711_decode_host(law, b1.data(), v1.data(), 0) == 0 && v1[0] == 1234);
      CHECK(pn_g711_encode_host(law, v1.data(), b1.data(), 0) == 0 && b1[0] == 0xAB); }
    // NULL is refused whatever n
    { std::vector<uint8_t> b1(1, 0xAB); std::vector<int16_t> v1(1, 1234);
      CHECK(pn_g711_decode_host(law, NULL, v1.data(), 1) == -1 && pn_g711_decode_host(law, b1.data(), NULL, 1) == -1 && v1[0] == 1234);
      CHECK(pn_g711_encode_host(law, NULL, b1.data(), 1) == -1 && pn_g711_encode_host(law, v1.data(), NULL, 1) == -1 && b1[0] == 0xAB);
      CHECK(pn_g711_decode_host(law, NULL, NULL, 0) == -1 && pn_g711_encode_host(law, NULL, NULL, 0) == -1); }
  }
  // known answers
  CHECK(pn_g711_enc_ulaw(0) == 0xFF && pn_g711_enc_ulaw(-1) == 0x7F && pn_g711_enc_ulaw(32767) == 0x80 && pn_g711_enc_ulaw(-32768) == 0x00);
  CHECK(pn_g711_enc_ulaw(-4) == 0x7F && pn_g711_enc_ulaw(-5) == 0x7E);
  CHECK(pn_g711_enc_alaw(0) == 0xD5 && pn_g711_enc_alaw(-1) == 0x55 && pn_g711_enc_alaw(32767) == 0xAA && pn_g711_enc_alaw(-32768) == 0x2A);
  CHECK(pn_g711_dec_ulaw(0xFF) == 0 && pn_g711_dec_ulaw(0x7F) == 0 && pn_g711_dec_alaw(0xD5) == 8 && pn_g711_dec_alaw(0x55) == -8);
  // a bad law: nothing read or written
  for (int bad : {-1, 2, 255, 0x7fffffff, (int)0x80000000}) {
    std::vector<uint8_t> b1(1, 0xAB); std::vector<int16_t> v1(1, 1234);
    CHECK(!pn_g711_law_ok(bad));
    CHECK(pn_g711_decode_host(bad, b1.data(), v1.data(), 1) == -1 && v1[0] == 1234);
    CHECK(pn_g711_encode_host(bad, v1.data(), b1.data(), 1) == -1 && b1[0] == 0xAB);
  }
  // lists of laws, exactly sized: the first bad index is named
  { std::vector<int32_t> w = {0, 1, 1, 0, 1};
    CHECK(pn_g711_laws_list_check(w.data(), 5) == 0 && pn_g711_laws_list_check(w.data(), 0) == 0 && pn_g711_laws_list_check(NULL, 0) == 0);
    CHECK(pn_g711_laws_list_check(NULL, 3) == -1 && pn_g711_laws_list_check(w.data(), -1) == -1);
    for (int at = 0; at < 5; at++)
      for (int32_t bad : {2, -1, 8000, (int32_t)0x80000000}) {
        std::vector<int32_t> t(w);
        t[at] = bad;
        if (at < 4) t[4] = 7;                                  // a later bad one is not the one named
        CHECK(pn_g711_laws_list_check(t.data(), 5) == -1);
        char want[32];
        snprintf(want, sizeof(want), "at index %d:", at);
        CHECK(strstr(pn_last_error(), want) != NULL);
      } }
  // a law change: the id rule first (distinct, in range), then the laws
  { const int B = 5;
    std::vector<int32_t> ids = {4, 0, 2}, w = {1, 0, 1};
    CHECK(pn_g711_laws_set_check(B, ids.data(), 3, w.data()) == 0);
    CHECK(pn_g711_laws_set_check(B, ids.data(), 0, NULL) == 0 && pn_g711_laws_set_check(B, NULL, 0, NULL) == 0);
    CHECK(pn_g711_laws_set_check(B, ids.data(), 3, NULL) == -1);
    CHECK(pn_g711_laws_set_check(B, NULL, 3, w.data()) == -1);
    { std::vector<int32_t> t = {4, 0, 4}; CHECK(pn_g711_laws_set_check(B, t.data(), 3, w.data()) == -1 && strstr(pn_last_error(), "twice")); }
    { std::vector<int32_t> t = {4, 5, 2}; CHECK(pn_g711_laws_set_check(B, t.data(), 3, w.data()) == -1 && strstr(pn_last_error(), "out of range")); }
    { std::vector<int32_t> t = {4, -1, 2}; CHECK(pn_g711_laws_set_check(B, t.data(), 3, w.data()) == -1); }
    { std::vector<int32_t> t = {0, 1, 2, 3, 4, 0}, w6(6, 0); CHECK(pn_g711_laws_set_check(B, t.data(), 6, w6.data()) == -1); }
    { std::vector<int32_t> t = {1, 0, 2}; CHECK(pn_g711_laws_set_check(B, ids.data(), 3, t.data()) == -1 && strstr(pn_last_error(), "at index 2:")); } }
  puts("ok");
  return 0;
}
