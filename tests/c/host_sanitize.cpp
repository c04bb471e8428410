// CPU-only sanitizer harness (tests/test_hardening.py builds it with g++ -fsanitize=address,undefined -DPN_NO_HIP): the
// HIP-free host pieces of libpercepnet_hip — the PNW1 / RNNModel parsers (pn_model.cpp), the table builder (pn_tables.cpp),
// the weight packers (pn_pack.cpp) and the CLI helpers (pn_cli_util.h) — driven with valid, truncated, oversized and
// corrupted inputs; the table of a context's per-stream state (pn_state_layout.h): record offsets, ring phases, classes; the DSP
// half of a frame (pn_dsp_layout.h): slots, side entries, front-end families, profiling families; and the
// table of the network's layers (pn_network.h): kernel, weight format, shadows and launch geometry of every layer under every plan;
// and the host rules of the C-ABI (pn_host_rules.h): id lists in exactly-sized heap arrays, the header verdicts of a stream-state record.
// Any out-of-bounds access, overflow or leak-free violation aborts; the process prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"
#include "../../percepnet_amd/csrc/pn_pack.cpp"
#include "../../percepnet_amd/csrc/pn_tables.cpp"
#include "../../percepnet_amd/csrc/pn_cli_util.h"
#include "../../percepnet_amd/csrc/pn_network.h"
#include "../../percepnet_amd/csrc/pn_host_rules.h"
#include <stdio.h>
#include <string>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "host_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: host_sanitize <model.pnw>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  CHECK(f);
  std::vector<unsigned char> blob;
  unsigned char tmp[65536]; size_t n;
  while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) blob.insert(blob.end(), tmp, tmp + n);
  rewind(f);

  // tables
  { PnTables *t = new PnTables(); CHECK(pn_build_tables(t) == 0); CHECK(t->border[PN_NB - 1] == PN_SPEC_BINS); CHECK(t->tansig[200] > 0.999f); delete t; }

  // the state table.  Records: every entry with a record offset starts at its public PN_SS_* constant, the sections are
  // contiguous in offset order, and with the four tail words they fill the body
  { const int want[PN_SS_NSEC] = {PN_SS_HIST, PN_SS_SPEC, PN_SS_EY, PN_SS_CONV1, PN_SS_CONV2, PN_SS_GRU, PN_SS_GRU + 512, PN_SS_GRU + 1024,
                                  PN_SS_GRU + 1536, PN_SS_GRU_RB, PN_SS_SYNTH};
    int off = 0, nrec = 0;
    for (int k = 0; k < PN_SS_NSEC; k++)                     // section k = the entry with the k-th smallest offset
      for (int e = 0; e < PN_ST_COUNT; e++) {
        const PnStateEntry &L = pn_kState[e];
        if (pn_state_section(e) != k) continue;
        CHECK(L.rec_off == want[k]); CHECK(L.rec_off == off);
        off += L.live * L.cols; nrec++;
      }
    for (int e = 0; e < PN_ST_COUNT; e++) CHECK((pn_kState[e].rec_off >= 0) == (pn_state_section(e) >= 0));
    CHECK(nrec == PN_SS_NSEC); CHECK(off == PN_SS_TAIL); CHECK(off + 4 == PN_SS_BODY_WORDS); CHECK(PN_SS_BODY_WORDS == 13656); }
  // classes agree with the geometry; and the ring phases the active-set fix-up and the records both rest on: the slot a frame
  // writes is not live, after the frame `first` has advanced by one and the slot written is the newest live one
  for (int e = 0; e < PN_ST_COUNT; e++) {
    const PnStateEntry &L = pn_kState[e];
    CHECK(L.slots >= 1 && L.cols >= 1 && L.row_words >= (L.in_row ? L.slots : 1) * L.cols);
    if (L.cls == PN_CLS_RING) { CHECK(L.slots >= 2 && L.live == L.slots - 1); CHECK(L.counter == PN_CNT_T || L.counter == PN_CNT_TN); }
    else { CHECK(L.cls == PN_CLS_INPLACE || L.cls == PN_CLS_SCRATCH); CHECK(L.slots == 1 && L.live == 1 && L.counter == PN_CNT_NONE); }
    if (L.shadow != PN_SH_NONE) CHECK(L.padded && L.cols % 32 == 0 && L.cols == L.row_words);      // fragment-order shadows: whole column tiles of Bp rows
    if (L.cls != PN_CLS_RING) continue;
    for (int64_t t = 0; t < 24; t++)
      for (int64_t tn : {t, t + 1, t + 7}) {
        const int first = pn_state_first(L, t, tn), wr = pn_state_write(L, t, tn);
        CHECK(first >= 0 && first < L.slots && wr >= 0 && wr < L.slots);
        for (int j = 0; j < L.live; j++) CHECK((first + j) % L.slots != wr);
        CHECK(pn_state_first(L, t + 1, tn + 1) == (first + 1) % L.slots);
        CHECK((pn_state_first(L, t + 1, tn + 1) + L.live - 1) % L.slots == wr);
      }
  }

  // the DSP half of a frame.  The slots a launcher is handed are the phases the kernels were written against, and what the
  // back end reads at slot_r is where state_at (pn_context.h) puts the oldest live entry (j = 0) of a context's yring / eyring:
  // p + (first + j) % slots * slot_stride, with the stride a context keeps in st[] (pn_state_size of B rows)
  { float y[1], ey[1], *base[PN_ST_COUNT] = {};
    base[PN_ST_YRING] = y; base[PN_ST_EYRING] = ey;
    const size_t B = 19;
    const PnDspSide s = pn_dsp_side(base, NULL, B);
    for (int64_t t = 0; t < 48; t++) {
      const PnDspSlots k = pn_dsp_slots(t);
      CHECK(k.frame_t == t % 12 && k.slot_w == t % 6 && k.slot_r == (t + 1) % 6);
      CHECK((const float *)pn_dsp_spec(s, k.slot_r) == y + (t % 6 + 1 + 0) % 6 * (long long)(B * 2 * PN_SPEC_BINS));
      CHECK(pn_dsp_bands(s, k.slot_r) == ey + (t % 6 + 1 + 0) % 6 * (long long)(B * 36));
    } }
  // a side is exactly the table's non-network entries other than synth (the back end's), none of them shadowed
  { int n = 0;
    for (int e = 0; e < PN_ST_COUNT; e++) {
      bool in_side = false;
      for (int f : pn_kSideEntries) in_side = in_side || f == e;
      CHECK(in_side == (e < PN_ST_C1RING && e != PN_ST_SYNTH));
      if (in_side) { n++; CHECK(pn_kState[e].shadow == PN_SH_NONE); }
    }
    CHECK(n == 8 && sizeof(pn_kSideEntries) / sizeof(int) == 8);
    float buf[PN_ST_COUNT], *base[PN_ST_COUNT];
    for (int e = 0; e < PN_ST_COUNT; e++) base[e] = &buf[e];
    const PnDspSide s = pn_dsp_side(base, NULL, 19);
    CHECK(s.hist == base[PN_ST_HIST] && s.last_gain == base[PN_ST_LAST_GAIN] && (float *)s.last_period == base[PN_ST_LAST_PERIOD] && (float *)s.silence == base[PN_ST_SILENCE]);
    CHECK((float *)s.yring == base[PN_ST_YRING] && s.eyring == base[PN_ST_EYRING] && (float *)s.Ps == base[PN_ST_PS] && s.feat == base[PN_ST_FEAT] && !s.aux && s.rows == 19);
    CHECK((const float *)pn_dsp_spec(s, 2) == base[PN_ST_YRING] + 2 * pn_state_size(pn_kState[PN_ST_YRING], 19).slot_stride);
    CHECK(pn_dsp_bands(s, 5) == base[PN_ST_EYRING] + 5 * pn_state_size(pn_kState[PN_ST_EYRING], 19).slot_stride);
    // sizes: one side of a feature-generator pair is 47 148 bytes with its aux row
    size_t words = PN_AUX_STRIDE;
    for (int e : pn_kSideEntries) words += pn_state_size(pn_kState[e], 1).words;
    CHECK(words * 4 == 47148);
    CHECK(pn_state_size(pn_kState[PN_ST_HIST], 7).words == 7 * PN_HIST_STRIDE && pn_state_size(pn_kState[PN_ST_HIST], 7).slot_stride == PN_FRAME);
    CHECK(pn_state_size(pn_kState[PN_ST_C1RING], 256).words == 5 * 256 * 128 && pn_state_size(pn_kState[PN_ST_C1RING], 256).slot_stride == 256 * 128); }
  // the front-end families and the profiling families
  { CHECK(sizeof(pn_kFe) / sizeof(pn_kFe[0]) == 3);
    CHECK(pn_kFe[FE_MONO_G4].n == 1 && pn_kFe[FE_MONO_G2].n == 1 && pn_kFe[FE_SPLIT].n == 3);
    CHECK(pn_kFe[FE_MONO_G4].fam[0] == KF_FRONTEND && pn_kFe[FE_MONO_G2].fam[0] == KF_FRONTEND);
    CHECK(pn_kFe[FE_SPLIT].fam[0] == KF_FE_SPEC_IN && pn_kFe[FE_SPLIT].fam[1] == KF_FE_PITCH && pn_kFe[FE_SPLIT].fam[2] == KF_FE_SPEC_OUT);
    CHECK(!strcmp(pn_kFe[FE_MONO_G4].name, "g4") && !strcmp(pn_kFe[FE_MONO_G2].name, "g2") && !strcmp(pn_kFe[FE_SPLIT].name, "split"));
    const char *want[] = {"frontend", "fc", "conv1", "conv2", "gru512", "gru_rb", "fc_gb", "fc_rb", "backend", "fe_spec_in", "fe_pitch", "fe_spec_out"};
    CHECK(KF_COUNT == 12 && sizeof(pn_kFamilyName) / sizeof(pn_kFamilyName[0]) == 12);
    for (int i = 0; i < 12; i++) CHECK(!strcmp(pn_kFamilyName[i], want[i]));
    CHECK(!strcmp(pn_kFamilyName[KF_FRONTEND], "frontend") && !strcmp(pn_kFamilyName[KF_GRU512], "gru512") && !strcmp(pn_kFamilyName[KF_BACKEND], "backend") && !strcmp(pn_kFamilyName[KF_FE_SPEC_OUT], "fe_spec_out"));
    const int fam[PN_NLAYERS] = {KF_FC, KF_CONV1, KF_CONV2, KF_GRU512, KF_GRU512, KF_GRU512, KF_GRU512, KF_GRU_RB, KF_FC_GB, KF_FC_RB};
    for (int li = 0; li < PN_NLAYERS; li++) CHECK(pn_kNet[li].fam == fam[li]); }

  // the network table.  Every plan pn_plan_for can return — small and small_gru freely; narrow 1 outside STRICT, 2 in fp32 MFMA off
  // the small dense family; direct in fp32 MFMA off both small families; rg 1|2 with direct, 1|2|3 in the shadow-operand modes,
  // else 0 — in every mode: each layer's kernel is legal for the layer, reads the weight format the shared copy of (mode, narrow)
  // holds, packed with the column-tile rounding its launcher sizes its grid by, finds every shadow it reads or writes allocated, has a
// launcher for the layer's type, and is handed panels that launcher's rule (pn_kernel_geometry_ok, the launchers' own first call) accepts
  { int n_plans = 0;
    for (int mode : {PN_NN_MFMA, PN_NN_STRICT, PN_NN_MFMA_F16, PN_NN_MFMA_X3})
      for (int bits = 0; bits < 2 * 2 * 3 * 2 * 4; bits++) {
        PnPlan p = {FE_SPLIT, bits & 1, bits >> 1 & 1, bits / 4 % 3, bits / 12 & 1, bits / 24, 1};
        const bool f32 = mode == PN_NN_MFMA, x3 = pn_mode_x3(mode);
        if ((p.narrow == 1 && mode == PN_NN_STRICT) || (p.narrow == 2 && !(f32 && !p.small)) || (p.direct && !(f32 && !p.small && !p.small_gru))) continue;
        if (p.direct ? (p.rg < 1 || p.rg > 2) : (x3 ? p.rg < 1 : p.rg != 0)) continue;
        n_plans++;
        for (int li = 0; li < PN_NLAYERS; li++) {
          const PnNetLayer &R = pn_kNet[li];
          const int k = pn_layer_kernel(p, mode, li), N = pn_kGeom[li].nn;
          const bool gru = pn_kGeom[li].kind == PN_KIND_GRU;
          // (a) legal for the layer's type and the mode
          CHECK((k == PN_K_STRICT) == (mode == PN_NN_STRICT)); if (k == PN_K_X3) CHECK(x3);
          if (k == PN_K_N16 || k == PN_K_N48) CHECK(pn_layer_narrow(li) && N == PN_NB);
          if (k == PN_K_DIRECT || k == PN_K_BATCH_SH) CHECK(f32 && gru == (k == PN_K_DIRECT));
          // (b) the weights the kind reads are the ones built for (mode, narrow)
          CHECK(pn_kernel_weight_format(k) == pn_layer_weight_format(mode, p.narrow, li));
          CHECK(pn_kernel_ct_round(k, gru, N) == pn_layer_ct_round(mode, p.narrow, li));      // ... and so is their column-tile rounding
          // (c) shadows read (panels, GRU state) and written (the output; the gains that leave an x3 network have none) exist
          int width[5];
          for (int j = 0; j < R.n_in; j++) {
            width[j] = pn_kState[R.in[j].entry].cols;
            if (pn_kernel_reads_shadows(k)) CHECK(pn_state_shadowed(R.in[j].entry, p, mode));
          }
          if (pn_kernel_reads_shadows(k) && gru) CHECK(pn_state_shadowed(R.state, p, mode));
          if (pn_kernel_writes_shadow(k) && !(k == PN_K_X3 && R.out.entry == PN_ST_GR)) CHECK(pn_state_shadowed(R.out.entry, p, mode));
          // (d) the kind has a launcher for the layer's type (pn_network.cpp static_asserts its table of launchers against these
          // names), and that launcher's rule takes the panels
          CHECK(k >= 0 && k < PN_K_COUNT && pn_kernel_launcher(k, gru) != NULL);
          CHECK(pn_kernel_geometry_ok(k, gru, R.n_in, width, N) == 0);
        }
      }
    CHECK(n_plans == 4 + 2 * 24 + 16);
    // the rule is not vacuous: what each launcher is documented to refuse, it refuses (and a form that does not exist)
    const int w96[1] = {96}, w128[1] = {128}, w64[1] = {64};
    for (int k : {PN_K_BATCH, PN_K_BATCH_SH, PN_K_SMALL, PN_K_N48, PN_K_X3}) CHECK(pn_kernel_geometry_ok(k, false, 1, w96, 128) == -1);   // three K-tiles
    CHECK(pn_kernel_geometry_ok(PN_K_STRICT, false, 1, w96, 128) == 0);
    CHECK(pn_kernel_geometry_ok(PN_K_BATCH_SH, false, 1, w128, 34) == -1 && pn_kernel_geometry_ok(PN_K_BATCH, false, 1, w128, 34) == 0);
    CHECK(pn_kernel_geometry_ok(PN_K_N16, false, 1, w64, 34) == -1 && pn_kernel_geometry_ok(PN_K_N48, false, 1, w128, 49) == -1);
    CHECK(pn_kernel_geometry_ok(PN_K_X3, true, 1, w128, 96) == -1 && pn_kernel_geometry_ok(PN_K_DIRECT, true, 1, w128, 96) == -1);
    CHECK(pn_kernel_geometry_ok(PN_K_SMALL, true, 1, w96, 128) == -1 && pn_kernel_geometry_ok(PN_K_BATCH, true, 1, w96, 128) == 0);
    CHECK(pn_kernel_geometry_ok(PN_K_DIRECT, false, 1, w128, 128) == -1 && pn_kernel_geometry_ok(PN_K_N16, true, 1, w128, 128) == -1); }      // STRICT; fp16 operands, split precision; fp32 MFMA (6 direct, 4 small, 6 batch)

  // the id-list rule.  Every list is a heap array of exactly n ids, so that a read past ids[n - 1] aborts
  for (int B : {1, 5}) {
    typedef std::vector<int32_t> Ids;
    std::vector<uint8_t> mark(3, 7);                           // wrong size, stale content: the rule resizes and clears it
    auto ok = [&](const Ids &v, bool distinct, std::vector<uint8_t> *m = NULL) { return pn_ids_check(B, v.empty() ? NULL : v.data(), (int)v.size(), distinct, m) == 0; };
    auto says = [&](const std::string &want) { return std::string(pn_last_error()) == want; };
    const std::string range = " out of range [0, " + std::to_string(B) + ")";
    for (bool distinct : {false, true}) {
      CHECK(ok(Ids(), distinct));                              // empty list, with and without a pointer
      { Ids one(1, 0); CHECK(pn_ids_check(B, one.data(), 0, distinct) == 0); }
      CHECK(pn_ids_check(B, NULL, 1, distinct) == -1 && says("bad argument"));
      { Ids one(1, 0); CHECK(pn_ids_check(B, one.data(), -1, distinct) == -1 && says("bad argument")); }
      CHECK(pn_ids_check(B, NULL, -1, distinct) == -1 && says("bad argument"));
      for (int bad : {-1, B})                                  // out of range at the first and at the last position of a list of B
        for (int pos : {0, B - 1}) {
          Ids v(B); for (int i = 0; i < B; i++) v[i] = i;
          v[pos] = bad;
          CHECK(!ok(v, distinct) && says("stream id " + std::to_string(bad) + range));
        }
      Ids perm(B); for (int i = 0; i < B; i++) perm[i] = (2 * i + 1) % B;      // (2 is coprime to 1 and 5)
      CHECK(ok(perm, distinct, &mark));
      if (distinct) { CHECK(mark.size() == (size_t)B); for (int i = 0; i < B; i++) CHECK(mark[i] == 1); }
      else CHECK(mark.size() == 3 && mark[0] == 7);            // not distinct: the marks are not the rule's business
    }
    { Ids dup(2, B - 1);                                       // a duplicate: legal where the streams are only reset or read
      CHECK(ok(dup, false));
      if (B >= 2) CHECK(!ok(dup, true) && says("stream id " + std::to_string(B - 1) + " listed twice"));
      Ids over(B + 1, 0);                                      // a distinct list longer than B is refused by its count ...
      CHECK(!ok(over, true) && says(std::to_string(B + 1) + " stream ids in a context of " + std::to_string(B)));
      CHECK(ok(over, false));                                  // ... a list that may repeat is not
      over[B] = B; CHECK(!ok(over, true) && says(std::to_string(B + 1) + " stream ids in a context of " + std::to_string(B)));   // count before ids
      if (B >= 3) { Ids v = {1, 1, B}; CHECK(!ok(v, true) && says("stream id 1 listed twice")); }      // list order: the duplicate comes first
      if (B >= 3) { Ids v = {B, 1, 1}; CHECK(!ok(v, true) && says("stream id " + std::to_string(B) + range)); } }
    if (B == 5) {                                              // the marks are exactly the listed set, and a shorter list leaves none behind
      Ids a = {4, 0, 2}, b = {3};
      CHECK(ok(a, true, &mark)); CHECK(mark == std::vector<uint8_t>({1, 0, 1, 0, 1}));
      CHECK(ok(b, true, &mark)); CHECK(mark == std::vector<uint8_t>({0, 0, 0, 1, 0}));
      CHECK(ok(Ids(), true, &mark)); CHECK(mark == std::vector<uint8_t>(5, 0));
    }
  }

  // the record-header rule, for the stream-state record: a valid header, every length that cannot hold one, and every single-byte
  // corruption of bytes 0..47 against the verdict of its field in the documented order (magic, version, size, model)
  { unsigned char digest[32];
    for (int i = 0; i < 32; i++) digest[i] = (unsigned char)(37 * i + 11);
    uint32_t hdr[16];
    ss_header(hdr, digest, PN_NN_MFMA_X3);
    CHECK(hdr[0] == PN_STREAM_STATE_MAGIC && hdr[1] == PN_STREAM_STATE_VERSION && hdr[2] == PN_STREAM_STATE_BYTES && hdr[3] == (uint32_t)PN_NN_MFMA_X3);
    std::vector<unsigned char> rec(PN_STREAM_STATE_BYTES, 0);
    memcpy(rec.data(), hdr, sizeof(hdr));
    CHECK(rec[0] == 'P' && rec[1] == 'N' && rec[2] == 'S' && rec[3] == 'S');
    CHECK(ss_check_host(rec.data(), rec.size(), digest) == PN_SS_OK);
    for (size_t len = 0; len < 16; len++) {                    // exact-size heap copies: a read past the end aborts
      std::vector<unsigned char> t(rec.begin(), rec.begin() + len);
      CHECK(ss_check_host(len ? t.data() : (const void *)"", len, digest) == PN_SS_BAD_SIZE);
      CHECK(pn_record_header_check(len ? t.data() : (const unsigned char *)"", len, PN_STREAM_STATE_MAGIC, PN_STREAM_STATE_VERSION, "stream-state") == PN_SS_BAD_SIZE);
    }
    for (size_t len : {(size_t)16, (size_t)48, (size_t)64, rec.size() - 1}) {      // holds the words read first, is no record
      std::vector<unsigned char> t(rec.begin(), rec.begin() + len);
      CHECK(ss_check_host(t.data(), len, digest) == PN_SS_BAD_SIZE);
    }
    { std::vector<unsigned char> t(rec); t.push_back(0); CHECK(ss_check_host(t.data(), t.size(), digest) == PN_SS_BAD_SIZE); }
    for (int b = 0; b < 48; b++)
      for (int bit = 0; bit < 8; bit++) {
        std::vector<unsigned char> t(rec);
        t[b] ^= (unsigned char)(1 << bit);
        const int want = b < 4 ? PN_SS_BAD_MAGIC : b < 8 ? PN_SS_BAD_VERSION : b < 12 ? PN_SS_BAD_SIZE : b < 16 ? PN_SS_OK : PN_SS_BAD_MODEL;
        CHECK(ss_check_host(t.data(), t.size(), digest) == want);      // (word 3, the source's nn_mode, is not compared)
      }
    // the order of the verdicts: a record wrong in every field is refused for its magic, then its version, then its size, then its model
    { std::vector<unsigned char> t(rec);
      t[0] ^= 1; t[4] ^= 1; t[8] ^= 1; t[16] ^= 1;
      CHECK(ss_check_host(t.data(), t.size(), digest) == PN_SS_BAD_MAGIC); t[0] ^= 1;
      CHECK(ss_check_host(t.data(), t.size(), digest) == PN_SS_BAD_VERSION); t[4] ^= 1;
      CHECK(ss_check_host(t.data(), t.size(), digest) == PN_SS_BAD_SIZE); t[8] ^= 1;
      CHECK(ss_check_host(t.data(), t.size(), digest) == PN_SS_BAD_MODEL); }
    // the all-or-nothing walk names the first refused record and keeps its reason
    { std::vector<unsigned char> three(3 * rec.size());
      for (int i = 0; i < 3; i++) memcpy(&three[i * rec.size()], rec.data(), rec.size());
      auto check = [&](const void *r, size_t bytes) { return ss_check_host(r, bytes, digest); };
      CHECK(pn_records_check(three.data(), 3, rec.size(), check) == 0);
      three[2 * rec.size() + 5] ^= 1; three[1 * rec.size() + 20] ^= 1;
      CHECK(pn_records_check(three.data(), 3, rec.size(), check) == -1);
      CHECK(std::string(pn_last_error()) == "record 1 refused: stream-state record written under another model (pn_model_digest differs)");
      CHECK(pn_records_check(three.data(), 1, rec.size(), check) == 0); } }

  // CLI helpers
  { std::vector<int> d;
    CHECK(pn_cli_parse_devices("0,1", 2, d) && d.size() == 2); CHECK(!pn_cli_parse_devices("1,,2", 4, d)); CHECK(!pn_cli_parse_devices("1,", 4, d));
    CHECK(!pn_cli_parse_devices("x", 4, d)); CHECK(!pn_cli_parse_devices("4", 4, d)); CHECK(pn_cli_parse_devices("all", 3, d) && d.size() == 3);
    CHECK(!pn_cli_parse_devices("all", 0, d)); CHECK(!pn_cli_parse_devices("", 4, d)); CHECK(!pn_cli_parse_devices(NULL, 4, d));
    int tot = 0; for (int r = 0; r < 7; r++) { int a, c; pn_cli_shard(100, 7, r, &a, &c); CHECK(a == tot); tot += c; } CHECK(tot == 100); }

  // the valid container, from memory and from the FILE*
  pn_model *m = pn_model_from_blob(blob.data(), blob.size());
  CHECK(m);
  { pn_model *m2 = pn_model_from_file(f); CHECK(m2 && m2->n_floats == m->n_floats); pn_model_free(m2); }
  fclose(f);
  CHECK(pn_model_from_file(NULL) == NULL); CHECK(pn_model_from_blob(NULL, 0) == NULL);

  // every truncation near the headers, coarse steps elsewhere; one trailing byte
  { size_t off = 8; std::vector<size_t> cuts;
    for (size_t c = 0; c < 64; c++) cuts.push_back(c);
    for (int li = 0; li < PN_NLAYERS; li++) {
      size_t nb, nw, nr; const size_t tot = pn_layer_floats(pn_kGeom[li].kind, pn_kGeom[li].nin, pn_kGeom[li].nn, pn_kGeom[li].ks, &nb, &nw, &nr);
      for (size_t c = off > 4 ? off - 4 : 0; c < off + 28; c++) cuts.push_back(c);
      off += 24 + 4 * tot;
      cuts.push_back(off - 1); cuts.push_back(off - 4);
    }
    CHECK(off == blob.size());
    for (size_t c : cuts) if (c < blob.size()) {
      std::vector<unsigned char> t(blob.begin(), blob.begin() + c);          // exact-size copy: a read past the end is caught
      CHECK(pn_model_from_blob(t.data(), t.size()) == NULL);
    }
    std::vector<unsigned char> t(blob); t.push_back(0);
    CHECK(pn_model_from_blob(t.data(), t.size()) == NULL); }

  // header fields: absurd dimensions must be refused before any size is derived from them
  { size_t off = 8;
    const uint32_t vals[] = {0u, 1u, 2u, 3u, 7u, 0x10000u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    for (int li = 0; li < PN_NLAYERS; li++) {
      size_t nb, nw, nr; const size_t tot = pn_layer_floats(pn_kGeom[li].kind, pn_kGeom[li].nin, pn_kGeom[li].nn, pn_kGeom[li].ks, &nb, &nw, &nr);
      for (int fld = 0; fld < 6; fld++)
        for (uint32_t v : vals) {
          std::vector<unsigned char> t(blob);
          uint32_t orig; memcpy(&orig, &t[off + 4 * fld], 4);
          memcpy(&t[off + 4 * fld], &v, 4);
          pn_model *x = pn_model_from_blob(t.data(), t.size());
          if (fld < 4) CHECK((x != NULL) == (v == orig));                    // kind / inputs / neurons / kernel size are the topology
          pn_model_free(x);
        }
      off += 24 + 4 * tot;
    } }
  // wrong magic / layer count
  { std::vector<unsigned char> t(blob); t[0] = 'X'; CHECK(pn_model_from_blob(t.data(), t.size()) == NULL);
    t = blob; uint32_t nl = 11; memcpy(&t[4], &nl, 4); CHECK(pn_model_from_blob(t.data(), t.size()) == NULL);
    nl = 0xffffffffu; memcpy(&t[4], &nl, 4); CHECK(pn_model_from_blob(t.data(), t.size()) == NULL); }
  // random byte flips in the first 64 KB (headers of fc and conv1 + arrays): never a crash
  { uint32_t x = 2463534242u;
    for (int it = 0; it < 300; it++) {
      std::vector<unsigned char> t(blob);
      for (int k = 0; k < 4; k++) { x = x * 1664525u + 1013904223u; t[(x >> 8) % 65536] ^= (unsigned char)(x >> 24); }
      pn_model_free(pn_model_from_blob(t.data(), t.size()));
    } }

  // RNNModel path: a correct record set, then one with a wrong geometry, then NULL
  { DenseLayer d[3]; Conv1DLayer c[2]; GRULayer g[5];
    const int di[3] = {PN_L_FC, PN_L_FC_GB, PN_L_FC_RB};
    for (int i = 0; i < 3; i++) { const PnLayerHost &H = m->L[di[i]]; d[i] = {H.bias, H.w, H.nin, H.nn, H.act}; }
    for (int i = 0; i < 2; i++) { const PnLayerHost &H = m->L[PN_L_CONV1 + i]; c[i] = {H.bias, H.w, H.nin, H.ks, H.nn, H.act}; }
    for (int i = 0; i < 5; i++) { const PnLayerHost &H = m->L[PN_L_GRU1 + i]; g[i] = {H.bias, H.w, H.rw, H.nin, H.nn, H.act, H.reset_after}; }
    RNNModel r = {&d[0], &c[0], &c[1], &g[0], &g[1], &g[2], &g[3], &g[4], &d[1], &d[2]};
    pn_model *x = pn_model_from_rnnmodel(&r); CHECK(x); CHECK(!memcmp(x->storage, m->storage, m->n_floats * 4)); pn_model_free(x);
    g[2].nb_neurons = 1 << 30; CHECK(pn_model_from_rnnmodel(&r) == NULL); g[2].nb_neurons = 512;
    g[1].reset_after = 0; CHECK(pn_model_from_rnnmodel(&r) == NULL);
    CHECK(pn_model_from_rnnmodel(NULL) == NULL); }

  // packers: exactly-sized destinations, every layer, both tile orders
  for (int li = 0; li < PN_NLAYERS; li++) {
    const PnLayerHost &H = m->L[li];
    const int K = H.nin * H.ks, ncols = H.nn * (H.kind == PN_KIND_GRU ? 3 : 1), k_alloc = li == PN_L_FC ? PN_FEAT_STRIDE : K;
    const int ctr = pn_layer_ct_round(PN_NN_MFMA, 0, li);
    std::vector<float> wp(pn_packed_floats(k_alloc, ncols, ctr));
    pn_pack_weights(H.w, K, k_alloc, ncols, ctr, wp.data());
    if (H.rw) { std::vector<float> rp(pn_packed_floats(H.nn, ncols, 1)); pn_pack_weights(H.rw, H.nn, H.nn, ncols, 1, rp.data()); }
    if (H.kind == PN_KIND_DENSE && ncols <= 48) { std::vector<float> q(pn_packed_floats_n16(K, ncols)); pn_pack_weights_n16(H.w, K, ncols, q.data()); }
  }
  pn_model_free(m);
  pn_model_free(NULL);
  puts("ok");
  return 0;
}
