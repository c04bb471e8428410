// The ten layers of the gain network, described once — HIP-free (builds with -DPN_NO_HIP), checked on the CPU by
// tests/c/host_sanitize.cpp.  What each layer reads and writes (pn_kNet, in terms of pn_state_layout.h's entries), which kernel
// runs it under a plan (pn_layer_kernel), which packed weights that kernel reads (pn_layer_weight_format), which operand
// shadows it goes through, and what a kernel kind needs in order to be launched (pn_kKernelRule: the launcher of its dense and
// of its GRU form, the geometry that launcher refuses, the column-tile rounding of its packed weights): the launch loop and the
// weight upload (pn_network.cpp), the launchers (pn_nn*.hip), the shadow allocation (pn_context.cpp), pn_debug_check_launch and
// pn_plan_describe all ask here.  A new kernel variant is one new kind, one arm of pn_layer_kernel, one rule row and one launcher.
#pragma once
#include "pn_dsp_layout.h"    // the profiling families, and through it pn_plan.h and pn_state_layout.h
#include "pn_launch_check.h"  // the geometry predicates the rules are made of

// The A operand of a layer = the concatenation along K of n <= 5 row-major panels: base, row stride (floats) and valid columns of
// each; the MFMA path requires every panel to be readable (and zero) up to the next multiple of 32 and all panels to be equally wide
struct PnSegs { const float *p[5]; int ld[5]; int width[5]; int n; };

// ---- wiring (rnn.cpp:42-81) ---------------------------------------------------------------------------------------------------
// A slot of a state entry as a network step sees it: the j-th live one, oldest first, or (j == live) the slot this step writes —
// the newest FIFO entry of a conv layer, the new half of a GRU pair
struct PnRef { int entry, j; };
constexpr PnRef pn_ref_new(int e) { return PnRef{e, pn_kState[e].live}; }
struct PnNetLayer {
  int n_in; PnRef in[5];   // input panels, in K order; each as wide as its entry (fc: PN_FEAT_STRIDE, PN_NFEAT of them valid)
  PnRef out; int out_col;  // output: pn_kGeom[].nn columns from out_col on; the leading dimension is the entry's row width
  int state;               // GRU: the entry of its recurrent state (read: live slot 0; written: out), else -1
  int fam;                 // profiling family the launch is bracketed under (KF_*, pn_dsp_layout.h)
};
static constexpr PnNetLayer pn_kNet[PN_NLAYERS] = {
    {1, {{PN_ST_FEAT, 0}}, pn_ref_new(PN_ST_C1RING), 0, -1, KF_FC},                                                   // fc
    {5, {{PN_ST_C1RING, 0}, {PN_ST_C1RING, 1}, {PN_ST_C1RING, 2}, {PN_ST_C1RING, 3}, pn_ref_new(PN_ST_C1RING)},
     pn_ref_new(PN_ST_C2RING), 0, -1, KF_CONV1},                                                                      // conv1: [4 previous fc outputs | current] (nnet.cpp:182-200)
    {3, {{PN_ST_C2RING, 0}, {PN_ST_C2RING, 1}, pn_ref_new(PN_ST_C2RING)}, {PN_ST_C2OUT, 0}, 0, -1, KF_CONV2},         // conv2
    {1, {{PN_ST_C2OUT, 0}}, pn_ref_new(PN_ST_GRU1), 0, PN_ST_GRU1, KF_GRU512},                                        // gru1
    {1, {pn_ref_new(PN_ST_GRU1)}, pn_ref_new(PN_ST_GRU2), 0, PN_ST_GRU2, KF_GRU512},                                  // gru2: the UPDATED state of gru1
    {1, {pn_ref_new(PN_ST_GRU2)}, pn_ref_new(PN_ST_GRU3), 0, PN_ST_GRU3, KF_GRU512},                                  // gru3
    {1, {pn_ref_new(PN_ST_GRU3)}, pn_ref_new(PN_ST_GRU_GB), 0, PN_ST_GRU_GB, KF_GRU512},                              // gru_gb
    {2, {pn_ref_new(PN_ST_GRU3), {PN_ST_C2OUT, 0}}, pn_ref_new(PN_ST_RB), 0, PN_ST_RB, KF_GRU_RB},                    // gru_rb (rnn.cpp:67-69)
    {5, {{PN_ST_C2OUT, 0}, pn_ref_new(PN_ST_GRU1), pn_ref_new(PN_ST_GRU2), pn_ref_new(PN_ST_GRU3), pn_ref_new(PN_ST_GRU_GB)},
     {PN_ST_GR, 0}, 0, -1, KF_FC_GB},                                                                                 // fc_gb (rnn.cpp:72-77)
    {1, {pn_ref_new(PN_ST_RB)}, {PN_ST_GR, 0}, PN_NB, -1, KF_FC_RB},                                                  // fc_rb
};
constexpr int pn_net_k(int li) { return pn_kNet[li].n_in * pn_kState[pn_kNet[li].in[0].entry].cols; }   // columns the layer's K sweep covers
// the table and the topology agree: equally wide panels that add up to the layer's inputs (fc: the zero-padded feature panel),
// conv FIFOs read whole, an output as wide as the layer inside its entry's row, GRUs writing the new half of their own state
constexpr bool pn_net_ok() {
  for (int li = 0; li < PN_NLAYERS; li++) {
    const PnNetLayer &row = pn_kNet[li]; const PnGeom &geo = pn_kGeom[li]; const PnStateEntry &oent = pn_kState[row.out.entry];
    for (int j = 0; j < row.n_in; j++) {
      const PnRef &in = row.in[j];
      if (pn_kState[in.entry].cols != pn_kState[row.in[0].entry].cols || in.j > pn_kState[in.entry].live) return false;
      if (geo.kind == PN_KIND_CONV1D && (row.n_in != geo.ks || geo.ks != pn_kState[in.entry].slots || in.entry != row.in[0].entry || in.j != j)) return false;
    }
    if (li == PN_L_FC ? (pn_net_k(li) != PN_FEAT_STRIDE || geo.nin != PN_NFEAT) : pn_net_k(li) != geo.nin * geo.ks) return false;
    if (row.out_col + geo.nn > oent.cols || (row.out.entry != PN_ST_GR && oent.cols != geo.nn) || oent.row_words != oent.cols) return false;
    if ((geo.kind == PN_KIND_GRU) != (row.state >= 0) || (row.state >= 0 && (row.out.entry != row.state || row.out.j != pn_kState[row.state].live))) return false;
  }
  return pn_kNet[PN_L_FC_RB].out_col == pn_kGeom[PN_L_FC_GB].nn && pn_kGeom[PN_L_FC_GB].nn + pn_kGeom[PN_L_FC_RB].nn == pn_kState[PN_ST_GR].cols;
}
static_assert(pn_net_ok(), "layer wiring (pn_kNet), topology (pn_kGeom) and state table (pn_kState) agree");

// ---- the kernel of a layer ----------------------------------------------------------------------------------------------------
// strict: reference-order kernels (pn_nn.hip); batch: fp32 batch GEMM (pn_nn.hip); batch_sh: the same, also writing the fp32
// fragment-order shadow of its output (pn_dense_mfma_ps_kernel); small: small-batch family (pn_nn_small.hip); n16 / n48: 16x16x4
// tiles for the 34-wide layers, one wave per tile (pn_nn_small.hip) / batch form (pn_nn_n48.hip); x3: fp16 matrix cores from operand
// shadows, split precision or fp16 operands (pn_nn_x3.hip); direct: fp32 GRU step from fragment-order fp32 shadows (pn_nn_d.hip)
enum { PN_K_STRICT, PN_K_BATCH, PN_K_BATCH_SH, PN_K_SMALL, PN_K_N16, PN_K_N48, PN_K_X3, PN_K_DIRECT, PN_K_COUNT };
constexpr bool pn_mode_x3(int nn_mode) { return nn_mode == PN_NN_MFMA_X3 || nn_mode == PN_NN_MFMA_F16; }   // shadow-operand modes
constexpr bool pn_layer_narrow(int li) { return pn_kGeom[li].kind == PN_KIND_DENSE && pn_kGeom[li].nn <= 48; }   // fc_gb, fc_rb
// The only place that spells the precedence.  The exceptions: in the shadow-operand modes fc (70 inputs) and fc_rb (K = 128) stay
// fp32; gru_rb (1024 -> 128) crosses over with the dense layers (small), not with the 512-wide GRUs (small_gru); under the direct
// family every dense layer stays on the batch kernels and conv2 alone also writes the shadow the GRUs read; n48 is fc_gb only.
constexpr int pn_layer_kernel(const PnPlan &p, int nn_mode, int li) {
  const int fp32 = p.small ? PN_K_SMALL : PN_K_BATCH;
  if (nn_mode == PN_NN_STRICT) return PN_K_STRICT;
  if (pn_mode_x3(nn_mode) && li != PN_L_FC && li != PN_L_FC_RB) return PN_K_X3;
  if (pn_kGeom[li].kind == PN_KIND_GRU) return p.direct ? PN_K_DIRECT : (li == PN_L_GRU_RB ? fp32 : (p.small_gru ? PN_K_SMALL : PN_K_BATCH));
  if (pn_layer_narrow(li) && p.narrow == 1) return PN_K_N16;
  if (li == PN_L_FC_GB && p.narrow == 2) return PN_K_N48;
  return p.direct && li == PN_L_CONV2 ? PN_K_BATCH_SH : fp32;
}
constexpr bool pn_kernel_reads_shadows(int k) { return k == PN_K_X3 || k == PN_K_DIRECT; }      // input panels and the GRU state
constexpr bool pn_kernel_writes_shadow(int k) { return pn_kernel_reads_shadows(k) || k == PN_K_BATCH_SH; }   // of its output, where the entry keeps one
// does entry e keep an operand shadow in a context of this mode and plan?
constexpr bool pn_state_shadowed(int e, const PnPlan &p, int nn_mode) {
  return pn_kState[e].shadow != PN_SH_NONE && (pn_mode_x3(nn_mode) || (p.direct && pn_kState[e].shadow == PN_SH_MODES_DIRECT));
}

// ---- the packed weights of a layer ----------------------------------------------------------------------------------------------
// raw: the nnet_data.h arrays as they are (w, rw); f32: fp32 tiles of pn_pack_weights (wp, rwp); f32_n16: those plus the 16x16x4
// packing of pn_pack_weights_n16 (wq); x3: fp16 planes of pn_pack_weights_x3 (wp, rwp), pn_weight_planes of them
enum { PN_WF_RAW, PN_WF_F32, PN_WF_F32_N16, PN_WF_X3 };
constexpr int pn_kernel_weight_format(int k) {
  return k == PN_K_STRICT ? PN_WF_RAW : (k == PN_K_X3 ? PN_WF_X3 : (k == PN_K_N16 || k == PN_K_N48 ? PN_WF_F32_N16 : PN_WF_F32));
}
constexpr int pn_weight_planes(int nn_mode) { return nn_mode == PN_NN_MFMA_X3 ? 2 : 1;  }   // hi + lo (split precision) or hi only
// What the shared device copy of (nn_mode, narrow) — the two plan-dependent parts of its cache key — holds for layer li: what the
// layer's kernel reads under that narrow setting.  No other plan field may change it (host_sanitize.cpp checks every plan).
constexpr int pn_layer_weight_format(int nn_mode, int narrow, int li) {
  return pn_kernel_weight_format(pn_layer_kernel(PnPlan{0, 0, 0, narrow, 0, 0, 1}, nn_mode, li));
}

// ---- what a kind needs to be launched -------------------------------------------------------------------------------------------
// The launcher of a kind's dense / conv form and of its GRU form, by the name its refusals carry; NULL: the kind has no such form.
// pn_network.cpp's table of the launchers themselves is static_asserted against this one.
struct PnKernelRule { const char *dense, *gru; };
static constexpr PnKernelRule pn_kKernelRule[PN_K_COUNT] = {
    {"pn_launch_dense_strict", "pn_launch_gru_strict"},   // strict
    {"pn_launch_dense", "pn_launch_gru"},                 // batch
    {"pn_launch_dense", NULL},                            // batch_sh: the batch launcher, handed the shadow of its output
    {"pn_launch_dense_small", "pn_launch_gru_small"},     // small
    {"pn_launch_dense_n16", NULL},                        // n16
    {"pn_launch_dense_n48", NULL},                        // n48
    {"pn_launch_dense_x3", "pn_launch_gru_x3"},           // x3
    {NULL, "pn_launch_gru_d"},                            // direct
};
constexpr const char *pn_kernel_launcher(int k, bool gru) { return gru ? pn_kKernelRule[k].gru : pn_kKernelRule[k].dense; }
// Column-tile rounding of the kind's packed input weights (pn_pack_weights / pn_pack_weights_x3: column tiles per block of the
// kernel that reads them): what the upload packs with and the launcher sizes its grid by.  A GRU's gates are whole tiles.
constexpr int pn_kernel_ct_round(int k, bool gru, int N) { return gru ? 1 : ((k == PN_K_X3 ? N >= 128 : N % 128 == 0) ? 4 : 2); }
constexpr int pn_layer_ct_round(int nn_mode, int narrow, int li) {      // ... of layer li in the shared copy of (nn_mode, narrow)
  return pn_kernel_ct_round(pn_layer_kernel(PnPlan{0, 0, 0, narrow, 0, 0, 1}, nn_mode, li), pn_kGeom[li].kind == PN_KIND_GRU, pn_kGeom[li].nn);
}
// 0, or -1 (pn_set_error names the launcher) where the launcher of (k, gru) refuses n_panels input panels of width[] columns
// and N neurons.  Every launcher begins with this call; pn_debug_check_launch and the harness make the same one.
static inline int pn_kernel_geometry_ok(int k, bool gru, int n_panels, const int *width, int N) {
  const char *who = k >= 0 && k < PN_K_COUNT ? pn_kernel_launcher(k, gru) : NULL;
  if (!who) { pn_set_error("kernel kind %d has no %s launcher", k, gru ? "GRU" : "dense"); return -1; }
  if (k == PN_K_STRICT || (gru && k == PN_K_BATCH)) return 0;       // strict: one lane per output, any geometry; the fp32 batch GRU launcher checks nothing
  if (k == PN_K_N16) return pn_check_n16_geometry(who, n_panels, width, N16_DEPTH);
  if (gru) return k == PN_K_SMALL ? pn_check_gru_small_geometry(who, n_panels, width, N) : pn_check_gru_geometry(who, n_panels, width, N);   // : x3, direct
  const bool fp32 = k == PN_K_BATCH || k == PN_K_BATCH_SH || k == PN_K_SMALL;      // zero-fill a ragged last tile; n48 and x3 read whole tiles
  if (pn_check_dense_geometry(who, n_panels, width, !fp32)) return -1;
  if (k == PN_K_BATCH_SH && pn_kernel_ct_round(k, gru, N) != 4) { pn_set_error("%s: a shadow output needs whole 128-column blocks", who); return -1; }
  if (k == PN_K_N48 && (N < 1 || N > PN_N48_COLS)) { pn_set_error("%s: %d output columns (1..%d)", who, N, PN_N48_COLS); return -1; }
  return 0;
}

// ---- describe -------------------------------------------------------------------------------------------------------------------
// a kernel kind as pn_ctx_describe spells it; rg: rows per wave / 32, 3 = 64 rows with the GRUs on the paired-phase kernel
static inline const char *pn_kernel_kind_name(int k, int nn_mode, int rg, bool gru) {
  static const char *const x3[2][3] = {{"f16_rows32", "f16_rows64", "f16_rows64_paired"}, {"x3_rows32", "x3_rows64", "x3_rows64_paired"}};
  if (k == PN_K_X3) return x3[nn_mode == PN_NN_MFMA_X3][rg == 3 && gru ? 2 : rg >= 2];
  if (k == PN_K_DIRECT) return rg >= 2 ? "direct_rows64" : "direct_rows32";
  return k == PN_K_SMALL ? "small" : (k == PN_K_N16 ? "n16" : (k == PN_K_N48 ? "n48" : "batch"));
}
// The family part of pn_ctx_describe, "nn=... frontend=...": snprintf's result.  dense= is conv1's kernel, gru= gru1's, gru_rb=
// gru_rb's, narrow= fc_gb's and fc_rb's (one word where they agree)
static inline int pn_plan_describe(const PnPlan &p, int nn_mode, char *buf, size_t n) {
  const char *nn = nn_mode == PN_NN_STRICT ? "strict" : (nn_mode == PN_NN_MFMA_F16 ? "mfma_f16" : (nn_mode == PN_NN_MFMA_X3 ? "mfma_x3" : "mfma_f32"));
  auto name = [&](int li) { return pn_kernel_kind_name(pn_layer_kernel(p, nn_mode, li), nn_mode, p.rg, pn_kGeom[li].kind == PN_KIND_GRU); };
  const int gb = pn_layer_kernel(p, nn_mode, PN_L_FC_GB), rb = pn_layer_kernel(p, nn_mode, PN_L_FC_RB);
  char narrow[32];
  if (gb == rb) snprintf(narrow, sizeof(narrow), "%s", name(PN_L_FC_GB));
  else snprintf(narrow, sizeof(narrow), "fc_gb:%s+fc_rb:%s", gb == PN_K_X3 ? "x3" : name(PN_L_FC_GB), gb == PN_K_X3 && rb != PN_K_N16 ? "fp32" : name(PN_L_FC_RB));
  return snprintf(buf, n, "nn=%s dense=%s gru=%s gru_rb=%s narrow=%s frontend=%s", nn, name(PN_L_CONV1), name(PN_L_GRU1), name(PN_L_GRU_RB), narrow,
                  pn_kFe[p.fe].name);
}
