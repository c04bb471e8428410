// The kernel families of a context, chosen once, at creation, from its batch size and network mode — HIP-free, so that the
// regime map can be checked without a GPU (pn_debug_plan, tests/test_plan_host.py).  pn_plan_for is the only reader of the
// family overrides; a context keeps the plan it was created with whatever the environment does afterwards.
#pragma once
#include <stdlib.h>
#include <string.h>
#include "../../include/percepnet_hip.h"

// front end: three phase kernels (pn_dsp_fe_split_*.hip), or the single-launch kernel with four / two streams per wavefront
// (pn_dsp_fe.hip, pn_dsp_fe_g2.hip)
enum { FE_MONO_G4 = 0, FE_MONO_G2 = 1, FE_SPLIT = 2 };
#define PN_MAX_CHAINS 4

struct PnPlan {
  int fe;                // FE_*
  int small, small_gru;  // 1: the small-batch kernels (pn_nn_small.hip) for the dense layers and gru_rb / for the 512-wide GRUs
  int narrow;            // fc_gb, fc_rb: 0 batch GEMM, 1 the 16x16x4 kernel (n16), 2 fc_gb on its batch form (n48, pn_nn_n48.hip)
  int direct;            // fp32 MFMA: GRU steps on the direct-operand kernels (pn_nn_d.hip)
  int rg;                // rows per wave / 32: 1|2|3 in the shadow-operand modes (pn_nn_x3.hip), 1|2 in the direct family, else 0
  int chains;            // row-range chains of the network (launch_rnn), 1..PN_MAX_CHAINS
};

static inline int pn_plan_env(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }

static inline PnPlan pn_plan_for(int n_streams, int nn_mode) {
  const int n = n_streams;
  const bool f32 = nn_mode == PN_NN_MFMA, x3 = nn_mode == PN_NN_MFMA_X3 || nn_mode == PN_NN_MFMA_F16;
  PnPlan p;
  // Front end: the phase-split kernels at every batch size, measured 0.102 vs 0.124 ms (g2) at 1024 streams, 0.130 vs 0.166 (g4)
  // at 4096, 1.32 vs 2.37 at 65536 (profiles/r03e_*).  PERCEPNET_FE=split|mono|g4|g2 overrides (PERCEPNET_FE_G2=0|1 is the older
  // spelling of g4 / g2).
  const char *fe = getenv("PERCEPNET_FE"), *g2 = getenv("PERCEPNET_FE_G2");
  if (fe && !strcmp(fe, "split")) p.fe = FE_SPLIT;
  else if (fe && (!strcmp(fe, "mono") || !strcmp(fe, "g4"))) p.fe = FE_MONO_G4;
  else if (fe && !strcmp(fe, "g2")) p.fe = FE_MONO_G2;
  else if (g2) p.fe = atoi(g2) ? FE_MONO_G2 : FE_MONO_G4;
  else p.fe = FE_SPLIT;
  // Small-batch family (one 32x32 tile and one accumulator chain per wave, 3-4x more blocks; same numerics).  Measured
  // crossovers (profiles/r02f_small_batch_study.txt): the dense/conv kernels win up to 4096 streams, the gate-per-wave GRU up
  // to ~1500.  PERCEPNET_SMALL_ROWS / PERCEPNET_SMALL_GRU_ROWS override them (0 = never).
  const int small_rows = pn_plan_env("PERCEPNET_SMALL_ROWS", 4096);
  p.small = n <= small_rows;
  p.small_gru = n <= pn_plan_env("PERCEPNET_SMALL_GRU_ROWS", small_rows < 1536 ? small_rows : 1536);
  // Narrow layers on 16x16x4 MFMA tiles up to 20480 streams in every MFMA mode (in the shadow-operand modes that is fc_rb;
  // fc_gb runs on their own kernels); measured fc_gb 0.026 vs 0.056 ms at 1024 streams, 0.082 vs 0.101 at 16384, 0.327 vs
  // 0.180 at 65536 where the batch GEMM's operand reuse wins.  PERCEPNET_N16_ROWS overrides.  Above it, fp32 fc_gb runs on
  // the batch form of the same instruction; PERCEPNET_N48=0 puts it back on the 32-column batch GEMM.
  const bool n16 = nn_mode != PN_NN_STRICT && n <= pn_plan_env("PERCEPNET_N16_ROWS", 20480);
  const bool n48 = f32 && !p.small && !n16 && pn_plan_env("PERCEPNET_N48", 1) != 0;
  p.narrow = n16 ? 1 : (n48 ? 2 : 0);
  // Direct-operand GRU kernels from 24 576 fp32 streams.  Measured against the batch family, same box, default chain rule
  // (profiles/r06_direct_operand_gru.log): frame time -0.6 % at 24 576 streams, -1.1 % at 32 768, -1.2 % at 61 440 / 66 560,
  // -1.4 % at 69 632 (the 512 -> 512 step at 65 536: 1.552 -> 1.523 ms), even at 16 384, +1.4 % at 8192 (too few blocks per
  // launch).  PERCEPNET_NN_DIRECT=0|1 overrides, PERCEPNET_NN_DIRECT_RG=1|2 the rows per wave.
  p.direct = f32 && !p.small && !p.small_gru && pn_plan_env("PERCEPNET_NN_DIRECT", n >= 24576) != 0;
  // Rows per wave: 2 row groups of 32 (256-row blocks, two per CU: fewest operand bytes per MFMA, best when the grid fills the
  // chip several times over) or 1 (128-row blocks, three per CU: twice the blocks, shorter chains — shadow-operand modes measured
  // 0.45 vs 0.60 ms per frame at 1024 streams, 0.60 vs 0.68 at 4096, equal at 16 384, 0.60 vs 0.585 per GRU step at 65 536).
  // PERCEPNET_X3_RG=1|2|3 overrides; 3 = 64 rows per wave with the GRUs on the paired-phase kernel (pn_gru_x3p_kernel), opt-in
  // only — measured at parity with the one-tile-per-block kernel (0.305 vs 0.291 ms fp16 operands, 0.57 vs
  // 0.59 ms split precision).
  const int rg_env = pn_plan_env(p.direct ? "PERCEPNET_NN_DIRECT_RG" : "PERCEPNET_X3_RG", 0);
  if (p.direct) p.rg = (rg_env == 1 || rg_env == 2) ? rg_env : (n >= 32768 ? 2 : 1);
  else if (x3) p.rg = (rg_env >= 1 && rg_env <= 3) ? rg_env : (n >= 32768 ? 2 : 1);
  else p.rg = 0;
  // Row-range chains (launch_rnn), large fp32 contexts only: two unless the batch fits EVERY layer's rounds exactly — a multiple
  // of 32 768 streams (8 rounds of the 512-wide layers, 2 of the 128-wide GRU) whose 128-row tile count also fits the 34-wide
  // layers' single column block (<= 512 tiles or a multiple of 512): 32 768, 65 536, 131 072, ...  Measured
  // (profiles/r06_row_chains.log): two chains win 0.6-2 % at 20 480, 49 152, 61 440, 69 632 and every size off the 4096-stream
  // grid, and change nothing at 32 768 / 65 536 (+-0.03 ms) — where a second compute stream would only be one more hardware
  // queue for the pipelined host path's copy streams to stay clear of (HIP has four by default).  With the direct-operand GRU
  // kernels (256-row blocks, 8 instead of 16 rounds per 512-wide layer at 65 536 streams, longer drains) two chains win at the
  // exact fits from 65 536 streams too: 9.02 / 9.03 / 9.07 -> 8.93 / 8.99 / 8.96 ms per frame at 65 536, 17.99 -> 17.85 at
  // 131 072, even at 32 768 (profiles/r06_direct_operand_gru.log H).  PN_NN_CHAINS=1..4 overrides.
  p.chains = 1;
  if (f32 && !p.small && !p.small_gru) {
    const int mt = (n + 127) / 128;
    const bool exact = (n % 32768 == 0) && (mt <= 512 || mt % 512 == 0) && !(p.direct && n >= 65536);
    int k = pn_plan_env("PN_NN_CHAINS", (n > 16384 && !exact) ? 2 : 1);
    if (k < 1) k = 1;
    if (k > PN_MAX_CHAINS) k = PN_MAX_CHAINS;
    while (k > 1 && n < k * 4096) k--;      // a chain of fewer than 4096 rows is the small-batch regime: not worth a stream
    p.chains = k;
  }
  return p;
}

// Rows per block of the family's chained kernels, and the first row of chain 1: equal shares rounded up to whole tiles, the
// last chain takes what is left (0 with one chain)
static inline size_t pn_plan_tile(const PnPlan &p) { return p.direct ? 128 * (size_t)p.rg : 128; }
static inline size_t pn_plan_share(const PnPlan &p, size_t n_streams) {
  const size_t k = p.chains, tile = pn_plan_tile(p);
  return k > 1 ? ((n_streams + k - 1) / k + tile - 1) / tile * tile : 0;
}
