// The DSP half of a frame, described once — HIP-free (builds with -DPN_NO_HIP), checked on the CPU by tests/c/host_sanitize.cpp.
// The kernel families a frame's launches are profiled under (one list: the KF_* indices and their public names), one
// DenoiseState's worth of front-end buffers (PnDspSide: the state-table entries a front end reads and writes, resolved from
// their base pointers), the ring slots of the frame at counter t (pn_dsp_slots, from pn_state_layout.h's phases), the input
// of a frame (PnDspIn) and the front-end families (pn_kFe: describe name, launches, profiling family of each).  A context
// (pn_context.cpp) and the training-feature generator (pn_featgen.cpp) both run their front ends from here.
#pragma once
#include "pn_plan.h"
#include "pn_state_layout.h"

// ---- profiling families (pn_kernel_count / pn_kernel_name / pn_ctx_kernel_time) ---------------------------------------------------
#define PN_KERNEL_FAMILIES(X) \
  X(FRONTEND, frontend) X(FC, fc) X(CONV1, conv1) X(CONV2, conv2) X(GRU512, gru512) X(GRU_RB, gru_rb) X(FC_GB, fc_gb) X(FC_RB, fc_rb) \
  X(BACKEND, backend) X(FE_SPEC_IN, fe_spec_in) X(FE_PITCH, fe_pitch) X(FE_SPEC_OUT, fe_spec_out)
#define PN_KF_ENUM(id, name) KF_##id,
#define PN_KF_NAME(id, name) #name,
enum { PN_KERNEL_FAMILIES(PN_KF_ENUM) KF_COUNT };
static constexpr const char *pn_kFamilyName[KF_COUNT] = {PN_KERNEL_FAMILIES(PN_KF_NAME)};
#undef PN_KF_ENUM
#undef PN_KF_NAME

// ---- a DSP side -------------------------------------------------------------------------------------------------------------------
// What compute_frame_features keeps and produces for one signal: a context has one, the feature generator one per analysed
// signal.  synth, gr and the I/O rows belong to the back end (the generator feeds the NOISY side's spectra through the SPEECH
// state's synthesis memory).  aux: optional [rows][PN_AUX_STRIDE] side outputs of the training-feature path, not a state entry.
static constexpr int pn_kSideEntries[8] = {PN_ST_HIST, PN_ST_LAST_GAIN, PN_ST_LAST_PERIOD, PN_ST_SILENCE, PN_ST_YRING, PN_ST_EYRING, PN_ST_PS, PN_ST_FEAT};
struct PnDspSide {
  float *hist, *last_gain; int *last_period, *silence; float2 *yring; float *eyring; float2 *Ps; float *feat, *aux;
  size_t rows;           // streams the unpadded entries were sized for (pn_state_size): the rings' slots lie this many rows apart
};
static inline PnDspSide pn_dsp_side(float *const base[PN_ST_COUNT], float *aux, size_t rows) {
  return PnDspSide{base[PN_ST_HIST], base[PN_ST_LAST_GAIN], (int *)base[PN_ST_LAST_PERIOD], (int *)base[PN_ST_SILENCE], (float2 *)base[PN_ST_YRING],
                   base[PN_ST_EYRING], (float2 *)base[PN_ST_PS], base[PN_ST_FEAT], aux, rows};
}

// ---- the slots of a frame -----------------------------------------------------------------------------------------------------------
// frame_t: the history slot frame t writes; slot_w: the look-ahead slot it writes (Y(t), Ey(t)); slot_r: the oldest live
// look-ahead slot = X(t), Ex(t) (pn_dsp_fe.hip: Y(t-5)), which the back end reads too.  The kernels take ONE slot_w / slot_r for
// the spectra and their band energies:
static_assert(pn_kState[PN_ST_YRING].slots == pn_kState[PN_ST_EYRING].slots && pn_kState[PN_ST_YRING].live == pn_kState[PN_ST_EYRING].live &&
              pn_kState[PN_ST_YRING].counter == PN_CNT_T && pn_kState[PN_ST_EYRING].counter == PN_CNT_T && pn_kState[PN_ST_HIST].counter == PN_CNT_T &&
              pn_kState[PN_ST_HIST].slots == PN_HIST_FRAMES, "yring and eyring share slots and live count; every DSP ring follows t");
struct PnDspSlots { int frame_t, slot_w, slot_r; };
constexpr PnDspSlots pn_dsp_slots(int64_t t) {
  return PnDspSlots{pn_state_write(pn_kState[PN_ST_HIST], t, 0), pn_state_write(pn_kState[PN_ST_YRING], t, 0), pn_state_first(pn_kState[PN_ST_YRING], t, 0)};
}
// a look-ahead slot of a side: its spectra and their band energies, one pn_state_size slot stride (in words) apart
static inline const float *pn_dsp_slot(const PnDspSide &s, int entry, const void *base, int slot) {
  return (const float *)base + slot * pn_state_size(pn_kState[entry], s.rows).slot_stride;
}
static inline const float2 *pn_dsp_spec(const PnDspSide &s, int slot) { return (const float2 *)pn_dsp_slot(s, PN_ST_YRING, s.yring, slot); }
static inline const float *pn_dsp_bands(const PnDspSide &s, int slot) { return pn_dsp_slot(s, PN_ST_EYRING, s.eyring, slot); }

// a frame's input: stream s's 480 samples at p + s * stride, int16 (sample = (float)v * i16_scale: 1/32768 for the CLI,
// main.cpp:34; 1 for the training binary, denoise.cpp:41,697) or float
struct PnDspIn { const void *p; int is_i16; long long stride; float i16_scale; };

// ---- the front-end families ---------------------------------------------------------------------------------------------------------
// Same results, bit for bit.  split: spec_in and pitch are independent of each other, spec_out needs both.
struct PnFeFamily { const char *name; int n; int fam[3]; };     // pn_ctx_describe's word, launches per frame, profiling family of each
static constexpr PnFeFamily pn_kFe[3] = {
    {"g4", 1, {KF_FRONTEND}},                                    // FE_MONO_G4 (pn_dsp_fe.hip)
    {"g2", 1, {KF_FRONTEND}},                                    // FE_MONO_G2 (pn_dsp_fe_g2.hip)
    {"split", 3, {KF_FE_SPEC_IN, KF_FE_PITCH, KF_FE_SPEC_OUT}},  // FE_SPLIT   (pn_dsp_fe_split_s.hip, pn_dsp_fe_split_p.hip)
};
static_assert(FE_MONO_G4 == 0 && FE_MONO_G2 == 1 && FE_SPLIT == 2, "pn_kFe is indexed by FE_*");
