"""ctypes binding of libpercepnet_hip.so (include/percepnet_hip.h) — the host-side mirror of the
reference's frame-engine interface for Python callers (tests, bench).

There is deliberately no fallback: if the HIP library is missing or no GPU is usable, loading /
context creation raises.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libpercepnet_hip.so")

NN_MFMA, NN_STRICT, NN_MFMA_F16, NN_MFMA_X3 = 0, 1, 2, 3
FRAME = 480
# per-stream state records (include/percepnet_hip.h): size, and the PN_SS_* verdicts of a refused record
STREAM_STATE_BYTES = 54688
SS_OK, SS_BAD_MAGIC, SS_BAD_VERSION, SS_BAD_SIZE, SS_BAD_MODEL, SS_BAD_ARG = 0, -1, -2, -3, -4, -5
SS_BAD_RATE = -6          # pn_rate_state_check: a record of another rate
# batched rate converter (include/percepnet_hip.h pn_rate): the rates it takes, taps per phase
RATES = (8000, 16000, 24000)
MIXED_RATES = (8000, 16000, 24000, 48000)     # the rate of a STREAM of a mixed converter (pn_rate_create_mixed); 48000 is a copy
RATES_ALL = RATES + (32000,)                  # every rate a converter takes: 32000 is the rational 3:2 row (n = 320), the others 48000 / L
MIXED_RATES_ALL = (8000, 16000, 24000, 32000, 48000)
RATE_MIXED_ROW = 480                          # PN_RATE_MIXED_ROW: samples between two low-rate rows of a mixed converter
RATE_TAPS = 16
G711_ULAW, G711_ALAW = 0, 1                   # PN_G711_*: the law of a stream's 8-bit rows (pn_rate_set_stream_laws)
CONF_NONE, CONF_MAX_MEMBERS = -1, 32          # PN_CONF_*: no conference; the most streams one holds (pn_rate_set_stream_confs)
MIX_REPORT_WORDS = 4                          # PN_MIX_REPORT_WORDS: words of one record of the mix report (pn_rate_set_mix_report)
MIX_SELECTED, MIX_MUTED, MIX_IN_CONF = 1, 2, 4                      # its flags
MIX_REPORT_DTYPE = np.dtype([("level", "<f4"), ("flags", "<u4"), ("mix_peak", "<f4"), ("mix_clipped", "<i4")])
# packet-loss concealment (include/percepnet_hip.h "packet-loss concealment"): PN_PLC_*
PLC_HIST, PLC_P_MIN, PLC_P_MAX = 1920, 240, 720
PLC_REPORT_WORDS = 4
PLC_CONCEALED, PLC_CROSSFADE, PLC_SILENT = 1, 2, 4                  # its flags
PLC_REPORT_DTYPE = np.dtype([("flags", "<u4"), ("period", "<u4"), ("run", "<u4"), ("lost", "<u4")])
# comfort noise (include/percepnet_hip.h "comfort noise"): PN_CNG_*
CNG_MAX_ORDER, CNG_SID_BYTES, CNG_DEFAULT_LEVEL, CNG_DEFAULT_SEED = 12, 14, 60, 0x434e4731
CNG_REPORT_WORDS = 4
CNG_REPORT_DTYPE = np.dtype([("run", "<u4"), ("total", "<u4"), ("gain", "<f4"), ("counter", "<u4")])
# the DTX send side (include/percepnet_hip.h "DTX send side"): PN_DTX_*
DTX_N_PARAMS = 9
DTX_THR, DTX_FLOOR_UP, DTX_FLOOR_DRIFT, DTX_FLOOR_MIN, DTX_HANGOVER, DTX_SMOOTH, DTX_UPDATE_DB, DTX_MAX_INTERVAL, DTX_ORDER = range(9)   # parameter indices
DTX_REPORT_WORDS, DTX_STATE_WORDS = 8, 24
DTX_FRAME, DTX_SID, DTX_NONE = 0, 1, 2                                             # the decision, report word 0
DTX_ON, DTX_ACTIVE, DTX_HANGOVER_FRAME, DTX_NONFINITE = 1, 2, 4, 8                 # its flags, the low byte of report word 1
# word1: flags | L << 8 | hang << 16; sid: the last emitted SID; count: the SIDs emitted since the clear, mod 2^16
DTX_REPORT_DTYPE = np.dtype([("decision", "<u4"), ("word1", "<u4"), ("energy", "<f4"), ("floor", "<f4"), ("sid", "u1", (14,)), ("count", "<u2")])
# automatic level control (include/percepnet_hip.h "automatic level control"): PN_AGC_*
AGC_N_PARAMS = 8
AGC_MAX_GAIN, AGC_MIN_GAIN, AGC_GATE_RMS, AGC_ATTACK, AGC_RELEASE, AGC_STEP_UP, AGC_STEP_DOWN, AGC_CEILING = range(8)   # parameter indices
AGC_REPORT_WORDS = 4
AGC_ON, AGC_ADAPTED, AGC_LIMITED, AGC_AT_MAX, AGC_AT_MIN, AGC_HELD_LOST = 1, 2, 4, 8, 16, 32   # its flags
AGC_REPORT_DTYPE = np.dtype([("gain", "<f4"), ("level", "<f4"), ("flags", "<u4"), ("peak", "<f4")])
AGC_STATE_DTYPE = np.dtype([("level", "<f4"), ("gain", "<f4"), ("adapted", "<u4"), ("spare", "<u4")])   # the four state words of agc_frame
# output limiter (include/percepnet_hip.h "output limiter"): PN_LIM_*
LIM_N_PARAMS = 2
LIM_RELEASE, LIM_HOLD = range(2)                                                # parameter indices
LIM_REPORT_WORDS = 4
LIM_ON, LIM_ATTACK, LIM_HOLDING, LIM_RELEASING, LIM_ACTIVE, LIM_NONFINITE = 1, 2, 4, 8, 16, 32   # its flags
LIM_REPORT_DTYPE = np.dtype([("gain", "<f4"), ("peak", "<f4"), ("flags", "<u4"), ("limited", "<u4")])
LIM_STATE_DTYPE = np.dtype([("gain", "<f4"), ("hold", "<u4"), ("limited", "<u4"), ("spare", "<u4")])   # the four state words of lim_frame
# DTMF detection (include/percepnet_hip.h "DTMF detection"): PN_DTMF_*
DTMF_N_PARAMS = 7
DTMF_MIN_RMS, DTMF_PURITY, DTMF_TWIST_FWD, DTMF_TWIST_REV, DTMF_REL, DTMF_ON_FRAMES, DTMF_OFF_FRAMES = range(7)   # parameter indices
DTMF_REPORT_WORDS, DTMF_STATE_WORDS = 4, 24
DTMF_ON, DTMF_HIT, DTMF_BEGIN, DTMF_END, DTMF_HELD_LOST = 1, 2, 4, 8, 16          # its flags, the low byte of report word 0
DTMF_REPORT_DTYPE = np.dtype([("word0", "<u4"), ("dur", "<u4"), ("count", "<u4"), ("last4", "<u4")])   # word0: flags | cur << 8 | ended << 16
# DTMF removal (include/percepnet_hip.h "DTMF removal"): PN_DTMF_CLAMP_*
DTMF_CLAMP_N_PARAMS = 4
DTMF_CLAMP_PRE, DTMF_CLAMP_POST, DTMF_CLAMP_VOLUME, DTMF_CLAMP_TS_PER_FRAME = range(4)   # parameter indices
DTMF_CLAMP_REPORT_WORDS, DTMF_CLAMP_STATE_WORDS = 4, 4
DTMF_CLAMP_ON, DTMF_CLAMP_MUTED, DTMF_CLAMP_FADE_OUT, DTMF_CLAMP_FADE_IN, DTMF_CLAMP_LATE, DTMF_CLAMP_EVENT, DTMF_CLAMP_EVENT_END = 1, 2, 4, 8, 16, 32, 64   # report word 0
DTMF_CLAMP_REPORT_DTYPE = np.dtype([("flags", "<u4"), ("event", "<u4"), ("event_end", "<u4"), ("muted", "<u4")])   # event, event_end: RFC 4733 payloads, 0 for none
DTMF_CLAMP_DELAY = 6         # output row t is input row t - 6: events run this many frames ahead of the audio they describe
DTMF_ROWS_PER_PASS = 2048    # the kernel's grid covers this many rows at once (csrc/pn_launch.h PN_DTMF_MAX_BLOCKS blocks of four); beyond it a block makes further passes
# call-state records (include/percepnet_hip.h "call-state records"): PN_RATE_CALL_*, PN_CALL_*
SS_BAD_STATE = -7         # pn_rate_call_state_check: a body that breaks an invariant, an unknown section, words in an absent section
RATE_CALL_MAGIC, RATE_CALL_VERSION, RATE_CALL_STATE_BYTES = 0x53434E50, 1, 10640
CALL_PLC, CALL_AGC, CALL_LIM, CALL_MIX = 1, 2, 4, 8                             # the section mask
CALL_W_HIST, CALL_W_Q, CALL_W_META, CALL_W_AGC, CALL_W_LIM, CALL_W_MIX, CALL_BODY_WORDS = 0, 1920, 2640, 2644, 2648, 2652, 2656   # body word offsets
# per-stream frame report (include/percepnet_hip.h pn_ctx_set_report): one record of PN_REPORT_WORDS 32-bit words per stream
REPORT_WORDS = 8
REPORT_DTYPE = np.dtype([("in_peak", "<f4"), ("in_energy", "<f4"), ("out_peak", "<f4"), ("out_energy", "<f4"), ("gain_mean", "<f4"),
                         ("pitch_period", "<i4"), ("out_clipped", "<i4"), ("flags", "<u4")])

_vp = ctypes.c_void_p
_lib = None


class PercepNetError(RuntimeError):
    pass


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64; if torch is going
    # to be used in this process (tests, bench) it must be loaded BEFORE this library so that
    # both bind to the same runtime copy (loading order reversed, torch reports "No HIP GPUs").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = os.environ.get("PERCEPNET_LIB", LIB_PATH)   # override: tuning variants (build.build_variant)
    if not os.path.exists(path):
        raise PercepNetError(
            f"{path} is missing: build it with `python -m percepnet_amd.build` (no CPU fallback exists)")
    L = ctypes.CDLL(path)
    L.pn_last_error.restype = ctypes.c_char_p
    L.pn_version.restype = ctypes.c_char_p
    L.pn_model_from_blob.restype = _vp
    L.pn_model_from_blob.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.pn_model_free.argtypes = [_vp]
    L.pn_ctx_create.restype = _vp
    L.pn_ctx_create.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]
    L.pn_ctx_destroy.argtypes = [_vp]
    L.pn_ctx_reset.argtypes = [_vp]
    L.pn_ctx_reset_streams.argtypes = [_vp, _vp, ctypes.c_int]
    L.pn_ctx_n_streams.argtypes = [_vp]
    L.pn_ctx_frames_done.restype = ctypes.c_int64
    L.pn_ctx_frames_done.argtypes = [_vp]
    L.pn_ctx_device_bytes.restype = ctypes.c_size_t
    L.pn_ctx_device_bytes.argtypes = [_vp]
    L.pn_ctx_describe.argtypes = [_vp, ctypes.c_char_p, ctypes.c_size_t]
    if hasattr(L, "pn_ctx_weight_bytes"):
        L.pn_ctx_weight_bytes.restype = ctypes.c_size_t
        L.pn_ctx_weight_bytes.argtypes = [_vp]
    for name in ("pn_process_f32", "pn_process_i16", "pn_process_host_f32", "pn_process_host_i16"):
        getattr(L, name).argtypes = [_vp, _vp, _vp, _vp]
    L.pn_process_i16_multi.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int]
    if hasattr(L, "pn_process_i16_active"):                 # (a round-4 library loaded through PERCEPNET_LIB for A/B timing has none of these)
        for name in ("pn_process_f32_active", "pn_process_i16_active", "pn_submit_host_f32_active", "pn_submit_host_i16_active"):
            if hasattr(L, name):
                getattr(L, name).argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int]
        L.pn_debug_check_launch.argtypes = [ctypes.c_int] * 4
        L.pn_ctx_debug_inject_launch_failure.argtypes = [_vp, ctypes.c_int]
    for name in ("pn_submit_host_f32", "pn_submit_host_i16"):
        getattr(L, name).argtypes = [_vp, _vp, _vp, _vp]
    L.pn_host_wait.argtypes = [_vp]
    if hasattr(L, "pn_ctx_pipe_streams"):
        L.pn_ctx_pipe_streams.argtypes = [_vp]
        L.pn_ctx_pipe_streams.restype = ctypes.c_char_p
    if hasattr(L, "pn_host_frames_delivered"):
        L.pn_host_frames_delivered.argtypes = [_vp]
        L.pn_host_frames_delivered.restype = ctypes.c_int64
    L.pn_host_alloc.argtypes = [ctypes.c_size_t]
    L.pn_host_alloc.restype = _vp
    L.pn_host_free.argtypes = [_vp]
    L.pn_host_free.restype = None
    L.pn_ctx_synchronize.argtypes = [_vp]
    L.pn_ctx_set_postfilter.argtypes = [_vp, ctypes.c_int]
    L.pn_ctx_read_features.argtypes = [_vp, _vp, _vp]
    L.pn_ctx_read_features_dev.argtypes = [_vp, _vp, _vp]
    L.pn_ctx_compute_rnn_host.argtypes = [_vp, _vp, _vp]
    L.pn_ctx_set_rnn_state_host.argtypes = [_vp] * 8
    L.pn_ctx_get_rnn_state_host.argtypes = [_vp] * 8
    if hasattr(L, "pn_stream_state_bytes"):
        L.pn_stream_state_bytes.restype = ctypes.c_size_t
        L.pn_stream_state_bytes.argtypes = []
        L.pn_stream_state_check.argtypes = [_vp, ctypes.c_size_t, _vp]
        for name in ("pn_ctx_export_streams", "pn_ctx_export_streams_host", "pn_ctx_import_streams_host"):
            getattr(L, name).argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_ctx_import_streams.argtypes = [_vp, _vp, ctypes.c_int, _vp, _vp]
    if hasattr(L, "pn_atten_limit_factor"):
        L.pn_atten_limit_factor.restype = ctypes.c_float
        L.pn_atten_limit_factor.argtypes = [ctypes.c_float]
        L.pn_ctx_set_atten_limit.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_ctx_get_atten_limit.argtypes = [_vp, _vp]
    if hasattr(L, "pn_ctx_set_report"):
        for name in ("pn_ctx_set_report", "pn_ctx_set_output_saturate"):
            getattr(L, name).argtypes = [_vp, ctypes.c_int]
        for name in ("pn_ctx_read_report", "pn_ctx_read_report_dev", "pn_host_next_report"):
            getattr(L, name).argtypes = [_vp, _vp]
    if hasattr(L, "pn_rate_create"):
        for name in ("pn_rate_frame_samples", "pn_rate_delay_samples"):
            getattr(L, name).argtypes = [ctypes.c_int]
        L.pn_rate_taps.argtypes = [ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int]
        L.pn_rate_state_bytes.restype = ctypes.c_size_t
        L.pn_rate_state_bytes.argtypes = [ctypes.c_int]
        L.pn_rate_state_check.argtypes = [_vp, ctypes.c_size_t, ctypes.c_int]
        L.pn_rate_create.restype = _vp
        L.pn_rate_create.argtypes = [_vp, ctypes.c_int]
        L.pn_rate_destroy.argtypes = [_vp]
        L.pn_rate_destroy.restype = None
        L.pn_rate_reset.argtypes = [_vp]
        L.pn_rate_reset_streams.argtypes = [_vp, _vp, ctypes.c_int]
        for name in ("pn_rate_up_f32", "pn_rate_up_i16", "pn_rate_down_f32", "pn_rate_down_i16"):
            getattr(L, name).argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int]
        for name in ("pn_rate_process_f32", "pn_rate_process_i16", "pn_rate_process_host_f32", "pn_rate_process_host_i16"):
            getattr(L, name).argtypes = [_vp, _vp, _vp, _vp]
        for name in ("pn_rate_process_f32_active", "pn_rate_process_i16_active"):
            getattr(L, name).argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int]
        for name in ("pn_rate_export_streams_host", "pn_rate_import_streams_host"):
            getattr(L, name).argtypes = [_vp, _vp, ctypes.c_int, _vp]
    if hasattr(L, "pn_rate_create_mixed"):
        for name in ("pn_rate_mixed_frame_samples", "pn_rate_mixed_delay_samples"):
            getattr(L, name).argtypes = [ctypes.c_int]
        L.pn_rate_mixed_rates_check.argtypes = [_vp, ctypes.c_int]
        L.pn_rate_create_mixed.restype = _vp
        L.pn_rate_create_mixed.argtypes = [_vp, _vp]
        for name in ("pn_rate_is_mixed", "pn_rate_row_samples"):
            getattr(L, name).argtypes = [_vp]
        L.pn_rate_set_stream_rates.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_rate_get_stream_rates.argtypes = [_vp, _vp]
    if hasattr(L, "pn_rate_submit_host_i16"):
        for name in ("pn_rate_submit_host_f32", "pn_rate_submit_host_i16"):
            getattr(L, name).argtypes = [_vp, _vp, _vp, _vp]
        for name in ("pn_rate_submit_host_f32_active", "pn_rate_submit_host_i16_active"):
            getattr(L, name).argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int]
        L.pn_rate_host_pipeline_prepare.argtypes = [_vp]
        L.pn_rate_state_max_bytes.restype = ctypes.c_size_t
        L.pn_rate_state_max_bytes.argtypes = []
        L.pn_rate_record_stride.restype = ctypes.c_size_t
        L.pn_rate_record_stride.argtypes = [_vp]
        L.pn_rate_export_streams.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_rate_import_streams.argtypes = [_vp, _vp, ctypes.c_int, _vp, _vp]
        L.pn_rate_set_profiling.argtypes = [_vp, ctypes.c_int]
        L.pn_rate_kernel_time.argtypes = [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]
        L.pn_rate_reset_profile.argtypes = [_vp]
    if hasattr(L, "pn_g711_decode"):
        for name in ("pn_g711_decode", "pn_g711_encode"):
            getattr(L, name).argtypes = [ctypes.c_int, _vp, _vp, ctypes.c_size_t]
        L.pn_rate_laws_check.argtypes = [_vp, ctypes.c_int]
        L.pn_rate_set_stream_laws.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_rate_get_stream_laws.argtypes = [_vp, _vp]
        for name in ("pn_rate_up_g711", "pn_rate_down_g711"):
            getattr(L, name).argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int]
        for name in ("pn_rate_process_g711", "pn_rate_process_host_g711", "pn_rate_submit_host_g711"):
            getattr(L, name).argtypes = [_vp, _vp, _vp, _vp]
        for name in ("pn_rate_process_g711_active", "pn_rate_submit_host_g711_active"):
            getattr(L, name).argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int]
    if hasattr(L, "pn_rate_set_stream_confs"):
        L.pn_rate_confs_check.argtypes = [_vp, ctypes.c_int, ctypes.c_int]
        L.pn_rate_set_stream_confs.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_rate_get_stream_confs.argtypes = [_vp, _vp]
        L.pn_rate_mix_f32.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int]
    if hasattr(L, "pn_rate_set_conf_speakers"):
        L.pn_rate_mix_gains_check.argtypes = [_vp, ctypes.c_int]
        L.pn_mix_level.restype = ctypes.c_float
        L.pn_mix_level.argtypes = [_vp]
        L.pn_mix_select.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp]
        for name in ("pn_rate_set_stream_mix_gains", "pn_rate_set_conf_speakers"):
            getattr(L, name).argtypes = [_vp, _vp, ctypes.c_int, _vp]
        for name in ("pn_rate_get_stream_mix_gains", "pn_rate_get_conf_speakers", "pn_rate_read_mix_report", "pn_rate_read_mix_report_dev"):
            getattr(L, name).argtypes = [_vp, _vp]
        L.pn_rate_set_mix_hold.argtypes = [_vp, ctypes.c_float]
        L.pn_rate_get_mix_hold.restype = ctypes.c_float
        L.pn_rate_get_mix_hold.argtypes = [_vp]
        L.pn_rate_set_mix_report.argtypes = [_vp, ctypes.c_int]
    if hasattr(L, "pn_rate_set_plc"):
        L.pn_plc_pitch.argtypes = [_vp]
        L.pn_plc_period.argtypes = [_vp, ctypes.c_int, _vp]
        L.pn_plc_gain.restype = ctypes.c_float
        L.pn_plc_gain.argtypes = [ctypes.c_int64]
        for name in ("pn_rate_set_plc", "pn_rate_set_plc_report"):
            getattr(L, name).argtypes = [_vp, ctypes.c_int]
        L.pn_rate_set_lost.argtypes = [_vp, _vp, ctypes.c_int]
        L.pn_rate_plc_f32.argtypes = [_vp, _vp, _vp, ctypes.c_int]
        for name in ("pn_rate_read_plc_report", "pn_rate_read_plc_report_dev"):
            getattr(L, name).argtypes = [_vp, _vp]
    if hasattr(L, "pn_rate_set_cng"):
        L.pn_cng_sid_decode.argtypes = [_vp, _vp, _vp, _vp]
        L.pn_cng_level.restype = ctypes.c_float
        L.pn_cng_level.argtypes = [ctypes.c_int]
        L.pn_cng_frame.argtypes = [_vp, _vp, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]
        for name in ("pn_rate_set_cng", "pn_rate_set_cng_report"):
            getattr(L, name).argtypes = [_vp, ctypes.c_int]
        L.pn_rate_set_cng_seed.argtypes = [_vp, ctypes.c_uint32]
        L.pn_rate_set_stream_sid.argtypes = [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int]
        L.pn_rate_set_silent.argtypes = [_vp, _vp, ctypes.c_int]
        L.pn_rate_cng_f32.argtypes = [_vp, _vp, _vp, ctypes.c_int]
        for name in ("pn_rate_get_cng_seed", "pn_rate_get_stream_sid", "pn_rate_read_cng_report", "pn_rate_read_cng_report_dev", "pn_rate_debug_cng_state"):
            getattr(L, name).argtypes = [_vp, _vp]
    if hasattr(L, "pn_rate_set_agc"):
        for name in ("pn_agc_default_params", "pn_agc_params_check"):
            getattr(L, name).argtypes = [_vp]
        L.pn_agc_frame.argtypes = [_vp, ctypes.c_float, _vp, _vp, _vp, ctypes.c_int]
        L.pn_rate_agc_targets_check.argtypes = [_vp, ctypes.c_int]
        for name in ("pn_rate_set_agc", "pn_rate_set_agc_report"):
            getattr(L, name).argtypes = [_vp, ctypes.c_int]
        for name in ("pn_rate_set_agc_params", "pn_rate_get_agc_params", "pn_rate_get_stream_agc_targets", "pn_rate_read_agc_report",
                     "pn_rate_read_agc_report_dev"):
            getattr(L, name).argtypes = [_vp, _vp]
        L.pn_rate_set_stream_agc_targets.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_rate_agc_f32.argtypes = [_vp, _vp, _vp, ctypes.c_int]
    if hasattr(L, "pn_rate_set_stream_limiter"):
        for name in ("pn_lim_default_params", "pn_lim_params_check"):
            getattr(L, name).argtypes = [_vp]
        L.pn_lim_frame.argtypes = [_vp, ctypes.c_float, _vp, _vp, _vp, _vp]
        L.pn_rate_limiter_ceilings_check.argtypes = [_vp, ctypes.c_int]
        L.pn_rate_set_limiter_report.argtypes = [_vp, ctypes.c_int]
        for name in ("pn_rate_set_limiter_params", "pn_rate_get_limiter_params", "pn_rate_get_stream_limiter", "pn_rate_read_limiter_report",
                     "pn_rate_read_limiter_report_dev"):
            getattr(L, name).argtypes = [_vp, _vp]
        L.pn_rate_set_stream_limiter.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_rate_lim_f32.argtypes = [_vp, _vp, _vp, ctypes.c_int]
    if hasattr(L, "pn_rate_export_call_state"):
        L.pn_rate_call_state_bytes.restype = ctypes.c_size_t
        L.pn_rate_call_state_bytes.argtypes = []
        L.pn_rate_call_state_check.argtypes = [_vp, ctypes.c_size_t]
        L.pn_rate_call_state_sections.argtypes = [_vp]
        for name in ("pn_rate_export_call_state", "pn_rate_export_call_state_host", "pn_rate_import_call_state_host"):
            getattr(L, name).argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_rate_import_call_state.argtypes = [_vp, _vp, ctypes.c_int, _vp, _vp]
    if hasattr(L, "pn_rate_set_stream_dtmf"):
        for name in ("pn_dtmf_default_params", "pn_dtmf_params_check"):
            getattr(L, name).argtypes = [_vp]
        L.pn_dtmf_frame.argtypes = [_vp, _vp, _vp, ctypes.c_int, _vp]
        L.pn_dtmf_tables.argtypes = [_vp, _vp, _vp]
        L.pn_rate_set_dtmf_report.argtypes = [_vp, ctypes.c_int]
        for name in ("pn_rate_set_dtmf_params", "pn_rate_get_dtmf_params", "pn_rate_get_stream_dtmf", "pn_rate_read_dtmf_report",
                     "pn_rate_read_dtmf_report_dev", "pn_rate_debug_dtmf_state"):
            getattr(L, name).argtypes = [_vp, _vp]
        L.pn_rate_set_stream_dtmf.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_rate_dtmf_f32.argtypes = [_vp, _vp, _vp, ctypes.c_int]
    if hasattr(L, "pn_rate_set_stream_dtmf_clamp"):
        L.pn_dtmf_clamp_default_params.argtypes = [_vp]
        L.pn_dtmf_clamp_params_check.argtypes = [_vp, _vp]
        L.pn_dtmf_clamp_frame.argtypes = [_vp, _vp, _vp, _vp, _vp]
        L.pn_dtmf_event_payload.restype = ctypes.c_uint32
        L.pn_dtmf_event_payload.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]
        L.pn_rate_set_dtmf_clamp_report.argtypes = [_vp, ctypes.c_int]
        for name in ("pn_rate_set_dtmf_clamp_params", "pn_rate_get_dtmf_clamp_params", "pn_rate_get_stream_dtmf_clamp", "pn_rate_read_dtmf_clamp_report",
                     "pn_rate_read_dtmf_clamp_report_dev", "pn_rate_debug_dtmf_clamp_state", "pn_rate_debug_set_dtmf_report"):
            getattr(L, name).argtypes = [_vp, _vp]
        L.pn_rate_set_stream_dtmf_clamp.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        L.pn_rate_dtmf_clamp_f32.argtypes = [_vp, _vp, _vp, ctypes.c_int]
    if hasattr(L, "pn_rate_set_stream_dtx"):
        for name in ("pn_dtx_default_params", "pn_dtx_params_check"):
            getattr(L, name).argtypes = [_vp]
        L.pn_dtx_frame.argtypes = [_vp, _vp, _vp, ctypes.c_int, _vp]
        L.pn_dtx_sid_from_acorr.argtypes = [_vp, ctypes.c_int, _vp]
        L.pn_dtx_level.argtypes = [ctypes.c_float]
        L.pn_rate_set_dtx_report.argtypes = [_vp, ctypes.c_int]
        for name in ("pn_rate_set_dtx_params", "pn_rate_get_dtx_params", "pn_rate_get_stream_dtx", "pn_rate_read_dtx_report",
                     "pn_rate_read_dtx_report_dev", "pn_rate_debug_dtx_state"):
            getattr(L, name).argtypes = [_vp, _vp]
        L.pn_rate_set_stream_dtx.argtypes = [_vp, _vp, ctypes.c_int, _vp]
        for name in ("pn_rate_dtx_f32", "pn_rate_dtx_i16", "pn_rate_dtx_g711"):
            getattr(L, name).argtypes = [_vp, _vp, _vp, ctypes.c_int]
    if hasattr(L, "pn_host_pipeline_prepare"):
        L.pn_host_pipeline_prepare.argtypes = [_vp]
    L.pn_ctx_debug_copy.restype = ctypes.c_longlong
    L.pn_ctx_debug_copy.argtypes = [_vp, ctypes.c_int, _vp, ctypes.c_longlong]
    L.pn_ctx_set_profiling.argtypes = [_vp, ctypes.c_int]
    L.pn_kernel_name.restype = ctypes.c_char_p
    L.pn_kernel_name.argtypes = [ctypes.c_int]
    L.pn_ctx_kernel_time.argtypes = [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_int64)]
    L.pn_ctx_reset_profile.argtypes = [_vp]
    L.pn_featgen_create.restype = _vp
    L.pn_featgen_create.argtypes = [ctypes.c_int, ctypes.c_int, _vp]
    L.pn_featgen_destroy.argtypes = [_vp]
    L.pn_featgen_reset.argtypes = [_vp]
    L.pn_featgen_synchronize.argtypes = [_vp]
    L.pn_featgen_device_bytes.restype = ctypes.c_size_t
    L.pn_featgen_device_bytes.argtypes = [_vp]
    L.pn_featgen_process_i16.argtypes = [_vp, _vp, _vp, _vp, _vp]
    L.pn_featgen_process_i16_files.argtypes = [_vp, _vp, _vp, ctypes.c_int, _vp, _vp]
    L.pn_featgen_process_host_i16_files.argtypes = [_vp, _vp, _vp, ctypes.c_int, _vp, _vp]
    L.pn_featgen_run_files.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
    _lib = L
    return L


def _err(L):
    return L.pn_last_error().decode(errors="replace")


class Model:
    def __init__(self, blob):
        self.L = load_library()
        self.h = self.L.pn_model_from_blob(blob, len(blob))
        if not self.h:
            raise PercepNetError(_err(self.L))

    def close(self):
        if self.h:
            self.L.pn_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """B independent streams advanced one 10 ms frame per call (pn_ctx)."""

    def __init__(self, model, n_streams, device=0, nn_mode=NN_MFMA, stream=None):
        self.L = model.L
        self.model = model
        self.n_streams = int(n_streams)
        self.h = self.L.pn_ctx_create(model.h, device, self.n_streams, nn_mode, stream)
        if not self.h:
            raise PercepNetError(_err(self.L))

    def close(self):
        if self.h:
            self.L.pn_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise PercepNetError(_err(self.L))

    def reset(self):
        self._chk(self.L.pn_ctx_reset(self.h))

    def reset_streams(self, ids):
        """rnnoise_init for the streams `ids` only (the others keep running): include/percepnet_hip.h pn_ctx_reset_streams."""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).ravel())
        self._chk(self.L.pn_ctx_reset_streams(self.h, a.ctypes.data, int(a.size)))

    def synchronize(self):
        self._chk(self.L.pn_ctx_synchronize(self.h))

    def set_postfilter(self, enable):
        """Optional envelope post-filter on the gains (reference post_filtering, denoise.cpp:216-250)."""
        self._chk(self.L.pn_ctx_set_postfilter(self.h, int(bool(enable))))

    def set_atten_limit(self, ids, db):
        """Attenuation limit in dB of the distinct streams `ids` (include/percepnet_hip.h pn_ctx_set_atten_limit): `db` is one
        value for all of them or one per id; 0 = bypass, math.inf = off.  Ordered with the frames like reset_streams."""
        a = self._ids(ids)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(db, dtype=np.float32), a.shape))
        self._chk(self.L.pn_ctx_set_atten_limit(self.h, a.ctypes.data, int(a.size), v.ctypes.data))

    def set_report(self, on):
        """Per-stream frame report from the next frame on (include/percepnet_hip.h pn_ctx_set_report): read_report()."""
        self._chk(self.L.pn_ctx_set_report(self.h, int(bool(on))))

    def set_output_saturate(self, on):
        """int16 outputs saturate at the ends of the range instead of wrapping (pn_ctx_set_output_saturate)."""
        self._chk(self.L.pn_ctx_set_output_saturate(self.h, int(bool(on))))

    def read_report(self):
        """-> REPORT_DTYPE [n_streams]: the last frame's records (synchronising; raises while the report is off)."""
        rep = np.empty(self.n_streams, REPORT_DTYPE)
        self._chk(self.L.pn_ctx_read_report(self.h, rep.ctypes.data))
        return rep

    def read_report_dev(self, d_report):
        """Device-pointer twin of read_report (async on the context's stream): [n_streams][REPORT_WORDS] 32-bit words."""
        self._chk(self.L.pn_ctx_read_report_dev(self.h, d_report))

    def atten_limit(self):
        """-> float32 [n_streams]: the attenuation limits as set, in dB (inf = off)."""
        out = np.empty(self.n_streams, np.float32)
        self._chk(self.L.pn_ctx_get_atten_limit(self.h, out.ctypes.data))
        return out

    def device_bytes(self):
        return self.L.pn_ctx_device_bytes(self.h)

    def weight_bytes(self):
        return self.L.pn_ctx_weight_bytes(self.h)

    def describe(self):
        """{"nn": ..., "dense": "small"|"batch", "gru": ..., "gru_rb": ..., "frontend": ...}: the kernel families in use."""
        buf = ctypes.create_string_buffer(256)
        if self.L.pn_ctx_describe(self.h, buf, len(buf)) < 0:
            raise PercepNetError("pn_ctx_describe failed")
        return dict(kv.split("=", 1) for kv in buf.value.decode().split())

    # device-pointer entry points (ints, e.g. torch.Tensor.data_ptr())
    def process_i16_dev(self, d_in, d_out, d_gr=None):
        self._chk(self.L.pn_process_i16(self.h, d_in, d_out, d_gr))

    def process_f32_dev(self, d_in, d_out, d_gr=None):
        self._chk(self.L.pn_process_f32(self.h, d_in, d_out, d_gr))

    def process_i16_active_dev(self, d_in, d_out, d_gr, ids):
        """One frame for the streams `ids` only; every other stream keeps all of its state and its output rows
        (include/percepnet_hip.h pn_process_i16_active; reference contract: src/denoise.cpp:508-547, one call per stream)."""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).ravel())
        self._chk(self.L.pn_process_i16_active(self.h, d_in, d_out, d_gr, a.ctypes.data, int(a.size)))

    def process_f32_active_dev(self, d_in, d_out, d_gr, ids):
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).ravel())
        self._chk(self.L.pn_process_f32_active(self.h, d_in, d_out, d_gr, a.ctypes.data, int(a.size)))

    def debug_inject_launch_failure(self, enable):
        self._chk(self.L.pn_ctx_debug_inject_launch_failure(self.h, int(bool(enable))))

    # pipelined host-buffer entry points (raw host pointers; the buffers should be pinned and must outlive delivery)
    # h_report (optional): this frame's report records go there too, [n_streams][REPORT_WORDS] words, under h_out's lifetime rule
    def submit_host_i16(self, h_in, h_out, h_gr=None, h_report=None):
        if h_report is not None:
            self._chk(self.L.pn_host_next_report(self.h, h_report))
        self._chk(self.L.pn_submit_host_i16(self.h, h_in, h_out, h_gr))

    def submit_host_i16_active(self, h_in, h_out, h_gr, ids, h_report=None):
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).ravel())
        if h_report is not None:
            self._chk(self.L.pn_host_next_report(self.h, h_report))
        self._chk(self.L.pn_submit_host_i16_active(self.h, h_in, h_out, h_gr, a.ctypes.data, int(a.size)))

    def host_pipeline_prepare(self):
        """Builds the pipelined host path now (pn_host_pipeline_prepare) instead of inside the first submit: tens of milliseconds
        of queue probing that a caller on a real-time clock spends before its first frame arrives."""
        self._chk(self.L.pn_host_pipeline_prepare(self.h))

    def frames_delivered(self):
        """Frames of the pipelined host path (the context's or a converter's) whose output has landed; non-blocking."""
        n = int(self.L.pn_host_frames_delivered(self.h))
        if n < 0:
            raise PercepNetError(_err(self.L))
        return n

    def pipe_streams(self):
        """'nn' / 'hl' ...: how the copy streams of the pipelined host path were obtained ('' before the first submit)"""
        return self.L.pn_ctx_pipe_streams(self.h).decode() if hasattr(self.L, "pn_ctx_pipe_streams") else ""

    def host_wait(self):
        self._chk(self.L.pn_host_wait(self.h))

    # host numpy entry points
    def process_i16(self, frame, want_gr=True):
        frame = np.ascontiguousarray(frame, dtype=np.int16).reshape(self.n_streams, FRAME)
        out = np.empty_like(frame)
        gr = np.empty((self.n_streams, 68), np.float32) if want_gr else None
        self._chk(self.L.pn_process_host_i16(self.h, frame.ctypes.data, out.ctypes.data,
                                             gr.ctypes.data if want_gr else None))
        return out, gr

    def process_f32(self, frame, want_gr=True):
        frame = np.ascontiguousarray(frame, dtype=np.float32).reshape(self.n_streams, FRAME)
        out = np.empty_like(frame)
        gr = np.empty((self.n_streams, 68), np.float32) if want_gr else None
        self._chk(self.L.pn_process_host_f32(self.h, frame.ctypes.data, out.ctypes.data,
                                             gr.ctypes.data if want_gr else None))
        return out, gr

    def run_pcm(self, pcm):
        """percepNet_run semantics (main.cpp:30-39) for a batch: pcm int16 [B, n_frames*480] ->
        (out int16 [B, (n_frames-1)*480] with the first output frame dropped, gr [B, n_frames, 68])."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n_streams, -1)
        n = pcm.shape[1] // FRAME
        out = np.zeros((self.n_streams, max(n - 1, 0) * FRAME), np.int16)
        gr = np.zeros((self.n_streams, n, 68), np.float32)
        for t in range(n):
            o, g = self.process_i16(pcm[:, t * FRAME:(t + 1) * FRAME])
            gr[:, t] = g
            if t > 0:
                out[:, (t - 1) * FRAME:t * FRAME] = o
        return out, gr

    def read_features(self):
        feat = np.empty((self.n_streams, 70), np.float32)
        sil = np.empty(self.n_streams, np.int32)
        self._chk(self.L.pn_ctx_read_features(self.h, feat.ctypes.data, sil.ctypes.data))
        return feat, sil

    def read_features_dev(self, d_feat, d_sil=None):
        """Device-pointer twin of read_features (async on the context's stream)."""
        self._chk(self.L.pn_ctx_read_features_dev(self.h, d_feat, d_sil))

    def compute_rnn(self, feat):
        feat = np.ascontiguousarray(feat, dtype=np.float32).reshape(self.n_streams, 70)
        gr = np.empty((self.n_streams, 68), np.float32)
        self._chk(self.L.pn_ctx_compute_rnn_host(self.h, feat.ctypes.data, gr.ctypes.data))
        return gr

    RNN_STATE_SHAPES = (("conv1", 4 * 128), ("conv2", 2 * 512), ("gru1", 512), ("gru2", 512), ("gru3", 512),
                        ("gru_gb", 512), ("gru_rb", 128))

    def get_rnn_state(self):
        """-> {name: float32 [n_streams, n]} in the reference's RNNState layout (nnet_data.h:28-38)."""
        st = {k: np.empty((self.n_streams, n), np.float32) for k, n in self.RNN_STATE_SHAPES}
        self._chk(self.L.pn_ctx_get_rnn_state_host(self.h, *[st[k].ctypes.data for k, _ in self.RNN_STATE_SHAPES]))
        return st

    def set_rnn_state(self, st):
        arrs = [np.ascontiguousarray(st[k], dtype=np.float32).reshape(self.n_streams, n) if k in st else None
                for k, n in self.RNN_STATE_SHAPES]
        self._chk(self.L.pn_ctx_set_rnn_state_host(self.h, *[a.ctypes.data if a is not None else None for a in arrs]))

    # per-stream state records: moving live streams between slots, contexts, devices and processes
    @staticmethod
    def _ids(ids):
        return np.ascontiguousarray(np.asarray(ids, dtype=np.int32).ravel())

    def export_streams(self, ids):
        """-> uint8 [n, STREAM_STATE_BYTES]: the whole state of the streams `ids` (pn_ctx_export_streams_host)."""
        a = self._ids(ids)
        rec = np.empty((a.size, STREAM_STATE_BYTES), np.uint8)
        self._chk(self.L.pn_ctx_export_streams_host(self.h, a.ctypes.data, int(a.size), rec.ctypes.data))
        return rec

    def import_streams(self, ids, records):
        """Records from export_streams (any context of the same model) into the distinct streams `ids`; all or nothing
        (pn_ctx_import_streams_host)."""
        a = self._ids(ids)
        rec = np.ascontiguousarray(records, dtype=np.uint8)
        if rec.size != a.size * STREAM_STATE_BYTES:
            raise PercepNetError(f"{rec.size} record bytes for {a.size} streams (a record has {STREAM_STATE_BYTES})")
        self._chk(self.L.pn_ctx_import_streams_host(self.h, a.ctypes.data, int(a.size), rec.ctypes.data))

    def export_streams_dev(self, ids, d_records):
        """Device form (async on the context's stream): records [n][STREAM_STATE_BYTES] at device address d_records."""
        a = self._ids(ids)
        self._chk(self.L.pn_ctx_export_streams(self.h, a.ctypes.data, int(a.size), d_records))

    def import_streams_dev(self, ids, d_records, d_status):
        """Device form (async): d_status (device int32 [n]) receives SS_OK or the SS_BAD_* verdict of each record."""
        a = self._ids(ids)
        self._chk(self.L.pn_ctx_import_streams(self.h, a.ctypes.data, int(a.size), d_records, d_status))

    def debug_copy(self, which, n_floats):
        """Internal device buffer `which` (see pn_ctx_debug_copy in percepnet_hip.h) -> float32[n_floats] (tests/tools)."""
        buf = np.empty(n_floats, np.float32)
        n = self.L.pn_ctx_debug_copy(self.h, which, buf.ctypes.data, buf.nbytes)
        if n < 0:
            raise PercepNetError(_err(self.L))
        return buf[:n // 4]

    def set_profiling(self, on):
        self._chk(self.L.pn_ctx_set_profiling(self.h, 1 if on else 0))

    def reset_profile(self):
        self._chk(self.L.pn_ctx_reset_profile(self.h))

    def kernel_times(self):
        """-> {family: (total_ms, launches)} from HIP events on the context's stream."""
        out = {}
        for i in range(self.L.pn_kernel_count()):
            name = self.L.pn_kernel_name(i)
            ms = ctypes.c_double()
            n = ctypes.c_int64()
            self._chk(self.L.pn_ctx_kernel_time(self.h, name, ctypes.byref(ms), ctypes.byref(n)))
            out[name.decode()] = (ms.value, n.value)
        return out


def atten_limit_factor(db):
    """The mix factor lam = 10^(-db/20) the engine uses for an attenuation limit of `db` dB (pn_atten_limit_factor, host only):
    1.0 at 0 dB, 0.0 (off) for inf and beyond ~758.6 dB, NaN for a negative or NaN db."""
    return float(load_library().pn_atten_limit_factor(float(db)))


def stream_state_check(record, model):
    """PN_SS_OK (0) or the PN_SS_BAD_* verdict a context of `model` gives the bytes `record` (host only, no GPU)."""
    L = load_library()
    b = np.ascontiguousarray(np.frombuffer(bytes(record), np.uint8)) if not isinstance(record, np.ndarray) else \
        np.ascontiguousarray(record, dtype=np.uint8)
    return int(L.pn_stream_state_check(b.ctypes.data if b.size else None, b.size, model.h))


def rate_frame_samples(rate_hz):
    """Samples per 10 ms frame at rate_hz: 80 | 160 | 240 | 320; -1 for a rate no converter takes (pn_rate_frame_samples, host only)."""
    return int(load_library().pn_rate_frame_samples(int(rate_hz)))


def rate_delay_samples(rate_hz):
    """Input-to-output delay of a converted stream in samples at rate_hz: 512 | 992 | 1472 | 1952; -1 for a refused rate (host only)."""
    return int(load_library().pn_rate_delay_samples(int(rate_hz)))


def rate_taps(rate_hz, down=False):
    """The converter's fp32 taps for k = -D..D, D = 16 L for a rate of 48000 M / L: h (up) or g = h M / L (down); 32000 is
    (L, M) = (3, 2) and its h the table of 16000 (pn_rate_taps, host only)."""
    L = load_library()
    t = np.empty(2 * RATE_TAPS * 6 + 1, np.float32)    # PN_RATE_MAX_TAPS: room for the longest table; the library says how many it wrote
    n = int(L.pn_rate_taps(int(rate_hz), int(bool(down)), t.ctypes.data, int(t.size)))
    if n < 0:
        raise PercepNetError(_err(L))
    return t[:n].copy()


def rate_state_bytes(rate_hz):
    """Bytes of one converter state record at rate_hz: 912 | 528 | 400 | 336; 0 for a refused rate (host only)."""
    return int(load_library().pn_rate_state_bytes(int(rate_hz)))


def rate_state_max_bytes():
    """Bytes of the largest converter state record (8000 Hz: 912): the stride of a mixed converter's device-side records (host only)."""
    return int(load_library().pn_rate_state_max_bytes())


def rate_state_check(record, rate_hz):
    """PN_SS_OK (0) or the PN_SS_BAD_* verdict a converter of rate_hz gives the bytes `record` (host only, no GPU)."""
    L = load_library()
    b = np.ascontiguousarray(np.frombuffer(bytes(record), np.uint8)) if not isinstance(record, np.ndarray) else \
        np.ascontiguousarray(record, dtype=np.uint8)
    return int(L.pn_rate_state_check(b.ctypes.data if b.size else None, b.size, int(rate_hz)))


def rate_call_state_bytes():
    """Bytes of one call-state record, whatever the stream's rate: 10640 (pn_rate_call_state_bytes, host only)."""
    return int(load_library().pn_rate_call_state_bytes())


def rate_call_state_check(record):
    """PN_SS_OK (0) or the PN_SS_BAD_* verdict of the bytes `record` as a call-state record (pn_rate_call_state_check, host only)."""
    L = load_library()
    b = np.ascontiguousarray(np.frombuffer(bytes(record), np.uint8)) if not isinstance(record, np.ndarray) else \
        np.ascontiguousarray(record).view(np.uint8).reshape(-1)
    return int(L.pn_rate_call_state_check(b.ctypes.data if b.size else None, b.size))


def rate_mixed_frame_samples(rate_hz):
    """Samples per 10 ms frame of a stream of a mixed converter: 80 | 160 | 240 | 320 | 480; -1 for any other rate (host only)."""
    return int(load_library().pn_rate_mixed_frame_samples(int(rate_hz)))


def rate_mixed_delay_samples(rate_hz):
    """Input-to-output delay in samples at rate_hz of a stream of a mixed converter: 512 | 992 | 1472 | 1952 | 2880; -1 (host only)."""
    return int(load_library().pn_rate_mixed_delay_samples(int(rate_hz)))


def g711_decode(law, codes):
    """G.711 bytes -> int16 of the same shape, law = G711_ULAW | G711_ALAW (pn_g711_decode, host only)."""
    L = load_library()
    b = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.empty(b.shape, np.int16)
    if L.pn_g711_decode(int(law), b.ctypes.data, out.ctypes.data, b.size) != 0:
        raise PercepNetError(_err(L))
    return out


def g711_encode(law, pcm):
    """int16 -> G.711 bytes of the same shape, law = G711_ULAW | G711_ALAW (pn_g711_encode, host only)."""
    L = load_library()
    v = np.ascontiguousarray(pcm, dtype=np.int16)
    out = np.empty(v.shape, np.uint8)
    if L.pn_g711_encode(int(law), v.ctypes.data, out.ctypes.data, v.size) != 0:
        raise PercepNetError(_err(L))
    return out


def rate_confs_check(confs, n_streams):
    """Raises PercepNetError naming the first entry of `confs` that is neither CONF_NONE nor a conference of a converter of
    n_streams streams, a number in [0, n_streams) (pn_rate_confs_check, host only)."""
    L = load_library()
    a = np.ascontiguousarray(np.asarray(confs, dtype=np.int32).ravel())
    if L.pn_rate_confs_check(a.ctypes.data, int(a.size), int(n_streams)) != 0:
        raise PercepNetError(_err(L))


def rate_mix_gains_check(gains):
    """Raises PercepNetError naming the first entry of `gains` that is no send gain of the conference mix, a finite value >= 0
    (pn_rate_mix_gains_check, host only)."""
    L = load_library()
    a = np.ascontiguousarray(np.asarray(gains, dtype=np.float32).ravel())
    if L.pn_rate_mix_gains_check(a.ctypes.data, int(a.size)) != 0:
        raise PercepNetError(_err(L))


def mix_level(row):
    """The level E of one talker's 480 contributions (the send gain already applied) in the mix kernel's summation order
    (pn_mix_level, host only) -> numpy float32 scalar."""
    a = np.ascontiguousarray(row, dtype=np.float32).ravel()
    if a.size != 480:
        raise PercepNetError(f"a row of {a.size} samples: a 48 kHz row has 480")
    return np.float32(load_library().pn_mix_level(a.ctypes.data))


def mix_select(levels, n_max):
    """Which of one conference's talkers (their levels, ascending slot order) the loudest-N rule selects (pn_mix_select, host
    only): n_max = 0 selects everybody -> bool [k]."""
    L = load_library()
    a = np.ascontiguousarray(np.asarray(levels, dtype=np.float32).ravel())
    sel = np.zeros(max(int(a.size), 1), np.uint8)
    if L.pn_mix_select(a.ctypes.data, int(a.size), int(n_max), sel.ctypes.data) < 0:
        raise PercepNetError(_err(L))
    return sel[:a.size].astype(bool)


def plc_pitch(hist):
    """The lag P in [PLC_P_MIN, PLC_P_MAX] the concealer finds on a history of PLC_HIST samples, newest last (pn_plc_pitch, host only)."""
    a = np.ascontiguousarray(hist, dtype=np.float32).ravel()
    if a.size != PLC_HIST:
        raise PercepNetError(f"a history of {a.size} samples: the concealer keeps {PLC_HIST}")
    return int(load_library().pn_plc_pitch(a.ctypes.data))


def plc_period(hist, P):
    """The period buffer q[0..P) of a history and a lag (pn_plc_period, host only) -> float32 [P]."""
    L = load_library()
    a = np.ascontiguousarray(hist, dtype=np.float32).ravel()
    if a.size != PLC_HIST:
        raise PercepNetError(f"a history of {a.size} samples: the concealer keeps {PLC_HIST}")
    q = np.empty(max(int(P), 1), np.float32)
    if L.pn_plc_period(a.ctypes.data, int(P), q.ctypes.data) != 0:
        raise PercepNetError(_err(L))
    return q


def plc_gain(m):
    """g(m): the gain of the synthetic sample m samples into a loss (pn_plc_gain, host only) -> numpy float32 scalar."""
    return np.float32(load_library().pn_plc_gain(int(m)))


def cng_sid(level, coeffs=()):
    """A SID of CNG_SID_BYTES bytes from a level L (-dBov) and up to 12 quantised reflection coefficients N_i -> uint8 [14].  Nothing is
    checked here: the library refuses what the rule excludes."""
    n = list(coeffs)
    sid = np.zeros(CNG_SID_BYTES, np.uint8)
    sid[0], sid[1] = min(len(n), 255), int(level) & 0xff
    sid[2:2 + min(len(n), CNG_MAX_ORDER)] = n[:CNG_MAX_ORDER]
    return sid


def _cng_sid(sid):
    a = np.ascontiguousarray(sid, dtype=np.uint8).ravel()
    if a.size != CNG_SID_BYTES:
        raise PercepNetError(f"a SID of {a.size} bytes: the converter's has {CNG_SID_BYTES} (M, L, N_1..N_12)")
    return a


def cng_sid_decode(sid):
    """(g, k[12], M) of a SID (pn_cng_sid_decode, host only); raises PercepNetError for byte values the rule excludes."""
    L = load_library()
    a, g, k, M = _cng_sid(sid), ctypes.c_float(0), np.zeros(CNG_MAX_ORDER, np.float32), ctypes.c_int32(0)
    if L.pn_cng_sid_decode(a.ctypes.data, ctypes.byref(g), k.ctypes.data, ctypes.byref(M)) != 0:
        raise PercepNetError(_err(L))
    return np.float32(g.value), k, int(M.value)


def cng_level(level):
    """The rms of level L in -dBov, the rule's table entry (pn_cng_level, host only) -> numpy float32 scalar; NaN outside [0, 127]."""
    return np.float32(load_library().pn_cng_level(int(level)))


def cng_frame(sid, state, seed, slot, cont, n):
    """One comfort-noise row of n samples of the stream in `slot` (pn_cng_frame, host only).  state: uint32 [16], updated in place
    -> (row float32 [n], report uint32 [4])."""
    L = load_library()
    a = _cng_sid(sid)
    if not (isinstance(state, np.ndarray) and state.dtype == np.uint32 and state.size == 16 and state.flags.c_contiguous):
        raise PercepNetError("state: a contiguous uint32 array of 16 words")
    row, rep = np.empty(max(int(n), 1), np.float32), np.zeros(4, np.uint32)
    if L.pn_cng_frame(a.ctypes.data, state.ctypes.data, int(seed) & 0xffffffff, int(slot), 1 if cont else 0, int(n), row.ctypes.data, rep.ctypes.data) != 0:
        raise PercepNetError(_err(L))
    return row[:int(n)], rep


def agc_default_params():
    """-> float32 [AGC_N_PARAMS]: the level control's default parameters (pn_agc_default_params, host only)."""
    p = np.empty(AGC_N_PARAMS, np.float32)
    load_library().pn_agc_default_params(p.ctypes.data)
    return p


def _agc_params(params):
    p = np.ascontiguousarray(params, dtype=np.float32).ravel()
    if p.size != AGC_N_PARAMS:
        raise PercepNetError(f"{p.size} AGC parameters: a set has {AGC_N_PARAMS}")
    return p


def agc_params_check(params):
    """Raises PercepNetError naming the first parameter that is NaN or outside its range (pn_agc_params_check, host only)."""
    L = load_library()
    if L.pn_agc_params_check(_agc_params(params).ctypes.data) != 0:
        raise PercepNetError(_err(L))


def agc_frame(params, target, state, row, concealed=False):
    """One frame of the level control on one row of 480 samples (pn_agc_frame, host only).  state: AGC_STATE_DTYPE scalar array
    (np.zeros((), AGC_STATE_DTYPE) is fresh), updated IN PLACE -> (float32 [480] the levelled row, the flags)."""
    L = load_library()
    y = np.ascontiguousarray(row, dtype=np.float32).ravel()
    if y.size != 480:
        raise PercepNetError(f"a row of {y.size} samples: the level control takes 480")
    if not isinstance(state, np.ndarray) or state.dtype != AGC_STATE_DTYPE or state.size != 1 or not state.flags.c_contiguous or not state.flags.writeable:
        raise PercepNetError("state: one writable AGC_STATE_DTYPE record")
    out = np.empty(480, np.float32)
    flags = L.pn_agc_frame(_agc_params(params).ctypes.data, float(np.float32(target)), state.ctypes.data, y.ctypes.data, out.ctypes.data, 1 if concealed else 0)
    if flags < 0:
        raise PercepNetError(_err(L))
    return out, int(flags)


def lim_default_params():
    """-> float32 [LIM_N_PARAMS]: the output limiter's default parameters (pn_lim_default_params, host only)."""
    p = np.empty(LIM_N_PARAMS, np.float32)
    load_library().pn_lim_default_params(p.ctypes.data)
    return p


def _lim_params(params):
    p = np.ascontiguousarray(params, dtype=np.float32).ravel()
    if p.size != LIM_N_PARAMS:
        raise PercepNetError(f"{p.size} limiter parameters: a set has {LIM_N_PARAMS}")
    return p


def lim_params_check(params):
    """Raises PercepNetError naming the first parameter that is NaN or outside its range (pn_lim_params_check, host only)."""
    L = load_library()
    if L.pn_lim_params_check(_lim_params(params).ctypes.data) != 0:
        raise PercepNetError(_err(L))


def lim_frame(params, ceiling, state, row, want_report=False):
    """One frame of the output limiter on one row of 480 samples (pn_lim_frame, host only).  state: LIM_STATE_DTYPE scalar array
    (np.zeros((), LIM_STATE_DTYPE) is fresh), updated IN PLACE -> (float32 [480] the limited row, the flags[, the LIM_REPORT_DTYPE row])."""
    L = load_library()
    y = np.ascontiguousarray(row, dtype=np.float32).ravel()
    if y.size != 480:
        raise PercepNetError(f"a row of {y.size} samples: the limiter takes 480")
    if not isinstance(state, np.ndarray) or state.dtype != LIM_STATE_DTYPE or state.size != 1 or not state.flags.c_contiguous or not state.flags.writeable:
        raise PercepNetError("state: one writable LIM_STATE_DTYPE record")
    out = np.empty(480, np.float32)
    rep = np.zeros((), LIM_REPORT_DTYPE)
    flags = L.pn_lim_frame(_lim_params(params).ctypes.data, float(np.float32(ceiling)), state.ctypes.data, y.ctypes.data, out.ctypes.data,
                           rep.ctypes.data if want_report else None)
    if flags < 0:
        raise PercepNetError(_err(L))
    return (out, int(flags), rep) if want_report else (out, int(flags))


def dtx_default_params():
    """-> float32 [DTX_N_PARAMS]: the DTX send side's default parameters (pn_dtx_default_params, host only).  Not tuned on speech."""
    p = np.empty(DTX_N_PARAMS, np.float32)
    load_library().pn_dtx_default_params(p.ctypes.data)
    return p


def _dtx_params(params):
    p = np.ascontiguousarray(params, dtype=np.float32).ravel()
    if p.size != DTX_N_PARAMS:
        raise PercepNetError(f"{p.size} DTX parameters: a set has {DTX_N_PARAMS}")
    return p


def dtx_params_check(params):
    """Raises PercepNetError naming the first parameter that is NaN, outside its range or no whole number where one is asked
    (pn_dtx_params_check, host only)."""
    L = load_library()
    if L.pn_dtx_params_check(_dtx_params(params).ctypes.data) != 0:
        raise PercepNetError(_err(L))


def dtx_frame(params, state, row):
    """One frame of the DTX send side on one float row (80, 160, 240, 320 or 480 samples) of an enabled stream (pn_dtx_frame, host
    only).  state: uint32 [DTX_STATE_WORDS] (zeros are fresh), updated IN PLACE -> (the decision, the DTX_REPORT_DTYPE row)."""
    L = load_library()
    x = np.ascontiguousarray(row, dtype=np.float32).ravel()
    if not isinstance(state, np.ndarray) or state.dtype != np.uint32 or state.size != DTX_STATE_WORDS or not state.flags.c_contiguous or not state.flags.writeable:
        raise PercepNetError(f"state: {DTX_STATE_WORDS} writable contiguous uint32 words")
    rep = np.zeros((), DTX_REPORT_DTYPE)
    decision = L.pn_dtx_frame(_dtx_params(params).ctypes.data, state.ctypes.data, x.ctypes.data, int(x.size), rep.ctypes.data)
    if decision < 0:
        raise PercepNetError(_err(L))
    return int(decision), rep


def dtx_sid_from_acorr(R, order):
    """The SID of the noise statistics R[0..12] at the given order (pn_dtx_sid_from_acorr, host only): the Levinson step alone ->
    uint8 [14]: M, the level of R[0], N_1..N_M, zeros."""
    L = load_library()
    r = np.ascontiguousarray(R, dtype=np.float32).ravel()
    if r.size != 13:
        raise PercepNetError(f"{r.size} autocorrelation lags: the step takes 13, R[0..12]")
    sid = np.zeros(CNG_SID_BYTES, np.uint8)
    if L.pn_dtx_sid_from_acorr(r.ctypes.data, int(order), sid.ctypes.data) < 0:
        raise PercepNetError(_err(L))
    return sid


def dtx_level(mean_square):
    """L in -dBov of a mean square: how many of the rule's 127 edges lie above it (pn_dtx_level, host only)."""
    return int(load_library().pn_dtx_level(ctypes.c_float(float(np.float32(mean_square)))))


def dtmf_default_params():
    """-> float32 [DTMF_N_PARAMS]: the DTMF detector's default parameters (pn_dtmf_default_params, host only)."""
    p = np.empty(DTMF_N_PARAMS, np.float32)
    load_library().pn_dtmf_default_params(p.ctypes.data)
    return p


def _dtmf_params(params):
    p = np.ascontiguousarray(params, dtype=np.float32).ravel()
    if p.size != DTMF_N_PARAMS:
        raise PercepNetError(f"{p.size} DTMF parameters: a set has {DTMF_N_PARAMS}")
    return p


def dtmf_params_check(params):
    """Raises PercepNetError naming the first parameter that is NaN, outside its range or no whole number where one is asked
    (pn_dtmf_params_check, host only)."""
    L = load_library()
    if L.pn_dtmf_params_check(_dtmf_params(params).ctypes.data) != 0:
        raise PercepNetError(_err(L))


def dtmf_tables():
    """-> (ct float32 [8, 480], st float32 [8, 480], rot float32 [16] = cr then ci): the detector's tables (pn_dtmf_tables, host only)."""
    ct, st, rot = np.empty((8, 480), np.float32), np.empty((8, 480), np.float32), np.empty(16, np.float32)
    L = load_library()
    if L.pn_dtmf_tables(ct.ctypes.data, st.ctypes.data, rot.ctypes.data) != 0:
        raise PercepNetError(_err(L))
    return ct, st, rot


def dtmf_frame(params, state, row, concealed=False):
    """One frame of the DTMF detector on one row of 480 samples of an enabled stream (pn_dtmf_frame, host only).  state: uint32
    [DTMF_STATE_WORDS] (zeros are fresh), updated IN PLACE -> (the flags, the DTMF_REPORT_DTYPE row)."""
    L = load_library()
    x = np.ascontiguousarray(row, dtype=np.float32).ravel()
    if x.size != 480:
        raise PercepNetError(f"a row of {x.size} samples: the detector takes 480")
    if not isinstance(state, np.ndarray) or state.dtype != np.uint32 or state.size != DTMF_STATE_WORDS or not state.flags.c_contiguous or not state.flags.writeable:
        raise PercepNetError(f"state: {DTMF_STATE_WORDS} writable contiguous uint32 words")
    rep = np.zeros((), DTMF_REPORT_DTYPE)
    flags = L.pn_dtmf_frame(_dtmf_params(params).ctypes.data, state.ctypes.data, x.ctypes.data, 1 if concealed else 0, rep.ctypes.data)
    if flags < 0:
        raise PercepNetError(_err(L))
    return int(flags), rep


def dtmf_clamp_default_params():
    """-> int32 [DTMF_CLAMP_N_PARAMS]: DTMF removal's default parameters (pn_dtmf_clamp_default_params, host only)."""
    p = np.empty(DTMF_CLAMP_N_PARAMS, np.int32)
    load_library().pn_dtmf_clamp_default_params(p.ctypes.data)
    return p


def _dtmf_clamp_params(params):
    p = np.asarray(params).ravel()
    if p.size != DTMF_CLAMP_N_PARAMS:
        raise PercepNetError(f"{p.size} DTMF removal parameters: a set has {DTMF_CLAMP_N_PARAMS}")
    if not np.issubdtype(p.dtype, np.integer) and not np.all(p == np.floor(p)):
        raise PercepNetError("DTMF removal parameters are whole numbers")
    return np.ascontiguousarray(p, dtype=np.int32)


def dtmf_clamp_params_check(params, dtmf_params=None):
    """Raises PercepNetError naming the first parameter outside its range or, with the detector's parameters given, a guard that is
    not in time: on_frames + pre > 5 (pn_dtmf_clamp_params_check, host only)."""
    L = load_library()
    d = _dtmf_params(dtmf_params) if dtmf_params is not None else None
    if L.pn_dtmf_clamp_params_check(_dtmf_clamp_params(params).ctypes.data, d.ctypes.data if d is not None else None) != 0:
        raise PercepNetError(_err(L))


def dtmf_event_payload(digit, end, volume, dur, ts_per_frame):
    """-> the RFC 4733 payload of `digit` (a character or its code) after dur frames as a 32-bit value, to be sent big-endian; 0 for
    a digit that is none (pn_dtmf_event_payload, host only)."""
    code = ord(digit) if isinstance(digit, str) else int(digit)
    return int(load_library().pn_dtmf_event_payload(code, 1 if end else 0, int(volume), int(dur) & 0xffffffff, int(ts_per_frame)))


def dtmf_clamp_frame(params, state, det_report, row):
    """One frame of DTMF removal on one row of 480 samples of a stream with removal on (pn_dtmf_clamp_frame, host only).  state:
    uint32 [DTMF_CLAMP_STATE_WORDS] (zeros are fresh), row: float32 [480], both updated IN PLACE; det_report: the detector's four
    report words of this frame, None: detection off -> (the flags, the DTMF_CLAMP_REPORT_DTYPE row).  The in-time condition is not
    checked here."""
    L = load_library()
    if not isinstance(row, np.ndarray) or row.dtype != np.float32 or row.size != 480 or not row.flags.c_contiguous or not row.flags.writeable:
        raise PercepNetError("row: 480 writable contiguous float32 samples")
    if not isinstance(state, np.ndarray) or state.dtype != np.uint32 or state.size != DTMF_CLAMP_STATE_WORDS or not state.flags.c_contiguous or not state.flags.writeable:
        raise PercepNetError(f"state: {DTMF_CLAMP_STATE_WORDS} writable contiguous uint32 words")
    det = None
    if det_report is not None:
        det = np.ascontiguousarray(np.asarray(det_report).view(np.uint32) if isinstance(det_report, np.ndarray) and det_report.dtype == DTMF_REPORT_DTYPE else det_report,
                                   dtype=np.uint32).ravel()
        if det.size != DTMF_REPORT_WORDS:
            raise PercepNetError(f"a detector report row of {det.size} words: it has {DTMF_REPORT_WORDS}")
    rep = np.zeros((), DTMF_CLAMP_REPORT_DTYPE)
    flags = L.pn_dtmf_clamp_frame(_dtmf_clamp_params(params).ctypes.data, state.ctypes.data, det.ctypes.data if det is not None else None, row.ctypes.data, rep.ctypes.data)
    if flags < 0:
        raise PercepNetError(_err(L))
    return int(flags), rep


class RateConverter:
    """8, 16, 24 or 32 kHz streams through a 48 kHz Context (pn_rate): a converter beside `ctx` for all of its streams at ONE rate.
    It borrows the context (device, n_streams, HIP stream): close the converter before the context."""

    def __init__(self, ctx, rate_hz):
        self.L = ctx.L
        self.ctx = ctx
        self.rate = int(rate_hz)
        self.n_streams = ctx.n_streams
        self.h = self.L.pn_rate_create(ctx.h, self.rate)
        if not self.h:
            raise PercepNetError(_err(self.L))
        self.frame = rate_frame_samples(self.rate)
        self.state_bytes = rate_state_bytes(self.rate)

    def close(self):
        if self.h:
            if self.ctx.h:                      # (a context closed first has taken the device buffers' stream with it)
                self.L.pn_rate_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise PercepNetError(_err(self.L))

    @staticmethod
    def _ids(ids):
        if ids is None:
            return None, 0
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).ravel())
        return a, int(a.size)

    def reset(self):
        self._chk(self.L.pn_rate_reset(self.h))

    def reset_streams(self, ids):
        """The converter's half of a slot reset (pn_rate_reset_streams): call Context.reset_streams for the same slots."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_reset_streams(self.h, a.ctypes.data, n))

    # the two kernels on their own: device pointers (ints); ids None = every stream
    def _kernel(self, name, d_in, d_out, ids):
        a, n = self._ids(ids)
        self._chk(getattr(self.L, name)(self.h, d_in, d_out, a.ctypes.data if a is not None else None, n))

    def up_f32_dev(self, d_in, d_out48, ids=None):
        self._kernel("pn_rate_up_f32", d_in, d_out48, ids)

    def up_i16_dev(self, d_in, d_out48, ids=None):
        self._kernel("pn_rate_up_i16", d_in, d_out48, ids)

    def down_f32_dev(self, d_in48, d_out, ids=None):
        self._kernel("pn_rate_down_f32", d_in48, d_out, ids)

    def down_i16_dev(self, d_in48, d_out, ids=None):
        self._kernel("pn_rate_down_i16", d_in48, d_out, ids)

    # G.711 rows (one byte per sample, a law per stream): the byte twins of the int16 entry points
    def set_stream_laws(self, ids, laws):
        """Streams `ids` continue under `laws` (G711_ULAW | G711_ALAW) from the next frame on (pn_rate_set_stream_laws):
        asynchronous, ordered like reset_streams; a setting that resets, rate changes and records leave alone."""
        a, n = self._ids(ids)
        w = np.ascontiguousarray(np.asarray(laws, dtype=np.int32).ravel())
        if w.size != n:
            raise PercepNetError(f"{w.size} laws for {n} streams")
        self._chk(self.L.pn_rate_set_stream_laws(self.h, a.ctypes.data, n, w.ctypes.data))

    def stream_laws(self):
        """-> int32 [n_streams]: the laws as last set (pn_rate_get_stream_laws); mu-law for every stream of a new converter."""
        w = np.empty(self.n_streams, np.int32)
        self._chk(self.L.pn_rate_get_stream_laws(self.h, w.ctypes.data))
        return w

    def up_g711_dev(self, d_in, d_out48, ids=None):
        self._kernel("pn_rate_up_g711", d_in, d_out48, ids)

    def down_g711_dev(self, d_in48, d_out, ids=None):
        self._kernel("pn_rate_down_g711", d_in48, d_out, ids)

    def process_g711_dev(self, d_in, d_out, d_gr=None, ids=None):
        if ids is None:
            self._chk(self.L.pn_rate_process_g711(self.h, d_in, d_out, d_gr))
        else:
            a, n = self._ids(ids)
            self._chk(self.L.pn_rate_process_g711_active(self.h, d_in, d_out, d_gr, a.ctypes.data, n))

    def process_g711(self, frame, want_gr=True):
        return self._host("pn_rate_process_host_g711", frame, np.uint8, want_gr)

    def submit_host_g711(self, h_in, h_out, h_gr=None, h_report=None, ids=None):
        self._submit("g711", h_in, h_out, h_gr, h_report, ids)

    def run_g711(self, codes):
        """percepnet_run --rate R --g711 semantics for a batch: codes uint8 [B, n_frames * frame] under the streams' laws -> uint8
        [B, (n_frames - 1) * frame] (the first output frame dropped, like run_pcm)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(self.n_streams, -1)
        f, n = self.frame, codes.shape[1] // self.frame
        out = np.zeros((self.n_streams, max(n - 1, 0) * f), np.uint8)
        for t in range(n):
            o, _ = self.process_g711(codes[:, t * f:(t + 1) * f], want_gr=False)
            if t > 0:
                out[:, (t - 1) * f:t * f] = o
        return out

    # conferences: every member hears the fp32 sum of the OTHER members' enhanced 48 kHz rows, members in ascending slot order
    def set_stream_confs(self, ids, confs):
        """Streams `ids` continue in the conferences `confs` (CONF_NONE, or a number in [0, n_streams)) from the next frame on
        (pn_rate_set_stream_confs): asynchronous, ordered like set_stream_laws; a setting that resets, rate changes and records
        leave alone.  A conference holds at most CONF_MAX_MEMBERS streams.  A member that only listens is fed silence and stays
        on the id list; mixes clip, so turn Context.set_output_saturate on."""
        a, n = self._ids(ids)
        w = np.ascontiguousarray(np.asarray(confs, dtype=np.int32).ravel())
        if w.size != n:
            raise PercepNetError(f"{w.size} conferences for {n} streams")
        self._chk(self.L.pn_rate_set_stream_confs(self.h, a.ctypes.data, n, w.ctypes.data))

    def stream_confs(self):
        """-> int32 [n_streams]: the conferences as last set (pn_rate_get_stream_confs); CONF_NONE everywhere on a new converter."""
        w = np.empty(self.n_streams, np.int32)
        self._chk(self.L.pn_rate_get_stream_confs(self.h, w.ctypes.data))
        return w

    def mix_f32_dev(self, d_in48, d_out48, ids=None):
        """The mix kernel on its own (pn_rate_mix_f32): device rows [n_streams][480] float, which must not overlap."""
        self._kernel("pn_rate_mix_f32", d_in48, d_out48, ids)

    # loudest-N talkers, send gains, hold and the mix report: settings of the conference mix, ordered like set_stream_confs
    def set_stream_mix_gains(self, ids, gains):
        """Streams `ids` send into their conferences with `gains` (finite, >= 0; 0 mutes: the member still hears) from the next
        frame on (pn_rate_set_stream_mix_gains)."""
        a, n = self._ids(ids)
        w = np.ascontiguousarray(np.asarray(gains, dtype=np.float32).ravel())
        if w.size != n:
            raise PercepNetError(f"{w.size} gains for {n} streams")
        self._chk(self.L.pn_rate_set_stream_mix_gains(self.h, a.ctypes.data, n, w.ctypes.data))

    def stream_mix_gains(self):
        """-> float32 [n_streams]: the send gains as last set (pn_rate_get_stream_mix_gains); 1 everywhere on a new converter."""
        w = np.empty(self.n_streams, np.float32)
        self._chk(self.L.pn_rate_get_stream_mix_gains(self.h, w.ctypes.data))
        return w

    def set_conf_speakers(self, confs, max_speakers):
        """The conferences numbered `confs` mix their `max_speakers` loudest talkers only, 0 = everybody, at most
        CONF_MAX_MEMBERS (pn_rate_set_conf_speakers); the number keeps its cap while the conference is empty."""
        a, n = self._ids(confs)
        w = np.ascontiguousarray(np.asarray(max_speakers, dtype=np.int32).ravel())
        if w.size != n:
            raise PercepNetError(f"{w.size} caps for {n} conferences")
        self._chk(self.L.pn_rate_set_conf_speakers(self.h, a.ctypes.data, n, w.ctypes.data))

    def conf_speakers(self):
        """-> int32 [n_streams], indexed by conference number (pn_rate_get_conf_speakers); 0 everywhere on a new converter."""
        w = np.empty(self.n_streams, np.int32)
        self._chk(self.L.pn_rate_get_conf_speakers(self.h, w.ctypes.data))
        return w

    def set_mix_hold(self, d):
        """The hold factor of the talkers' levels, in [0, 1); 0 = no hold (pn_rate_set_mix_hold).  Zeroes every stream's level."""
        self._chk(self.L.pn_rate_set_mix_hold(self.h, float(d)))

    def mix_hold(self):
        return float(self.L.pn_rate_get_mix_hold(self.h))

    def set_mix_report(self, on):
        self._chk(self.L.pn_rate_set_mix_report(self.h, 1 if on else 0))

    def read_mix_report(self):
        """-> MIX_REPORT_DTYPE [n_streams]: the records of the last mix (pn_rate_read_mix_report, synchronising)."""
        rep = np.empty(self.n_streams, MIX_REPORT_DTYPE)
        self._chk(self.L.pn_rate_read_mix_report(self.h, rep.ctypes.data))
        return rep

    def read_mix_report_dev(self, d_report):
        """The same into device memory [n_streams][4] words, asynchronous on the context's stream (pn_rate_read_mix_report_dev)."""
        self._chk(self.L.pn_rate_read_mix_report_dev(self.h, d_report))

    # packet-loss concealment: a lost stream's 48 kHz row is synthesised from its history, between the up-conversion and the engine
    def set_plc(self, on):
        """Packet-loss concealment on or off (pn_rate_set_plc); the first enable allocates the per-stream state."""
        self._chk(self.L.pn_rate_set_plc(self.h, 1 if on else 0))

    def set_lost(self, ids):
        """Streams `ids` are lost in the NEXT frame submitted on this converter, and only in that one (pn_rate_set_lost):
        asynchronous, ordered like set_stream_laws; calls before one frame add up.  Refused while PLC is off."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_set_lost(self.h, a.ctypes.data if a is not None else None, n))

    def plc_f32_dev(self, d_x48, ids=None):
        """The concealer on its own, in place on device rows [n_streams][480] float (pn_rate_plc_f32); it consumes the marks."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_plc_f32(self.h, d_x48, a.ctypes.data if a is not None else None, n))

    def set_plc_report(self, on):
        self._chk(self.L.pn_rate_set_plc_report(self.h, 1 if on else 0))

    def read_plc_report(self):
        """-> PLC_REPORT_DTYPE [n_streams]: the records of the last frame (pn_rate_read_plc_report, synchronising)."""
        rep = np.empty(self.n_streams, PLC_REPORT_DTYPE)
        self._chk(self.L.pn_rate_read_plc_report(self.h, rep.ctypes.data))
        return rep

    def read_plc_report_dev(self, d_report):
        """The same into device memory [n_streams][4] words, asynchronous on the context's stream (pn_rate_read_plc_report_dev)."""
        self._chk(self.L.pn_rate_read_plc_report_dev(self.h, d_report))

    # comfort noise: a silent (DTX) stream's row is filled with the noise its SID describes, at its own rate, in front of the up-conversion
    def set_cng(self, on):
        """Comfort noise on or off (pn_rate_set_cng); the first enable allocates the per-stream state, the decoded SIDs and the rows."""
        self._chk(self.L.pn_rate_set_cng(self.h, 1 if on else 0))

    def set_cng_seed(self, seed):
        """The converter's excitation seed from the next frame on (pn_rate_set_cng_seed); CNG_DEFAULT_SEED on a new converter."""
        self._chk(self.L.pn_rate_set_cng_seed(self.h, int(seed) & 0xffffffff))

    def cng_seed(self):
        v = ctypes.c_uint32(0)
        self._chk(self.L.pn_rate_get_cng_seed(self.h, ctypes.byref(v)))
        return int(v.value)

    def set_stream_sid(self, ids, sids):
        """The SIDs of streams `ids`: uint8 [n][CNG_SID_BYTES] rows of (M, L, N_1..N_12) (pn_rate_set_stream_sid); a setting ordered
        like set_stream_laws, valid with comfort noise off.  All or nothing."""
        a, n = self._ids(ids)
        w = np.ascontiguousarray(np.asarray(sids, dtype=np.uint8).reshape(-1, CNG_SID_BYTES))
        if w.shape[0] != n:
            raise PercepNetError(f"{w.shape[0]} SIDs for {n} streams")
        self._chk(self.L.pn_rate_set_stream_sid(self.h, a.ctypes.data if a is not None else None, n, w.ctypes.data, CNG_SID_BYTES))

    def stream_sids(self):
        """-> uint8 [n_streams][CNG_SID_BYTES]: the SIDs as last set (pn_rate_get_stream_sid); the default everywhere on a new converter."""
        w = np.empty((self.n_streams, CNG_SID_BYTES), np.uint8)
        self._chk(self.L.pn_rate_get_stream_sid(self.h, w.ctypes.data))
        return w

    def set_silent(self, ids):
        """Streams `ids` are silent in the NEXT frame submitted on this converter, and only in that one (pn_rate_set_silent): their rows
        are comfort noise, their input rows are not read; calls before one frame add up.  Refused while comfort noise is off."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_set_silent(self.h, a.ctypes.data if a is not None else None, n))

    def cng_f32_dev(self, d_x48, ids=None):
        """Comfort noise on its own: the listed streams' rows generated and up-converted into device rows [n_streams][480] float
        (pn_rate_cng_f32); other rows are not touched."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_cng_f32(self.h, d_x48, a.ctypes.data if a is not None else None, n))

    def set_cng_report(self, on):
        self._chk(self.L.pn_rate_set_cng_report(self.h, 1 if on else 0))

    def read_cng_report(self):
        """-> CNG_REPORT_DTYPE [n_streams]: a stream's record is of its last generated row (pn_rate_read_cng_report, synchronising)."""
        rep = np.empty(self.n_streams, CNG_REPORT_DTYPE)
        self._chk(self.L.pn_rate_read_cng_report(self.h, rep.ctypes.data))
        return rep

    def read_cng_report_dev(self, d_report):
        """The same into device memory [n_streams][4] words, asynchronous on the context's stream (pn_rate_read_cng_report_dev)."""
        self._chk(self.L.pn_rate_read_cng_report_dev(self.h, d_report))

    def debug_cng_state(self):
        """-> uint32 [n_streams][16]: b[12], counter, prev, run, total (tests; synchronising)."""
        st = np.empty((self.n_streams, 16), np.uint32)
        self._chk(self.L.pn_rate_debug_cng_state(self.h, st.ctypes.data))
        return st

    # automatic level control: a levelled stream's enhanced 48 kHz row is brought towards its target RMS, between the engine and the mix
    def set_agc(self, on):
        """Automatic level control on or off (pn_rate_set_agc); the first enable allocates the per-stream state and targets."""
        self._chk(self.L.pn_rate_set_agc(self.h, 1 if on else 0))

    def set_agc_params(self, params):
        """The converter's AGC_N_PARAMS parameters from the next frame on (pn_rate_set_agc_params); refused as a whole, naming the
        first that is NaN or outside its range."""
        self._chk(self.L.pn_rate_set_agc_params(self.h, _agc_params(params).ctypes.data))

    def agc_params(self):
        """-> float32 [AGC_N_PARAMS] as last set (pn_rate_get_agc_params); agc_default_params() on a new converter."""
        p = np.empty(AGC_N_PARAMS, np.float32)
        self._chk(self.L.pn_rate_get_agc_params(self.h, p.ctypes.data))
        return p

    def set_stream_agc_targets(self, ids, targets):
        """Streams `ids` are levelled towards the RMS `targets` (in (0, 1]; 0 = not levelled) from the next frame on
        (pn_rate_set_stream_agc_targets): asynchronous, ordered like set_stream_mix_gains; the state stays.  Refused while AGC is off."""
        a, n = self._ids(ids)
        w = np.ascontiguousarray(np.asarray(targets, dtype=np.float32).ravel())
        if w.size != n:
            raise PercepNetError(f"{w.size} targets for {n} streams")
        self._chk(self.L.pn_rate_set_stream_agc_targets(self.h, a.ctypes.data, n, w.ctypes.data))

    def stream_agc_targets(self):
        """-> float32 [n_streams]: the targets as last set (pn_rate_get_stream_agc_targets); 0 everywhere on a new converter."""
        w = np.empty(self.n_streams, np.float32)
        self._chk(self.L.pn_rate_get_stream_agc_targets(self.h, w.ctypes.data))
        return w

    def agc_f32_dev(self, d_y48, ids=None):
        """The level control on its own, in place on device rows [n_streams][480] float (pn_rate_agc_f32); nobody counts as concealed."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_agc_f32(self.h, d_y48, a.ctypes.data if a is not None else None, n))

    def set_agc_report(self, on):
        self._chk(self.L.pn_rate_set_agc_report(self.h, 1 if on else 0))

    def read_agc_report(self):
        """-> AGC_REPORT_DTYPE [n_streams]: the records of the last frame that ran the level control (pn_rate_read_agc_report, synchronising)."""
        rep = np.empty(self.n_streams, AGC_REPORT_DTYPE)
        self._chk(self.L.pn_rate_read_agc_report(self.h, rep.ctypes.data))
        return rep

    def read_agc_report_dev(self, d_report):
        """The same into device memory [n_streams][4] words, asynchronous on the context's stream (pn_rate_read_agc_report_dev)."""
        self._chk(self.L.pn_rate_read_agc_report_dev(self.h, d_report))

    # the output limiter: a per-stream gain as the last stage in front of the down-conversion keeps a limited stream's output under its ceiling
    def set_stream_limiter(self, ids, ceilings):
        """Streams `ids` are limited to the `ceilings` (in [1/1024, 1]; 0 = not limited) from the next frame on
        (pn_rate_set_stream_limiter): asynchronous, ordered like set_stream_agc_targets; the state stays."""
        a, n = self._ids(ids)
        w = np.ascontiguousarray(np.asarray(ceilings, dtype=np.float32).ravel())
        if w.size != n:
            raise PercepNetError(f"{w.size} ceilings for {n} streams")
        self._chk(self.L.pn_rate_set_stream_limiter(self.h, a.ctypes.data, n, w.ctypes.data))

    def stream_limiter(self):
        """-> float32 [n_streams]: the ceilings as last set (pn_rate_get_stream_limiter); 0 everywhere on a new converter."""
        w = np.empty(self.n_streams, np.float32)
        self._chk(self.L.pn_rate_get_stream_limiter(self.h, w.ctypes.data))
        return w

    def set_limiter_params(self, params):
        """The converter's LIM_N_PARAMS parameters from the next frame on (pn_rate_set_limiter_params); refused as a whole, naming the
        first that is NaN or outside its range."""
        self._chk(self.L.pn_rate_set_limiter_params(self.h, _lim_params(params).ctypes.data))

    def limiter_params(self):
        """-> float32 [LIM_N_PARAMS] as last set (pn_rate_get_limiter_params); lim_default_params() on a new converter."""
        p = np.empty(LIM_N_PARAMS, np.float32)
        self._chk(self.L.pn_rate_get_limiter_params(self.h, p.ctypes.data))
        return p

    def lim_f32_dev(self, d_o48, ids=None):
        """The output limiter on its own, in place on device rows [n_streams][480] float (pn_rate_lim_f32)."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_lim_f32(self.h, d_o48, a.ctypes.data if a is not None else None, n))

    def set_limiter_report(self, on):
        self._chk(self.L.pn_rate_set_limiter_report(self.h, 1 if on else 0))

    def read_limiter_report(self):
        """-> LIM_REPORT_DTYPE [n_streams]: the records of the last frame that ran the limiter (pn_rate_read_limiter_report, synchronising)."""
        rep = np.empty(self.n_streams, LIM_REPORT_DTYPE)
        self._chk(self.L.pn_rate_read_limiter_report(self.h, rep.ctypes.data))
        return rep

    def read_limiter_report_dev(self, d_report):
        """The same into device memory [n_streams][4] words, asynchronous on the context's stream (pn_rate_read_limiter_report_dev)."""
        self._chk(self.L.pn_rate_read_limiter_report_dev(self.h, d_report))

    # one whole frame, device pointers: [n_streams][frame] in and out at the low rate, d_gr [n_streams][68] or None
    def process_f32_dev(self, d_in, d_out, d_gr=None, ids=None):
        if ids is None:
            self._chk(self.L.pn_rate_process_f32(self.h, d_in, d_out, d_gr))
        else:
            a, n = self._ids(ids)
            self._chk(self.L.pn_rate_process_f32_active(self.h, d_in, d_out, d_gr, a.ctypes.data, n))

    def process_i16_dev(self, d_in, d_out, d_gr=None, ids=None):
        if ids is None:
            self._chk(self.L.pn_rate_process_i16(self.h, d_in, d_out, d_gr))
        else:
            a, n = self._ids(ids)
            self._chk(self.L.pn_rate_process_i16_active(self.h, d_in, d_out, d_gr, a.ctypes.data, n))

    # host numpy entry points (synchronous)
    def _host(self, name, frame, dtype, want_gr):
        frame = np.ascontiguousarray(frame, dtype=dtype).reshape(self.n_streams, self.frame)
        out = np.empty_like(frame)
        gr = np.empty((self.n_streams, 68), np.float32) if want_gr else None
        self._chk(getattr(self.L, name)(self.h, frame.ctypes.data, out.ctypes.data, gr.ctypes.data if want_gr else None))
        return out, gr

    def process_f32(self, frame, want_gr=True):
        return self._host("pn_rate_process_host_f32", frame, np.float32, want_gr)

    def process_i16(self, frame, want_gr=True):
        return self._host("pn_rate_process_host_i16", frame, np.int16, want_gr)

    def run_pcm(self, pcm):
        """percepnet_run --rate semantics for a batch: pcm int16 [B, n_frames * frame] -> out int16 [B, (n_frames - 1) * frame]
        (the first output frame dropped, like Context.run_pcm)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n_streams, -1)
        f, n = self.frame, pcm.shape[1] // self.frame
        out = np.zeros((self.n_streams, max(n - 1, 0) * f), np.int16)
        for t in range(n):
            o, _ = self.process_i16(pcm[:, t * f:(t + 1) * f], want_gr=False)
            if t > 0:
                out[:, (t - 1) * f:t * f] = o
        return out

    # pipelined host-buffer entry points: a converter's frame through the CONTEXT's pipeline (raw host pointers to rows of
    # [n_streams][frame]; the buffers should be pinned and must outlive delivery: Context.host_wait / frames_delivered).
    # h_report: this frame's 48 kHz report records (pn_host_next_report); ids: only those streams advance.  On a mixed converter
    # the part of an output row behind a stream's own samples is unspecified.
    def _submit(self, kind, h_in, h_out, h_gr, h_report, ids):
        if h_report is not None:
            self._chk(self.L.pn_host_next_report(self.ctx.h, h_report))
        if ids is None:
            self._chk(getattr(self.L, f"pn_rate_submit_host_{kind}")(self.h, h_in, h_out, h_gr))
        else:
            a, n = self._ids(ids)
            self._chk(getattr(self.L, f"pn_rate_submit_host_{kind}_active")(self.h, h_in, h_out, h_gr, a.ctypes.data, n))

    def submit_host_i16(self, h_in, h_out, h_gr=None, h_report=None, ids=None):
        self._submit("i16", h_in, h_out, h_gr, h_report, ids)

    def submit_host_f32(self, h_in, h_out, h_gr=None, h_report=None, ids=None):
        self._submit("f32", h_in, h_out, h_gr, h_report, ids)

    def host_pipeline_prepare(self):
        """The converter's second staging pair and the context's pipeline, now instead of inside the first submit."""
        self._chk(self.L.pn_rate_host_pipeline_prepare(self.h))

    # device-side records (async on the context's stream): records record_stride() bytes apart at a 16-byte aligned address
    def record_stride(self):
        """Bytes between two device-side records: state_bytes of the rate, or rate_state_max_bytes() on a mixed converter."""
        return int(self.L.pn_rate_record_stride(self.h))

    def export_streams_dev(self, ids, d_records):
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_export_streams(self.h, a.ctypes.data, n, d_records))

    def import_streams_dev(self, ids, d_records, d_status):
        """d_status (device int32 [n]) receives SS_OK or the SS_BAD_* verdict of each record against its slot's rate."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_import_streams(self.h, a.ctypes.data, n, d_records, d_status))

    # DTMF detection: an enabled stream's 48 kHz row is read behind the concealer and in front of the engine; the audio is untouched
    def set_stream_dtmf(self, ids, on):
        """Detection on or off for the streams `ids` from the next frame on (pn_rate_set_stream_dtmf): asynchronous, ordered like
        set_stream_limiter.  `on`: one value for all of them or one per id.  A stream that was off starts from the fresh state."""
        a, n = self._ids(ids)
        w = np.asarray(on).astype(bool).astype(np.uint8).ravel()
        if w.size == 1:
            w = np.repeat(w, n)
        if w.size != n:
            raise PercepNetError(f"{w.size} switches for {n} streams")
        w = np.ascontiguousarray(w)
        self._chk(self.L.pn_rate_set_stream_dtmf(self.h, a.ctypes.data, n, w.ctypes.data))

    def stream_dtmf(self):
        """-> uint8 [n_streams]: the switches as last set (pn_rate_get_stream_dtmf); 0 everywhere on a new converter."""
        w = np.empty(self.n_streams, np.uint8)
        self._chk(self.L.pn_rate_get_stream_dtmf(self.h, w.ctypes.data))
        return w

    def set_dtmf_params(self, params):
        """The converter's DTMF_N_PARAMS parameters from the next frame on (pn_rate_set_dtmf_params); refused as a whole, naming the
        first bad one."""
        self._chk(self.L.pn_rate_set_dtmf_params(self.h, _dtmf_params(params).ctypes.data))

    def dtmf_params(self):
        """-> float32 [DTMF_N_PARAMS] as last set (pn_rate_get_dtmf_params); dtmf_default_params() on a new converter."""
        p = np.empty(DTMF_N_PARAMS, np.float32)
        self._chk(self.L.pn_rate_get_dtmf_params(self.h, p.ctypes.data))
        return p

    def dtmf_f32_dev(self, d_x48, ids=None):
        """The detector on its own over device rows [n_streams][480] float, which it only reads (pn_rate_dtmf_f32); nobody counts as concealed."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_dtmf_f32(self.h, d_x48, a.ctypes.data if a is not None else None, n))

    def set_dtmf_report(self, on):
        self._chk(self.L.pn_rate_set_dtmf_report(self.h, 1 if on else 0))

    def read_dtmf_report(self):
        """-> DTMF_REPORT_DTYPE [n_streams]: the records of the last frame that ran the detector (pn_rate_read_dtmf_report, synchronising)."""
        rep = np.empty(self.n_streams, DTMF_REPORT_DTYPE)
        self._chk(self.L.pn_rate_read_dtmf_report(self.h, rep.ctypes.data))
        return rep

    def dtmf_state(self):
        """-> uint32 [n_streams, DTMF_STATE_WORDS]: the detector's state words (pn_rate_debug_dtmf_state, synchronising): for tests."""
        st = np.empty((self.n_streams, DTMF_STATE_WORDS), np.uint32)
        self._chk(self.L.pn_rate_debug_dtmf_state(self.h, st.ctypes.data))
        return st

    def read_dtmf_report_dev(self, d_report):
        """The same into device memory [n_streams][4] words, asynchronous on the context's stream (pn_rate_read_dtmf_report_dev)."""
        self._chk(self.L.pn_rate_read_dtmf_report_dev(self.h, d_report))

    # the DTX send side: an enabled stream's OUTPUT row is read behind the down-conversion; the audio is untouched
    def set_stream_dtx(self, ids, on):
        """The DTX send side on or off for the streams `ids` from the next frame on (pn_rate_set_stream_dtx): asynchronous, ordered like
        set_stream_dtmf.  `on`: one value for all of them or one per id.  A stream that was off starts from the fresh state."""
        a, n = self._ids(ids)
        w = np.asarray(on).astype(bool).astype(np.uint8).ravel()
        if w.size == 1:
            w = np.repeat(w, n)
        if w.size != n:
            raise PercepNetError(f"{w.size} switches for {n} streams")
        w = np.ascontiguousarray(w)
        self._chk(self.L.pn_rate_set_stream_dtx(self.h, a.ctypes.data, n, w.ctypes.data))

    def stream_dtx(self):
        """-> uint8 [n_streams]: the switches as last set (pn_rate_get_stream_dtx); 0 everywhere on a new converter."""
        w = np.empty(self.n_streams, np.uint8)
        self._chk(self.L.pn_rate_get_stream_dtx(self.h, w.ctypes.data))
        return w

    def set_dtx_params(self, params):
        """The converter's DTX_N_PARAMS parameters from the next frame on (pn_rate_set_dtx_params); refused as a whole, naming the
        first bad one."""
        self._chk(self.L.pn_rate_set_dtx_params(self.h, _dtx_params(params).ctypes.data))

    def dtx_params(self):
        """-> float32 [DTX_N_PARAMS] as last set (pn_rate_get_dtx_params); dtx_default_params() on a new converter."""
        p = np.empty(DTX_N_PARAMS, np.float32)
        self._chk(self.L.pn_rate_get_dtx_params(self.h, p.ctypes.data))
        return p

    def dtx_dev(self, d_out_rows, fmt="f32", ids=None):
        """The stage on its own over device OUTPUT rows [n_streams][row_samples] of format "f32", "i16" or "g711", which it only reads
        (pn_rate_dtx_f32 / _i16 / _g711)."""
        a, n = self._ids(ids)
        self._chk(getattr(self.L, "pn_rate_dtx_" + fmt)(self.h, d_out_rows, a.ctypes.data if a is not None else None, n))

    def set_dtx_report(self, on):
        self._chk(self.L.pn_rate_set_dtx_report(self.h, 1 if on else 0))

    def read_dtx_report(self):
        """-> DTX_REPORT_DTYPE [n_streams]: a stream's record is of the last launch that had it on its list (pn_rate_read_dtx_report,
        synchronising)."""
        rep = np.empty(self.n_streams, DTX_REPORT_DTYPE)
        self._chk(self.L.pn_rate_read_dtx_report(self.h, rep.ctypes.data))
        return rep

    def read_dtx_report_dev(self, d_report):
        """The same into device memory [n_streams][8] words, asynchronous on the context's stream (pn_rate_read_dtx_report_dev)."""
        self._chk(self.L.pn_rate_read_dtx_report_dev(self.h, d_report))

    def dtx_state(self):
        """-> uint32 [n_streams, DTX_STATE_WORDS]: the stage's state words (pn_rate_debug_dtx_state, synchronising): for tests."""
        st = np.empty((self.n_streams, DTX_STATE_WORDS), np.uint32)
        self._chk(self.L.pn_rate_debug_dtx_state(self.h, st.ctypes.data))
        return st

    # DTMF removal: a detected digit is muted in the stream's enhanced 48 kHz row, behind the engine and in front of the level control
    def set_stream_dtmf_clamp(self, ids, on):
        """Removal on or off for the streams `ids` from the next frame on (pn_rate_set_stream_dtmf_clamp): asynchronous, ordered like
        set_stream_dtmf.  `on`: one value for all of them or one per id.  A stream that was off starts from the fresh state.  Refused
        while the detector's on_frames + pre > 5.  It acts on streams whose detection is on too."""
        a, n = self._ids(ids)
        w = np.asarray(on).astype(bool).astype(np.uint8).ravel()
        if w.size == 1:
            w = np.repeat(w, n)
        if w.size != n:
            raise PercepNetError(f"{w.size} switches for {n} streams")
        w = np.ascontiguousarray(w)
        self._chk(self.L.pn_rate_set_stream_dtmf_clamp(self.h, a.ctypes.data, n, w.ctypes.data))

    def stream_dtmf_clamp(self):
        """-> uint8 [n_streams]: the switches as last set (pn_rate_get_stream_dtmf_clamp); 0 everywhere on a new converter."""
        w = np.empty(self.n_streams, np.uint8)
        self._chk(self.L.pn_rate_get_stream_dtmf_clamp(self.h, w.ctypes.data))
        return w

    def set_dtmf_clamp_params(self, params):
        """The converter's DTMF_CLAMP_N_PARAMS parameters from the next frame on (pn_rate_set_dtmf_clamp_params); refused as a whole,
        naming the first bad one or the two values that are not in time."""
        self._chk(self.L.pn_rate_set_dtmf_clamp_params(self.h, _dtmf_clamp_params(params).ctypes.data))

    def dtmf_clamp_params(self):
        """-> int32 [DTMF_CLAMP_N_PARAMS] as last set (pn_rate_get_dtmf_clamp_params); dtmf_clamp_default_params() on a new converter."""
        p = np.empty(DTMF_CLAMP_N_PARAMS, np.int32)
        self._chk(self.L.pn_rate_get_dtmf_clamp_params(self.h, p.ctypes.data))
        return p

    def dtmf_clamp_f32_dev(self, d_y48, ids=None):
        """The removal stage on its own over device rows [n_streams][480] float, in place (pn_rate_dtmf_clamp_f32); it reads the
        detector's report rows as the last detector launch, or set_dtmf_report_rows, left them."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_dtmf_clamp_f32(self.h, d_y48, a.ctypes.data if a is not None else None, n))

    def set_dtmf_clamp_report(self, on):
        self._chk(self.L.pn_rate_set_dtmf_clamp_report(self.h, 1 if on else 0))

    def read_dtmf_clamp_report(self):
        """-> DTMF_CLAMP_REPORT_DTYPE [n_streams]: the records of the last frame that ran the stage (pn_rate_read_dtmf_clamp_report,
        synchronising).  The events are about the input: DTMF_CLAMP_DELAY frames ahead of the audio they describe."""
        rep = np.empty(self.n_streams, DTMF_CLAMP_REPORT_DTYPE)
        self._chk(self.L.pn_rate_read_dtmf_clamp_report(self.h, rep.ctypes.data))
        return rep

    def read_dtmf_clamp_report_dev(self, d_report):
        """The same into device memory [n_streams][4] words, asynchronous on the context's stream (pn_rate_read_dtmf_clamp_report_dev)."""
        self._chk(self.L.pn_rate_read_dtmf_clamp_report_dev(self.h, d_report))

    def dtmf_clamp_state(self):
        """-> uint32 [n_streams, DTMF_CLAMP_STATE_WORDS]: the removal state words (pn_rate_debug_dtmf_clamp_state, synchronising): for tests."""
        st = np.empty((self.n_streams, DTMF_CLAMP_STATE_WORDS), np.uint32)
        self._chk(self.L.pn_rate_debug_dtmf_clamp_state(self.h, st.ctypes.data))
        return st

    def set_dtmf_report_rows(self, rows):
        """TESTS ONLY: uint32 [n_streams, 4] overwrite the detector's report rows — the buffer read_dtmf_report reads too — so that
        dtmf_clamp_f32_dev can run over hand-made rows (pn_rate_debug_set_dtmf_report, synchronising; it allocates what removal
        needs).  The next detector launch overwrites them again."""
        w = np.ascontiguousarray(rows, dtype=np.uint32)
        if w.size != self.n_streams * DTMF_REPORT_WORDS:
            raise PercepNetError(f"{w.size} words: the detector's report has {self.n_streams * DTMF_REPORT_WORDS}")
        self._chk(self.L.pn_rate_debug_set_dtmf_report(self.h, w.ctypes.data))

    # call-state records (include/percepnet_hip.h "call-state records"): the PLC, AGC, limiter and level state, one size for every
    # rate; imported BEHIND import_streams, which zeroes those states.  Defined here once: a mixed converter uses them unchanged
    def call_state_sections(self):
        """-> the CALL_* mask of the states this converter holds (pn_rate_call_state_sections)."""
        m = int(self.L.pn_rate_call_state_sections(self.h))
        if m < 0:
            raise PercepNetError(_err(self.L))
        return m

    def export_call_state_dev(self, ids, d_records):
        """Records RATE_CALL_STATE_BYTES apart at a 16-byte aligned device address, asynchronous (pn_rate_export_call_state)."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_export_call_state(self.h, a.ctypes.data, n, d_records))

    def import_call_state_dev(self, ids, d_records, d_status):
        """d_status (device int32 [n]) receives SS_OK or the SS_BAD_* verdict of each record; a refused record leaves its stream
        as it was, the others are imported (pn_rate_import_call_state)."""
        a, n = self._ids(ids)
        self._chk(self.L.pn_rate_import_call_state(self.h, a.ctypes.data, n, d_records, d_status))

    def export_call_state(self, ids):
        """-> uint8 [n, RATE_CALL_STATE_BYTES]: the call state of the streams `ids` (pn_rate_export_call_state_host)."""
        a, n = self._ids(ids)
        rec = np.empty((n, RATE_CALL_STATE_BYTES), np.uint8)
        self._chk(self.L.pn_rate_export_call_state_host(self.h, a.ctypes.data, n, rec.ctypes.data))
        return rec

    def import_call_state(self, ids, records):
        """Records from export_call_state of any converter into the distinct streams `ids`; every record is checked first, all
        or nothing (pn_rate_import_call_state_host)."""
        a, n = self._ids(ids)
        rec = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
        if rec.size != n * RATE_CALL_STATE_BYTES:
            raise PercepNetError(f"{rec.size} record bytes for {n} streams (a call-state record has {RATE_CALL_STATE_BYTES})")
        self._chk(self.L.pn_rate_import_call_state_host(self.h, a.ctypes.data, n, rec.ctypes.data))

    # timing of the two kernels inside a frame (HIP events owned by the converter; off by default)
    def set_profiling(self, on):
        self._chk(self.L.pn_rate_set_profiling(self.h, 1 if on else 0))

    def reset_profile(self):
        self._chk(self.L.pn_rate_reset_profile(self.h))

    def kernel_times(self, names=("rate_up", "rate_down")):
        """-> {"rate_up": (total_ms, launches), "rate_down": (...)}; names: which kernels ("rate_mix" is the conference mix,
        "rate_plc" the packet-loss concealer, "rate_agc" the level control, "rate_lim" the output limiter, "rate_dtmf" the DTMF detector,
        "rate_clamp" DTMF removal, "rate_cng" comfort noise, "rate_dtx" the DTX send side)"""
        out = {}
        for name in names:
            ms = ctypes.c_double()
            n = ctypes.c_int64()
            self._chk(self.L.pn_rate_kernel_time(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def export_streams(self, ids):
        """-> uint8 [n, state_bytes]: the converter's state of the streams `ids` (pn_rate_export_streams_host)."""
        a, n = self._ids(ids)
        rec = np.empty((n, self.state_bytes), np.uint8)
        self._chk(self.L.pn_rate_export_streams_host(self.h, a.ctypes.data, n, rec.ctypes.data))
        return rec

    def import_streams(self, ids, records):
        """Records from export_streams of a converter of the same rate into the distinct streams `ids`; all or nothing."""
        a, n = self._ids(ids)
        rec = np.ascontiguousarray(records, dtype=np.uint8)
        if rec.size != n * self.state_bytes:
            raise PercepNetError(f"{rec.size} record bytes for {n} streams (a record at {self.rate} Hz has {self.state_bytes})")
        self._chk(self.L.pn_rate_import_streams_host(self.h, a.ctypes.data, n, rec.ctypes.data))


class MixedRateConverter(RateConverter):
    """8, 16, 24, 32 and 48 kHz streams in ONE Context (pn_rate_create_mixed): a RateConverter with a rate per stream.  Every method
    of RateConverter works on rows of RATE_MIXED_ROW = 480 samples, of which stream s uses the first rate_mixed_frame_samples(its
    rate); the rest of an input row is ignored and the rest of an output row is left as it was (the host entry points return it
    as zeros).  rates: one per stream, or None for all 48000."""

    def __init__(self, ctx, rates=None):
        self.L = ctx.L
        self.ctx = ctx
        self.rate = None
        self.n_streams = ctx.n_streams
        a = None if rates is None else np.ascontiguousarray(np.asarray(rates, dtype=np.int32).ravel())
        if a is not None and a.size != self.n_streams:
            raise PercepNetError(f"{a.size} rates for {self.n_streams} streams")
        self.h = self.L.pn_rate_create_mixed(ctx.h, a.ctypes.data if a is not None else None)
        if not self.h:
            raise PercepNetError(_err(self.L))
        self.frame = int(self.L.pn_rate_row_samples(self.h))

    def set_stream_rates(self, ids, rates):
        """Streams `ids` continue at `rates` from the next frame on, with zeroed converter tails (pn_rate_set_stream_rates):
        asynchronous, ordered like reset_streams.  A slot that starts a new call also needs Context.reset_streams."""
        a, n = self._ids(ids)
        r = np.ascontiguousarray(np.asarray(rates, dtype=np.int32).ravel())
        if r.size != n:
            raise PercepNetError(f"{r.size} rates for {n} streams")
        self._chk(self.L.pn_rate_set_stream_rates(self.h, a.ctypes.data, n, r.ctypes.data))

    def stream_rates(self):
        """-> int32 [n_streams]: the rates as last set (pn_rate_get_stream_rates)."""
        r = np.empty(self.n_streams, np.int32)
        self._chk(self.L.pn_rate_get_stream_rates(self.h, r.ctypes.data))
        return r

    def _host(self, name, frame, dtype, want_gr):
        frame = np.ascontiguousarray(frame, dtype=dtype).reshape(self.n_streams, self.frame)
        out = np.zeros_like(frame)
        gr = np.empty((self.n_streams, 68), np.float32) if want_gr else None
        self._chk(getattr(self.L, name)(self.h, frame.ctypes.data, out.ctypes.data, gr.ctypes.data if want_gr else None))
        return out, gr

    def run_pcm(self, pcm):
        """percepnet_run --rates semantics: pcm = one int16 array per stream at that stream's rate -> a list of int16 arrays,
        stream s with (frames_s - 1) * n_s samples (first output frame and partial tail dropped).  Streams may differ in length:
        one that has ended is fed silence."""
        if len(pcm) != self.n_streams:
            raise PercepNetError(f"{len(pcm)} arrays for {self.n_streams} streams")
        pcm = [np.ascontiguousarray(p, dtype=np.int16).ravel() for p in pcm]
        ns = [rate_mixed_frame_samples(r) for r in self.stream_rates()]
        frames = [p.size // n for p, n in zip(pcm, ns)]
        out = [np.zeros(max(f - 1, 0) * n, np.int16) for f, n in zip(frames, ns)]
        row = np.zeros((self.n_streams, self.frame), np.int16)
        for t in range(max(frames, default=0)):
            row[:] = 0
            for s, (p, n) in enumerate(zip(pcm, ns)):
                if t < frames[s]:
                    row[s, :n] = p[t * n:(t + 1) * n]
            o, _ = self.process_i16(row, want_gr=False)
            for s, n in enumerate(ns):
                if 0 < t < frames[s]:
                    out[s][(t - 1) * n:t * n] = o[s, :n]
        return out

    def run_g711(self, codes):
        """percepnet_run --rates .. --g711 semantics: codes = one uint8 array per stream at that stream's rate and under its law
        -> a list of uint8 arrays, like run_pcm.  A stream that has ended is fed silence."""
        if len(codes) != self.n_streams:
            raise PercepNetError(f"{len(codes)} arrays for {self.n_streams} streams")
        codes = [np.ascontiguousarray(p, dtype=np.uint8).ravel() for p in codes]
        ns = [rate_mixed_frame_samples(r) for r in self.stream_rates()]
        idle = [0xD5 if w == G711_ALAW else 0xFF for w in self.stream_laws()]
        frames = [p.size // n for p, n in zip(codes, ns)]
        out = [np.zeros(max(f - 1, 0) * n, np.uint8) for f, n in zip(frames, ns)]
        row = np.zeros((self.n_streams, self.frame), np.uint8)
        for t in range(max(frames, default=0)):
            for s, (p, n) in enumerate(zip(codes, ns)):
                row[s] = idle[s]
                if t < frames[s]:
                    row[s, :n] = p[t * n:(t + 1) * n]
            o, _ = self.process_g711(row, want_gr=False)
            for s, n in enumerate(ns):
                if 0 < t < frames[s]:
                    out[s][(t - 1) * n:t * n] = o[s, :n]
        return out

    def _record_rate(self, ids):
        a, n = self._ids(ids)
        rates = self.stream_rates()
        ok = n > 0 and a.min() >= 0 and a.max() < self.n_streams
        return a, n, (int(rates[a[0]]) if ok else 0)

    def export_streams(self, ids):
        """-> uint8 [n, rate_state_bytes(R)]: the converter state of the streams `ids`, which share the rate R != 48000."""
        a, n, rate = self._record_rate(ids)
        rec = np.empty((n, rate_state_bytes(rate) if rate in RATES_ALL else 16), np.uint8)
        self._chk(self.L.pn_rate_export_streams_host(self.h, a.ctypes.data, n, rec.ctypes.data))
        return rec

    def import_streams(self, ids, records):
        """Records of rate R into the distinct streams `ids`, all of which run at R now (set_stream_rates first); all or nothing."""
        a, n, rate = self._record_rate(ids)
        rec = np.ascontiguousarray(records, dtype=np.uint8)
        want = rate_state_bytes(rate) if rate in RATES_ALL else 0
        if n and want and rec.size != n * want:
            raise PercepNetError(f"{rec.size} record bytes for {n} streams (a record at {rate} Hz has {want})")
        if n and not want:                     # (a 48000 slot or a bad id: the library words the refusal; it reads no record)
            rec = np.zeros(16, np.uint8)
        self._chk(self.L.pn_rate_import_streams_host(self.h, a.ctypes.data, n, rec.ctypes.data))


class FeatGen:
    """Batched training-feature generator (pn_featgen): the reference's `percepNet <speech> <noisy>
    <count> <output>` binary (train(), denoise.cpp:603-787) for n_pairs pairs in lock-step."""

    def __init__(self, n_pairs, device=0, stream=None):
        self.L = load_library()
        self.n_pairs = int(n_pairs)
        self.h = self.L.pn_featgen_create(device, self.n_pairs, stream)
        if not self.h:
            raise PercepNetError(_err(self.L))

    def close(self):
        if self.h:
            self.L.pn_featgen_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise PercepNetError(_err(self.L))

    def reset(self):
        self._chk(self.L.pn_featgen_reset(self.h))

    def synchronize(self):
        self._chk(self.L.pn_featgen_synchronize(self.h))

    def device_bytes(self):
        return self.L.pn_featgen_device_bytes(self.h)

    def process_dev(self, d_speech, d_noisy, d_records, d_test_pcm=None):
        """One frame; device pointers (ints): [n_pairs][480] i16 x2 -> [n_pairs][138] f32 (+ [n_pairs][480] i16)."""
        self._chk(self.L.pn_featgen_process_i16(self.h, d_speech, d_noisy, d_records, d_test_pcm))

    def process_files_dev(self, d_speech, d_noisy, n_frames, d_records, d_test_pcm=None):
        self._chk(self.L.pn_featgen_process_i16_files(self.h, d_speech, d_noisy, n_frames, d_records, d_test_pcm))

    def run(self, speech, noisy, want_test_pcm=True):
        """speech, noisy: int16 [n_pairs, n_frames*480] -> (records [n_pairs, n_frames, 138] f32,
        test_output [n_pairs, n_frames, 480] i16 or None).  Continues from the current state."""
        speech = np.ascontiguousarray(speech, dtype=np.int16).reshape(self.n_pairs, -1)
        noisy = np.ascontiguousarray(noisy, dtype=np.int16).reshape(self.n_pairs, -1)
        n = min(speech.shape[1], noisy.shape[1]) // 480
        speech = np.ascontiguousarray(speech[:, :n * 480]); noisy = np.ascontiguousarray(noisy[:, :n * 480])
        rec = np.empty((self.n_pairs, n, 138), np.float32)
        pcm = np.empty((self.n_pairs, n, 480), np.int16) if want_test_pcm else None
        self._chk(self.L.pn_featgen_process_host_i16_files(self.h, speech.ctypes.data, noisy.ctypes.data, n,
                                                           rec.ctypes.data, pcm.ctypes.data if want_test_pcm else None))
        return rec, pcm


def featgen_run_files(jobs, device=0, test_pcm=False):
    """jobs: [(speech_path, noisy_path, count, output_path), ...] — pn_featgen_run_files."""
    L = load_library()
    n = len(jobs)
    arr = lambda xs: (ctypes.c_char_p * n)(*[x.encode() if x is not None else None for x in xs])
    sp, no, out = arr([j[0] for j in jobs]), arr([j[1] for j in jobs]), arr([j[3] for j in jobs])
    cnt = (ctypes.c_int * n)(*[int(j[2]) for j in jobs])
    to = arr([j[3] + ".test_output.pcm" for j in jobs]) if test_pcm else None
    ti = arr([j[3] + ".test_input.pcm" for j in jobs]) if test_pcm else None
    if L.pn_featgen_run_files(device, n, sp, no, cnt, out, to, ti) != 0:
        raise PercepNetError(_err(L))
