"""numpy model of the output stage (percepnet_amd/csrc/pn_outstage.hip; include/percepnet_hip.h pn_ctx_set_report and
pn_ctx_set_output_saturate), imported as `from tests import report_model`: the two int16 casts of t = o * 32768 and the clip
count, pinned to hand-worked values by tests/test_report_host.py, and the report a stream must show for given float outputs."""
import numpy as np

from percepnet_amd import api
from tests import backend_model as bm

F32 = np.float32
DELAY_FRAMES = 6          # the engine's input-to-output delay: 2880 samples


def cast_t(t, saturate):
    """t (fp32, already o * 32768) -> int16: the CLI's wrap (truncate, low 16 bits), or the saturating cast
    (t >= 32768 -> 32767, t <= -32769 -> -32768, NaN -> 0, else trunc)."""
    t = np.asarray(t, F32)
    if not saturate:
        return bm.f2s(t)
    inner = np.trunc(np.where(np.isnan(t), F32(0), t))
    out = np.where(t >= F32(32768), F32(32767), np.where(t <= F32(-32769), F32(-32768), inner))
    return out.astype(np.int16)


def clipped_t(t):
    """Which t lie outside the open interval (-32769, 32768); NaN counts."""
    t = np.asarray(t, F32)
    return ~((t > F32(-32769)) & (t < F32(32768)))


def cast(o, saturate):
    return cast_t(np.asarray(o, F32) * F32(32768), saturate)


def count_clipped(o):
    """Float outputs [..., 480] -> out_clipped [...]"""
    return clipped_t(np.asarray(o, F32) * F32(32768)).sum(axis=-1).astype(np.int32)


def check_report(rep, o, gr, silence, period, x_in, where=""):
    """One frame's records `rep` (REPORT_DTYPE [n]) against the float outputs o [n, 480], the g|r tap [n, 68], the silence
    flags and pitch periods [n] of a plain context, and the aligned input frame x_in (int16 [n, 480]; zeros before a stream's
    seventh frame).  Exact words are compared exactly; the two energies within a relative 3e-5 of the float64 sum — any fp32
    summation order of 480 non-negative products is within gamma_481 * 2^-24 ~ 2.9e-5 — and gain_mean within 3e-6 (gamma_34)."""
    assert rep.dtype == api.REPORT_DTYPE
    o = np.asarray(o, F32)
    x = np.asarray(x_in, np.int16).astype(F32) / F32(32768)
    assert np.array_equal(rep["in_peak"], np.abs(x).max(axis=-1)), f"in_peak {where}"
    assert np.array_equal(rep["out_peak"], np.abs(o).max(axis=-1)), f"out_peak {where}"
    assert np.array_equal(rep["out_clipped"], count_clipped(o)), f"out_clipped {where}"
    assert np.array_equal(rep["pitch_period"], np.asarray(period, np.int32)), f"pitch_period {where}"
    assert np.array_equal(rep["flags"], (np.asarray(silence) != 0).astype(np.uint32)), f"flags {where}"
    for name, v, tol in (("in_energy", x, 3e-5), ("out_energy", o, 3e-5)):
        want = (v.astype(np.float64) ** 2).sum(axis=-1)
        assert np.all(np.abs(rep[name].astype(np.float64) - want) <= tol * want), f"{name} {where}"
    want = np.asarray(gr, F32)[..., :34].astype(np.float64).sum(axis=-1) / 34
    assert np.all(np.abs(rep["gain_mean"].astype(np.float64) - want) <= 3e-6 * np.abs(want)), f"gain_mean {where}"
