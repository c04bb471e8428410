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


def scaled(o):
    """t = o * 32768 in fp32: what is cast and counted (a product beyond FLT_MAX is +-inf)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(o, F32) * F32(32768)


def cast(o, saturate):
    return cast_t(scaled(o), saturate)


def count_clipped(o):
    """Float outputs [..., 480] -> out_clipped [...]"""
    return clipped_t(scaled(o)).sum(axis=-1).astype(np.int32)


def peak(v):
    """Rows of samples [..., 480] -> the record's peak word: the fmax-style maximum of |v| from 0, so a NaN sample is ignored
    (a row of 480 NaNs gives 0) and an infinite one gives +inf."""
    return np.fmax.reduce(np.abs(np.asarray(v, F32)), axis=-1, initial=F32(0))


def energy_matches(got, v, tol=3e-5):
    """Does the fp32 word `got` [...] hold the record's energy of the rows v [..., 480]?  The kernel's fixed-order fp32 sum of
    the separately rounded fp32 products v * v:
      * one NaN sample makes it NaN;
      * otherwise a product that overflows fp32 (|v| > sqrt(FLT_MAX), an infinite sample included) makes it +inf, and so does
        a sum beyond FLT_MAX;
      * otherwise it lies within a relative `tol` of the float64 sum (any fp32 summation order of 480 non-negative products is
        within gamma_481 * 2^-24 ~ 2.9e-5); a float64 sum more than `tol` beyond FLT_MAX must be +inf."""
    got, v = np.asarray(got, F32), np.asarray(v, F32)
    big = float(np.finfo(F32).max)
    with np.errstate(over="ignore", invalid="ignore"):
        nan = np.isnan(v).any(axis=-1)
        inf = ~nan & np.isinf(v * v).any(axis=-1)
        want = (np.where(np.isfinite(v), v, F32(0)).astype(np.float64) ** 2).sum(axis=-1)
        near = np.abs(got.astype(np.float64) - want) <= tol * want
    must_inf = inf | (want * (1 - tol) > big)
    return np.where(nan, np.isnan(got), np.where(must_inf, got == F32(np.inf), near))


def edge_rows(hand_t):
    """The rows that tests/test_gpu_cast_edges.py imposes as one frame of float outputs o [480], from the t column of
    tests/test_report_host.HAND (tests/test_report_host.py checks what is said here, without a GPU):
      E  every finite t of the table as o = t / 32768 (exact: a power of two; a t too small to have an o is left out), in-range and
         out-of-range values alternating and repeated over the frame, so that each of the 60 owning lanes of the output stage's
         wave (8 samples per lane) holds both kinds; |o| <= 1e5, so the energy is finite
      N  quiet NaN, +inf, -inf, FLT_MAX, -FLT_MAX among in-range samples (11 samples that do not fit)
      P  one NaN (sample 137) among in-range samples
      A  480 NaNs
      C  seeded in-range noise (control)
      None  zeros: a stream that keeps its zero record"""
    def noise(seed, scale):
        return (np.random.default_rng(seed).uniform(-1.0, 1.0, 480) * scale).astype(F32)
    big = np.finfo(F32).max
    t = np.array([v for v in hand_t if np.isfinite(v)], F32)
    t = t[(t / F32(32768)) * F32(32768) == t]
    out = clipped_t(t)
    a, b = t[~out], t[out]
    n = min(a.size, b.size)
    cycle = np.concatenate([np.stack([a[:n], b[:n]], axis=1).ravel(), a[n:], b[n:]])     # in, out, in, out, ... then the rest
    rows = {"E": np.resize(cycle, 480) / F32(32768), "N": noise(11, 0.9), "P": noise(12, 0.5), "A": np.full(480, np.nan, F32),
            "C": noise(13, 0.999), None: np.zeros(480, F32)}
    for at, v in ((5, np.nan), (77, np.nan), (300, np.nan), (13, np.inf), (250, np.inf), (40, -np.inf), (411, -np.inf),
                  (100, big), (479, big), (0, -big), (222, -big)):
        rows["N"][at] = v
    rows["P"][137] = np.nan
    return rows


def check_levels(rep, side, v, where=""):
    """The peak and energy words of one side ("in" | "out") of the records `rep` against that side's float rows v [n, 480]."""
    assert np.array_equal(rep[side + "_peak"], peak(v)), f"{side}_peak {where}"
    assert np.all(energy_matches(rep[side + "_energy"], v)), f"{side}_energy {where}"


def check_report(rep, o, gr, silence, period, x_in, where=""):
    """One frame's records `rep` (REPORT_DTYPE [n]) against the float outputs o [n, 480], the g|r tap [n, 68], the silence
    flags and pitch periods [n] of a plain context, and the aligned input frame x_in (int16 [n, 480], or the float rows a float
    entry point was given; zeros before a stream's seventh frame).  Exact words are compared exactly; the two energies within a
    relative 3e-5 of the float64 sum — any fp32 summation order of 480 non-negative products is within gamma_481 * 2^-24 ~ 2.9e-5
    — and gain_mean within 3e-6 (gamma_34).  Non-finite rows follow include/percepnet_hip.h: a peak ignores NaN samples, an
    energy is NaN with one NaN sample and +inf on overflow otherwise (peak, energy_matches), NaN counts in out_clipped, and
    gain_mean is NaN when a gain is."""
    assert rep.dtype == api.REPORT_DTYPE
    o = np.asarray(o, F32)
    x_in = np.asarray(x_in)
    x = x_in.astype(F32) if x_in.dtype.kind == "f" else x_in.astype(np.int16).astype(F32) / F32(32768)
    check_levels(rep, "in", x, where)
    check_levels(rep, "out", o, where)
    assert np.array_equal(rep["out_clipped"], count_clipped(o)), f"out_clipped {where}"
    assert np.array_equal(rep["pitch_period"], np.asarray(period, np.int32)), f"pitch_period {where}"
    assert np.array_equal(rep["flags"], (np.asarray(silence) != 0).astype(np.uint32)), f"flags {where}"
    want = np.asarray(gr, F32)[..., :34].astype(np.float64).sum(axis=-1) / 34
    got = rep["gain_mean"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.where(np.isnan(want), np.isnan(got), np.abs(got - want) <= 3e-6 * np.abs(want))
    assert np.all(ok), f"gain_mean {where}"
