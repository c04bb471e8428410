"""Idle-line and subnormal signal levels on the GPU (-m gpu): the rows of tests/tiny_levels.py through every kernel a tiny sample
passes through, against the CPU oracle (tests/test_tiny_levels_host.py: equal to the compiled reference on every one of these
rows, and different from its own flush-to-zero mutant in every zone) and against the numpy models of the other fp32 kernels.

  Z1  +-1..4 LSB of a 16-bit line, floats 1e-4.5 .. 1e-6: find_best_pitch compares subnormal numerators -> the pitch period
  Z2  1e-13 .. 1e-18: band energies and their products are subnormal                                   -> the features
  Z3  1e-18.5 .. 1e-22.5: the pitch correlations are subnormal                                         -> the pitch period
  Z4  1e-27 .. 1e-40.5: spectra and output samples are subnormal                                       -> the output
  Z5  <= 1e-41: the input is subnormal                                                                 -> the stage taps

Every comparison with the oracle is bit for bit; a mismatch is reported as row, zone, frame and the first tap that differs, in the
order of the data path (history, Y, X, period, P, features, silence, g|r, output).  The batch is tiny_levels.batch(): 118 streams,
four zones in every wavefront of the split pitch kernel, 20 frames."""
import os

import numpy as np
import pytest

from percepnet_amd import api
from tests import backend_model as bm
from tests import families
from tests import rate_model as rmod
from tests import report_model as rm
from tests import tiny_levels as tl
from test_gpu_parity import F16_GR_TOL, GR_TOL, PCM_TOL_LSB
from test_gpu_rate import Pair, dev_full, taps, to_dev, to_host
from test_gpu_stages import BINS, STRIDE, _logical_history

pytestmark = pytest.mark.gpu
F32 = np.float32
T = tl.T
PATH = ("hist", "Y", "X", "period", "P", "feat", "silence", "gr", "out")      # the order of the data path
TAPS = ("hist", "Y", "X", "period", "P")


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex64:
        a = a.view(F32)
    return a.view(np.uint32) if a.dtype == F32 else a


def fr(x, t, n=480):
    return np.ascontiguousarray(x[:, t * n:(t + 1) * n])


def run_f32(model, names, mode=api.NN_STRICT, fe=None, with_taps=True, setup=None, per_frame=None):
    """The rows `names` through a float context, frame by frame -> {key: [B, T, ...]}: out, gr, feat, silence and (with_taps) the
    stage taps of tests/test_gpu_stages.py.  fe: PERCEPNET_FE, set around the context's creation only."""
    x = tl.stack(names)
    B = len(names)
    if fe is not None:
        os.environ["PERCEPNET_FE"] = fe
    try:
        ctx = api.Context(model, B, nn_mode=mode)
    finally:
        os.environ.pop("PERCEPNET_FE", None)
    if fe is not None:
        assert ctx.describe()["frontend"] == {"split": "split", "mono": "g4", "g2": "g2"}[fe]
    if setup:
        setup(ctx)
    got = {k: [] for k in (PATH if with_taps else ("feat", "silence", "gr", "out"))}
    for t in range(T):
        o, g = ctx.process_f32(fr(x, t))
        f, s = ctx.read_features()
        got["out"].append(o); got["gr"].append(g); got["feat"].append(f); got["silence"].append(s)
        if with_taps:
            ring = ctx.debug_copy(12, B * STRIDE).reshape(B, STRIDE)
            got["hist"].append(_logical_history(ring, t))
            yr = ctx.debug_copy(10, 6 * B * BINS * 2).view(np.complex64).reshape(6, B, BINS)
            got["Y"].append(yr[t % 6].copy()); got["X"].append(yr[(t + 1) % 6].copy())
            got["P"].append(ctx.debug_copy(11, B * BINS * 2).view(np.complex64).reshape(B, BINS).copy())
            got["period"].append(ctx.debug_copy(13, B).view(np.int32).copy())
        if per_frame:
            per_frame(ctx, t, o, g)
    ctx.close()
    return {k: np.stack(v, 1) for k, v in got.items()}


@pytest.fixture(scope="module")
def want(oracle):
    """The oracle side, once: {row name: {key: [T, ...]}} with the keys of PATH (spectra cut to the 400 bins the engine keeps),
    and the full-width X, P for the back-end model."""
    out = {}
    for name, r in tl.rows().items():
        st = oracle.stages(r.x)
        o, gr = oracle.run_float(r.x)
        cut = lambda a: np.ascontiguousarray(a[:, :BINS])
        out[name] = dict(hist=st["comb_buf"], Y=cut(st["Y"]), X=cut(st["X"]), period=st["period"], P=cut(st["P"]),
                         feat=st["feat"], silence=st["silence"], gr=gr, out=o.reshape(T, 480), X481=st["X"], P481=st["P"])
    return out


def differences(got, ref, names, keys):
    """got {key: [B, T, ...]} against ref {name: {key: [T, ...]}} bit for bit -> one line per differing stream: row, zone, first
    frame that differs and the first tap of the data path that differs in it."""
    R = tl.rows()
    lines = []
    for i, name in enumerate(names):
        first = None
        for k in keys:
            ne = _bits(got[k][i]) != _bits(ref[name][k])
            bad = np.flatnonzero(ne.reshape(T, -1).any(axis=1))
            if bad.size and (first is None or bad[0] < first[0]):
                first = (int(bad[0]), k, int(bad.size), int(ne.sum()))
        if first:
            lines.append(f"stream {i} row {name} zone {R[name].zone}: frame {first[0]}, first differing tap {first[1]} "
                         f"({first[2]} frames, {first[3]} words of it differ)")
    return lines


def assert_same(got, ref, names, keys, what):
    lines = differences(got, ref, names, keys)
    R = tl.rows()
    zones = sorted({R[n].zone for n in names})
    tally = {z: sum(f"zone {z}:" in ln for ln in lines) for z in zones}
    assert not lines, f"{what}: {len(lines)} of {len(names)} streams differ, by zone {tally}\n" + "\n".join(lines[:40])


@pytest.fixture(scope="module")
def strict0(model):
    saved = {k: os.environ.pop(k) for k in families.FAMILY_ENV if k in os.environ}      # (module scope: before the autouse fixture)
    try:
        return run_f32(model, tl.batch(0))
    finally:
        os.environ.update(saved)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_strict_float_entry_point_bit_for_bit(strict0, want):
    names = tl.batch(0)
    assert len(names) % 16 != 0
    assert_same(strict0, want, names, PATH, "STRICT, default families, process_f32")


def test_the_oracle_side_is_not_vacuous(want):
    R = tl.rows()
    z1 = {int(p) for n, r in R.items() if r.zone == "Z1" for p in want[n]["period"]}
    assert len(z1) >= 10, z1                                                        # the Z1 rows' periods move
    assert sum(int(tl.subnormal(want[n]["out"]).sum()) for n, r in R.items() if r.zone == "Z4") > 10000
    assert sum(int(tl.subnormal(want[n]["Y"].view(F32)).sum()) for n, r in R.items() if r.zone == "Z5") > 10000
    assert all(not want[n]["out"].any() for n, r in R.items() if r.zone == "Z5")    # only the taps see Z5


# ---------------------------------------------------------------------------------------------------------------- 2
def grid_names():
    return [n for n, r in tl.rows().items() if r.grid]


def run_i16(model, pcm, mode=api.NN_STRICT, setup=None, report=False):
    B = pcm.shape[0]
    ctx = api.Context(model, B, nn_mode=mode)
    if setup:
        setup(ctx)
    got = {k: [] for k in ("out", "gr", "feat", "silence", "report")}
    for t in range(T):
        o, g = ctx.process_i16(fr(pcm, t))
        f, s = ctx.read_features()
        got["out"].append(o); got["gr"].append(g); got["feat"].append(f); got["silence"].append(s)
        got["report"].append(ctx.read_report() if report else np.zeros(B, api.REPORT_DTYPE))
    ctx.close()
    return {k: np.stack(v, 1) for k, v in got.items()}


def test_int16_entry_point(model, oracle):
    names = grid_names()
    R = tl.rows()
    pcm = np.stack([tl.pcm_of(R[n]) for n in names])
    ro, rg, rf, rs = oracle.run_batch(pcm)
    got = run_i16(model, pcm)
    for k, ref in (("feat", rf), ("silence", rs), ("gr", rg)):
        bad = [(names[i], R[names[i]].zone, int(np.flatnonzero((_bits(got[k][i]) != _bits(ref[i])).reshape(T, -1).any(axis=1))[0]))
               for i in range(len(names)) if not np.array_equal(_bits(got[k][i]), _bits(ref[i]))]
        assert not bad, f"{k} (row, zone, first frame): {bad}"
    out = got["out"][:, 1:].reshape(len(names), -1)
    assert np.array_equal(out, ro), [names[i] for i in range(len(names)) if not np.array_equal(out[i], ro[i])]
    # what PCM sees and what it does not: the synth streams come out, +-1 LSB of dither comes out as digital zero
    assert all(ro[names.index(f"synth{s}")].any() for s in tl.FILLERS)
    assert not ro[names.index("dither1")].any() and rg[names.index("dither1")].any()
    # the saturating cast and the report on the same rows: nothing clips, so the PCM is the wrapping cast's
    sat = run_i16(model, pcm, setup=lambda c: (c.set_report(True), c.set_output_saturate(True)), report=True)
    assert np.array_equal(sat["out"], got["out"])
    assert not sat["report"]["out_clipped"].any()
    assert np.array_equal(sat["report"]["flags"], (rs != 0).astype(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("order", [1, 2])
def test_a_rows_bits_do_not_depend_on_its_place_or_neighbours(model, strict0, order):
    """The pitch kernel's wave-wide ballot and its DPP rows couple the four streams of a wavefront in control flow only: a row must
    come out with the bits it had in batch(0), whatever its three neighbours are and whichever 16 lanes it runs on."""
    first = {}
    for i, n in enumerate(tl.batch(0)):
        first.setdefault(n, {k: strict0[k][i] for k in PATH})
    names = tl.batch(order)
    moved = sum(a != b for a, b in zip(names, tl.batch(0)))
    assert moved > len(names) * 0.9
    assert_same(run_f32(model, names), first, names, PATH, f"batch({order}) against batch(0)")


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("fe", ["split", "mono", "g2"])
def test_every_front_end_family(model, want, fe):
    names = tl.batch(0)
    got = run_f32(model, names, fe=fe, with_taps=False)
    assert_same(got, want, names, ("feat", "silence", "gr", "out"), f"PERCEPNET_FE={fe}")


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("mode,tol", [("mfma", GR_TOL), ("x3", GR_TOL), ("f16", F16_GR_TOL)])
def test_network_modes_share_the_dsp(model, strict0, want, mode, tol):
    """The DSP does not depend on the network mode: features, silence and the four taps are STRICT's bits; g|r stays within the
    mode's tolerance of the oracle (tests/test_gpu_parity.py).  Outputs are not compared: the suite's absolute bound on them says
    nothing at these levels."""
    names = tl.batch(0)
    got = run_f32(model, names, mode={"mfma": api.NN_MFMA, "x3": api.NN_MFMA_X3, "f16": api.NN_MFMA_F16}[mode])
    ref = {i: {k: strict0[k][i] for k in PATH} for i in range(len(names))}
    R = tl.rows()
    lines = []
    for i, n in enumerate(names):
        for k in TAPS + ("feat", "silence"):
            if not np.array_equal(_bits(got[k][i]), _bits(ref[i][k])):
                frame = int(np.flatnonzero((_bits(got[k][i]) != _bits(ref[i][k])).reshape(T, -1).any(axis=1))[0])
                lines.append(f"stream {i} row {n} zone {R[n].zone}: frame {frame}, tap {k}")
                break
    assert not lines, f"{mode}: DSP taps differ from STRICT on {len(lines)} streams\n" + "\n".join(lines[:40])
    err = np.array([np.abs(got["gr"][i] - want[n]["gr"]).max() for i, n in enumerate(names)])
    worst = int(err.argmax())
    assert err.max() <= tol, f"{mode}: g|r off by {err.max()} on row {names[worst]} zone {R[names[worst]].zone}"


# ---------------------------------------------------------------------------------------------------------------- 6
def test_attenuation_limit_against_the_backend_model(model, oracle, want):
    """6 dB on every second stream: the float output against tests/backend_model.py fed the oracle's X, P, silence and the
    engine's own g|r, bit for bit (tests/test_gpu_atten_limit.py); the other streams are the unlimited engine, the oracle's."""
    names = tl.batch(0)
    B = len(names)
    limited = np.arange(0, B, 2)
    got = run_f32(model, names, with_taps=False, setup=lambda c: c.set_atten_limit(limited, 6.0))
    backend = bm.BackendModel(oracle)
    lam = bm.factor(6.0)[0]
    R = tl.rows()
    lines = []
    for i, n in enumerate(names):
        w = want[n]
        assert np.array_equal(_bits(got["gr"][i]), _bits(w["gr"])), f"g|r depends on the limit: row {n}"
        ref = backend.run(w["X481"], w["P481"], w["silence"], got["gr"][i], lam if i % 2 == 0 else F32(0))
        if i % 2:
            assert np.array_equal(_bits(ref), _bits(w["out"])), f"the model is not the oracle on row {n}"
        bad = np.flatnonzero((_bits(ref) != _bits(got["out"][i])).any(axis=1))
        if bad.size:
            lines.append(f"stream {i} row {n} zone {R[n].zone} lam {lam if i % 2 == 0 else 0}: first at frame {bad[0]}, {bad.size} frames")
    assert not lines, f"{len(lines)} streams differ from the back-end model\n" + "\n".join(lines[:40])
    changed = sum(not np.array_equal(_bits(got["out"][i]), _bits(want[names[i]]["out"])) for i in limited)
    assert changed > len(limited) // 2, "the limit changed nothing: the variant did not run"
    z4 = [i for i in limited if R[names[i]].zone == "Z4"]
    assert z4 and sum(int(tl.subnormal(got["out"][i]).sum()) for i in z4) > 1000          # the mix itself ran on subnormals


def test_postfilter_on_the_int16_grid_rows(model, oracle):
    """As tests/test_gpu_parity.py::test_postfilter_option: g|r untouched, PCM within 1 LSB of the oracle's post-filtered PCM (the
    warped gain goes through sinf)."""
    names = grid_names()
    R = tl.rows()
    pcm = np.stack([tl.pcm_of(R[n]) for n in names])
    got = run_i16(model, pcm, setup=lambda c: c.set_postfilter(True))
    ro, rg = zip(*[oracle.run_pcm(p, postfilter=True) for p in pcm])
    plain = oracle.run_batch(pcm, want_feat=False)[0]
    assert np.array_equal(_bits(got["gr"]), _bits(np.stack(rg)))
    d = np.abs(got["out"][:, 1:].reshape(len(names), -1).astype(np.int32) - np.stack(ro).astype(np.int32))
    assert d.max() <= PCM_TOL_LSB, (names[int(d.max(axis=1).argmax())], int(d.max()))
    assert np.abs(np.stack(ro).astype(np.int32) - plain.astype(np.int32)).max() > 50                  # the stage does something


def test_frame_report_and_saturating_cast(model, want):
    """The records of a float context with the report and the saturating cast on, after every frame: peaks exact (a subnormal peak
    included), nothing clipped, period / flags / gain_mean as report_model.check_report checks them, and both energies within
    3e-5 * want + 960 * 2^-150 of the float64 sum (tiny_levels.energy_matches_tiny)."""
    names = tl.batch(0)
    B = len(names)
    x = tl.stack(names).reshape(B, T, 480)
    R = tl.rows()
    per = np.stack([want[n]["period"] for n in names])
    sil = np.stack([want[n]["silence"] for n in names])
    seen = dict(sub_peak=0, sub_energy=0)

    def check(ctx, t, o, gr):
        rep = ctx.read_report()
        assert rep.dtype == api.REPORT_DTYPE
        xin = x[:, t - rm.DELAY_FRAMES] if t >= rm.DELAY_FRAMES else np.zeros((B, 480), F32)
        for side, v in (("in", xin), ("out", o)):
            bad = np.flatnonzero(_bits(rep[side + "_peak"]) != _bits(rm.peak(v)))
            assert bad.size == 0, f"{side}_peak frame {t}: " + ", ".join(f"{names[i]} ({R[names[i]].zone})" for i in bad[:8])
            bad = np.flatnonzero(~tl.energy_matches_tiny(rep[side + "_energy"], v))
            assert bad.size == 0, f"{side}_energy frame {t}: " + ", ".join(
                f"{names[i]} ({R[names[i]].zone}) got {rep[side + '_energy'][i]!r} want {(v[i].astype(np.float64) ** 2).sum()!r}" for i in bad[:8])
            seen["sub_peak"] += int(tl.subnormal(rep[side + "_peak"]).sum())
            seen["sub_energy"] += int(tl.subnormal(rep[side + "_energy"]).sum())
        assert not rep["out_clipped"].any() and np.array_equal(rep["out_clipped"], rm.count_clipped(o)), t
        assert np.array_equal(rep["pitch_period"], per[:, t]), f"pitch_period frame {t}"
        assert np.array_equal(rep["flags"], (sil[:, t] != 0).astype(np.uint32)), f"flags frame {t}"
        w = gr[:, :34].astype(np.float64).sum(axis=-1) / 34
        assert np.all(np.abs(rep["gain_mean"].astype(np.float64) - w) <= 3e-6 * np.abs(w)), f"gain_mean frame {t}"

    got = run_f32(model, names, with_taps=False, setup=lambda c: (c.set_report(True), c.set_output_saturate(True)), per_frame=check)
    assert_same(got, want, names, ("out", "gr"), "float samples are never altered by the report or the saturating cast")
    assert seen["sub_peak"] > 100 and seen["sub_energy"] > 100, seen


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("rate", rmod.RATES)
def test_rate_converter_kernels_on_the_ladder(model, rate):
    """The float ladder decimated to the low rate through the up kernel, and at 48 kHz through the down kernel, against the exact
    float32 models of tests/rate_model.py bit for bit (tests/test_gpu_rate.py at ordinary levels): 4 frames, so that both tails
    cross frame boundaries."""
    import torch
    frames = 4
    names = [n for n in tl.rows() if n.startswith("f1e")]
    R = tl.rows()
    x48 = tl.stack(names)[:, :frames * 480]
    B = len(names)
    h, g = taps(rate)
    p = Pair(model, B, rate)
    L, n = p.L, p.n
    xlow = np.ascontiguousarray(x48[:, ::L])
    up, down = rmod.Up(B, L, h), rmod.Down(B, L, g)
    sub = 0
    for t in range(frames):
        d_in, d_out = to_dev(fr(xlow, t, n)), dev_full((B, 480), torch.float32, float("nan"))
        p.rc.up_f32_dev(d_in.data_ptr(), d_out.data_ptr())
        got, ref = to_host(p.ctx, d_out), up(fr(xlow, t, n))
        bad = np.flatnonzero((_bits(got) != _bits(ref)).any(axis=1))
        assert bad.size == 0, f"up {rate} Hz frame {t}: " + ", ".join(f"{names[i]} ({R[names[i]].zone})" for i in bad[:8])
        sub += int(tl.subnormal(ref).sum())
        d_in, d_out = to_dev(fr(x48, t)), dev_full((B, n), torch.float32, float("nan"))
        p.rc.down_f32_dev(d_in.data_ptr(), d_out.data_ptr())
        got, ref = to_host(p.ctx, d_out), down(fr(x48, t))
        bad = np.flatnonzero((_bits(got) != _bits(ref)).any(axis=1))
        assert bad.size == 0, f"down {rate} Hz frame {t}: " + ", ".join(f"{names[i]} ({R[names[i]].zone})" for i in bad[:8])
        sub += int(tl.subnormal(ref).sum())
    p.close()
    assert F32(1e-30) * F32(1e-10) != 0 and sub > 1000, "the models' own sums must run through subnormals"
