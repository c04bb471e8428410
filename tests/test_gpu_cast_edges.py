"""The three device casts float -> int16 and the frame report at their edge values (-m gpu): the back end's fused cast
(percepnet_amd/csrc/pn_dsp.hip), the output stage (pn_outstage.hip) and the rate converter's down kernel (pn_rate.hip), all on the
one pair of functions of pn_pcm.h, against include/percepnet_hip.h as tests/report_model.py models it and as
tests/test_report_host.py pins that model to hand-worked values.

The lever.  The back end computes o[i] = (960 * re) * win[i] + synth_mem[i] and rewrites synth_mem from the same frame's second
half; a stream-state record carries synth_mem verbatim (PN_SS_SYNTH, 480 words) and the import checks only the header.  So: export
the records of a fresh context (valid header, zero body), write chosen floats into the synthesis words, import, process ONE
all-zero frame: every spectrum is zero, o is the chosen row, and the frame after is all zeros again.  That holds in every network
mode, with the post-filter on and with an attenuation limit set (both act on zero spectra), which is how all four int16
instantiations of the back end are reached.  Known non-effects, accepted by same_o() and by nothing else: an imposed -0 may come
back as +0 (0 * win + -0), and a NaN comes back as some quiet NaN (the rows use quiet NaNs).
test_lever establishes this on the GPU with a plain float context, the path the rest of the suite holds bit-equal to the CPU
oracle; every other check compares against that read-back and the numpy models, never against the kernel under test.

Rows of one imposed frame (480 samples; built by report_model.edge_rows, whose construction tests/test_report_host.py checks):
  E  every finite value of test_report_host.HAND's t as o = t / 32768 (exact: a power of two), in-range and out-of-range
     alternating, repeated over the frame so that each of the 60 owning lanes of the output stage's wave (8 samples per lane)
     holds both kinds; |o| <= 91 553, so the energy is finite and check_report's 3e-5 bound applies
  N  quiet NaN, +inf, -inf, FLT_MAX, -FLT_MAX among ordinary samples: peak +inf, energy NaN
  P  one NaN among in-range samples: peak the finite maximum, energy NaN, one clipped sample
  A  480 NaNs: peak 0, 480 clipped, PCM all 0 in both casts
  C  seeded in-range noise (control)
Batches: B = 5 in the order E N P A C and reversed — the output stage and the rate kernels run four streams per block, so row 4
sits alone in a second, partial block, and each edge row is seen in both; B = 1 with E; and B = 5 with N and E in slots 1 and 4
only, where the three streams that keep their zero records must return zeros and a clean report."""
import os
import re

import numpy as np
import pytest

from percepnet_amd import api
from tests import families
from tests import rate_model as rmod
from tests import report_model as rm
from tests.test_report_host import HAND

pytestmark = pytest.mark.gpu
MODES = {"mfma": api.NN_MFMA, "strict": api.NN_STRICT}
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_BYTES = 64               # PN_STREAM_STATE_HEADER_BYTES


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


def synth_word():
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    assert re.search(r"^#define PN_STREAM_STATE_HEADER_BYTES 64$", hdr, re.M)
    return int(re.search(r"^#define PN_SS_SYNTH (\d+)$", hdr, re.M).group(1))


# ------------------------------------------------------------------------------------------------------------------ rows
LAYOUTS = {"ENPAC": ["E", "N", "P", "A", "C"], "CAPNE": ["C", "A", "P", "N", "E"], "E": ["E"], "zNzzE": [None, "N", None, None, "E"]}


def same_o(got, want):
    """Float read-backs: the same bits, or both NaN, or both zero."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    return got.shape == want.shape and bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
                                                   | ((got == 0) & (want == 0))))


def impose(ctx, rows):
    """The lever: the context's streams (fresh, or just reset) get rows [B, 480] as their synthesis overlap memory."""
    B, w = ctx.n_streams, synth_word()
    rec = ctx.export_streams(np.arange(B))
    body = rec[:, HEADER_BYTES:].view(F32)
    assert rec.shape == (B, api.STREAM_STATE_BYTES) and not body[:, w:w + 480].any()
    body[:, w:w + 480] = rows
    assert np.array_equal(rec[:, HEADER_BYTES + 4 * w:HEADER_BYTES + 4 * (w + 480)].view(np.uint32), np.asarray(rows, F32).view(np.uint32))
    for r in rec:
        assert api.stream_state_check(r, ctx.model) == api.SS_OK
    ctx.import_streams(np.arange(B), rec)


class Runs:
    """The rows (report_model.edge_rows; tests/test_report_host.py checks their construction) and every run of them, each
    distinct run made once for the module."""

    def __init__(self, model):
        self.model, self.rows, self.done = model, rm.edge_rows([h[0] for h in HAND]), {}

    def imposed(self, layout):
        return np.stack([self.rows[r] for r in LAYOUTS[layout]])

    def run(self, mode, layout, entry, pf=False, limit=None, report=False, saturate=False):
        """A fresh context with the layout's rows imposed, then two all-zero frames through the entry point "f32" | "i16" ->
        {"out": [2, B, 480], "rep": [2, B] records or None, and for a float run "gr", "sil", "per"}."""
        key = (mode, layout, entry, pf, limit, report, saturate)
        if key in self.done:
            return self.done[key]
        rows = self.imposed(layout)
        B = rows.shape[0]
        ctx = api.Context(self.model, B, nn_mode=MODES[mode])
        ctx.set_postfilter(pf)
        if limit is not None:
            ctx.set_atten_limit(np.arange(B), limit)
        ctx.set_report(report)
        ctx.set_output_saturate(saturate)
        impose(ctx, rows)
        res = {"out": [], "rep": [], "gr": [], "sil": [], "per": []}
        for t in range(2):
            if entry == "f32":
                o, gr = ctx.process_f32(np.zeros((B, 480), F32))
                res["gr"].append(gr); res["sil"].append(ctx.read_features()[1]); res["per"].append(ctx.debug_copy(13, B).view(np.int32).copy())
            else:
                o = ctx.process_i16(np.zeros((B, 480), np.int16), want_gr=False)[0]
            res["out"].append(o)
            if report:
                res["rep"].append(ctx.read_report())
        ctx.close()
        self.done[key] = {k: (np.stack(v) if v else None) for k, v in res.items()}
        return self.done[key]

    def reference(self, mode, layout):
        """The plain float context's read-back, checked as test_lever states it: the reference of everything else."""
        ref = self.run(mode, layout, "f32")
        assert same_o(ref["out"][0], self.imposed(layout)), f"{mode} {layout}: frame 0 must return the imposed rows"
        assert not ref["out"][1].any(), f"{mode} {layout}: frame 1 must be all zeros"
        return ref


@pytest.fixture(scope="module")
def runs(model):
    return Runs(model)


def check_records(rep, ref, layout, rows, where):
    """Both frames' records against the extended model, and against what the rows are built to show."""
    B = rep.shape[1]
    for t in range(2):
        rm.check_report(rep[t], ref["out"][t], ref["gr"][t], ref["sil"][t], ref["per"][t], np.zeros((B, 480), np.int16), f"{where} {layout} frame {t}")
    for name in ("out_peak", "out_energy", "out_clipped", "in_peak", "in_energy"):
        assert not rep[1][name].any(), f"{where} {layout}: {name} of frame 1 — nothing may outlive the imposed frame"
    for s, r in enumerate(LAYOUTS[layout]):
        got = rep[0][s]
        seen = f"{where} {layout} slot {s} row {r}: peak {got['out_peak']} energy {got['out_energy']} clipped {got['out_clipped']}"
        if r == "N":
            assert got["out_peak"] == np.inf and np.isnan(got["out_energy"]) and got["out_clipped"] == 11, seen
        elif r == "P":
            assert got["out_peak"] == np.abs(np.delete(rows["P"], 137)).max() and np.isnan(got["out_energy"]) and got["out_clipped"] == 1, seen
        elif r == "A":
            assert got["out_peak"] == 0 and np.isnan(got["out_energy"]) and got["out_clipped"] == 480, seen
        elif r == "C":
            assert got["out_peak"] == np.abs(rows["C"]).max() and got["out_energy"] > 0 and got["out_clipped"] == 0, seen
        elif r == "E":
            assert got["out_peak"] == F32(3e9) / F32(32768) and np.isfinite(got["out_energy"]), seen
            assert got["out_clipped"] == rm.clipped_t(rows["E"] * F32(32768)).sum() >= 60, seen
        else:
            assert got["out_peak"] == 0 and got["out_energy"] == 0 and got["out_clipped"] == 0, "a stream with a zero record shows a clean report: " + seen


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("mode", list(MODES))
def test_lever(runs, mode):
    """A plain float context with nothing enabled returns the imposed rows on frame 0 and zeros on frame 1."""
    for layout in LAYOUTS:
        ref = runs.reference(mode, layout)
        want = runs.imposed(layout)
        fin = np.isfinite(want) & (want != 0)
        assert np.array_equal(ref["out"][0].view(np.uint32)[fin], want.view(np.uint32)[fin])
        assert np.array_equal(np.isnan(ref["out"][0]), np.isnan(want)) and np.array_equal(ref["out"][0] == np.inf, want == np.inf)
        assert not ref["out"][1].any()
        # the post-filter and a 0 dB limit act on zero spectra: the same float rows
        for pf, limit in ((True, None), (False, 0.0), (True, 0.0)):
            alt = runs.run(mode, layout, "f32", pf=pf, limit=limit)
            assert same_o(alt["out"][0], ref["out"][0]) and not alt["out"][1].any(), (mode, layout, pf, limit)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("mode", list(MODES))
def test_fused_cast(runs, mode):
    """process_i16 with neither report nor saturation: the back end's own cast, in its four int16 instantiations."""
    for layout in LAYOUTS:
        ref = runs.reference(mode, layout)
        want = rm.cast(ref["out"][0], False)
        assert np.array_equal(want, rm.cast(runs.imposed(layout), False))
        for pf in (False, True):
            for limit in (None, 0.0):
                got = runs.run(mode, layout, "i16", pf=pf, limit=limit)["out"]
                assert got.dtype == np.int16 and np.array_equal(got[0], want), (mode, layout, pf, limit)
                assert not got[1].any(), (mode, layout, pf, limit)
        for s, r in enumerate(LAYOUTS[layout]):
            if r in ("A", None):
                assert not want[s].any()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("mode", list(MODES))
def test_output_stage_wrap(runs, mode):
    for layout in LAYOUTS:
        ref = runs.reference(mode, layout)
        fused = runs.run(mode, layout, "i16")["out"]
        got = runs.run(mode, layout, "i16", report=True)
        assert np.array_equal(got["out"], fused), "wrap mode through the stage is the fused cast, bit for bit"
        assert np.array_equal(got["out"][0], rm.cast(ref["out"][0], False)) and not got["out"][1].any()
        check_records(got["rep"], ref, layout, runs.rows, f"{mode} wrap")


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("mode", list(MODES))
def test_output_stage_saturate(runs, mode):
    for layout in LAYOUTS:
        ref = runs.reference(mode, layout)
        want = rm.cast(ref["out"][0], True)
        wrap = runs.run(mode, layout, "i16", report=True)
        sat = runs.run(mode, layout, "i16", report=True, saturate=True)
        alone = runs.run(mode, layout, "i16", saturate=True)
        for got in (sat["out"], alone["out"]):
            assert np.array_equal(got[0], want) and not got[1].any(), (mode, layout)
        assert sat["rep"].tobytes() == wrap["rep"].tobytes(), "the records do not depend on the cast"
        check_records(sat["rep"], ref, layout, runs.rows, f"{mode} saturate")
        for s, r in enumerate(LAYOUTS[layout]):
            if r in ("A", None):
                assert not want[s].any()
            if r == "E":
                assert not np.array_equal(want[s], wrap["out"][0][s]) and {-32768, 32767} <= set(want[s].tolist())


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("mode", list(MODES))
def test_float_entry_point_with_the_report_on(runs, mode):
    """Float rows are never altered, also in saturate mode, and the records — out_clipped too — are those of the int16 run."""
    for layout in LAYOUTS:
        ref = runs.reference(mode, layout)
        wrap = runs.run(mode, layout, "i16", report=True)
        for saturate in (False, True):
            got = runs.run(mode, layout, "f32", report=True, saturate=saturate)
            assert same_o(got["out"][0], ref["out"][0]) and same_o(got["out"][0], runs.imposed(layout)) and not got["out"][1].any()
            assert got["rep"].tobytes() == wrap["rep"].tobytes(), (mode, layout, saturate)
        check_records(got["rep"], ref, layout, runs.rows, f"{mode} float")


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("mode", list(MODES))
def test_input_side_of_the_report(model, mode):
    """in_peak / in_energy read whatever the float API put into the history ring: a NaN, an inf and a 1e30 sample in frame 0
    show in the record of frame 6 as the header says, and are gone from frame 7's."""
    B, T, D = 3, 8, rm.DELAY_FRAMES
    x = (np.random.default_rng(21).uniform(-1.0, 1.0, (T, B, 480)) * 0.25).astype(F32)
    x[0, 0, 17], x[0, 1, 200], x[0, 2, 333] = np.nan, np.inf, 1e30
    plain, rep_ctx = api.Context(model, B, nn_mode=MODES[mode]), api.Context(model, B, nn_mode=MODES[mode])
    rep_ctx.set_report(True)
    for t in range(T):
        o, gr = plain.process_f32(x[t])
        sil, per = plain.read_features()[1], plain.debug_copy(13, B).view(np.int32).copy()
        o2, gr2 = rep_ctx.process_f32(x[t])
        rep = rep_ctx.read_report()
        same = lambda a, b: bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
        assert same(o2, o) and same(gr2, gr), t
        rm.check_report(rep, o, gr, sil, per, x[t - D] if t >= D else np.zeros((B, 480), F32), f"{mode} frame {t}")
        if t < D:
            assert not rep["in_peak"].any() and not rep["in_energy"].any()
        if t == D:
            assert rep["in_peak"][0] == np.abs(np.delete(x[0, 0], 17)).max() and np.isnan(rep["in_energy"][0])
            assert rep["in_peak"][1] == np.inf and rep["in_energy"][1] == np.inf
            assert rep["in_peak"][2] == F32(1e30) and rep["in_energy"][2] == np.inf
        if t > D:
            assert np.isfinite(rep["in_peak"]).all() and np.isfinite(rep["in_energy"]).all() and rep["in_energy"].all()
    plain.close(); rep_ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()                   # the context runs on its own non-blocking stream
    return t


def same_z(got, want):
    """fp32 rows: the same bits, or both NaN (numpy's and the GPU's default NaNs differ in sign)."""
    return got.shape == want.shape and got.dtype == want.dtype and bool(np.all((got.view(np.uint32) == want.view(np.uint32))
                                                                               | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("rate", rmod.RATES)
def test_rate_down_cast_at_the_edges(model, rate):
    """down_i16_dev filters before it casts, so z is steered rather than imposed: rate_model.cast_edge_rows (single samples,
    amplitudes found on the numpy model alone; tests/test_rate_host.py checks the same precondition without a GPU)."""
    import torch
    L = rmod.factor(rate)
    n = 480 // L
    g = api.rate_taps(rate, True)
    for B in (5, 1):
        o = rmod.cast_edge_rows(B, L, g)
        down = rmod.Down(B, L, g)
        with np.errstate(all="ignore"):
            z = np.stack([down(f) for f in o])
            t = z * F32(32768)
        for name, mask in rmod.t_classes(t).items():
            assert np.all(mask.sum(axis=(0, 2)) >= 1), f"precondition: every row reaches {name}"
        assert not o[-1].any() and np.isnan(z[-1]).any(axis=1).all(), "the frame of zeros still carries NaN through the tail"
        ctx = api.Context(model, B)
        rc = api.RateConverter(ctx, rate)
        for kind in ("f32", "wrap", "saturate"):
            rc.reset()
            ctx.set_output_saturate(kind == "saturate")
            for f in range(o.shape[0]):
                d_in = to_dev(o[f])
                if kind == "f32":
                    d_out = torch.full((B, n), 7.0, dtype=torch.float32, device="cuda:0")
                    torch.cuda.synchronize()
                    rc.down_f32_dev(d_in.data_ptr(), d_out.data_ptr())
                    ctx.synchronize()
                    assert same_z(d_out.cpu().numpy(), z[f]), f"{rate} Hz B={B} f32 frame {f}"
                else:
                    d_out = torch.full((B, n), 12345, dtype=torch.int16, device="cuda:0")
                    torch.cuda.synchronize()
                    rc.down_i16_dev(d_in.data_ptr(), d_out.data_ptr())
                    ctx.synchronize()
                    want = rmod.to_i16(z[f], kind == "saturate")
                    assert np.array_equal(d_out.cpu().numpy(), want), f"{rate} Hz B={B} {kind} frame {f}"
        rc.close(); ctx.close()


def test_rate_chain_casts_the_imposed_rows(model, runs):
    """16 kHz, one chained case: the rows E N P A C imposed through the synthesis record, zeros fed to rc.process_i16 (their
    up-conversion is zeros), so the down kernel filters and casts exactly the lever's read-back."""
    rate, layout, B = 16000, "ENPAC", 5
    L = rmod.factor(rate)
    ref = runs.reference("mfma", layout)
    g = api.rate_taps(rate, True)
    ctx = api.Context(model, B)
    rc = api.RateConverter(ctx, rate)
    for saturate in (False, True):
        ctx.reset(); rc.reset()
        ctx.set_output_saturate(saturate)
        impose(ctx, runs.imposed(layout))
        down = rmod.Down(B, L, g)
        for f in range(2):
            got = rc.process_i16(np.zeros((B, 480 // L), np.int16), want_gr=False)[0]
            with np.errstate(all="ignore"):
                z = down(ref["out"][f])
            if f == 0 and not saturate:
                n_out = rm.count_clipped(z)
                assert 0 < n_out[0] < z.shape[1] and n_out[4] == 0, "row E leaves the int16 range after the filter, and not everywhere"
            assert np.array_equal(got, rmod.to_i16(z, saturate)), f"saturate={saturate} frame {f}"
    rc.close(); ctx.close()
