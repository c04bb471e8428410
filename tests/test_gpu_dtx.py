"""The DTX send side of the rate converter (-m gpu): include/percepnet_hip.h "DTX send side"; kernel percepnet_amd/csrc/pn_rate_dtx.hip,
host side pn_rate.cpp (pn_rate_set_stream_dtx / pn_rate_dtx_f32, _i16, _g711 and the hook behind the down-conversion in rate_frame), the
rule pn_dtx_rules.h, bindings api.RateConverter.set_stream_dtx / dtx_dev / read_dtx_report / dtx_state.

The oracle is the numpy model tests/dtx_model.py; every comparison is equality of bits, state and report.  The stage writes no audio:
wherever a frame runs with streams switched on, a twin converter with nobody switched on gives the same rows and g|r.

Shapes: 67 streams for the kernel alone — one more than a wavefront's lanes, and no multiple of the block's four rows — with a third
of them switched off; 7 streams over all five rates for the mixed formats and whole frames; 5 for the closed loop with comfort noise."""
import numpy as np
import pytest

from percepnet_amd import api
from tests import cng_model as cm
from tests import dtx_model as dm
from tests import g711_model as gm
from tests import test_dtx_host as th
from tests import test_gpu_plc as tpl
from tests import test_gpu_rate as tg
from tests import test_gpu_rate_pipe as tp

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
Twin, same, to_dev, to_host, dev_full = tpl.Twin, tpl.same, tg.to_dev, tg.to_host, tg.dev_full
QUICK = np.array([4.0, 0.1, 1.5, 1e-10, 3, 0.1, 1, 4, 12], F32)       # a short hangover, a fast drift, a SID every fourth frame, order 12
SHORT = np.array([4.0, 0.1, 1.0023, 1e-10, 2, 0.1, 2, 0, 10], F32)    # the defaults with a hangover of two
# whole frames: what the engine leaves of a pause is not known here, so the least floor is set above it (-64 dBov): a pause of 1e-4 rms
# at the input is never active, whatever floor the first rows behind the converter's delay have left
HOOK = np.array([4.0, 0.1, 1.5, 1e-7, 3, 0.1, 1, 4, 12], F32)


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in tpl.families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


class At48(Twin):
    """every stream at 48000 Hz: rows of 480 samples (a single-rate converter takes 8000 .. 32000; this is the mixed one)"""

    def __init__(self, model, B):
        self.B = B
        self.ctx = api.Context(model, B)
        self.rates = [48000] * B
        self.rc = api.MixedRateConverter(self.ctx, self.rates)
        self.rc.set_stream_laws(list(range(B)), [s % 2 for s in range(B)])
        self.w = self.rc.frame
        self.rc.set_profiling(True)


def report_words(rc):
    return np.ascontiguousarray(rc.read_dtx_report()).view(U32).reshape(rc.n_streams, dm.REPORT_WORDS)


def assert_model(rc, m, what):
    st, rep = rc.dtx_state(), report_words(rc)
    for s in range(m.B):
        assert same(st[s], m.state[s]), f"{what}: state of stream {s}: {st[s]} != {m.state[s]}"
        assert same(rep[s], m.report[s]), f"{what}: report of stream {s}: {rep[s]} != {m.report[s]}"
        if rep[s, 0] == dm.SID:
            th.check_sid(rep[s].view(np.uint8)[16:30])


def enable(tw, m, ids, params):
    tw.rc.set_dtx_params(params)
    tw.rc.set_dtx_report(True)
    tw.rc.set_stream_dtx(ids, 1)
    m.params = np.asarray(params, F32).copy()
    m.set_on(ids, True)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("rate", (8000, 16000, 24000, 32000, 48000))
def test_the_stage_alone_is_the_model(model, rate):
    B, T = 67, 40
    a = Twin(model, B, rate) if rate != 48000 else At48(model, B)
    ns = a.ns()[0]
    assert a.w == ns
    m = dm.Dtx(B, ns)
    on = [s for s in range(B) if s % 3 != 1]
    enable(a, m, on, QUICK if rate in (8000, 24000, 48000) else SHORT)
    assert a.rc.stream_dtx().tolist() == [int(s % 3 != 1) for s in range(B)] and same(a.rc.dtx_params(), m.params)
    x = th.hand_rows(B, ns, T, seed=rate)
    seen = set()
    for t in range(T):
        a.rc.dtx_dev(to_dev(x[t]).data_ptr(), "f32")
        m.frame(x[t])
        assert_model(a.rc, m, f"{rate} Hz row {t}")
        seen |= set(m.report[on, 0].tolist())
    assert seen == {dm.FRAME, dm.SID, dm.NONE}, "the rows reach every decision"
    assert not m.report[[s for s in range(B) if s % 3 == 1]].any() and m.state[on, dm.W_FRAMES].min() > 30
    assert a.rc.kernel_times(("rate_dtx",))["rate_dtx"][1] == T
    a.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def as_format(x, kind, laws):
    """float rows -> the call's format, and the floats the stage sees"""
    if kind == "f32":
        return np.array(x, F32), np.array(x, F32)
    i16 = np.rint(np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=1.0, neginf=-1.0) * 32768).clip(-32768, 32767).astype(np.int16)
    rows = i16 if kind == "i16" else gm.encode_rows(laws, i16)
    return rows, dm.samples(rows, kind, laws)


@pytest.mark.parametrize("kind", ("i16", "g711"))
def test_a_mixed_converter_in_the_integer_formats(model, kind):
    import torch
    B, T = 7, 30
    a = Twin(model, B, "mixed")
    laws = [s % 2 for s in range(B)]
    m = dm.Dtx(B, a.ns())
    assert sorted(set(a.ns())) == [80, 160, 240, 320, 480] and a.w == 480
    enable(a, m, [0, 1, 2, 3, 4, 6], QUICK)
    ns = list(a.ns())
    decisions = set()
    for t in range(T):
        if t == 15:                                      # a rate change in the middle clears the slot: it starts again, at the new row length
            a.rc.set_stream_rates([2], [8000])
            ns[2] = 80
            m.ns[2] = 80
            m.clear([2])
            assert not a.rc.dtx_state()[2].any() and a.rc.dtx_state()[3].any()
        x = np.zeros((B, 480), F32)
        for s in range(B):
            x[s, :ns[s]] = th.hand_rows(B, ns[s], 40, seed=5)[t + 5, s]
        rows, seen = as_format(x, kind, laws)
        for s in range(B):                               # what lies behind a stream's own samples is never read
            rows[s, ns[s]:] = tpl.SENTINEL[kind]
        d = to_dev(rows)
        a.rc.dtx_dev(d.data_ptr(), kind)
        m.frame(seen)
        assert_model(a.rc, m, f"{kind} row {t}")
        assert same(to_host(a.ctx, d), rows), "the rows are only read"
        decisions |= set(m.report[[0, 1, 2, 3, 4, 6], 0].tolist())
    assert decisions == {dm.FRAME, dm.SID, dm.NONE} and not m.report[5].any() and not m.state[5].any()
    a.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_active_lists(model):
    B, T = 7, 12
    a = Twin(model, B, 16000)
    m = dm.Dtx(B, 160)
    enable(a, m, list(range(B)), QUICK)
    x = th.hand_rows(B, 160, 40, seed=11)
    lists = [None, [6, 0, 3], [], [5], None, [1, 2, 4], [], [0, 6, 5, 4, 3, 2, 1], [3], None, [2], None]
    for t in range(T):
        before = (a.rc.dtx_state(), report_words(a.rc))
        a.rc.dtx_dev(to_dev(x[t]).data_ptr(), "f32", ids=lists[t])
        m.frame(x[t], ids=lists[t])
        assert_model(a.rc, m, f"row {t}")
        off = [s for s in range(B) if lists[t] is not None and s not in lists[t]]
        for s in off:
            assert same(a.rc.dtx_state()[s], before[0][s]) and same(report_words(a.rc)[s], before[1][s]), f"row {t}: stream {s} is off the list"
    assert a.rc.kernel_times(("rate_dtx",))["rate_dtx"][1] == T - 2, "an empty list launches nothing"
    with pytest.raises(api.PercepNetError, match="listed twice"):
        a.rc.dtx_dev(to_dev(x[0]).data_ptr(), "f32", ids=[1, 1])
    with pytest.raises(api.PercepNetError, match="16-byte aligned"):
        a.rc.dtx_dev(to_dev(x[0]).data_ptr() + 4, "f32")
    assert_model(a.rc, m, "a refused call changes nothing")
    a.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def paused(kind, B, w, T):
    """speech-like rows with two pauses of low noise, in the call's format"""
    x = np.array(tpl.inputs("f32", B, w, seed=6, frames=T))
    rng = np.random.default_rng(77)
    for t in range(T):
        if 6 <= t < 16 or t >= 20:
            x[t] = (rng.standard_normal((B, w)) * 1e-4).astype(F32)
    if kind == "f32":
        return x
    i16 = np.rint(x.astype(np.float64) * 32768).clip(-32768, 32767).astype(np.int16)
    return i16 if kind == "i16" else np.stack([gm.encode_rows([s % 2 for s in range(B)], r) for r in i16])


@pytest.mark.parametrize("kind", ("f32", "i16", "g711"))
def test_the_frame_hook_reads_the_frames_own_output_rows(model, kind):
    B, T = 7, 26
    a, c = Twin(model, B, "mixed"), Twin(model, B, "mixed")
    m = dm.Dtx(B, a.ns())
    on = [0, 1, 2, 3, 4, 6]
    enable(a, m, on, HOOK)
    laws = [s % 2 for s in range(B)]
    x = paused(kind, B, a.w, T)
    decisions = set()
    for t in range(T):
        ids = None if t % 5 else [6, 4, 3, 2, 0]
        ga, gc = tpl.frame(a, kind, x[t], ids), tpl.frame(c, kind, x[t], ids)
        tpl.assert_frame(a, ga, gc, ids, f"{kind} frame {t}: the audio and g|r are the twin's,")
        m.frame(dm.samples(ga[0], kind, laws), ids=ids)
        assert_model(a.rc, m, f"{kind} frame {t}")
        decisions |= set(m.report[on, 0].tolist())
    assert decisions == {dm.FRAME, dm.SID, dm.NONE}
    ta, tc = a.rc.kernel_times(("rate_dtx", "rate_down")), c.rc.kernel_times(("rate_dtx", "rate_down"))
    assert ta["rate_dtx"][1] == T == ta["rate_down"][1], "one scope a frame"
    assert tc["rate_dtx"] == (0.0, 0) and not c.rc.dtx_state().any(), "nobody ever enabled: nothing is launched"
    a.close()
    c.close()


def test_the_frame_hook_on_the_pipelined_path(model):
    """two frames in flight: the report of every frame goes to device memory behind its submit, asynchronously, and is read at the end"""
    import torch
    B, T = 7, 26
    a, c = Twin(model, B, "mixed"), Twin(model, B, "mixed")
    m = dm.Dtx(B, a.ns())
    on = [0, 1, 2, 3, 4, 6]
    enable(a, m, on, HOOK)
    x = paused("f32", B, a.w, T)
    d_rep = dev_full((T, B, dm.REPORT_WORDS), torch.int32, -1)
    rot_a, rot_c = tp.Rot(a.ctx, 480, "f32", b=B), tp.Rot(c.ctx, 480, "f32", b=B)

    def submit_a(t, h_in, h_out, h_gr, h_rep):
        a.rc.submit_host_f32(h_in, h_out, h_gr)
        a.rc.read_dtx_report_dev(d_rep.data_ptr() + t * B * dm.REPORT_WORDS * 4)

    got = rot_a.run(x, submit_a)
    want = rot_c.run(x, lambda t, h_in, h_out, h_gr, h_rep: c.rc.submit_host_f32(h_in, h_out, h_gr))
    rep = to_host(a.ctx, d_rep).view(U32)
    for t in range(T):
        for s, n in enumerate(a.ns()):
            assert same(got[t][0][s, :n], want[t][0][s, :n]) and same(got[t][1][s], want[t][1][s]), f"frame {t} stream {s}: the twin's audio"
        m.frame(got[t][0])
        assert same(rep[t], m.report), f"frame {t}: report"
    assert same(a.rc.dtx_state(), m.state) and set(rep[:, on, 0].ravel().tolist()) == {dm.FRAME, dm.SID, dm.NONE}
    rot_a.free()
    rot_c.free()
    a.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_what_clears_the_state(model):
    B = 5
    a = Twin(model, B, "mixed")
    m = dm.Dtx(B, a.ns())
    every = list(range(B))
    enable(a, m, [0, 1, 2, 3], QUICK)
    tick = [0]

    def warm(what):
        for _ in range(3):
            x = np.zeros((B, 480), F32)
            for s in range(B):
                x[s, :m.ns[s]] = th.hand_rows(B, int(m.ns[s]), 40, seed=21)[tick[0] % 40, s]
            a.rc.dtx_dev(to_dev(x).data_ptr(), "f32")
            m.frame(x)
            tick[0] += 1
        assert_model(a.rc, m, what)
        return a.rc.dtx_state()

    def cleared(st, ids, what):
        now = a.rc.dtx_state()
        for s in every:
            assert (not now[s].any()) if s in ids else same(now[s], st[s]), f"{what}: stream {s}"
        m.clear(ids)

    st = warm("start")
    assert st[:4].any(axis=1).all() and not st[4].any(), "a stream that is off has no state"
    a.rc.set_stream_confs([0, 1], [0, 0])
    a.rc.set_mix_hold(0.5)
    a.rc.set_stream_dtx([4], 1)
    m.set_on([4], True)
    a.rc.set_stream_dtx([2], 1)                          # on while on: nothing
    cleared(st, [], "a conference change, a hold change, another stream's switch and a switch that is on already leave the state")
    st = warm("those")
    a.rc.set_stream_dtx([1], 0)
    a.rc.set_stream_dtx([1], 1)
    cleared(st, [1], "switching a stream on")
    st = warm("switching a stream on")
    a.rc.reset_streams([1, 3])
    cleared(st, [1, 3], "pn_rate_reset_streams")
    st = warm("pn_rate_reset_streams")
    a.rc.set_stream_rates([0, 4], [16000, 8000])
    m.ns[[0, 4]] = (160, 80)
    cleared(st, [0, 4], "pn_rate_set_stream_rates")
    st = warm("pn_rate_set_stream_rates")
    rec = a.rc.export_streams([2])
    a.rc.import_streams([2], rec)
    cleared(st, [2], "pn_rate_import_streams_host")
    st = warm("pn_rate_import_streams_host")
    d_rec, d_status = tp.dev_bytes((2, a.rc.record_stride()), 0xAB), tp.dev_i32(2)
    a.rc.export_streams_dev([3, 1], d_rec.data_ptr())
    a.rc.import_streams_dev([3, 1], d_rec.data_ptr(), d_status.data_ptr())
    cleared(st, [1, 3], "pn_rate_import_streams")
    st = warm("pn_rate_import_streams")
    a.rc.reset()
    cleared(st, every, "pn_rate_reset")
    warm("pn_rate_reset")
    assert a.rc.stream_dtx().tolist() == [1] * B and same(a.rc.dtx_params(), QUICK), "switches and parameters are settings"
    a.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_closed_loop_with_the_receive_side(model):
    """converter A's decisions drive converter B frame by frame: FRAME -> B receives A's output row; SID -> the SID is set, the stream
    is silent; NONE -> silent.  B generates comfort noise exactly where A decided SID or NONE"""
    Bn, T = 5, 80
    a, b = Twin(model, Bn, 8000), Twin(model, Bn, 8000)
    m = dm.Dtx(Bn, 80)
    enable(a, m, list(range(Bn)), HOOK)
    b.rc.set_cng(True)
    b.rc.set_cng_report(True)
    rng = np.random.default_rng(5)
    runs = np.zeros(Bn, np.int64)
    totals = np.zeros(Bn, np.int64)
    counts = np.zeros(3, np.int64)
    for t in range(T):
        x = (rng.standard_normal((Bn, 80)) * 1e-4).astype(F32)
        for s in range(Bn):
            if (t // (6 + s)) % 3 == 0:                  # talk spurts of a length per stream
                x[s] += (0.2 * np.sin(2 * np.pi * (0.02 + 0.01 * s) * (np.arange(80) + 80 * t))).astype(F32)
        ga = tpl.frame(a, "f32", x)
        m.frame(ga[0])
        assert_model(a.rc, m, f"frame {t}")
        rep = a.rc.read_dtx_report()
        sid = [s for s in range(Bn) if rep["decision"][s] == dm.SID]
        quiet = [s for s in range(Bn) if rep["decision"][s] != dm.FRAME]
        if sid:
            b.rc.set_stream_sid(sid, rep["sid"][sid])
            assert same(b.rc.stream_sids()[sid], rep["sid"][sid])
        if quiet:
            b.rc.set_silent(quiet)
        tpl.frame(b, "f32", ga[0])
        for s in range(Bn):
            runs[s] = runs[s] + 1 if s in quiet else 0
            totals[s] += s in quiet
            counts[rep["decision"][s]] += 1
        got = b.rc.read_cng_report()
        for s in range(Bn):
            assert got["total"][s] == totals[s] and (runs[s] == 0 or got["run"][s] == runs[s]), f"frame {t} stream {s}: B's runs are A's pauses"
    assert counts.min() > 0 and counts.sum() == Bn * T, counts
    a.close()
    b.close()
