"""Comfort noise on the rate converter (-m gpu): include/percepnet_hip.h "comfort noise"; kernel percepnet_amd/csrc/pn_rate_cng.hip, host
side pn_rate.cpp (pn_rate_set_cng / pn_rate_set_stream_sid / pn_rate_set_silent / pn_rate_cng_f32 and the hook in rate_frame), the rule
pn_cng_rules.h, bindings api.RateConverter.set_cng / set_stream_sid / set_silent / cng_f32_dev / read_cng_report.

The oracle of the noise is the numpy model tests/cng_model.py.  The contract of a whole frame: a silent frame is, bit for bit, the frame
of a FLOAT converter whose caller had supplied the model's noise row — so converter A marks streams silent (their input rows poisoned)
and converter B, which never enables the stage, is fed the model's rows as ordinary input.  The up-conversion behind the stand-alone
stage is checked against tests/rate_model.py at 8000 Hz.  rate_model's up_f32 states the integer factors of a single-rate converter only
(no 48000, no rational 32000, no factor per stream), so on the mixed converter the reference is NOT rate_model: it is the up kernel of a
second converter — unchanged by this stage and pinned by its own tests (test_gpu_rate*.py) — fed the model's rows over the same list.
Every comparison is equality of bits; no tolerance.

Shapes: 67 streams with 65 listed for the kernel alone — a second wavefront with one live lane; 7 streams over all five rates for
whole frames of 16: the engine's delay of six frames, a pause on frames 3 to 9, and the return to speech."""
import numpy as np
import pytest

from percepnet_amd import api
from tests import cng_model as cm
from tests import g711_model as gm
from tests import rate_model as rmod
from tests import test_gpu_plc as tpl
from tests import test_gpu_rate as tg
from tests import test_gpu_rate_pipe as tp

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED = 0xC0FFEE
T = 16
PAUSE = range(3, 10)
Twin, same, to_dev, to_host, dev_full = tpl.Twin, tpl.same, tg.to_dev, tg.to_host, tg.dev_full


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in tpl.families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


def sid_of(s, variant=0):
    """M in {0, 1, 12} and every fourth stream at the extreme coefficients; levels from the loudest to the quietest"""
    rng = np.random.default_rng(9000 + 7 * s + variant)
    M = (0, 1, 12)[(s + variant) % 3]
    N = [(0, 254)[(i + s) % 2] for i in range(M)] if s % 4 == 0 else rng.integers(0, 255, M).tolist()
    if s % 8 == 2:
        N = [0] * M
    if s % 8 == 6:
        N = [254] * M
    return cm.sid((20, 0, 127, 45, 60, 1, 126)[(s + variant) % 7], N)


def cng_on(tw, seed=SEED):
    tw.rc.set_cng(True)
    tw.rc.set_cng_seed(seed)
    sids = np.stack([sid_of(s) for s in range(tw.B)])
    tw.rc.set_stream_sid(list(range(tw.B)), sids)
    m = cm.Cng(tw.B, tw.ns(), seed)
    m.set_sid(list(range(tw.B)), sids)
    return m


def low_rows(tw, ids, rows):
    """the model's rows of the streams ids as input rows [B][w] of the converter, zeros elsewhere"""
    x = np.zeros((tw.B, tw.w), F32)
    for i, s in enumerate(ids):
        x[s, :tw.ns()[s]] = rows[i, :tw.ns()[s]]
    return x


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", (8000, "mixed"), ids=str)
def test_the_stage_alone_is_the_model_through_the_up_conversion(model, case):
    import torch
    B = 67
    a, b = Twin(model, B, case), Twin(model, B, case)
    m = cng_on(a)
    a.rc.set_cng_report(True)
    assert a.rc.cng_seed() == SEED and same(a.rc.stream_sids(), m.sids)
    listed = [s for s in reversed(range(B)) if s not in (5, 40)]
    assert len(listed) == 65
    up = rmod.Up(B, 6, tg.taps(8000)[0]) if case == 8000 else None
    for t in range(8):
        if t == 4:                                       # a SID change inside the run: the gain ramps across this row
            ch = [s for s in range(B) if s % 2]
            sids = np.stack([sid_of(s, 1) for s in ch])
            a.rc.set_stream_sid(ch, sids)
            m.set_sid(ch, sids)
        x48 = dev_full((B, 480), torch.float32, 777.0)
        a.rc.cng_f32_dev(x48.data_ptr(), ids=listed)
        got = to_host(a.ctx, x48).copy()
        low = low_rows(a, listed, m.frame(listed))
        assert np.isfinite(low).all() and np.count_nonzero(low[listed[0]]) > 0
        if up is not None:
            want = up(low)
        else:
            y48 = dev_full((B, 480), torch.float32, 777.0)
            b.rc.up_f32_dev(to_dev(low).data_ptr(), y48.data_ptr(), ids=listed)
            want = to_host(b.ctx, y48).copy()
        for s in range(B):
            if s in listed:
                assert same(got[s], want[s]), f"{case} row {t} stream {s}"
            else:
                assert (got[s] == 777.0).all(), f"{case} row {t}: the row of unlisted stream {s} is untouched"
        assert same(a.rc.debug_cng_state(), m.state), f"{case} row {t}: state"
        assert same(a.rc.read_cng_report().view(np.uint32).reshape(B, 4), m.report), f"{case} row {t}: report"
    rep = a.rc.read_cng_report()
    assert rep["run"][listed].tolist() == [8] * 65 and rep["total"][[5, 40]].tolist() == [0, 0]
    times = a.rc.kernel_times(("rate_cng", "rate_up"))
    assert times["rate_cng"][1] == 8 and times["rate_up"][1] == 8
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def script(mode, B):
    """-> per frame: (silent streams, lost streams, the id list or None).  Stream 4 leaves the list on frame 5 of the "active" script
    with its mark set (the mark is dropped, its run ends); stream 2 is lost on frame 10, right behind its pause, and on frame 6 lost AND
    silent (lost wins) in the "plc_conf" script"""
    silent = {1, 2, 3, 4, 6}
    rows = []
    for t in range(T):
        sil = sorted(silent) if t in PAUSE else []
        lost, ids = [], None
        if mode == "active":
            ids = [s for s in (6, 0, 5, 4, 3, 2, 1) if not (s == 4 and t == 5) and not (s == 0 and t % 4 == 3)]
        if mode == "plc_conf":
            lost = [2] if t in (6, 10) else []
        rows.append((sil, lost, ids))
    return rows


def run_twin(model, mode, kind="f32"):
    """-> per frame (A's rows, B's rows, ids, who was generated): A marks, B is fed the model's rows"""
    B = 7
    plc = mode == "plc_conf"
    a, b = Twin(model, B, "mixed", plc=plc), Twin(model, B, "mixed", plc=plc)
    m = cng_on(a)
    if mode == "plc_conf":
        for tw in (a, b):
            tw.rc.set_stream_confs([0, 1, 2, 5], [0, 0, 0, 0])
    x = tpl.inputs(kind, B, a.w, seed=3, frames=T)
    laws = [s % 2 for s in range(B)]
    res = []
    for t, (sil, lost, ids) in enumerate(script(mode, B)):
        if t == 6:                                       # a SID change inside the pause
            a.rc.set_stream_sid([1, 6], np.stack([sid_of(1, 1), sid_of(6, 1)]))
            m.set_sid([1, 6], np.stack([sid_of(1, 1), sid_of(6, 1)]))
        adv = list(range(B)) if ids is None else ids
        gen = [s for s in adv if s in sil and s not in lost]
        noise = low_rows(a, gen, m.frame(gen))
        xa = tpl.poison(x[t], sil, kind)
        xb = np.array(x[t]) if kind == "f32" else rmod.from_i16(x[t] if kind == "i16" else gm.decode_rows(laws, x[t]))
        for s in gen:
            xb[s] = noise[s]
        if sil:
            a.rc.set_silent(sil)
        for tw in (a, b):
            if lost:
                tw.rc.set_lost(lost)
        res.append((tpl.frame(a, kind, xa, ids), tpl.frame(b, "f32", xb, ids), adv, gen))
    st = a.rc.debug_cng_state()
    a.close()
    b.close()
    return res, st, m


@pytest.mark.parametrize("mode", ("sync", "active", "plc_conf"))
def test_a_silent_frame_is_the_frame_of_a_converter_fed_the_models_row(model, mode):
    res, st, m = run_twin(model, mode)
    ns = [api.rate_mixed_frame_samples(r) for r in [tpl.MIXED_RATES[s % 5] for s in range(7)]]
    for t, (ga, gb, adv, gen) in enumerate(res):
        for s in adv:
            assert same(ga[0][s, :ns[s]], gb[0][s, :ns[s]]), f"{mode} frame {t} stream {s}"
            assert same(ga[1][s], gb[1][s]), f"{mode} frame {t} g|r of stream {s}"
    assert same(st, m.state), "the state behind the script is the model's"
    assert all(len(r[3]) > 0 for r in res[3:10]) and not any(r[3] for r in res[:3] + res[10:])
    if mode == "plc_conf":
        assert 2 not in res[6][3] and st[2, cm.W_TOTAL] == 6, "lost wins: the row of frame 6 was concealed, not generated"
    if mode == "active":
        assert 4 not in res[5][3] and st[4, cm.W_RUN] == 4 and st[4, cm.W_TOTAL] == 6, "a mark off the list is dropped and ends the run"


def test_marks_and_a_sid_change_between_submits_on_the_pipelined_path(model):
    B = 7
    want, _, _ = run_twin(model, "sync")
    p = Twin(model, B, "mixed")
    m = cng_on(p)
    x = tpl.inputs("f32", B, p.w, seed=3, frames=T)
    sc = script("sync", B)
    xs = np.stack([tpl.poison(x[t], sc[t][0], "f32") for t in range(T)])
    rot = tp.Rot(p.ctx, 480, "f32", b=B)

    def submit(t, h_in, h_out, h_gr, h_rep):
        if t == 6:
            p.rc.set_stream_sid([1, 6], np.stack([sid_of(1, 1), sid_of(6, 1)]))   # no wait before or after
        if sc[t][0]:
            p.rc.set_silent(sc[t][0])
        p.rc.submit_host_f32(h_in, h_out, h_gr)

    got = rot.run(xs, submit)
    for t in range(T):
        for s, n in enumerate(p.ns()):
            assert same(got[t][0][s, :n], want[t][0][0][s, :n]) and same(got[t][1][s], want[t][0][1][s]), f"frame {t} stream {s}"
    rot.free()
    p.close()


@pytest.mark.parametrize("kind", ("i16", "g711"))
def test_integer_and_g711_rows(model, kind):
    """the silent streams against converter B's float rows through the cast and the companding; the others against a converter that
    never enables the stage"""
    B = 7
    res, _, _ = run_twin(model, "sync", kind)
    c = Twin(model, B, "mixed")
    x = tpl.inputs(kind, B, c.w, seed=3, frames=T)
    laws = [s % 2 for s in range(B)]
    for t, (ga, gb, adv, gen) in enumerate(res):
        gc = tpl.frame(c, kind, x[t])
        for s, n in enumerate(c.ns()):
            if s in (0, 5):
                assert same(ga[0][s, :n], gc[0][s, :n]) and same(ga[1][s], gc[1][s]), f"{kind} frame {t}: stream {s} is never silent"
            i16 = rmod.to_i16(gb[0][s, :n], False)
            assert same(ga[0][s, :n], i16 if kind == "i16" else gm.encode(laws[s], i16)), f"{kind} frame {t} stream {s}"
            assert same(ga[1][s], gb[1][s])
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_off_means_off(model):
    B = 7
    a, c = Twin(model, B, "mixed"), Twin(model, B, "mixed")
    cng_on(a)
    a.rc.set_cng_report(True)
    x = tpl.inputs("f32", B, a.w, seed=4, frames=4)
    for t in range(4):
        ga, gc = tpl.frame(a, "f32", x[t]), tpl.frame(c, "f32", x[t])
        tpl.assert_frame(a, ga, gc, None, f"frame {t}:")
    ta, tc = a.rc.kernel_times(("rate_cng", "rate_up", "rate_down")), c.rc.kernel_times(("rate_cng", "rate_up", "rate_down"))
    assert ta["rate_cng"] == (0.0, 0) and tc["rate_cng"] == (0.0, 0), "nobody marked: the kernel is not launched"
    assert ta["rate_up"][1] == tc["rate_up"][1] == 4 and ta["rate_down"][1] == 4, "one up-conversion a frame"
    assert not a.rc.debug_cng_state().any() and a.rc.read_cng_report().tolist() == [(0, 0, 0.0, 0)] * B
    a.rc.set_cng(False)
    with pytest.raises(api.PercepNetError, match="comfort noise is off"):
        a.rc.set_silent([1])
    with pytest.raises(api.PercepNetError, match="comfort noise is off"):
        a.rc.cng_f32_dev(dev_full((B, 480), __import__("torch").float32, 0.0).data_ptr())
    with pytest.raises(api.PercepNetError, match="comfort noise is off"):
        c.rc.set_silent([1])
    a.close()
    c.close()


def test_a_loud_silent_stream_reports_no_digit(model):
    """L = 20 white noise, the loud case, under the DTMF detector for 12 frames"""
    B = 3
    a = Twin(model, B, 8000)
    a.rc.set_cng(True)
    a.rc.set_stream_sid([0, 1, 2], np.stack([cm.sid(20)] * 3))
    a.rc.set_stream_dtmf([0, 1, 2], [1, 1, 1])
    a.rc.set_dtmf_report(True)
    x = np.zeros((B, a.w), F32)
    for t in range(12):
        a.rc.set_silent([0, 2])
        tpl.frame(a, "f32", x)
        rep = a.rc.read_dtmf_report()
        assert ((rep["word0"] >> 8) == 0).all() and (rep["count"] == 0).all(), f"frame {t}: no digit"
    assert a.rc.debug_cng_state()[:, cm.W_TOTAL].tolist() == [12, 0, 12]
    a.close()


def test_what_clears_the_state(model):
    """Each event of the clear list zeroes the listed streams' device state AND the host's knowledge of their runs (whether a row
    continues a run is the host's): the row behind the event is the first of a run (run 1, gain g without a ramp from a prev of 0)
    while every other stream's run goes on.  The tails import in both forms, host and device"""
    import torch
    B = 5
    a = Twin(model, B, "mixed")
    m = cng_on(a)
    a.rc.set_cng_report(True)
    every = list(range(B))

    def warm(what):
        x48 = dev_full((B, 480), torch.float32, 0.0)
        a.rc.cng_f32_dev(x48.data_ptr())
        m.frame(every)
        st = a.rc.debug_cng_state()
        assert same(st, m.state), f"{what}: the rows behind it are the model's, ramp and run included"
        assert same(a.rc.read_cng_report().view(np.uint32).reshape(B, 4), m.report), what
        return st

    def cleared(st, ids, what):
        now = a.rc.debug_cng_state()
        for s in every:
            assert (not now[s].any()) if s in ids else same(now[s], st[s]), f"{what}: stream {s}"
        m.clear(ids)

    st = warm("start")
    a.rc.set_stream_confs([0, 1], [0, 0])
    sid = np.stack([cm.sid(30, [100, 200])])
    a.rc.set_stream_sid([2], sid)
    m.set_sid([2], sid)
    cleared(st, [], "a conference change and a SID change leave the state")
    a.rc.reset_streams([1, 3])
    cleared(st, [1, 3], "pn_rate_reset_streams")
    st = warm("pn_rate_reset_streams")
    assert st[:, cm.W_RUN].tolist() == [2, 1, 2, 1, 2]
    a.rc.set_stream_rates([0, 4], [16000, 8000])
    m.ns[[0, 4]] = (160, 80)
    cleared(st, [0, 4], "pn_rate_set_stream_rates")
    st = warm("pn_rate_set_stream_rates")
    assert st[:, cm.W_RUN].tolist() == [1, 2, 3, 2, 1]
    rec = a.rc.export_streams([2])
    a.rc.import_streams([2], rec)
    cleared(st, [2], "pn_rate_import_streams_host")
    st = warm("pn_rate_import_streams_host")
    assert st[:, cm.W_RUN].tolist() == [2, 3, 1, 3, 2]
    d_rec, d_status = tp.dev_bytes((2, a.rc.record_stride()), 0xAB), tp.dev_i32(2)
    a.rc.export_streams_dev([3, 1], d_rec.data_ptr())
    a.rc.import_streams_dev([3, 1], d_rec.data_ptr(), d_status.data_ptr())
    cleared(st, [1, 3], "pn_rate_import_streams")
    assert to_host(a.ctx, d_status).tolist() == [api.SS_OK] * 2
    st = warm("pn_rate_import_streams")
    assert st[:, cm.W_RUN].tolist() == [3, 1, 2, 1, 3]
    a.rc.reset()
    cleared(st, every, "pn_rate_reset")
    st = warm("pn_rate_reset")
    assert st[:, cm.W_RUN].tolist() == [1] * B
    a.rc.set_cng(False)
    a.rc.set_cng(True)
    cleared(st, every, "on again")
    m.tick += 1                                          # (disabling drops the marks like a frame: the tick moves on)
    st = warm("on again")
    assert st[:, cm.W_RUN].tolist() == [1] * B and st[:, cm.W_TOTAL].tolist() == [1] * B
    a.close()
