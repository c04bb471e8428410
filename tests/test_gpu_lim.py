"""Output limiter on the rate converter (-m gpu): include/percepnet_hip.h "output limiter"; kernel percepnet_amd/csrc/pn_rate_lim.hip,
host side pn_rate.cpp (pn_rate_set_stream_limiter / pn_rate_set_limiter_params / pn_rate_lim_f32 and the hook in rate_frame), the rule
pn_lim_rules.h, bindings api.RateConverter.set_stream_limiter / set_limiter_params / lim_f32_dev / read_limiter_report.

The oracle is the numpy float32 model tests/lim_model.py: alone for the kernel, and for whole frames inside the composition
pn_rate_up_* -> [the PLC model's row] -> pn_process_f32[_active] -> [the AGC model] -> [pn_rate_mix_f32] -> the limiter model on the
host -> pn_rate_down_* on a SECOND context and converter that never sets a ceiling.  Every comparison is equality of bits; no tolerance.
The device's state words have no reader of their own: the report row carries the gain and the limited count of every frame, and the
hold count shows in the flags of the frames that follow (HOLDING, then RELEASING), which are compared frame by frame.

Shapes: contexts of 3 and 19 streams, neither a multiple of the kernel's four rows a block, so the last block is partial, and with the
mixed ceilings one block holds rows that are off, attacking, holding, releasing and non-finite at the same time.  Whole-frame tests
run 12 frames: six of the engine's delay and six of signal."""
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import agc_model as am
from tests import lim_model as lm
from tests import plc_model as pm
from tests import test_gpu_agc as ta
from tests import test_gpu_plc as tq
from tests import test_gpu_rate_pipe as tp
from tests.test_agc_host import hostile_rows, voice

pytestmark = pytest.mark.gpu
F32 = np.float32
BS = (3, 19)
T = 12
KT = 40
SENT = 777.0
D = lm.DEFAULTS
FAMILIES = ("rate_up", "rate_down", "rate_mix", "rate_plc", "rate_agc", "rate_lim")
Twin, inputs, frame, assert_frame, same, to_dev, to_host, dev_full, torch_dtype, SENTINEL = (
    tq.Twin, tq.inputs, tq.frame, tq.assert_frame, tq.same, tq.to_dev, tq.to_host, tq.dev_full, tq.torch_dtype, tq.SENTINEL)
model = tq.model
default_families = tq.default_families
conf_setup = ta.conf_setup


def ceilings_of(B):
    """mixed ceilings, 0 (not limited) among them"""
    return [(0.05, 0.0, 0.5, 0.02, 1.0, 0.0, 1.0 / 1024.0)[s % 7] for s in range(B)]


def lim_twin(model, B, case="mixed", ceilings=None, plc=False, report=True):
    tw = Twin(model, B, case, plc=plc)
    tw.rc.set_limiter_report(report)
    tw.rc.set_stream_limiter(list(range(B)), ceilings_of(B) if ceilings is None else ceilings)
    return tw


def lim_model(B, ceilings=None, params=None):
    m = lm.Lim(B, params)
    m.set_ceilings(range(B), ceilings_of(B) if ceilings is None else ceilings)
    return m


def assert_report(tw, m, what):
    rep = tw.rc.read_limiter_report()
    assert rep.tobytes() == m.report.tobytes(), f"{what}: report\n{rep}\n{m.report}"


def launches(tw, name="rate_lim"):
    return tw.rc.kernel_times((name,))[name][1]


def composed(tw, lim, kind, x, ids=None, mix=False, agc=None, plc=None, lost=()):
    """The same frame by hand on a twin without a ceiling (and without AGC or PLC): up, [the PLC model's frame on the host rows], the
    engine, [the AGC model's frame on the host], [the mix kernel], the limiter model's frame on the host, down -> (out rows, g|r)"""
    import torch
    nan = float("nan")
    adv = list(range(tw.B)) if ids is None else list(ids)
    up = [s for s in adv if s not in lost]
    d_in = to_dev(np.array(x))
    x48, y48, d_gr = dev_full((tw.B, 480), torch.float32, nan), dev_full((tw.B, 480), torch.float32, nan), dev_full((tw.B, 68), torch.float32, nan)
    if len(up) == tw.B:
        getattr(tw.rc, f"up_{kind}_dev")(d_in.data_ptr(), x48.data_ptr())
    elif up:
        getattr(tw.rc, f"up_{kind}_dev")(d_in.data_ptr(), x48.data_ptr(), ids=up)
    if plc is not None:
        x48 = to_dev(plc.frame(to_host(tw.ctx, x48).copy(), lost=lost, ids=ids))
    if ids is None:
        tw.ctx.process_f32_dev(x48.data_ptr(), y48.data_ptr(), d_gr.data_ptr())
    else:
        tw.ctx.process_f32_active_dev(x48.data_ptr(), y48.data_ptr(), d_gr.data_ptr(), ids)
    o48 = y48
    if agc is not None:
        o48 = to_dev(agc.frame(to_host(tw.ctx, y48).copy(), ids=ids, concealed=lost))
    if mix:
        y48 = o48
        o48 = dev_full((tw.B, 480), torch.float32, nan)
        tw.rc.mix_f32_dev(y48.data_ptr(), o48.data_ptr(), ids=ids)
    o48 = to_dev(lim.frame(to_host(tw.ctx, o48).copy(), ids=ids))
    d_out = dev_full((tw.B, tw.w), torch_dtype(kind), SENTINEL[kind])
    getattr(tw.rc, f"down_{kind}_dev")(o48.data_ptr(), d_out.data_ptr(), ids=ids)
    return to_host(tw.ctx, d_out).copy(), to_host(tw.ctx, d_gr).copy()


# ---------------------------------------------------------------------------------------------------------------- 1
_kernel_rows = {}


def kernel_rows(B):
    """[KT, B, 480]: per stream a voice at its own level whose loudness rises over the frames and bursts at its own frames, so that the
    streams cross their ceilings at different frames and indices, with one hostile row per frame from frame 3 on, walking over the streams"""
    if B not in _kernel_rows:
        rows = np.empty((KT, B, 480), F32)
        t = np.arange(KT)
        for s in range(B):
            v = voice(0.004 * (1 + s % 5), KT, f0=100.0 + 9.0 * s)
            env = (1.0 + t / 8.0) * np.where((t + 3 * s) % 13 == 0, 12.0, 1.0) * np.where((t // 6 + s) % 3 == 0, 0.2, 1.0)
            rows[:, s] = v * env.astype(F32)[:, None]
        h = list(hostile_rows().values())
        for f in range(3, KT):
            rows[f, (5 * f) % B] = h[f % len(h)]
        rows.setflags(write=False)
        _kernel_rows[B] = rows
    return _kernel_rows[B]


@pytest.mark.parametrize("B", BS)
def test_the_kernel_alone_against_the_model(model, B):
    tw, m = lim_twin(model, B), lim_model(B)
    x = kernel_rows(B)
    seen, ks = 0, set()
    rng = np.random.default_rng(78)
    for t in range(KT):
        ids = None
        if t % 4 == 2:                                                   # an ids list shorter than B, in any order; the others keep rows, states, report rows
            ids = [int(v) for v in rng.permutation(B)[:max(1, B - 1 - t % 3)]]
        if t == 15:                                                      # a parameter change between two frames
            p = np.array([1.5, 1.0], F32)
            tw.rc.set_limiter_params(p)
            m.params = p
            assert same(tw.rc.limiter_params(), p)
        if t == 25:                                                      # a ceiling change: the state stays
            chg, new = [0, B - 1, 1], [0.0, 0.3, 0.01]
            tw.rc.set_stream_limiter(chg, new)
            m.set_ceilings(chg, new)
        rows = np.array(x[t])
        for s in range(B):
            if m.ceilings[s] == 0 or (ids is not None and s not in ids):
                rows[s] = SENT                                           # a sentinel where nothing may be read as a sample or written
        d = to_dev(rows)
        tw.rc.lim_f32_dev(d.data_ptr(), ids=ids)
        got = to_host(tw.ctx, d)
        want = m.frame(rows, ids=ids)
        for s in range(B):
            assert same(got[s], want[s]), f"frame {t} stream {s} (ceiling {m.ceilings[s]}, listed {ids is None or s in ids}, flags {m.report[s]['flags']}, k {m.k[s]})"
            if m.ceilings[s] == 0 or (ids is not None and s not in ids):
                assert (got[s] == F32(SENT)).all()
        assert_report(tw, m, f"frame {t}")
        for s in range(B) if ids is None else ids:
            seen |= int(m.report[s]["flags"])
            ks.add(int(m.k[s]))
    assert seen == lm.ON | lm.ATTACK | lm.HOLDING | lm.RELEASING | lm.ACTIVE | lm.NONFINITE, f"every flag ({seen})"
    assert len(ks - {-1}) >= 3, f"attacks at several indices ({sorted(ks)})"
    g = m.gains()
    on = [s for s in range(B) if m.ceilings[s] != 0]
    assert (g[on] > 0).all() and (g[on] <= 1).all() and len(set(g[on].tolist())) > 1
    assert same(tw.rc.stream_limiter(), m.ceilings) and launches(tw) == KT
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("B,case,kind,mode,agc", ((3, 8000, "f32", "none", False), (3, 32000, "g711", "conf", False), (19, "mixed", "i16", "conf", True),
                                                  (19, "mixed", "f32", "loudest", True), (19, "mixed", "g711", "none", False), (19, 32000, "i16", "loudest", False),
                                                  (19, 8000, "i16", "conf", True)), ids=str)
def test_whole_frame_against_the_composition(model, B, case, kind, mode, agc):
    a, b, plain = lim_twin(model, B, case), Twin(model, B, case), Twin(model, B, case)
    conf_setup((a, b, plain), B, mode)
    m = lim_model(B)
    agc_m = None
    if agc:                                                              # targets high enough that a sum of levelled voices passes the members' ceilings
        targets, p = [0.3] * B, am.DEFAULTS.copy()
        p[am.STEP_UP] = 2.0                                              # the gain may double per frame: levelled within the six frames of signal
        a.rc.set_agc(True)
        a.rc.set_agc_params(p)
        a.rc.set_stream_agc_targets(list(range(B)), targets)
        agc_m = ta.agc_model(B, targets, p)
    x = inputs(kind, B, a.w, 21)
    rng = np.random.default_rng(6)
    differs, attacked, flags = False, set(), 0
    for t in range(T):
        ids = sorted(int(v) for v in rng.permutation(B)[:B - 1]) if t in (8, 10) else None        # the _active entry points
        got = frame(a, kind, x[t], ids)
        want = composed(b, m, kind, x[t], ids, mix=mode != "none", agc=agc_m)
        assert_frame(a, got, want, ids, f"{case} {kind} {mode} frame {t}:")
        if ids is None:
            assert_report(a, m, f"frame {t}")
        for s in range(B) if ids is None else ids:
            flags |= int(m.report[s]["flags"])
            if m.report[s]["flags"] & lm.ATTACK:
                attacked.add(s)
        differs |= agc or not same(got[0], frame(plain, kind, x[t], ids)[0])
    print(f"{case} {kind} {mode} agc {agc}: attacked {sorted(attacked)}, flags {flags}, gains {m.gains().tolist()}")
    assert attacked, "at least one row attacked: the case does not pass vacuously"
    if agc and mode != "none":
        confs = a.rc.stream_confs()
        assert any(confs[s] != api.CONF_NONE and m.ceilings[s] >= 0.5 for s in attacked), "a mix of levelled voices passed a member's ceiling of 0.5 or 1"
    assert differs, "the limited output is not the plain one"
    assert launches(a) == T and launches(b) == 0
    for tw in (a, b, plain):
        tw.close()


def test_whole_frame_with_the_concealer_and_an_active_list(model):
    B = 3
    ceil = [0.02, 0.0, 0.05]
    a, b = lim_twin(model, B, 16000, ceilings=ceil, plc=True), Twin(model, B, 16000)
    m, plc = lim_model(B, ceil), pm.Plc(B)
    x = inputs("i16", B, a.w, 23, 14)
    losses = {8: [0], 9: [0], 11: [2]}
    for t in range(14):
        lost = losses.get(t, [])
        ids = [0, 2] if t == 12 else None
        rows = tq.poison(x[t], lost, "i16")
        tq.mark(a.rc, lost)
        got = frame(a, "i16", rows, ids)
        want = composed(b, m, "i16", rows, ids, plc=plc, lost=lost)
        assert_frame(a, got, want, ids, f"frame {t}:")
    assert m.state["limited"][0] > 0 and m.state[1].tobytes() == bytes(16)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_pipelined_path_with_a_setting_call_between_two_submits(model):
    B = 19
    x = inputs("i16", B, 480, 22)
    rng = np.random.default_rng(57)
    ids_at = [None if t % 3 else sorted(int(v) for v in rng.permutation(B)[:B - 2]) for t in range(T)]

    def settings(tw, t):
        if t == 7:
            tw.rc.set_stream_limiter([1, 4, 5], [0.5, 0.0, 0.003])
        if t == 9:
            tw.rc.set_limiter_params(np.array([2.0, 0.0], F32))
        if t == 10:
            tw.rc.set_stream_limiter([1, 2], [0.004, 0.0])

    sync = lim_twin(model, B)
    want = []
    for t in range(T):
        settings(sync, t)
        want.append(frame(sync, "i16", x[t], ids_at[t]))
    plain = Twin(model, B)
    differs = [not same(want[t][0], frame(plain, "i16", x[t], ids_at[t])[0]) for t in range(T)]
    assert any(differs[6:]), "the ceilings act on these rows"
    sync.close()
    plain.close()
    p = lim_twin(model, B)
    rot = tp.Rot(p.ctx, 480, "i16", b=B)

    def submit(t, h_in, h_out, h_gr, h_rep):
        settings(p, t)                                                   # no wait before or after
        p.rc.submit_host_i16(h_in, h_out, h_gr, ids=ids_at[t])

    got = rot.run(np.array(x), submit)
    for t in range(T):
        for s in range(B) if ids_at[t] is None else ids_at[t]:
            n = tq.nof(p.rates[s])
            assert same(got[t][0][s, :n], want[t][0][s, :n]) and same(got[t][1][s], want[t][1][s]), f"frame {t} stream {s}"
    assert p.ctx.frames_delivered() == T and launches(p) == T
    p.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("B", BS)
def test_nothing_new_while_off(model, B):
    never, plain = Twin(model, B, "mixed"), Twin(model, B, "mixed")
    zero = Twin(model, B, "mixed")
    zero.rc.set_limiter_report(True)
    zero.rc.set_stream_limiter([0, B - 1], [0.5, 0.01])                  # ceilings, and every one of them 0 again
    zero.rc.set_limiter_params(np.array([1.5, 7.0], F32))
    zero.rc.set_stream_limiter([B - 1, 0], [0.0, -0.0])
    conf_setup((never, plain, zero), B, "conf")
    n = 0
    for kind in ("f32", "i16", "g711"):
        x = inputs(kind, B, 480, 24, 8)
        for t in range(8):
            want = frame(plain, kind, x[t])
            for tw, what in ((never, "never set"), (zero, "every ceiling 0 again")):
                assert_frame(tw, frame(tw, kind, x[t]), want, None, f"{what}: {kind} frame {t}:")
            n += 1
    for tw in (never, zero):
        times = tw.rc.kernel_times(FAMILIES)
        assert times["rate_lim"] == (0.0, 0), "no ceiling, no launch"
        for name in FAMILIES[:-1]:
            assert times[name][1] == launches(plain, name), name
    assert launches(plain, "rate_up") == launches(plain, "rate_down") == launches(plain, "rate_mix") == n
    assert not np.signbit(zero.rc.stream_limiter()).any() and (zero.rc.stream_limiter() == 0).all()
    # with one ceiling set a frame launches the kernel once, and nothing else more
    zero.rc.set_stream_limiter([1], [1.0])
    frame(zero, "f32", inputs("f32", B, 480, 24, 8)[0])
    assert launches(zero) == 1 and launches(zero, "rate_down") == n + 1 and launches(zero, "rate_mix") == n + 1
    for tw in (never, plain, zero):
        tw.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_refusals_change_nothing(model):
    B = 3
    tw = Twin(model, B, 8000)
    d = to_dev(np.zeros((B, 480), F32))
    assert same(tw.rc.limiter_params(), D) and same(tw.rc.stream_limiter(), np.zeros(B, F32))
    with pytest.raises(api.PercepNetError, match="pn_rate_set_limiter_report"):
        tw.rc.read_limiter_report()
    tw.rc.set_limiter_report(True)
    tw.rc.set_stream_limiter([2, 0], [0.2, -0.0])
    # a frame of state to lose: stream 2 attacks
    rows = np.stack([voice(0.3, 1)[0]] * B)
    d_rows = to_dev(rows)
    tw.rc.lim_f32_dev(d_rows.data_ptr())
    rep = tw.rc.read_limiter_report()
    assert rep[2]["flags"] == lm.ON | lm.ATTACK | lm.ACTIVE and rep[0].tolist() == (1.0, 0.0, 0, 0)
    before = launches(tw)
    for ids, c, word in (([B], [0.1], "out of range"), ([-1], [0.1], "out of range"), ([1, 1], [0.1, 0.1], "twice"), ([0, 1], [0.1, np.nan], "index 1"),
                         ([1], [1.5], "index 0"), ([1], [-0.1], "index 0"), ([0, 1, 2], [0.5, 0.5, 0.0009], "index 2")):
        with pytest.raises(api.PercepNetError, match=word):
            tw.rc.set_stream_limiter(ids, c)
    tw.rc.set_stream_limiter([], [])
    got = tw.rc.stream_limiter()
    assert same(got, np.array([0.0, 0.0, 0.2], F32)) and not np.signbit(got[0])
    for p, word in (([0.5, 2.0], r"index 0 \(release\)"), ([1.5, 2.5], r"index 1 \(hold\)"), ([np.nan, -1.0], r"index 0 \(release\)"), ([1.0, 1001.0], r"index 1 \(hold\)")):
        with pytest.raises(api.PercepNetError, match=word):
            tw.rc.set_limiter_params(np.array(p, F32))
    assert same(tw.rc.limiter_params(), D)
    with pytest.raises(api.PercepNetError, match="aligned"):
        tw.rc.lim_f32_dev(d.data_ptr() + 4)
    with pytest.raises(api.PercepNetError, match="twice"):
        tw.rc.lim_f32_dev(d.data_ptr(), ids=[1, 1])
    with pytest.raises(api.PercepNetError, match="rate_lim"):
        tw.rc.kernel_times(("rate_xyz",))
    assert launches(tw) == before == 1
    # the state and the settings are what they were: the next frame is the model's second frame
    m = lim_model(B, [0.0, 0.0, 0.2])
    m.frame(rows)
    quiet = np.stack([voice(0.01, 1)[0]] * B)
    d_q = to_dev(quiet)
    tw.rc.lim_f32_dev(d_q.data_ptr())
    assert same(to_host(tw.ctx, d_q), m.frame(quiet))
    assert_report(tw, m, "behind the refusals")
    assert m.report[2]["flags"] == lm.ON | lm.HOLDING | lm.ACTIVE
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("form", ("host", "dev"))
def test_lifecycle_gives_the_listed_slots_a_fresh_state(model, form):
    import torch
    B = 19
    ceil = [0.05] * B
    tw, m = lim_twin(model, B, "mixed", ceilings=ceil), lim_model(B, ceil)
    # the first frame attacks everywhere; the quiet frames behind it hold and release, so a fresh state (gain 1, the row kept) shows
    x = np.stack([voice(0.004 * (s + 1), 30, f0=110.0 + 7 * s) for s in range(B)], axis=1)
    x[0] *= F32(40.0)
    t = 0

    def tick(ids=None):
        nonlocal t
        d = to_dev(np.array(x[t]))
        tw.rc.lim_f32_dev(d.data_ptr(), ids=ids)
        want = m.frame(x[t], ids=ids)
        got = to_host(tw.ctx, d)
        for s in range(B) if ids is None else ids:
            assert same(got[s], want[s]), f"tick {t} stream {s}"
        assert_report(tw, m, f"tick {t}")
        t += 1

    for _ in range(3):
        tick()
    assert (m.gains() < 1.0).all() and (m.state["hold"] == 0).all(), "every stream has left the fresh gain"
    tw.rc.reset_streams([1, 4])
    m.reset([1, 4])
    tick()
    assert m.state["limited"][1] < m.state["limited"][0]
    tick(ids=[0, 1, 2])                                                  # a stream that does not advance keeps its state
    tw.rc.set_stream_rates([2, 7], [16000, 48000])
    m.reset([2, 7])
    tick()
    eight = [s for s in range(B) if tw.rates[s] == 8000][:3]
    if form == "host":
        tw.rc.import_streams(eight[1:], tw.rc.export_streams([eight[0]] * 2))
    else:
        stride = tw.rc.record_stride()
        d_rec, d_st = dev_full((2, stride), torch.uint8, 0), dev_full((2,), torch.int32, 99)
        tw.rc.export_streams_dev([eight[0]] * 2, d_rec.data_ptr())
        tw.rc.import_streams_dev(eight[1:], d_rec.data_ptr(), d_st.data_ptr())
        assert to_host(tw.ctx, d_st).tolist() == [api.SS_OK] * 2
    m.reset(eight[1:])
    tick()
    assert m.state["limited"][eight[0]] == t and m.state["limited"][eight[1]] <= 1, "the slot that was only exported keeps its state"
    tick()
    tw.rc.reset()
    m.reset()
    x[t] *= F32(40.0)                                                    # attack again everywhere
    tick()
    assert (m.state["limited"] == 1).all()
    # law, conference, mix and AGC settings leave the state alone; ceilings, parameters and the report switch survived everything
    tw.rc.set_stream_laws([0, 5], [1, 0])
    tw.rc.set_stream_confs([0, 5, 6], [3, 3, 3])
    tw.rc.set_stream_mix_gains([5], [0.5])
    tw.rc.set_agc(True)
    tick()
    assert (m.state["limited"] == 2).all() and same(tw.rc.stream_limiter(), np.full(B, 0.05, F32)) and same(tw.rc.limiter_params(), D)
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_limiter_equals_the_api_path(model, blob, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    frames = 12
    for opts, rate in ((["--rate", "8000"], 8000), ([], 48000)):
        n = tq.nof(rate)
        x = inputs("i16", 3, n, 26 + rate // 8000, frames)
        args = []
        for i in range(3):
            np.ascontiguousarray(x[:, i, :]).tofile(tmp_path / f"in{i}.pcm")
            args += [f"in{i}.pcm", f"out{i}.pcm"]
        run = subprocess.run([exe, "--model", "m.pnw"] + opts + ["--limiter", "0.01", "--limiter-hold", "1"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr
        got = [np.fromfile(tmp_path / f"out{i}.pcm", np.int16) for i in range(3)]
        plain = subprocess.run([exe, "--model", "m.pnw"] + opts + [a.replace("out", "plain") for a in args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0, plain.stderr
        tw = lim_twin(model, 3, rate if rate != 48000 else "mixed", ceilings=[np.float32("0.01")] * 3)
        tw.rc.set_limiter_params(np.array([D[lm.RELEASE], 1.0], F32))
        if rate == 48000:
            tw.rc.set_stream_rates([0, 1, 2], [48000] * 3)
            tw.rates, tw.w = [48000] * 3, 480
        want = [frame(tw, "i16", x[t])[0] for t in range(frames)]
        tw.close()
        for i in range(3):
            w = np.concatenate([want[t][i, :n] for t in range(1, frames)])
            assert got[i].size == w.size and np.array_equal(got[i], w), f"{rate} Hz pair {i}"
        assert not np.array_equal(got[0], np.fromfile(tmp_path / "plain0.pcm", np.int16))
