"""Automatic level control on the rate converter (-m gpu): include/percepnet_hip.h "automatic level control"; kernel
percepnet_amd/csrc/pn_rate_agc.hip, host side pn_rate.cpp (pn_rate_set_agc / pn_rate_set_stream_agc_targets / pn_rate_agc_f32 and the hook in
rate_frame), the rule pn_agc_rules.h, bindings api.RateConverter.set_agc / set_stream_agc_targets / agc_f32_dev / read_agc_report.

The oracle is the numpy float32 model tests/agc_model.py: alone for the kernel, and for whole frames inside the composition
pn_rate_up_* -> [the PLC model's row] -> pn_process_f32[_active] -> the model applied to the engine's rows on the host -> [pn_rate_mix_f32]
-> pn_rate_down_* on a SECOND context and converter that never enables AGC.  Every comparison is equality of bits; no tolerance.

Shapes: contexts of 3 and 19 streams, neither a multiple of the kernel's four rows a block.  Whole-frame tests run 12 frames: six of
the engine's delay and six of signal."""
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import agc_model as am
from tests import plc_model as pm
from tests import test_gpu_plc as tq
from tests import test_gpu_rate_pipe as tp
from tests.test_agc_host import hostile_rows, voice

pytestmark = pytest.mark.gpu
F32 = np.float32
BS = (3, 19)
T = 12
KT = 40
SENT = 777.0
D = am.DEFAULTS
Twin, inputs, frame, assert_frame, same, to_dev, to_host, dev_full, torch_dtype, SENTINEL = (
    tq.Twin, tq.inputs, tq.frame, tq.assert_frame, tq.same, tq.to_dev, tq.to_host, tq.dev_full, tq.torch_dtype, tq.SENTINEL)
model = tq.model
default_families = tq.default_families


def targets_of(B):
    """mixed targets, 0 (not levelled) among them"""
    return [(0.1, 0.0, 0.02, 0.05, 1.0, 0.0, 0.25)[s % 7] for s in range(B)]


def agc_twin(model, B, case="mixed", targets=None, plc=False, report=True):
    tw = Twin(model, B, case, plc=plc)
    tw.rc.set_agc(True)
    tw.rc.set_agc_report(report)
    tw.rc.set_stream_agc_targets(list(range(B)), targets_of(B) if targets is None else targets)
    return tw


def agc_model(B, targets=None, params=None):
    m = am.Agc(B, params)
    m.set_targets(range(B), targets_of(B) if targets is None else targets)
    return m


def assert_report(tw, m, what):
    rep = tw.rc.read_agc_report()
    assert rep.tobytes() == m.report.tobytes(), f"{what}: report\n{rep}\n{m.report}"


def launches(tw, name="rate_agc"):
    return tw.rc.kernel_times((name,))[name][1]


def composed(tw, agc, kind, x, ids=None, mix=False, plc=None, lost=()):
    """The same frame by hand on a twin without AGC (and without PLC): up, [the PLC model's frame on the host rows], the engine, the AGC
    model's frame on the engine's rows on the host, [the mix kernel], down -> (out rows, g|r, the levelled 48 kHz rows)"""
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
    h48 = agc.frame(to_host(tw.ctx, y48).copy(), ids=ids, concealed=lost)
    o48 = to_dev(h48)
    if mix:
        y48 = o48
        o48 = dev_full((tw.B, 480), torch.float32, nan)
        tw.rc.mix_f32_dev(y48.data_ptr(), o48.data_ptr(), ids=ids)
    d_out = dev_full((tw.B, tw.w), torch_dtype(kind), SENTINEL[kind])
    getattr(tw.rc, f"down_{kind}_dev")(o48.data_ptr(), d_out.data_ptr(), ids=ids)
    return to_host(tw.ctx, d_out).copy(), to_host(tw.ctx, d_gr).copy(), h48


# ---------------------------------------------------------------------------------------------------------------- 1
_kernel_rows = {}


def kernel_rows(B):
    """[KT, B, 480]: per stream a voice at its own level (5e-4 .. 0.6 RMS) that steps up 40x at frame 20 on every third stream and pauses
    on every fourth, with one hostile row per frame from frame 3 on, walking over the streams"""
    if B not in _kernel_rows:
        rng = np.random.default_rng(9100 + B)
        rows = np.empty((KT, B, 480), F32)
        for s in range(B):
            rms = 5e-4 * (1200.0 ** (s / max(B - 1, 1)))
            v = voice(rms, KT, f0=100.0 + 9.0 * s)
            if s % 3 == 0:
                v[20:] *= F32(40.0)
            if s % 4 == 1:
                v[10:18] = (rng.standard_normal((8, 480)) * 1e-4).astype(F32)
            rows[:, s] = v
        h = list(hostile_rows().values())
        for t in range(3, KT):
            rows[t, (5 * t) % B] = h[t % len(h)]
        rows.setflags(write=False)
        _kernel_rows[B] = rows
    return _kernel_rows[B]


@pytest.mark.parametrize("B", BS)
def test_the_kernel_alone_against_the_model(model, B):
    tw, m = agc_twin(model, B), agc_model(B)
    x = kernel_rows(B)
    seen = 0
    rng = np.random.default_rng(77)
    for t in range(KT):
        ids = None
        if t % 4 == 2:                                                   # an active list, in any order; the others keep rows, states, report rows
            ids = [int(v) for v in rng.permutation(B)[:max(1, B - 1 - t % 3)]]
        if t == 15:                                                      # a parameter change between two frames
            p = D.copy()
            p[[am.MAX_GAIN, am.ATTACK, am.STEP_UP, am.CEILING]] = (4.0, 1.0, 1.5, 0.5)
            tw.rc.set_agc_params(p)
            m.params = p
            assert same(tw.rc.agc_params(), p)
        if t == 25:                                                      # a target change: the state stays
            chg, new = [0, B - 1, 1], [0.0, 0.3, 0.07]
            tw.rc.set_stream_agc_targets(chg, new)
            m.set_targets(chg, new)
        rows = np.array(x[t])
        if ids is not None:
            for s in range(B):
                if s not in ids:
                    rows[s] = SENT
        d = to_dev(rows)
        tw.rc.agc_f32_dev(d.data_ptr(), ids=ids)
        got = to_host(tw.ctx, d)
        want = m.frame(rows, ids=ids)
        for s in range(B):
            assert same(got[s], want[s]), f"frame {t} stream {s} (target {m.targets[s]}, listed {ids is None or s in ids})"
            if ids is not None and s not in ids:
                assert (got[s] == F32(SENT)).all()
        assert_report(tw, m, f"frame {t}")
        for f in m.report["flags"]:
            seen |= int(f)
    assert seen == am.ON | am.ADAPTED | am.LIMITED | am.AT_MAX | am.AT_MIN, "every flag but HELD_LOST, which needs the concealer"
    g = m.gains()
    lev = [s for s in range(B) if m.targets[s] != 0]
    assert (g[lev] >= m.params[am.MIN_GAIN]).all() and (g[lev] <= D[am.MAX_GAIN]).all() and len(set(g[lev].tolist())) > 1
    assert same(tw.rc.stream_agc_targets(), m.targets) and launches(tw) == KT
    tw.close()


def test_refusals_change_nothing(model):
    B = 3
    tw = Twin(model, B, 8000)
    d = to_dev(np.zeros((B, 480), F32))
    assert same(tw.rc.agc_params(), D) and same(tw.rc.stream_agc_targets(), np.zeros(B, F32))
    for call in (lambda: tw.rc.set_stream_agc_targets([0], [0.1]), lambda: tw.rc.agc_f32_dev(d.data_ptr())):
        with pytest.raises(api.PercepNetError, match="pn_rate_set_agc"):
            call()
    with pytest.raises(api.PercepNetError, match="pn_rate_set_agc_report"):
        tw.rc.read_agc_report()
    tw.rc.set_agc(True)
    tw.rc.set_stream_agc_targets([2, 0], [0.2, -0.0])
    for ids, t, word in (([B], [0.1], "out of range"), ([-1], [0.1], "out of range"), ([1, 1], [0.1, 0.1], "twice"), ([0, 1], [0.1, np.nan], "index 1"),
                         ([1], [1.5], "index 0"), ([1], [-0.1], "index 0")):
        with pytest.raises(api.PercepNetError, match=word):
            tw.rc.set_stream_agc_targets(ids, t)
    tw.rc.set_stream_agc_targets([], [])
    got = tw.rc.stream_agc_targets()
    assert same(got, np.array([0.0, 0.0, 0.2], F32)) and not np.signbit(got[0])
    p = D.copy()
    p[am.STEP_DOWN] = 0.0
    with pytest.raises(api.PercepNetError, match=r"index 6 \(step_down\)"):
        tw.rc.set_agc_params(p)
    assert same(tw.rc.agc_params(), D)
    with pytest.raises(api.PercepNetError, match="aligned"):
        tw.rc.agc_f32_dev(d.data_ptr() + 4)
    with pytest.raises(api.PercepNetError, match="rate_agc"):
        tw.rc.kernel_times(("rate_xyz",))
    assert launches(tw) == 0
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def conf_setup(tws, B, mode):
    if mode == "none":
        return
    confs = [s % 4 if s < 16 else api.CONF_NONE for s in range(B)] if B > 3 else [0, 0, api.CONF_NONE]
    for tw in tws:
        tw.rc.set_stream_confs(list(range(B)), confs)
        tw.ctx.set_output_saturate(True)
        if mode == "loudest":
            tw.rc.set_conf_speakers([0, 1, 2, 3] if B > 3 else [0], [2, 1, 3, 2] if B > 3 else [1])
            tw.rc.set_stream_mix_gains([0, 1], [0.5, 2.0])


@pytest.mark.parametrize("B,case,kind,mode", ((3, 8000, "f32", "none"), (3, 32000, "g711", "conf"), (19, "mixed", "i16", "conf"), (19, "mixed", "f32", "loudest"),
                                              (19, "mixed", "g711", "none"), (19, 16000, "i16", "loudest")), ids=str)
def test_whole_frame_against_the_composition(model, B, case, kind, mode):
    a, b, plain = agc_twin(model, B, case), Twin(model, B, case), Twin(model, B, case)
    conf_setup((a, b, plain), B, mode)
    m = agc_model(B)
    x = inputs(kind, B, a.w, 11)
    rng = np.random.default_rng(5)
    differs = False
    for t in range(T):
        ids = sorted(int(v) for v in rng.permutation(B)[:B - 1]) if t in (8, 10) else None        # the _active entry points
        got = frame(a, kind, x[t], ids)
        want = composed(b, m, kind, x[t], ids, mix=mode != "none")
        assert_frame(a, got, want, ids, f"{case} {kind} {mode} frame {t}:")
        if ids is None:
            assert_report(a, m, f"frame {t}")
        differs |= not same(got[0], frame(plain, kind, x[t], ids)[0])
    assert differs, "the levelled output is not the plain one"
    assert launches(a) == T and launches(b) == 0
    for tw in (a, b, plain):
        tw.close()


def test_pipelined_path_with_a_setting_call_between_two_submits(model):
    B = 19
    x = inputs("i16", B, 480, 12)
    rng = np.random.default_rng(56)
    ids_at = [None if t % 3 else sorted(int(v) for v in rng.permutation(B)[:B - 2]) for t in range(T)]
    p2 = D.copy()
    p2[[am.MAX_GAIN, am.STEP_UP]] = (64.0, 2.0)

    def settings(tw, t):
        if t == 7:
            tw.rc.set_stream_agc_targets([1, 4, 5], [0.5, 0.0, 0.3])
        if t == 9:
            tw.rc.set_agc_params(p2)
        if t == 10:
            tw.rc.set_stream_agc_targets([1], [0.01])

    sync = agc_twin(model, B)
    want = []
    for t in range(T):
        settings(sync, t)
        want.append(frame(sync, "i16", x[t], ids_at[t]))
    sync.close()
    p = agc_twin(model, B)
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


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_lost_stream_holds_level_and_gain(model):
    B = 3
    a, b = agc_twin(model, B, 16000, targets=[0.1, 0.2, 0.0], plc=True), Twin(model, B, 16000)
    m, plc = agc_model(B, [0.1, 0.2, 0.0]), pm.Plc(B)
    x = inputs("i16", B, a.w, 13, 16)
    losses = {8: [1], 9: [1], 10: [1], 12: [0, 2]}
    for t in range(16):
        lost = losses.get(t, [])
        rows = tq.poison(x[t], lost, "i16")
        before = m.state.copy()
        tq.mark(a.rc, lost)
        got = frame(a, "i16", rows)
        want = composed(b, m, "i16", rows, plc=plc, lost=lost)
        assert_frame(a, got, want, None, f"frame {t}:")
        assert_report(a, m, f"frame {t}")
        rep = a.rc.read_agc_report()
        for s in lost:
            if m.targets[s] != 0:
                assert rep[s]["flags"] & am.HELD_LOST and not rep[s]["flags"] & am.ADAPTED
                assert m.state[s]["level"] == before[s]["level"] and m.state[s]["adapted"] == before[s]["adapted"]
                if not rep[s]["flags"] & am.LIMITED:
                    assert m.state[s]["gain"].tobytes() == (before[s]["gain"] if before[s]["gain"].view(np.uint32) else F32(1.0)).tobytes()
        for s in range(B):
            if s not in lost:
                assert not rep[s]["flags"] & am.HELD_LOST
    assert m.state["adapted"][1] > 0 and rep[2].tolist() == (1.0, 0.0, 0, 0.0)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("B", BS)
def test_nothing_new_while_off(model, B):
    never, plain = Twin(model, B, "mixed"), Twin(model, B, "mixed")
    zero = Twin(model, B, "mixed")
    zero.rc.set_agc(True)                                                # enabled, every target 0
    zero.rc.set_stream_agc_targets([0], [0.0])
    p = D.copy()
    p[[am.MAX_GAIN, am.MIN_GAIN]] = 1.0
    unity = agc_twin(model, B, "mixed", targets=[0.1] * B)               # enabled, levelled, Gmax = Gmin = 1
    unity.rc.set_agc_params(p)
    n = 0
    for kind in ("f32", "i16", "g711"):
        x = inputs(kind, B, 480, 14, 8)
        for t in range(8):
            want = frame(plain, kind, x[t])
            for tw, what in ((never, "never enabled"), (zero, "every target 0"), (unity, "unity gains")):
                assert_frame(tw, frame(tw, kind, x[t]), want, None, f"{what}: {kind} frame {t}:")
            n += 1
    rep = unity.rc.read_agc_report()
    assert (rep["gain"] == 1.0).all() and (rep["flags"] & am.ON).all(), "every stream is levelled, between gains of one"
    assert never.rc.kernel_times(("rate_agc",))["rate_agc"] == (0.0, 0), "a converter that never enables AGC launches what it always launched"
    assert zero.rc.kernel_times(("rate_agc",))["rate_agc"] == (0.0, 0), "no target, no launch"
    assert launches(unity) == n
    for name in ("rate_up", "rate_down"):
        assert launches(never, name) == launches(plain, name) == launches(unity, name) == n
    unity.rc.set_agc(False)
    assert_frame(unity, frame(unity, "f32", inputs("f32", B, 480, 15, 1)[0]), frame(plain, "f32", inputs("f32", B, 480, 15, 1)[0]), None, "off again:")
    assert launches(unity) == n, "while off nothing new is launched"
    for tw in (never, plain, zero, unity):
        tw.close()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("form", ("host", "dev"))
def test_lifecycle_gives_the_listed_slots_a_fresh_state(model, form):
    import torch
    B = 19
    tw, m = agc_twin(model, B, "mixed", targets=[0.1] * B), agc_model(B, [0.1] * B)
    x = np.stack([voice(0.004 * (s + 1), 30, f0=110.0 + 7 * s) for s in range(B)], axis=1)
    t = 0

    def tick(ids=None):
        nonlocal t
        d = to_dev(np.array(x[t]))
        tw.rc.agc_f32_dev(d.data_ptr(), ids=ids)
        want = m.frame(x[t], ids=ids)
        got = to_host(tw.ctx, d)
        for s in range(B) if ids is None else ids:
            assert same(got[s], want[s]), f"tick {t} stream {s}"
        assert_report(tw, m, f"tick {t}")
        t += 1

    for _ in range(5):
        tick()
    assert (m.gains() != 1.0).all(), "every stream has left the fresh gain"
    tw.rc.reset_streams([1, 4])
    m.reset([1, 4])
    tick()
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
    assert m.state["adapted"][eight[0]] == t and m.state["adapted"][eight[1]] == 1, "the slot that was only exported keeps its state"
    tick()
    tw.rc.reset()
    m.reset()
    tick()
    assert (m.state["adapted"] == 1).all()
    tick()
    tw.rc.set_agc(False)                                                 # disabling then enabling zeroes all; targets and parameters stay
    tw.rc.set_agc(True)
    m.reset()
    tick()
    assert (m.state["adapted"] == 1).all() and same(tw.rc.stream_agc_targets(), np.full(B, 0.1, F32))
    # law, conference and mix settings leave the state alone
    tw.rc.set_stream_laws([0, 5], [1, 0])
    tw.rc.set_stream_confs([0, 5, 6], [3, 3, 3])
    tw.rc.set_stream_mix_gains([5], [0.5])
    tick()
    assert (m.state["adapted"] == 2).all()
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_agc_equals_the_api_path(model, blob, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    frames = 12
    for opts, rate in ((["--rate", "8000"], 8000), ([], 48000)):
        n = tq.nof(rate)
        x = inputs("i16", 3, n, 16 + rate // 8000, frames)
        args = []
        for i in range(3):
            np.ascontiguousarray(x[:, i, :]).tofile(tmp_path / f"in{i}.pcm")
            args += [f"in{i}.pcm", f"out{i}.pcm"]
        run = subprocess.run([exe, "--model", "m.pnw"] + opts + ["--agc", "0.1", "--agc-max-gain", "8"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr
        got = [np.fromfile(tmp_path / f"out{i}.pcm", np.int16) for i in range(3)]
        plain = subprocess.run([exe, "--model", "m.pnw"] + opts + [a.replace("out", "plain") for a in args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0, plain.stderr
        tw = agc_twin(model, 3, rate if rate != 48000 else "mixed", targets=[np.float32("0.1")] * 3)
        p = D.copy()
        p[am.MAX_GAIN] = 8.0
        tw.rc.set_agc_params(p)
        if rate == 48000:
            tw.rc.set_stream_rates([0, 1, 2], [48000] * 3)
            tw.rates, tw.w = [48000] * 3, 480
        want = [frame(tw, "i16", x[t])[0] for t in range(frames)]
        tw.close()
        for i in range(3):
            w = np.concatenate([want[t][i, :n] for t in range(1, frames)])
            assert got[i].size == w.size and np.array_equal(got[i], w), f"{rate} Hz pair {i}"
        assert not np.array_equal(got[0], np.fromfile(tmp_path / "plain0.pcm", np.int16))
