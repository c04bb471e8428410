"""Packet-loss concealment on the rate converter (-m gpu): include/percepnet_hip.h "packet-loss concealment"; kernel
percepnet_amd/csrc/pn_rate_plc.hip, host side pn_rate.cpp (pn_rate_set_plc / pn_rate_set_lost / pn_rate_plc_f32 and the hook in rate_frame),
the rule pn_plc_rules.h, bindings api.RateConverter.set_plc / set_lost / plc_f32_dev / read_plc_report.

The oracle is the numpy float32 model tests/plc_model.py: alone for the kernel, and for whole frames inside the composition
pn_rate_up_* (over the streams that are not lost) -> the model's row substituted on the host -> pn_process_f32[_active] -> [pn_rate_mix_f32]
-> pn_rate_down_* on a SECOND context and converter that never enables PLC.  Every comparison is equality of bits; no tolerance.

Shapes: contexts of 3 and 19 streams, neither a multiple of the kernel's eight block groups nor of the row kernels' four streams a block.
Whole-frame tests run 12 frames: six of the engine's delay and six of signal, with the losses behind frame 6."""
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import families
from tests import plc_model as pm
from tests import test_gpu_rate as tg
from tests import test_gpu_rate_pipe as tp
from tests.test_plc_host import PERIODS, periodic_history

pytestmark = pytest.mark.gpu
F32 = np.float32
BS = (3, 19)
T = 12
MIXED_RATES = (8000, 16000, 24000, 32000, 48000)
DTYPE = {"f32": np.float32, "i16": np.int16, "g711": np.uint8}
SENTINEL = {"f32": 777.0, "i16": 12345, "g711": 0x5A}
to_dev, to_host = tg.to_dev, tg.to_host


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def nof(rate):
    return api.rate_mixed_frame_samples(rate)


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


def torch_dtype(kind):
    import torch
    return {"f32": torch.float32, "i16": torch.int16, "g711": torch.uint8}[kind]


def dev_full(shape, dtype, fill):
    return tg.dev_full(shape, dtype, fill)


class Twin:
    """A context of B streams and a converter beside it: mixed over MIXED_RATES (case "mixed") or single-rate (case = the rate)"""

    def __init__(self, model, B, case="mixed", plc=False):
        self.B = B
        self.ctx = api.Context(model, B)
        self.rates = [MIXED_RATES[s % 5] for s in range(B)] if case == "mixed" else [case] * B
        self.rc = api.MixedRateConverter(self.ctx, self.rates) if case == "mixed" else api.RateConverter(self.ctx, case)
        self.rc.set_stream_laws(list(range(B)), [s % 2 for s in range(B)])
        self.w = self.rc.frame
        self.rc.set_profiling(True)
        if plc:
            self.rc.set_plc(True)

    def ns(self):
        return [nof(r) for r in self.rates]

    def close(self):
        self.rc.close()
        self.ctx.close()


_inputs = {}


def inputs(kind, B, w, seed=0, frames=T):
    """[frames, B, w] seeded rows of a sample format: a voiced sound per stream (six harmonics of 90 .. 250 Hz at the row's rate,
    taken as if w samples were 10 ms) in gaussian noise, as float or int16; random bytes for G.711"""
    key = (kind, B, w, seed, frames)
    if key not in _inputs:
        rng = np.random.default_rng(8000 + 13 * seed + w + B)
        if kind == "g711":
            a = rng.integers(0, 256, (frames, B, w)).astype(np.uint8)
        else:
            t = np.arange(frames * w) / (100.0 * w)
            f0 = 90.0 + 160.0 * rng.uniform(size=B)
            v = sum(np.cos(2 * np.pi * k * f0[:, None] * t[None, :] + k) / k for k in range(1, 7)) * 0.15 + rng.standard_normal((B, frames * w)) * 0.02
            v = v.reshape(B, frames, w).transpose(1, 0, 2)
            a = v.clip(-1.0, 1.0 - 2.0 ** -15).astype(F32) if kind == "f32" else np.rint(v * 32768).clip(-32768, 32767).astype(np.int16)
        a.setflags(write=False)
        _inputs[key] = a
    return _inputs[key]


def frame(tw, kind, x, ids=None):
    """One frame through the converter's own entry point -> (out rows, g|r)"""
    import torch
    d_in = to_dev(np.array(x))
    d_out = dev_full((tw.B, tw.w), torch_dtype(kind), SENTINEL[kind])
    d_gr = dev_full((tw.B, 68), torch.float32, float("nan"))
    getattr(tw.rc, f"process_{kind}_dev")(d_in.data_ptr(), d_out.data_ptr(), d_gr.data_ptr(), ids=ids)
    return to_host(tw.ctx, d_out).copy(), to_host(tw.ctx, d_gr).copy()


def composed(tw, plc, kind, x, lost=(), ids=None, mix=False):
    """The same frame by hand on a twin without PLC: up over the streams that advance and are not lost, the model's frame on the
    host rows, the engine, [the mix kernel], down -> (out rows, g|r, the 48 kHz rows the engine was given)"""
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
    h48 = plc.frame(to_host(tw.ctx, x48).copy(), lost=lost, ids=ids)
    x48 = to_dev(h48)
    if ids is None:
        tw.ctx.process_f32_dev(x48.data_ptr(), y48.data_ptr(), d_gr.data_ptr())
    else:
        tw.ctx.process_f32_active_dev(x48.data_ptr(), y48.data_ptr(), d_gr.data_ptr(), ids)
    o48 = y48
    if mix:
        o48 = dev_full((tw.B, 480), torch.float32, nan)
        tw.rc.mix_f32_dev(y48.data_ptr(), o48.data_ptr(), ids=ids)
    d_out = dev_full((tw.B, tw.w), torch_dtype(kind), SENTINEL[kind])
    getattr(tw.rc, f"down_{kind}_dev")(o48.data_ptr(), d_out.data_ptr(), ids=ids)
    return to_host(tw.ctx, d_out).copy(), to_host(tw.ctx, d_gr).copy(), h48


def assert_frame(tw, got, want, ids, what):
    for s, n in enumerate(tw.ns()):
        if ids is None or s in ids:
            assert same(got[0][s, :n], want[0][s, :n]), f"{what} stream {s}"
            assert same(got[1][s], want[1][s]), f"{what} g|r of stream {s}"
        else:
            assert (got[0][s] == SENTINEL[{np.dtype(np.float32): "f32", np.dtype(np.int16): "i16", np.dtype(np.uint8): "g711"}[got[0].dtype]]).all(), \
                f"{what} the row of unlisted stream {s} is untouched"


def poison(x, lost, kind):
    """the input rows of the lost streams hold what must never be read: NaN, or the extreme code"""
    x = np.array(x)
    for s in lost:
        x[s] = np.nan if kind == "f32" else (-32768 if kind == "i16" else 0x80)
    return x


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("case", (8000, 32000, "mixed"), ids=str)
def test_plc_on_and_nothing_lost_changes_no_bit(model, case, B):
    a, b = Twin(model, B, case, plc=True), Twin(model, B, case)
    a.rc.set_plc_report(True)
    n = 0
    for kind in ("f32", "i16", "g711"):
        x = inputs(kind, B, a.w, frames=6)
        for t in range(6):
            got, want = frame(a, kind, x[t]), frame(b, kind, x[t])
            assert_frame(a, got, want, None, f"{case} {kind} frame {t}:")
            n += 1
    rep = a.rc.read_plc_report()
    assert rep.tolist() == [(0, 0, 0, 0)] * B
    ta, tb = a.rc.kernel_times(("rate_up", "rate_down", "rate_plc")), b.rc.kernel_times(("rate_up", "rate_down", "rate_plc"))
    assert ta["rate_plc"][1] == n and tb["rate_plc"] == (0.0, 0), "a converter that never enables PLC launches what it always launched"
    assert ta["rate_up"][1] == tb["rate_up"][1] == n and ta["rate_down"][1] == tb["rate_down"][1] == n
    a.rc.set_plc(False)
    got, want = frame(a, "f32", inputs("f32", B, a.w, 1, 1)[0]), frame(b, "f32", inputs("f32", B, a.w, 1, 1)[0])
    assert_frame(a, got, want, None, "PLC off again:")
    assert a.rc.kernel_times(("rate_plc",))["rate_plc"][1] == n, "while off nothing new is launched"
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 2
ROLES = ("never", "one", "two", "seven", "at0", "again", "offlist", "marked_idle")
SCRIPT_T = 14


def role_of(s, B):
    return ("seven", "again", "marked_idle")[s] if B == 3 else ROLES[s % 8]


def script(B):
    """-> per tick (ids or None, the streams marked lost): one script for all the roles"""
    ticks = []
    for t in range(SCRIPT_T):
        off, lost = set(), set()
        for s in range(B):
            role = role_of(s, B)
            if ((role == "one" and t == 5) or (role == "two" and t in (5, 6)) or (role == "seven" and 4 <= t <= 10) or (role == "at0" and t in (0, 1))
                    or (role == "again" and t in (4, 6, 7, 12)) or (role == "offlist" and t in (7, 8)) or (role == "marked_idle" and t in (5, 8))):
                lost.add(s)
            if (role == "offlist" and t in (3, 6, 9)) or (role == "marked_idle" and t == 5):
                off.add(s)
        ids = None if not off else [int(v) for v in np.random.default_rng(t).permutation([s for s in range(B) if s not in off])]
        ticks.append((ids, sorted(lost)))
    return ticks


def mark(rc, lost):
    """pn_rate_set_lost, in two calls where there are two streams to mark: calls before one frame add up"""
    if len(lost) > 1:
        rc.set_lost(lost[:1])
        rc.set_lost(lost[1:])
    elif lost:
        rc.set_lost(lost)


@pytest.mark.parametrize("B", BS)
def test_the_kernel_alone_against_the_model(model, B):
    tw = Twin(model, B, "mixed", plc=True)
    tw.rc.set_plc_report(True)
    m = pm.Plc(B)
    x = inputs("f32", B, 480, 2, SCRIPT_T)
    seen = set()
    for t, (ids, lost) in enumerate(script(B)):
        rows = poison(x[t], lost, "f32")
        d = to_dev(rows)
        mark(tw.rc, lost)
        tw.rc.plc_f32_dev(d.data_ptr(), ids=ids)
        got, rep = to_host(tw.ctx, d), tw.rc.read_plc_report()
        want = m.frame(rows.copy(), lost=lost, ids=ids)
        for s in range(B):
            if ids is None or s in ids:
                assert same(got[s], want[s]), f"tick {t} stream {s} ({role_of(s, B)})"
                assert rep[s].tolist() == m.report[s].tolist(), f"tick {t} report of stream {s} ({role_of(s, B)})"
                seen.add(int(rep[s]["flags"]))
            else:
                assert same(got[s], rows[s]), f"tick {t}: the row of unlisted stream {s} is untouched"
        assert np.isfinite(got[[s for s in range(B) if ids is None or s in ids]]).all()
    assert seen == {0, pm.CONCEALED, pm.CROSSFADE, pm.CONCEALED | pm.SILENT}
    for s in range(B):
        role = role_of(s, B)
        want_lost = {"never": 0, "one": 1, "two": 2, "seven": 7, "at0": 2, "again": 4, "offlist": 2, "marked_idle": 1}[role]
        assert m.lost[s] == want_lost, (s, role)
    assert tw.rc.kernel_times(("rate_plc",))["rate_plc"][1] == SCRIPT_T
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_periodic_histories_are_continued_bit_for_bit_on_the_device(model):
    B = 19
    tw = Twin(model, B, 8000, plc=True)
    tw.rc.set_plc_report(True)
    hw = [periodic_history(PERIODS[s % len(PERIODS)], s // len(PERIODS)) for s in range(B)]
    for t in range(4):
        d = to_dev(np.stack([h[480 * t:480 * (t + 1)] for h, _ in hw]))
        tw.rc.plc_f32_dev(d.data_ptr())
    tw.rc.set_lost(list(range(B)))
    d = to_dev(np.full((B, 480), np.nan, F32))
    tw.rc.plc_f32_dev(d.data_ptr())
    got, rep = to_host(tw.ctx, d), tw.rc.read_plc_report()
    for s in range(B):
        per = PERIODS[s % len(PERIODS)]
        assert same(got[s], hw[s][1]), f"stream {s}, period {per}"
        assert rep[s]["period"] % per == 0 and rep[s]["period"] == api.plc_pitch(hw[s][0]) and rep[s].tolist()[0::2] == (pm.CONCEALED, 1)
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def loss_script(B):
    """whole frames: per frame the lost streams — behind the engine's delay, one stream for two frames, another while the first recovers"""
    a, b = 1, B - 1
    return {6: [a], 7: [a], 8: [b], 10: [a, b]}


@pytest.mark.parametrize("B,case", ((3, 8000), (19, "mixed")), ids=str)
def test_whole_frame_against_the_composition(model, B, case):
    a, b = Twin(model, B, case, plc=True), Twin(model, B, case)
    m = pm.Plc(B)
    x = inputs("f32", B, a.w, 3)
    losses = loss_script(B)
    for t in range(T):
        lost = losses.get(t, [])
        rows = poison(x[t], lost, "f32")
        before = {s: a.rc.export_streams([s]) for s in lost if a.rates[s] != 48000}
        mark(a.rc, lost)
        got = frame(a, "f32", rows)
        want = composed(b, m, "f32", rows, lost)
        assert_frame(a, got, want, None, f"{case} frame {t}:")
        assert all(np.isfinite(got[0][s, :n]).all() for s, n in enumerate(a.ns())), f"frame {t}: a NaN input row of a lost stream reaches nobody"
        for s, rec in before.items():
            assert same(a.rc.export_streams([s])[0, 16:16 + 128], rec[0, 16:16 + 128]), f"frame {t}: the up-conversion tail of lost stream {s} is left as it was"
    assert m.lost.sum() == 5 and np.count_nonzero(got[0]) > 0
    times = a.rc.kernel_times(("rate_up", "rate_plc"))
    assert times["rate_plc"][1] == T and times["rate_up"][1] == T
    a.close()
    b.close()


def test_whole_frame_with_every_advancing_stream_lost(model):
    """an id list whose streams are all lost: no up-conversion launch at all, and the unlisted streams keep everything"""
    B = 3
    a, b = Twin(model, B, 16000, plc=True), Twin(model, B, 16000)
    m = pm.Plc(B)
    x = inputs("i16", B, a.w, 4)
    for t in range(T):
        ids, lost = ([2, 0], [0, 2]) if t == 8 else (None, [])
        rows = poison(x[t], lost, "i16")
        mark(a.rc, lost)
        got = frame(a, "i16", rows, ids)
        want = composed(b, m, "i16", rows, lost, ids)
        assert_frame(a, got, want, ids, f"frame {t}:")
    assert a.rc.kernel_times(("rate_up",))["rate_up"][1] == T - 1 and m.lost.tolist() == [1, 0, 1]
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_pipelined_path_equals_the_synchronous_one(model):
    B = 19
    sync = Twin(model, B, "mixed", plc=True)
    x = inputs("i16", B, 480, 5)
    rng = np.random.default_rng(55)
    ids_at = [sorted(int(v) for v in rng.permutation(B)[:B - (t % 3)]) for t in range(T)]
    lost_at = [[] if t < 6 else [ids_at[t][t % 5], ids_at[t][-1]] if t % 2 == 0 else [ids_at[t][3]] for t in range(T)]
    lost_at[10] = lost_at[10] + [s for s in range(B) if s not in ids_at[10]][:1]         # a marked stream that does not advance
    assert len(lost_at[10]) == 3
    want = []
    for t in range(T):
        mark(sync.rc, lost_at[t])
        want.append(frame(sync, "i16", poison(x[t], lost_at[t], "i16"), ids_at[t]))
    sync.close()
    p = Twin(model, B, "mixed", plc=True)
    rot = tp.Rot(p.ctx, 480, "i16", b=B)
    xs = np.stack([poison(x[t], lost_at[t], "i16") for t in range(T)])

    def submit(t, h_in, h_out, h_gr, h_rep):
        mark(p.rc, lost_at[t])                                                          # no wait before or after
        p.rc.submit_host_i16(h_in, h_out, h_gr, ids=ids_at[t])

    got = rot.run(xs, submit)
    for t in range(T):
        for s in ids_at[t]:
            n = nof(p.rates[s])
            assert same(got[t][0][s, :n], want[t][0][s, :n]) and same(got[t][1][s], want[t][1][s]), f"frame {t} stream {s}"
    assert p.ctx.frames_delivered() == T
    p.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_conference_listeners_hear_the_concealed_voice(model):
    B = 19
    confs = [s % 4 if s < 16 else api.CONF_NONE for s in range(B)]                       # four conferences of four, three streams alone
    a, b = Twin(model, B, "mixed", plc=True), Twin(model, B, "mixed")
    for tw in (a, b):
        tw.rc.set_stream_confs(list(range(B)), confs)
        tw.ctx.set_output_saturate(True)
    m = pm.Plc(B)
    x = inputs("i16", B, 480, 6)
    losses = {7: [1], 8: [1, 6], 9: [17]}
    differs = False
    for t in range(T):
        lost = losses.get(t, [])
        rows = poison(x[t], lost, "i16")
        mark(a.rc, lost)
        got = frame(a, "i16", rows)
        want = composed(b, m, "i16", rows, lost, mix=True)
        assert_frame(a, got, want, None, f"frame {t}:")
        if lost:
            differs |= bool(np.count_nonzero(want[2][lost]))
    assert differs, "the concealed rows carry signal"
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_resets_and_rate_changes_zero_the_state_and_refusals_change_nothing(model):
    B = 19
    tw = Twin(model, B, "mixed", plc=True)
    tw.rc.set_plc_report(True)
    m = pm.Plc(B)
    x = inputs("f32", B, 480, 7, 24)
    t = 0

    def tick(lost=(), ids=None):
        nonlocal t
        rows = poison(x[t], lost, "f32")
        d = to_dev(rows)
        mark(tw.rc, list(lost))
        tw.rc.plc_f32_dev(d.data_ptr(), ids=ids)
        got, rep = to_host(tw.ctx, d), tw.rc.read_plc_report()
        want = m.frame(rows.copy(), lost=lost, ids=ids)
        for s in range(B) if ids is None else ids:
            assert same(got[s], want[s]) and rep[s].tolist() == m.report[s].tolist(), f"tick {t} stream {s}"
        t += 1
        return got

    for _ in range(4):
        tick()
    # refusals: nothing changed, nothing launched
    launches = tw.rc.kernel_times(("rate_plc",))["rate_plc"][1]
    for bad, word in (([B], "out of range"), ([-1], "out of range"), ([2, 5, 2], "twice")):
        with pytest.raises(api.PercepNetError, match=word):
            tw.rc.set_lost(bad)
    tw.rc.set_lost([])
    tw.rc.set_plc(False)
    for call in (lambda: tw.rc.set_lost([1]), lambda: tw.rc.plc_f32_dev(to_dev(np.zeros((B, 480), F32)).data_ptr())):
        with pytest.raises(api.PercepNetError, match="pn_rate_set_plc"):
            call()
    tw.rc.set_plc(True)
    m.reset()                                   # on again after a pause: every stream starts with an empty history
    assert tw.rc.kernel_times(("rate_plc",))["rate_plc"][1] == launches
    for _ in range(4):
        got = tick()
    assert m.lost.sum() == 0, "none of the refused marks took"
    # a reset of streams 1 and 4: their following loss conceals from an empty history; stream 2's from its own
    tw.rc.reset_streams([1, 4])
    m.reset([1, 4])
    got = tick(lost=(1, 2))
    assert not got[1].any() and got[2].any() and m.report[1].tolist() == (pm.CONCEALED, 240, 1, 1)
    tick()
    # a rate change of stream 2 zeroes its state in the middle of nothing; a mark set before the change still holds
    for _ in range(3):
        tick()
    tw.rc.set_lost([2, 3])
    tw.rc.set_stream_rates([2], [16000])
    m.reset([2])
    rows = poison(x[t], (2, 3), "f32")
    d = to_dev(rows)
    tw.rc.plc_f32_dev(d.data_ptr())
    got = to_host(tw.ctx, d)
    want = m.frame(rows.copy(), lost=(2, 3))
    assert same(got, want) and not got[2].any() and got[3].any()
    t += 1
    tick()
    # the whole converter
    tw.rc.reset()
    m.reset()
    got = tick(lost=tuple(range(B)))
    assert not got.any() and tw.rc.read_plc_report()["lost"].tolist() == [1] * B
    # law, conference and mix settings leave the state alone
    tick()
    tick()
    tick()
    tick()
    tw.rc.set_stream_laws([0, 5], [1, 0])
    tw.rc.set_stream_confs([0, 5, 6], [3, 3, 3])
    tw.rc.set_stream_mix_gains([5], [0.5])
    got = tick(lost=(0, 5))
    assert got[0].any() and got[5].any()
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("form", ("host", "dev"))
def test_an_import_starts_the_slot_with_an_empty_history(model, form):
    """A single-rate converter, where no rate change precedes an import.  Slot 1 holds four rows of history and slot 2 is in the
    middle of a loss (r > 0, a period in q) when records are imported over both: slot 1's next lost frame is concealed with
    silence, not with the previous stream's voice, and slot 2's next received row is not cross-faded out of the stale period."""
    import torch
    B = 3
    tw = Twin(model, B, 8000, plc=True)
    tw.rc.set_plc_report(True)
    m = pm.Plc(B)
    x = inputs("f32", B, 480, 8, 8)

    def tick(t, lost=()):
        rows = poison(x[t], lost, "f32")
        d = to_dev(rows)
        mark(tw.rc, list(lost))
        tw.rc.plc_f32_dev(d.data_ptr())
        got, rep = to_host(tw.ctx, d), tw.rc.read_plc_report()
        want = m.frame(rows.copy(), lost=lost)
        assert same(got, want) and rep.tolist() == m.report.tolist(), f"tick {t}"
        return got, rows

    for t in range(4):
        tick(t)
    got, _ = tick(4, lost=(2,))
    assert got[2].any() and m.r[2] == 1, "slot 2 is inside a loss, with a period of its own"
    if form == "host":
        tw.rc.import_streams([1, 2], tw.rc.export_streams([0, 0]))
    else:
        stride = tw.rc.record_stride()
        d_rec = dev_full((2, stride), torch.uint8, 0)
        d_st = dev_full((2,), torch.int32, 99)
        tw.rc.export_streams_dev([0, 0], d_rec.data_ptr())
        tw.rc.import_streams_dev([1, 2], d_rec.data_ptr(), d_st.data_ptr())
        assert to_host(tw.ctx, d_st).tolist() == [api.SS_OK] * 2
    m.reset([1, 2])
    got, rows = tick(5, lost=(1,))
    assert not got[1].any() and m.report[1].tolist() == (pm.CONCEALED, 240, 1, 1), "concealed from an empty history"
    assert same(got[2], rows[2]) and m.report[2].tolist() == (0, 0, 0, 0), "no cross-fade out of the previous stream's period"
    assert m.report[0]["lost"] == 0 and m.hist[0].any(), "the slot that was only exported keeps its state"
    got, _ = tick(6, lost=(0,))
    assert got[0].any()
    tw.close()


def test_enabling_again_after_a_pause_starts_every_stream_with_an_empty_history(model):
    """the frames of the pause are missing from the histories, and a stream left inside a loss would cross-fade out of an old period"""
    B = 3
    tw = Twin(model, B, 8000, plc=True)
    tw.rc.set_plc_report(True)
    m = pm.Plc(B)
    x = inputs("f32", B, 480, 8, 8)
    for t in range(7):
        lost = (2,) if t == 4 else (0, 1) if t == 6 else ()
        if t == 5:
            tw.rc.set_plc(False)
            tw.rc.set_plc(True)
            m.reset()
        rows = poison(x[t], lost, "f32")
        d = to_dev(rows)
        mark(tw.rc, list(lost))
        tw.rc.plc_f32_dev(d.data_ptr())
        got, rep = to_host(tw.ctx, d), tw.rc.read_plc_report()
        assert same(got, m.frame(rows.copy(), lost=lost)) and rep.tolist() == m.report.tolist(), f"tick {t}"
    assert same(got[2], rows[2]) and rep[2].tolist() == (0, 0, 0, 0)
    assert got[0].any() and rep[0].tolist()[2:] == (1, 1), "one row of history since the pause: concealed from it, counted from zero"
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_loses_the_listed_frames_and_keeps_the_files_aligned(model, blob, tmp_path):
    """percepnet_run --plc --lose against the Python path, with --rate and, alone, at 48 kHz: the lost frames are read from the files
    and discarded, so every later frame stays aligned; the Python path is handed the extreme code in their place, which is never read"""
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    frames = 12
    for opts, rate in ((["--rate", "8000"], 8000), ([], 48000)):
        n = nof(rate)
        x = inputs("i16", 3, n, 9 + rate // 8000, frames)                       # [frames, 3, n]
        args = []
        for i in range(3):
            np.ascontiguousarray(x[:, i, :]).tofile(tmp_path / f"in{i}.pcm")
            args += [f"in{i}.pcm", f"out{i}.pcm"]
        lose = {0: [7, 8, 9], 2: [8]}
        run = subprocess.run([exe, "--model", "m.pnw"] + opts + ["--plc", "--lose", "0:7-9,2:8"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr
        got = [np.fromfile(tmp_path / f"out{i}.pcm", np.int16) for i in range(3)]
        plain = subprocess.run([exe, "--model", "m.pnw"] + opts + [a.replace("out", "plain") for a in args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0, plain.stderr
        tw = Twin(model, 3, rate if rate != 48000 else "mixed", plc=True)
        if rate == 48000:
            tw.rc.set_stream_rates([0, 1, 2], [48000] * 3)
            tw.rates, tw.w = [48000] * 3, 480
        want = []
        for t in range(frames):
            lost = [s for s, fs in lose.items() if t in fs]
            mark(tw.rc, lost)
            want.append(frame(tw, "i16", poison(x[t], lost, "i16"))[0])
        tw.close()
        for i in range(3):
            w = np.concatenate([want[t][i, :n] for t in range(1, frames)])
            assert got[i].size == w.size and np.array_equal(got[i], w), f"{rate} Hz pair {i}"
        assert np.array_equal(got[1], np.fromfile(tmp_path / "plain1.pcm", np.int16)), "a pair that loses nothing is what it is without --plc"
        assert not np.array_equal(got[0], np.fromfile(tmp_path / "plain0.pcm", np.int16))
