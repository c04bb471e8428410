"""Call-state records of the rate converter (-m gpu): include/percepnet_hip.h "call-state records"; kernel
percepnet_amd/csrc/pn_rate_call.hip, host side pn_rate.cpp (pn_rate_export_call_state / pn_rate_import_call_state and their _host
forms), layout and verdict pn_call_rules.h, bindings api.RateConverter.export_call_state[_dev] / import_call_state[_dev] /
call_state_sections, CLI percepnet_run --migrate-at.

Oracles: the numpy models of the four states (tests/plc_model.py, agc_model.py, lim_model.py, mix_sel_model.py) packed by
tests/call_state_model.py for the records themselves, and for the move an UNBROKEN run of the same streams.  Every comparison is
equality of bits; there is no tolerance anywhere.

Shapes: a source of B = 5 and a target of B = 7 contexts, five live streams at 8, 16, 48, 32 and 24 kHz, four of them in one
conference with loudest-2 and a hold, 22 frames (six of the engine's delay and sixteen of signal)."""
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import agc_model as am
from tests import call_state_model as cs
from tests import lim_model as lm
from tests import mix_sel_model as ms
from tests import plc_model as pm
from tests import test_gpu_plc as tq
from tests import test_gpu_rate_pipe as tp
from tests.test_agc_host import voice

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
same, to_dev, to_host, dev_full, nof = tq.same, tq.to_dev, tq.to_host, tq.dev_full, tq.nof
model = tq.model
default_families = tq.default_families
NONE = api.CONF_NONE
FAMILIES = ("rate_up", "rate_down", "rate_mix", "rate_plc", "rate_agc", "rate_lim")
REPORTS = ("mix", "plc", "agc", "limiter")

# ---- the five streams of a call, by stream (not by slot): a mover sets exactly these on the target
S = 5
RATES = (8000, 16000, 48000, 32000, 24000)
LAWS = (api.G711_ULAW, api.G711_ALAW, api.G711_ULAW, api.G711_ALAW, api.G711_ULAW)
CONFS = (0, 0, 0, 0, NONE)
GAINS = (1.0, 2.0, 1.0, 0.5, 1.0)
CAP, HOLD_D = 2, 0.9
TARGETS = (0.1, 0.05, 0.1, 0.2, 0.1)
CEILINGS = (0.05, 0.05, 0.02, 0.05, 0.03)
LIM_PARAMS = np.array([lm.DEFAULTS[lm.RELEASE], 3.0], F32)
HOME = (0, 1, 2, 3, 4)                  # the slots of the B = 5 source
AWAY = (5, 2, 6, 0, 3)                  # ... and of the B = 7 target: permuted, slots 1 and 4 stay idle
T = 22
LOSSES = {9: (0,), 10: (0, 4), 11: (0, 4)}     # frame -> the streams that lose it: stream 0 (8 kHz, in the conference) for three frames


class Rig:
    """A context of B streams and a mixed converter beside it with stream s of the call in slot slots[s] and, with `features`, every
    setting of the call: laws, the conference with its cap, send gains and hold, PLC, AGC targets, ceilings, all four reports"""

    def __init__(self, model, B, slots, features=True, plc=True, agc=True, lim=True, mix=True):
        self.B, self.slots = B, list(slots)
        self.ctx = api.Context(model, B)
        self.rates = [48000] * B
        for s, sl in enumerate(slots):
            self.rates[sl] = RATES[s]
        self.rc = api.MixedRateConverter(self.ctx, self.rates)
        self.w = self.rc.frame
        self.rc.set_profiling(True)
        self.rc.set_stream_laws(self.slots, list(LAWS))
        self.ctx.set_output_saturate(True)
        self.on = {"mix": False, "plc": False, "agc": False, "limiter": False}
        if not features:
            return
        if mix:
            self.rc.set_stream_confs(self.slots, list(CONFS))
            self.rc.set_conf_speakers([0], [CAP])
            self.rc.set_stream_mix_gains(self.slots, list(GAINS))
            self.rc.set_mix_hold(HOLD_D)
            self.rc.set_mix_report(True)
        if plc:
            self.rc.set_plc(True)
            self.rc.set_plc_report(True)
        if agc:
            self.rc.set_agc(True)
            self.rc.set_agc_report(True)
            self.rc.set_stream_agc_targets(self.slots, list(TARGETS))
        if lim:
            self.rc.set_limiter_params(LIM_PARAMS)
            self.rc.set_stream_limiter(self.slots, list(CEILINGS))
            self.rc.set_limiter_report(True)
        self.on = {"mix": mix, "plc": plc, "agc": agc, "limiter": lim}

    def ids(self):
        """the frame's list: None where the call fills the context, else its slots in ascending order (the _active entry points)"""
        return None if sorted(self.slots) == list(range(self.B)) else sorted(self.slots)

    def rows(self, x, kind):
        """x [S, 480] by stream -> [B, 480] by slot, idle slots silent"""
        r = np.full((self.B, 480), {"f32": 0.0, "i16": 0, "g711": 0xFF}[kind], tq.DTYPE[kind])
        r[self.slots] = x
        return r

    def reports(self):
        return {k: getattr(self.rc, f"read_{k}_report")()[self.slots].copy() for k in REPORTS if self.on[k]}

    def step(self, kind, x, lost=()):
        """one frame through the converter's own entry point -> (out rows, g|r, the four reports), by stream"""
        tq.mark(self.rc, sorted(self.slots[s] for s in lost))
        out, gr = tq.frame(self, kind, self.rows(x, kind), self.ids())
        return out[self.slots], gr[self.slots], self.reports()

    def close(self):
        self.rc.close()
        self.ctx.close()


_inputs = {}


def call_inputs(kind):
    """[T, S, 480]: stream s has its own rate's samples in the first n_s of its row; G.711 rows are the int16 rows in the stream's law"""
    if kind not in _inputs:
        x = np.zeros((T, S, 480), np.int16)
        for s in range(S):
            n = nof(RATES[s])
            x[:, s, :n] = tq.inputs("i16", S, n, 31, T)[:, s, :]
        if kind == "g711":
            g = np.full((T, S, 480), 0xFF, np.uint8)
            for s in range(S):
                g[:, s] = np.asarray(api.g711_encode(LAWS[s], x[:, s].reshape(-1)), np.uint8).reshape(T, 480)
            x = g
        elif kind == "f32":
            x = (x.astype(F32) / F32(32768.0)).astype(F32)
        x.setflags(write=False)
        _inputs[kind] = x
    return _inputs[kind]


def equal_frames(a, b):
    return same(a[0], b[0]) and same(a[1], b[1]) and all(a[2][k].tobytes() == b[2][k].tobytes() for k in a[2])


def export_all(src, form):
    """the three record kinds of the five streams, read only: (engine, tails, call state, the streams that have tails)"""
    import torch
    tails = [s for s in range(S) if RATES[s] != 48000]
    if form == "host":
        eng = src.ctx.export_streams(src.slots)
        tl = {r: src.rc.export_streams([src.slots[s] for s in tails if RATES[s] == r]) for r in sorted({RATES[s] for s in tails})}
        return eng, tl, src.rc.export_call_state(src.slots), tails
    d_eng = dev_full((S, api.STREAM_STATE_BYTES), torch.uint8, 0xEE)
    d_tl = dev_full((len(tails), src.rc.record_stride()), torch.uint8, 0xEE)
    d_cs = dev_full((S, api.RATE_CALL_STATE_BYTES), torch.uint8, 0xEE)
    src.ctx.export_streams_dev(src.slots, d_eng.data_ptr())
    src.rc.export_streams_dev([src.slots[s] for s in tails], d_tl.data_ptr())
    src.rc.export_call_state_dev(src.slots, d_cs.data_ptr())
    return d_eng, d_tl, d_cs, tails


def import_all(dst, form, rec, call_state=True, sync=True):
    """the mover's order on the target: (settings: Rig), the engine's record, the tails, the call state"""
    import torch
    eng, tl, call, tails = rec
    if form == "host":
        dst.ctx.import_streams(dst.slots, eng)
        for r, records in tl.items():
            dst.rc.import_streams([dst.slots[s] for s in tails if RATES[s] == r], records)
        if call_state:
            dst.rc.import_call_state(dst.slots, call)
        return
    st = [dev_full((S,), torch.int32, 99) for _ in range(3)]
    dst.ctx.import_streams_dev(dst.slots, eng.data_ptr(), st[0].data_ptr())
    dst.rc.import_streams_dev([dst.slots[s] for s in tails], tl.data_ptr(), st[1].data_ptr())
    if call_state:
        dst.rc.import_call_state_dev(dst.slots, call.data_ptr(), st[2].data_ptr())
    if sync:
        got = [to_host(dst.ctx, t).tolist() for t in st]
        assert got[0] == [0] * S and got[1][:len(tails)] == [0] * len(tails) and got[2] == ([0] * S if call_state else [99] * S), got
    return st


# ---------------------------------------------------------------------------------------------------------------- 1
COUNTS = (0, 1, 2, 3, 5, 4, 6)          # frames each stream of the B = 7 converter advances: every ring head 0..3, one never touched
KLOSS = {3: (4, 5, 6), 4: (4, 6)}       # tick -> lost: stream 4 ends in the middle of a loss (r = 2), 5 right behind one (r = 1), 6 a frame after (r = 0, P live)


def kernel_run(model):
    """The four kernels alone, tick by tick over active lists, with the models beside them -> (rig, plc, agc, lim, levels)"""
    import torch
    B = 7
    rig = Rig(model, B, (0, 1, 2, 3, 4), features=False)
    confs = [0, 0, 0, NONE, 0, 0, NONE]
    gains = [1.0, 2.0, 1.0, 1.0, 0.5, 1.0, 1.0]
    targets = [0.1, 0.0, 0.05, 0.2, 0.1, 0.1, 0.3]
    ceilings = [0.05, 0.02, 0.0, 0.05, 0.01, 0.05, 0.02]
    every = list(range(B))
    rig.rc.set_stream_confs(every, confs)
    rig.rc.set_conf_speakers([0], [CAP])
    rig.rc.set_stream_mix_gains(every, gains)
    rig.rc.set_mix_hold(HOLD_D)
    rig.rc.set_plc(True)
    rig.rc.set_agc(True)
    rig.rc.set_stream_agc_targets(every, targets)
    rig.rc.set_stream_limiter(every, ceilings)
    plc, agc, lim = pm.Plc(B), am.Agc(B), lm.Lim(B)
    agc.set_targets(every, targets)
    lim.set_ceilings(every, ceilings)
    levels, caps = np.zeros(B, F32), np.array([CAP] + [0] * (B - 1), np.int32)
    x = np.stack([voice(0.02 * (s + 1), max(COUNTS), f0=95.0 + 11.0 * s) for s in range(B)], axis=1)
    o_model = np.zeros((B, 480), F32)
    d_o = dev_full((B, 480), torch.float32, 0.0)
    for t in range(max(COUNTS)):
        ids = [s for s in range(B) if COUNTS[s] > t]
        lost = [s for s in KLOSS.get(t, ()) if s in ids]
        rows = np.array(x[t])
        d = to_dev(rows)
        tq.mark(rig.rc, lost)
        rig.rc.plc_f32_dev(d.data_ptr(), ids=ids)
        rig.rc.agc_f32_dev(d.data_ptr(), ids=ids)
        rig.rc.mix_f32_dev(d.data_ptr(), d_o.data_ptr(), ids=ids)
        rig.rc.lim_f32_dev(d_o.data_ptr(), ids=ids)
        y = agc.frame(plc.frame(rows, lost=lost, ids=ids), ids=ids)
        o_model, levels, _ = ms.mix(y, confs, ids=ids, out=o_model, gains=gains, caps=caps, hold=HOLD_D, levels=levels)
        o_model = lim.frame(o_model, ids=ids)
        assert same(to_host(rig.ctx, d), y) and same(to_host(rig.ctx, d_o), o_model), f"tick {t}: the models follow the kernels"
    return rig, plc, agc, lim, levels


def test_round_trip_against_the_model(model):
    import torch
    rig, plc, agc, lim, levels = kernel_run(model)
    B = rig.B
    assert plc.r.tolist() == [0, 0, 0, 0, 2, 1, 0] and plc.P[4] >= 240 and plc.P[6] >= 240 and plc.lost[6] == 2, "in a loss, right behind one, a frame behind one"
    assert agc.state[0].tobytes() == bytes(16) and lim.state[0].tobytes() == bytes(16) and not plc.hist[0].any(), "a stream never touched"
    assert (lim.state["hold"] > 0).any() and len({float(g) for g in agc.gains()}) > 2 and (levels > 0).any()
    assert rig.rc.call_state_sections() == cs.ALL
    ids = list(range(B)) + [4, 4]                                        # a duplicated id: two equal records
    want = np.stack([cs.pack(s, cs.ALL, plc, agc, lim, levels) for s in ids])
    got_host = rig.rc.export_call_state(ids)
    d_rec = dev_full((len(ids), api.RATE_CALL_STATE_BYTES), torch.uint8, 0xEE)
    rig.rc.export_call_state_dev(ids, d_rec.data_ptr())
    got_dev = to_host(rig.ctx, d_rec)
    for i, s in enumerate(ids):
        assert got_host[i].tobytes() == want[i].tobytes(), f"host form, stream {s} (advanced {COUNTS[s]} frames)"
        assert got_dev[i].tobytes() == want[i].tobytes(), f"device form, stream {s}"
        assert api.rate_call_state_check(got_host[i]) == api.SS_OK
    assert got_host[-1].tobytes() == got_host[-2].tobytes() == got_host[4].tobytes()
    # into the slots of another converter, reversed, and out again: the ring's phase is gone from the record, so the bytes return
    other = Rig(model, B, (0, 1, 2, 3, 4), features=False)
    for f in (lambda r: r.set_plc(True), lambda r: r.set_agc(True), lambda r: r.set_stream_limiter([0], [0.5]), lambda r: r.set_mix_hold(0.5)):
        f(other.rc)
    assert other.rc.call_state_sections() == cs.ALL
    other.rc.import_call_state(list(range(B))[::-1], got_host[:B])
    assert other.rc.export_call_state(list(range(B))[::-1]).tobytes() == got_host[:B].tobytes()
    # and the next tick of the four kernels on the moved state is the models' next tick
    rows = np.stack([voice(0.03, 1, f0=101.0 + 7 * s, start=9)[0] for s in range(B)])
    d = to_dev(rows[::-1].copy())
    other.rc.plc_f32_dev(d.data_ptr())
    other.rc.agc_f32_dev(d.data_ptr())                                   # (no target was set on `other`: the AGC kernel leaves rows and state)
    assert same(to_host(other.ctx, d)[::-1], plc.frame(rows.copy())), "the concealer continues from the imported history: a cross-fade, a third lost frame's neighbour"
    rig.close()
    other.close()


# ---------------------------------------------------------------------------------------------------------------- 2
_reference = {}


def reference(model, kind, cuts_wanted=True):
    """Twin A: the unbroken run of T frames on the B = 5 source, and — read only, between two of its frames — the records of every
    cut.  -> (frames, cuts {name: k}, records {(k, form): ...}).  A is also every split run's first half: a split run's frames 0..k
    ARE A's, since an export changes nothing (which the frames A goes on to give behind every export show too)."""
    if kind in _reference:
        return _reference[kind]
    x = call_inputs(kind)
    a = Rig(model, S, HOME)
    frames = [a.step(kind, x[t], LOSSES.get(t, ())) for t in range(T)]
    a.close()
    plc, agc, lim = [[f[2][k] for f in frames] for k in ("plc", "agc", "limiter")]
    cuts = {"mid_loss": 10, "after_loss": 11}
    assert plc[11]["flags"][0] & api.PLC_CONCEALED and plc[11]["run"][0] == 3 and plc[10]["run"][0] == 2, "frame 11 is the third lost frame of stream 0"
    assert plc[12]["flags"][0] & api.PLC_CROSSFADE and plc[12]["flags"][4] & api.PLC_CONCEALED == 0
    cuts["lim_hold"] = next(k for k in range(12, T - 4) if (lim[k + 1]["flags"] & api.LIM_HOLDING).any())
    cuts["agc_moving"] = next(k for k in range(12, T - 4) if k not in cuts.values() and
                              ((agc[k + 1]["gain"] != agc[k]["gain"]) & (agc[k + 1]["flags"] & api.AGC_ADAPTED != 0)).any())
    _reference[kind] = (frames, cuts)
    return _reference[kind]


def split_runs(model, kind, form, cuts):
    """A second pass of twin A that stops behind every cut k, exports (read only) and goes on; per cut two targets of B = 7 take the
    records — one in the mover's full order, the control without the call-state record — and run the rest -> {k: (moved, control)}"""
    x = call_inputs(kind)
    a = Rig(model, S, HOME)
    out = {}
    for t in range(T):
        a.step(kind, x[t], LOSSES.get(t, ()))
        if t not in cuts.values():
            continue
        rec = export_all(a, form)
        a.ctx.synchronize()                                              # the records are complete before another context's stream reads them
        arms = []
        for call_state in (True, False):
            b = Rig(model, 7, AWAY)
            import_all(b, form, rec, call_state=call_state)
            arms.append({u: b.step(kind, x[u], LOSSES.get(u, ())) for u in range(t + 1, T)})
            b.close()
        out[t] = arms
    a.close()
    return out


@pytest.mark.parametrize("form,kind", (("dev", "i16"), ("host", "g711")))
def test_a_split_run_equals_an_unbroken_run(model, form, kind):
    frames, cuts = reference(model, kind)
    assert len(set(cuts.values())) == 4, cuts
    runs = split_runs(model, kind, form, cuts)
    for name, k in cuts.items():
        moved, control = runs[k]
        for u in range(k + 1, T):
            assert same(moved[u][0], frames[u][0]), f"{name} (cut behind frame {k}): output of frame {u}"
            assert same(moved[u][1], frames[u][1]), f"{name}: g|r of frame {u}"
            for r in REPORTS:
                assert moved[u][2][r].tobytes() == frames[u][2][r].tobytes(), f"{name}: {r} report of frame {u}\n{moved[u][2][r]}\n{frames[u][2][r]}"
        # the control: today's move, without the call-state record, is NOT the unbroken run — in the outputs, not only in a report
        assert any(not same(control[u][0], frames[u][0]) for u in range(k + 1, T)), f"{name}: the move without the record changes nothing: the cut exercises nothing"
        assert not equal_frames(control[k + 1], frames[k + 1]), f"{name}: the first frame behind the cut already shows the lost state"
    print(f"{form} {kind}: cuts {cuts}")


def test_a_split_run_on_the_pipelined_path(model):
    """the export right behind the submit of frame k, the imports right in front of the submit of frame k + 1: no wait around either"""
    kind, k = "i16", 10
    frames, _ = reference(model, kind)
    x = call_inputs(kind)
    a, b = Rig(model, S, HOME), Rig(model, 7, AWAY)
    rot_a, rot_b = tp.Rot(a.ctx, 480, kind, b=S), tp.Rot(b.ctx, 480, kind, b=7)
    box = {}

    def submit_a(t, h_in, h_out, h_gr, h_rep):
        tq.mark(a.rc, sorted(a.slots[s] for s in LOSSES.get(t, ())))
        a.rc.submit_host_i16(h_in, h_out, h_gr)
        if t == k:
            box["rec"] = export_all(a, "dev")

    def submit_b(t, h_in, h_out, h_gr, h_rep):
        if t == k + 1:
            box["st"] = import_all(b, "dev", box["rec"], sync=False)
        tq.mark(b.rc, sorted(b.slots[s] for s in LOSSES.get(t, ())))
        b.rc.submit_host_i16(h_in, h_out, h_gr, ids=b.ids())

    rot_a.run(np.stack([a.rows(x[t], kind) for t in range(T)]), submit_a, frames=range(k + 1))
    a.ctx.synchronize()                                                  # the hand-over between two contexts' streams: the records are complete
    got = rot_b.run(np.stack([b.rows(x[t], kind) for t in range(T)]), submit_b, frames=range(k + 1, T))
    assert [to_host(b.ctx, t).tolist() for t in box["st"]] == [[0] * S, [0] * 4 + [99], [0] * S]
    for i, u in enumerate(range(k + 1, T)):
        for s in range(S):
            n = nof(RATES[s])
            assert same(got[i][0][AWAY[s], :n], frames[u][0][s, :n]) and same(got[i][1][AWAY[s]], frames[u][1][s]), f"frame {u} stream {s}"
    last = b.reports()
    for r in REPORTS:
        assert last[r].tobytes() == frames[T - 1][2][r].tobytes(), r
    for rig, rot in ((a, rot_a), (b, rot_b)):
        rig.close()
        rot.free()


# ---------------------------------------------------------------------------------------------------------------- 3
def warm(rig, seed, ticks=3):
    """state in every held section of every slot without the engine: the four kernels alone on voices, one lost frame"""
    import torch
    B = rig.B
    d_o = dev_full((B, 480), torch.float32, 0.0)
    for t in range(ticks):
        d = to_dev(np.stack([voice(0.01 * (1 + (s + seed) % 5), 1, f0=90.0 + 13.0 * s + seed, start=t)[0] for s in range(B)]))
        if rig.on["plc"]:
            if t == ticks - 1:
                rig.rc.set_lost([rig.slots[0]])
            rig.rc.plc_f32_dev(d.data_ptr())
        if rig.on["agc"]:
            rig.rc.agc_f32_dev(d.data_ptr())
        rig.rc.mix_f32_dev(d.data_ptr(), d_o.data_ptr())
        if rig.on["limiter"]:
            rig.rc.lim_f32_dev(d_o.data_ptr())
    rig.ctx.synchronize()


def section(rec, bit):
    lo, hi = cs.SECTION[bit]
    return np.ascontiguousarray(rec).view(U32).reshape(-1)[4 + lo:4 + hi]


def test_sections(model):
    import torch
    full = Rig(model, S, HOME)
    warm(full, 1)
    assert full.rc.call_state_sections() == cs.ALL
    before = full.rc.export_call_state(HOME)
    for bit in (cs.PLC, cs.AGC, cs.LIM, cs.MIX):
        assert all(section(before[s], bit).any() for s in (0, 1)), f"section {bit} of the warmed converter holds state"
    # a converter that holds the AGC alone
    only = Rig(model, S, HOME, plc=False, lim=False, mix=False)
    warm(only, 2)
    assert only.rc.call_state_sections() == cs.AGC
    rec = only.rc.export_call_state([3, 1])
    w = rec.view(U32).reshape(2, -1)
    assert w[:, :4].tolist() == [[cs.MAGIC, 1, cs.BYTES, cs.AGC]] * 2 and section(rec[0], cs.AGC).any()
    assert not any(section(rec[i], bit).any() for i in range(2) for bit in (cs.PLC, cs.LIM, cs.MIX)), "what is not held is zero"
    # ... into a converter that holds everything: the AGC row is written, the other three of THAT slot are zeroed, no other slot moves
    d_rec, d_st = to_dev(rec), dev_full((2,), torch.int32, 99)
    full.rc.import_call_state_dev([2, 4], d_rec.data_ptr(), d_st.data_ptr())
    assert to_host(full.ctx, d_st).tolist() == [0, 0]
    after = full.rc.export_call_state(HOME)
    for i, s in enumerate((2, 4)):
        assert section(after[s], cs.AGC).tobytes() == section(rec[i], cs.AGC).tobytes()
        assert not any(section(after[s], bit).any() for bit in (cs.PLC, cs.LIM, cs.MIX)), f"slot {s}: a fresh state where the record has none"
    for s in (0, 1, 3):
        assert after[s].tobytes() == before[s].tobytes()
    # a full record into a converter with PLC off: the other three are written, the PLC section is dropped, the status is OK
    noplc = Rig(model, S, HOME, plc=False)
    warm(noplc, 3)
    assert noplc.rc.call_state_sections() == cs.ALL & ~cs.PLC
    noplc.rc.import_call_state([0], before[1:2])
    got = noplc.rc.export_call_state([0])[0]
    assert got.view(U32)[3] == cs.ALL & ~cs.PLC and not section(got, cs.PLC).any()
    for bit in (cs.AGC, cs.LIM, cs.MIX):
        assert section(got, bit).tobytes() == section(before[1], bit).tobytes()
    # a converter that holds nothing: mask 0, all-zero bodies; an import is a no-op that reports OK and launches nothing of the features
    bare, plain = Rig(model, S, HOME, features=False), Rig(model, S, HOME, features=False)
    assert bare.rc.call_state_sections() == 0
    rec0 = bare.rc.export_call_state(HOME)
    assert rec0.tobytes() == np.stack([cs.empty().view(np.uint8)] * S).tobytes()
    d_full, d_st = to_dev(before), dev_full((S,), torch.int32, 99)
    bare.rc.import_call_state_dev(HOME, d_full.data_ptr(), d_st.data_ptr())
    assert to_host(bare.ctx, d_st).tolist() == [0] * S
    bare.rc.import_call_state(HOME, before)
    assert bare.rc.call_state_sections() == 0 and bare.rc.export_call_state(HOME).tobytes() == rec0.tobytes(), "nothing was allocated, nothing written"
    x = call_inputs("i16")
    for t in range(2):
        assert equal_frames(bare.step("i16", x[t]), plain.step("i16", x[t]))
    tb, tpn = bare.rc.kernel_times(FAMILIES), plain.rc.kernel_times(FAMILIES)
    assert all(tb[f][1] == tpn[f][1] for f in FAMILIES) and tb["rate_plc"][1] == tb["rate_agc"][1] == tb["rate_lim"][1] == tb["rate_mix"][1] == 0
    for r in (full, only, noplc, bare, plain):
        r.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def bad_records(good):
    """one good record -> name: (the record made hostile, the verdict)"""
    out = {}
    for name, word, value, verdict in (("magic", 0, 0x53524E50, api.SS_BAD_MAGIC), ("P", 4 + cs.W_META, 1000, api.SS_BAD_STATE),
                                       ("limiter gain 2.0", 4 + cs.W_LIM, int(np.array([2.0], F32).view(U32)[0]), api.SS_BAD_STATE)):
        r = good.copy()
        r.view(U32)[word] = value
        assert api.rate_call_state_check(r) == verdict == cs.verdict(r)
        out[name] = (r, verdict)
    return out


def test_refusals(model):
    import torch
    src, dst = Rig(model, S, HOME), Rig(model, 7, AWAY)
    warm(src, 4)
    warm(dst, 5, ticks=2)
    good = src.rc.export_call_state([0, 1, 2])
    every = list(range(7))
    before = dst.rc.export_call_state(every)
    assert all(before[s].tobytes() != good[i].tobytes() for s in every for i in range(3))
    for name, (bad, verdict) in bad_records(good[1]).items():
        # device form: the bad record sits in the middle of the call; its slot stays, the slots on either side are imported
        rec = np.stack([good[0], bad, good[2]])
        d_rec, d_st = to_dev(rec), dev_full((3,), torch.int32, 99)
        dst.rc.import_call_state_dev([4, 1, 6], d_rec.data_ptr(), d_st.data_ptr())
        assert to_host(dst.ctx, d_st).tolist() == [0, verdict, 0], name
        after = dst.rc.export_call_state(every)
        assert after[4].tobytes() == good[0].tobytes() and after[6].tobytes() == good[2].tobytes(), name
        for s in (0, 1, 2, 3, 5):
            assert after[s].tobytes() == before[s].tobytes(), f"{name}: slot {s} is untouched"
        dst.rc.import_call_state([4, 6], before[[4, 6]])                  # back to where it was
        assert dst.rc.export_call_state(every).tobytes() == before.tobytes()
        # host form: the same record refuses the whole call
        with pytest.raises(api.PercepNetError, match="record 1 refused"):
            dst.rc.import_call_state([4, 1, 6], rec)
        assert dst.rc.export_call_state(every).tobytes() == before.tobytes(), f"{name}: all or nothing"
    # refused on the host with -1: nothing is launched, so neither the state nor the status words move
    d_rec, d_st = to_dev(good), dev_full((3,), torch.int32, 99)
    d_odd = dev_full((3 * api.RATE_CALL_STATE_BYTES + 16,), torch.uint8, 0)
    for ids, ptr, st, word in (([4, 4, 6], d_rec.data_ptr(), d_st.data_ptr(), "twice"), ([4, 7, 6], d_rec.data_ptr(), d_st.data_ptr(), "out of range"),
                               ([4, -1, 6], d_rec.data_ptr(), d_st.data_ptr(), "out of range"), ([4, 1, 6], d_odd.data_ptr() + 4, d_st.data_ptr(), "aligned"),
                               ([4, 1, 6], d_rec.data_ptr(), None, "bad argument"), ([4, 1, 6], None, d_st.data_ptr(), "bad argument")):
        with pytest.raises(api.PercepNetError, match=word):
            dst.rc.import_call_state_dev(ids, ptr, st)
    for ids, ptr, word in (([0, 7], d_rec.data_ptr(), "out of range"), ([0, 1], d_odd.data_ptr() + 8, "aligned"), ([0, 1], None, "bad argument")):
        with pytest.raises(api.PercepNetError, match=word):
            dst.rc.export_call_state_dev(ids, ptr)
    for ids, rec, word in (([4, 4], good[:2], "twice"), ([9], good[:1], "out of range"), ([4, 1], good[:1], "record bytes")):
        with pytest.raises(api.PercepNetError, match=word):
            dst.rc.import_call_state(ids, rec)
    with pytest.raises(api.PercepNetError, match="out of range"):
        dst.rc.export_call_state([7])
    dst.rc.import_call_state_dev([], 0, 0)                               # n == 0: a no-op whatever the pointers
    dst.rc.export_call_state_dev([], 0)
    assert dst.rc.export_call_state([]).shape == (0, api.RATE_CALL_STATE_BYTES)
    assert to_host(dst.ctx, d_st).tolist() == [99] * 3 and dst.rc.export_call_state(every).tobytes() == before.tobytes()
    src.close()
    dst.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_nothing_new_while_unused(model):
    """a converter that never calls the new functions launches what it always launched, frame for frame; one that exports between its
    frames gives the same bits with the same launches, since an export writes nothing of the converter's"""
    never, reader = Rig(model, S, HOME), Rig(model, S, HOME)
    x = call_inputs("i16")
    n = 8
    for t in range(n):
        lost = (1,) if t == 5 else ()
        want = never.step("i16", x[t], lost)
        if t % 2:
            assert api.rate_call_state_check(reader.rc.export_call_state(HOME)[t % S]) == api.SS_OK
        assert equal_frames(reader.step("i16", x[t], lost), want), f"frame {t}"
    tn, tr = never.rc.kernel_times(FAMILIES), reader.rc.kernel_times(FAMILIES)
    for f in FAMILIES:
        assert tn[f][1] == tr[f][1], f
    assert tn["rate_up"][1] == tn["rate_down"][1] == tn["rate_mix"][1] == tn["rate_plc"][1] == tn["rate_agc"][1] == tn["rate_lim"][1] == n, tn
    never.close()
    reader.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_migrate_at_changes_no_byte(model, blob, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    frames, rates = 20, (8000, 16000, 48000)
    args = []
    for i, r in enumerate(rates):
        n = nof(r)
        np.ascontiguousarray(tq.inputs("i16", 3, n, 41, frames)[:, i, :]).tofile(tmp_path / f"in{i}.pcm")
        args += [f"in{i}.pcm", f"out{i}.pcm"]
    # pair 0 loses frames 8..11 and pair 2 frame 9: behind frame 9 one slot moves in the middle of a loss, one right behind a loss
    opts = ["--model", "m.pnw", "--rates", ",".join(str(r) for r in rates), "--saturate", "--plc", "--lose", "0:8-11,2:9", "--agc", "0.1", "--limiter", "0.05",
            "--limiter-hold", "3", "--conference", "0,0,0", "--conf-speakers", "2", "--verbose", "--no-numa"]
    plain = subprocess.run([exe] + opts + [a.replace("out", "plain") for a in args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "moved" not in plain.stderr, plain.stderr
    run = subprocess.run([exe] + opts + ["--migrate-at", "9"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "3 slots moved to a second context behind frame 9" in run.stderr, run.stderr
    for i, r in enumerate(rates):
        got, want = (tmp_path / f"out{i}.pcm").read_bytes(), (tmp_path / f"plain{i}.pcm").read_bytes()
        assert len(want) == 2 * (frames - 1) * nof(r) and got == want, f"--migrate-at 9: pair {i}"
    assert any(np.fromfile(tmp_path / f"out{i}.pcm", np.int16).any() for i in range(3)), "the files hold a signal"
    # refused with a message: no converter to move
    (tmp_path / "gone.pcm").unlink(missing_ok=True)
    run = subprocess.run([exe, "--model", "m.pnw", "--migrate-at", "3", "in2.pcm", "gone.pcm"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "--migrate-at needs a converter" in run.stderr and not (tmp_path / "gone.pcm").exists()
    run = subprocess.run([exe, "--model", "m.pnw", "--rate", "8000", "--migrate-at", "x", "in0.pcm", "gone.pcm"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "--migrate-at: expected a frame number" in run.stderr
