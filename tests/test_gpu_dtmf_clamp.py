"""DTMF removal on the rate converter (-m gpu): include/percepnet_hip.h "DTMF removal"; kernel percepnet_amd/csrc/pn_rate_dtmf_clamp.hip,
host side pn_rate.cpp (pn_rate_set_stream_dtmf_clamp / pn_rate_dtmf_clamp_f32 and the hook in rate_frame), the rule
pn_dtmf_clamp_rules.h, bindings api.RateConverter.set_stream_dtmf_clamp / dtmf_clamp_f32_dev / read_dtmf_clamp_report / dtmf_clamp_state.

The oracle is the numpy model tests/dtmf_clamp_model.py: alone for the kernel over hand-made detector report rows, and for whole frames
applied to the enhanced 48 kHz rows (y48) of a SECOND context and converter that never removes anything, with the detector's model
(tests/dtmf_model.py) on the 48 kHz input rows; behind it the existing models of the stages that follow (conf_model, mix_sel_model,
agc_model, rate_model, g711_model).  Every comparison is equality of bits (NaN-ness where a ramp meets a NaN); no tolerance.

The engine runs at an attenuation limit of 0 dB, the bypass, so that a tone comes out of it at all.

Shapes.  The kernel decides one row per thread, 64 a wave and 256 a block, and makes no passes: batches of 1, 5 and 9 streams for
everything, and for the kernel alone 65 and 257, one row above a wave and above a block."""
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import agc_model as am
from tests import conf_model as cm
from tests import dtmf_clamp_model as dcm
from tests import dtmf_model as dm
from tests import g711_model as gm
from tests import mix_sel_model as msm
from tests import rate_model as rmod
from tests import test_gpu_dtmf as td
from tests import test_gpu_plc as tq
from tests import test_gpu_rate_mixed as tmx
from tests import test_gpu_rate_pipe as tp
from tests.test_agc_host import voice

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
BS = (1, 5, 9)
T = 24
D, C = dm.DEFAULTS, dcm.DEFAULTS
frame, assert_frame, same, to_dev, to_host, dev_full = tq.frame, tq.assert_frame, tq.same, tq.to_dev, tq.to_host, tq.dev_full
model = tq.model
default_families = tq.default_families
Det = td.Det
FAMILIES = ("rate_up", "rate_down", "rate_mix", "rate_plc", "rate_agc", "rate_lim", "rate_dtmf")


@pytest.fixture(scope="module", autouse=True)
def tables():
    ct, st, rot = api.dtmf_tables()
    dm.use_tables(ct, st, rot)


class Pair:
    """A context of len(rates) streams at the bypass and a mixed converter beside it"""

    def __init__(self, model, rates, detect=None, remove=None):
        self.B, self.rates = len(rates), list(rates)
        self.ctx = api.Context(model, self.B)
        self.ctx.set_atten_limit(list(range(self.B)), 0.0)
        self.rc = api.MixedRateConverter(self.ctx, self.rates)
        self.rc.set_stream_laws(list(range(self.B)), [s % 2 for s in range(self.B)])
        self.w = self.rc.frame
        self.rc.set_profiling(True)
        if detect is not None:
            self.rc.set_dtmf_report(True)
            self.rc.set_stream_dtmf(list(range(self.B)), detect)
        if remove is not None:
            self.rc.set_dtmf_clamp_report(True)
            self.rc.set_stream_dtmf_clamp(list(range(self.B)), remove)

    def ns(self):
        return [tq.nof(r) for r in self.rates]

    def close(self):
        self.rc.close()
        self.ctx.close()


class Clamp:
    """The model over B streams: switches, states, the report rows as the kernel leaves them"""

    def __init__(self, B, on=None, params=None):
        self.B, self.params = B, C.copy() if params is None else np.asarray(params, np.int32)
        self.on = np.ones(B, bool) if on is None else np.asarray(on, bool).copy()
        self.state, self.report = dcm.fresh(B), np.zeros((B, 4), U32)

    def set(self, ids, on):
        for s, v in zip(ids, np.broadcast_to(on, (len(ids),))):
            if v and not self.on[s]:
                self.state[s] = 0
            self.on[s] = bool(v)

    def reset(self, ids=None):
        self.state[slice(None) if ids is None else list(ids)] = 0

    def frame(self, det, y, ids=None):
        """det [B, 4]: the detector's report rows of this frame (None: detection off), y [B, 480] -> y', the listed rows worked on"""
        adv = np.ones(self.B, bool) if ids is None else np.isin(np.arange(self.B), list(ids))
        st, out, rep, _ = dcm.frame(self.params, self.state, det, y, on=self.on & adv)
        self.state, self.report[adv] = st, rep[adv]
        return out

    def flags(self, s):
        return int(self.report[s, 0])


def assert_same_as_model(rc, m, what):
    rep, st = rc.read_dtmf_clamp_report().view(U32).reshape(-1, 4), rc.dtmf_clamp_state()
    assert np.array_equal(rep, m.report), f"{what}: report\n{rep}\n{m.report}"
    assert np.array_equal(st, m.state), f"{what}: state, streams {sorted(set(np.argwhere(st != m.state)[:, 0].tolist()))}"


def launches(p, name="rate_clamp"):
    return p.rc.kernel_times((name,))[name][1]


def on_of(B):
    return [s % 5 != 3 for s in range(B)]


# ---------------------------------------------------------------------------------------------------------------- 1: the stage alone
KT = 36


def det_word(flags, cur=0, ended=0):
    return flags | (ord(cur) if cur else 0) << 8 | (ord(ended) if ended else 0) << 16


def script(s):
    """[KT, 4]: hand-made detector report rows of stream s, every row kind of the stage in them, shifted by s % 5 frames.  Idle rows
    are `detector on, no digit`, or four zero words (detection off) on every third stream"""
    idle = (0, 0, 0, 0) if s % 3 == 2 else (dm.ON, 0, 7, ord("5"))
    rows = np.array([idle] * KT, U32)
    o = s % 5
    on = dm.ON | dm.HIT
    rows[2 + o] = (det_word(on, "5"), 4, 1, ord("5"))                  # a mark, two rows without, a mark: one row of zeros between two stretches
    rows[5 + o] = (det_word(on, "5"), 7, 1, ord("5"))
    # the second stretch has left by frame 12 + o, which fades in.  Then a BEGIN whose run is longer than the guard allows: LATE
    rows[13 + o] = (det_word(on | dm.BEGIN, "#"), 5, 2, ord("#"))
    rows[14 + o] = (det_word(on, "#"), 6, 2, ord("#"))
    rows[15 + o] = (det_word(dm.ON | dm.HELD_LOST, "#"), 6, 2, ord("#"))
    rows[16 + o] = (det_word(on | dm.END | dm.BEGIN, "1", "#"), 1, 3, ord("1"))
    rows[17 + o] = (det_word(on, "1"), 2, 3, ord("1"))
    rows[18 + o] = (det_word(dm.ON | dm.END, 0, "1"), 2, 3, ord("1"))
    rows[29 + o] = (det_word(on | dm.BEGIN, "D"), (3, 31, 40, 0xffffffff)[s % 4], 4, ord("D"))      # the shifts at their ends
    rows[30 + o] = (det_word(dm.ON | dm.END, 0, "D"), (3, 31, 40, 0xffffffff)[s % 4], 4, ord("D"))
    return rows


@pytest.mark.parametrize("B", BS + (65, 257))
def test_the_stage_alone_against_the_model(model, B):
    on = on_of(B)
    ctx = api.Context(model, B)
    rc = api.MixedRateConverter(ctx, [48000] * B)
    rc.set_profiling(True)
    rc.set_dtmf_clamp_report(True)
    rc.set_stream_dtmf_clamp(list(range(B)), on)
    m = Clamp(B, on)
    det = np.stack([script(s) for s in range(B)], axis=1)               # [KT, B, 4]
    rng = np.random.default_rng(4733 + B)
    y = rng.standard_normal((KT, B, 480)).astype(F32)
    seen, both = 0, False
    for t in range(KT):
        rows = y[t].copy()
        rows[(7 * t) % B] = np.nan                                       # a row of NaN a frame, walking over the streams
        ids = None
        if t % 4 == 1:
            ids = [int(v) for v in rng.permutation(B)]                   # a shuffled list of everybody
        elif t % 4 == 3 and B > 1:
            ids = [int(v) for v in rng.permutation(B)[:B - 1 - (t % 3 if B > 3 else 0)]]      # a list that leaves streams out: their state stays
        if t == 20:                                                      # a parameter change between two frames
            p = np.array([2, 3, 63, 160], np.int32)
            rc.set_dtmf_clamp_params(p)
            m.params = p
            assert np.array_equal(rc.dtmf_clamp_params(), p)
        rc.set_dtmf_report_rows(det[t])
        d = to_dev(rows)
        rc.dtmf_clamp_f32_dev(d.data_ptr(), ids=ids)
        got = to_host(ctx, d).copy()
        before = m.state.copy()
        want = m.frame(det[t], rows, ids=ids)
        assert cm.same(got, want), f"frame {t}: rows of streams {[s for s in range(B) if not cm.same(got[s], want[s])][:8]}"
        assert_same_as_model(rc, m, f"frame {t}")
        for s in range(B):
            listed = ids is None or s in ids
            f = m.flags(s) if listed and on[s] else 0
            if f & dcm.MUTED or f & (dcm.FADE_IN | dcm.FADE_OUT) == dcm.FADE_IN | dcm.FADE_OUT:
                assert got[s].tobytes() == bytes(1920), (t, s, "removed rows are +0.0, NaN or not")
            elif not f & (dcm.FADE_IN | dcm.FADE_OUT):
                assert same(got[s], rows[s]), (t, s, "a row at unity gain, of a stream that is off or not listed keeps its bits")
            if not (listed and on[s]):
                assert np.array_equal(m.state[s], before[s])
            if listed and on[s]:
                seen |= f
                both |= f & (dcm.FADE_IN | dcm.FADE_OUT) == dcm.FADE_IN | dcm.FADE_OUT
    assert seen == dcm.ON | dcm.MUTED | dcm.FADE_OUT | dcm.FADE_IN | dcm.LATE | dcm.EVENT | dcm.EVENT_END and both, "every row kind"
    assert (m.state[~m.on] == 0).all() and (m.report[~m.on] == 0).all() and m.state[m.on].any()
    assert rc.stream_dtmf_clamp().tolist() == [int(v) for v in on] and rc.kernel_times(("rate_clamp",))["rate_clamp"][1] == KT
    rc.close()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 2: whole frames
TONE_AT, TONE_N = 2, 4320                                                # the tone's first row, 90 ms of it
_key_inputs = {}


def key_inputs(B):
    """-> (x [T, B, 480] float32 at 48 kHz, span {stream: (first sample, behind the last)}): every third stream presses a key — 90 ms
    from somewhere in row 2 on over a little noise — the next speaks, the third is a quiet line"""
    if B not in _key_inputs:
        rng = np.random.default_rng(900 + B)
        x = np.zeros((B, T * 480))
        span = {}
        for s in range(B):
            if s % 3 == 0:
                a = TONE_AT * 480 + (37 * s + 11) % 480
                x[s] = rng.standard_normal(T * 480) * 0.001
                x[s, a:a + TONE_N] += dm.dual_tone(dm.DIGITS[(5 * s + 1) % 16], TONE_N, amp_row=(0.1, 0.25, 0.03)[(s // 3) % 3])
                span[s] = (a, a + TONE_N)
            elif s % 3 == 1:
                x[s] = voice(0.05, T, f0=100.0 + 9.0 * s).ravel()
            else:
                x[s] = rng.standard_normal(T * 480) * 0.01
        a = np.ascontiguousarray(x.reshape(B, T, 480).transpose(1, 0, 2)).astype(F32)
        a.setflags(write=False)
        _key_inputs[B] = (a, span)
    return _key_inputs[B]


def ids_at(B, t, lists):
    """the id list of frame t: a shuffled list of everybody once; stream 0 skips three frames in the middle of its digit"""
    if not lists:
        return None
    if t == 4:
        return [int(v) for v in np.random.default_rng(t).permutation(B)]
    if t in (6, 7, 10):
        return list(range(1, B))
    return None


_runs = {}


def sync_run(model, B, lists):
    """Run B of the whole-frame test through the synchronous entry point -> per frame (out, g|r), the final removal state and report;
    made once (the whole-frame test leaves its own behind)"""
    if (B, lists) not in _runs:
        x, _ = key_inputs(B)
        b = Pair(model, [48000] * B, detect=[True] * B, remove=on_of(B))
        outs = [frame(b, "f32", x[t], ids_at(B, t, lists)) for t in range(T)]
        _runs[B, lists] = (outs, b.rc.dtmf_clamp_state().copy(), b.rc.read_dtmf_clamp_report().copy())
        b.close()
    return _runs[B, lists]


@pytest.mark.parametrize("B,lists", ((1, False), (5, False), (9, False), (5, True), (9, True)), ids=str)
def test_whole_frame_against_a_run_that_never_removes(model, B, lists):
    x, span = key_inputs(B)
    det_on, on = [True] * B, on_of(B)
    a, b = Pair(model, [48000] * B, detect=det_on), Pair(model, [48000] * B, detect=det_on, remove=on)
    det, m = Det(B, det_on), Clamp(B, on)
    outs, muted_at = [], {s: [] for s in range(B)}
    for t in range(T):
        ids = ids_at(B, t, lists)
        ga, gb = frame(a, "f32", x[t], ids), frame(b, "f32", x[t], ids)
        det.frame(x[t], ids=ids)                                         # (48000 Hz float: the up-conversion is a copy, x48 is x)
        adv = range(B) if ids is None else ids
        y48 = np.where(np.isin(np.arange(B), list(adv))[:, None], ga[0], F32(0.0))      # run A's rows ARE its y48: the down-conversion is a copy too
        want = m.frame(det.report, y48, ids=ids)
        for s in adv:
            assert cm.same(gb[0][s], want[s]), f"frame {t} stream {s}"
            assert same(gb[1][s], ga[1][s]), f"frame {t} g|r of stream {s}"
            if m.flags(s) & dcm.MUTED:
                muted_at[s].append(t)
                assert gb[0][s].tobytes() == bytes(1920)
            if s not in span or not on[s]:
                assert same(gb[0][s], ga[0][s]), f"frame {t}: stream {s} has no digit removed and equals run A"
        assert_frame(b, gb, gb, ids, f"frame {t}:")                       # (the rows of unlisted streams keep their sentinel)
        assert_same_as_model(b.rc, m, f"frame {t}")
        td.assert_same_as_model(b, det, f"frame {t}: the detector is what it is without removal")
        assert not np.any(m.report[np.asarray(on)][:, 0] & dcm.LATE), f"frame {t}: nothing is late on any stream that removes"
        outs.append(gb)
    for s, (lo, hi) in span.items():
        if not on[s]:
            assert not muted_at[s]
            continue
        if lists and s == 0:                                             # stream 0 ran on its own frames only: its rows are counted in those
            assert len(muted_at[s]) >= TONE_N // 480
            continue
        for r in range(-(-lo // 480), hi // 480):                        # input rows wholly inside the tone
            assert r + dcm.DELAY in muted_at[s], f"stream {s}: input row {r} is muted six frames later"
        assert int(m.report[s, 3]) == len(muted_at[s]) and int(m.state[s, 2]) == len(muted_at[s])
    assert launches(b) == T and a.rc.kernel_times(("rate_clamp",))["rate_clamp"] == (0.0, 0)
    for name in FAMILIES:
        assert launches(a, name) == launches(b, name), name
    _runs[B, lists] = (outs, b.rc.dtmf_clamp_state().copy(), b.rc.read_dtmf_clamp_report().copy())
    a.close()
    b.close()


def test_pipelined_path_equals_the_synchronous_one(model):
    B, lists = 5, True
    outs, state, report = sync_run(model, B, lists)
    x, _ = key_inputs(B)
    p = Pair(model, [48000] * B, detect=[True] * B, remove=on_of(B))
    rot = tp.Rot(p.ctx, 480, "f32", b=B)

    def submit(t, h_in, h_out, h_gr, h_rep):
        p.rc.submit_host_f32(h_in, h_out, h_gr, ids=ids_at(B, t, lists))

    got = rot.run(np.array(x), submit)
    for t in range(T):
        ids = ids_at(B, t, lists)
        for s in range(B) if ids is None else ids:
            assert cm.same(got[t][0][s], outs[t][0][s]) and same(got[t][1][s], outs[t][1][s]), f"frame {t} stream {s}"
    assert np.array_equal(p.rc.dtmf_clamp_state(), state) and p.rc.read_dtmf_clamp_report().tobytes() == report.tobytes()
    assert p.ctx.frames_delivered() == T and launches(p) == T
    p.close()
    rot.free()


@pytest.mark.parametrize("kind,rate", (("i16", 16000), ("g711", 8000)))
def test_low_rate_streams_against_the_rate_and_g711_models(model, kind, rate):
    """int16 at 16 kHz and G.711 at 8 kHz on a mixed converter: run A by hand (up, the engine) gives x48 and y48; run B's output equals
    the down-conversion's model, the int16 cast and the G.711 encoder's model over the removal model's rows"""
    import torch
    B, frames = 5, 20
    on = on_of(B)
    a, b = Pair(model, [rate] * B), Pair(model, [rate] * B, detect=[True] * B, remove=on)
    x = td.tone_inputs(kind, a, frames)
    n = tq.nof(rate)
    det, m = Det(B), Clamp(B, on)
    down = [tmx.DownModel(rate) for _ in range(B)]
    nan = float("nan")
    muted = 0
    for t in range(frames):
        d_in = to_dev(np.array(x[t]))
        x48, y48, d_gr = dev_full((B, 480), torch.float32, nan), dev_full((B, 480), torch.float32, nan), dev_full((B, 68), torch.float32, nan)
        getattr(a.rc, f"up_{kind}_dev")(d_in.data_ptr(), x48.data_ptr())
        a.ctx.process_f32_dev(x48.data_ptr(), y48.data_ptr(), d_gr.data_ptr())
        gb = frame(b, kind, x[t])
        det.frame(to_host(a.ctx, x48).copy())
        want48 = m.frame(det.report, to_host(a.ctx, y48).copy())
        for s in range(B):
            v = rmod.to_i16(down[s](want48[s]), False)
            want = v if kind == "i16" else gm.encode(s % 2, v)
            assert same(np.ascontiguousarray(gb[0][s, :n]), np.ascontiguousarray(want)), f"{kind} frame {t} stream {s}"
            assert same(gb[1][s], to_host(a.ctx, d_gr)[s])
        assert_same_as_model(b.rc, m, f"{kind} frame {t}")
        td.assert_same_as_model(b, det, f"{kind} frame {t}")
        muted += int(np.count_nonzero(m.report[:, 0] & dcm.MUTED))
    assert muted >= 3 * 4 and not np.any(m.report[:, 0] & dcm.LATE), "digits were found and removed"
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 3: the stages behind it
_conf_x = {}


def conference_inputs():
    """[T, 3, 480]: member 0 speaks quietly and presses a key, loudly, for 90 ms; members 1 and 2 speak"""
    if not _conf_x:
        x = np.stack([voice(0.01, T, f0=110.0).ravel(), voice(0.05, T, f0=150.0).ravel(), voice(0.03, T, f0=205.0).ravel()]).astype(np.float64)
        a = TONE_AT * 480 + 77
        x[0, a:a + TONE_N] += dm.dual_tone("8", TONE_N, amp_row=0.25)
        _conf_x["x"] = np.ascontiguousarray(x.reshape(3, T, 480).transpose(1, 0, 2)).astype(F32)
        _conf_x["x"].setflags(write=False)
    return _conf_x["x"]


def test_conference_of_three_one_member_presses_a_key(model):
    """p: no conference, nothing removed: its rows are every member's y48.  plain, capped: conferences with removal on, loudest-N off
    and at 1; loud: the capped conference WITHOUT removal, to show what the tone does there"""
    B, confs = 3, [0, 0, 0]
    x = conference_inputs()
    everybody = list(range(B))
    p = Pair(model, [48000] * B)
    plain, capped = Pair(model, [48000] * B, detect=[True] * B, remove=[True] * B), Pair(model, [48000] * B, detect=[True] * B, remove=[True] * B)
    loud = Pair(model, [48000] * B, detect=[True] * B)
    for q in (plain, capped, loud):
        q.rc.set_stream_confs(everybody, confs)
    for q in (capped, loud):
        q.rc.set_conf_speakers([0], [1])
        q.rc.set_mix_report(True)
    det, m = Det(B), Clamp(B)
    caps = np.array([1, 0, 0], np.int32)
    lv, rep = None, None
    pressed, chosen_without = 0, 0
    for t in range(T):
        y48 = frame(p, "f32", x[t])[0]
        det.frame(x[t])
        clean = m.frame(det.report, y48)
        got = frame(plain, "f32", x[t])[0]
        assert cm.same(got, cm.mix(clean, confs)), f"frame {t}: the listeners hear the mix of the removed rows"
        got = frame(capped, "f32", x[t])[0]
        o, lv, rep = msm.mix(clean, confs, caps=caps, levels=lv, report=rep)
        assert cm.same(got, o) and msm.same_report(capped.rc.read_mix_report(), rep), f"frame {t}: loudest-1 over the removed rows"
        assert_same_as_model(capped.rc, m, f"frame {t}")
        frame(loud, "f32", x[t])
        if m.flags(0) & dcm.MUTED:
            pressed += 1
            assert not int(capped.rc.read_mix_report()["flags"][0]) & api.MIX_SELECTED, f"frame {t}: the presser is not selected during the digit"
            assert got[1].tobytes() == clean[2].tobytes() or got[1].tobytes() == bytes(1920), "member 1 hears member 2 or nobody, never the key"
            chosen_without += bool(int(loud.rc.read_mix_report()["flags"][0]) & api.MIX_SELECTED)
    assert pressed >= TONE_N // 480 and chosen_without >= TONE_N // 480 - 1, "without removal the tone wins loudest-1 in every row it fills"
    for q in (p, plain, capped, loud):
        q.close()


def test_level_control_holds_its_gain_across_the_muted_rows(model):
    B = 3
    x = conference_inputs()
    p, g = Pair(model, [48000] * B), Pair(model, [48000] * B, detect=[True] * B, remove=[True] * B)
    g.rc.set_agc(True)
    g.rc.set_agc_report(True)
    g.rc.set_stream_agc_targets(list(range(B)), [0.1] * B)
    det, m, agc = Det(B), Clamp(B), am.Agc(B)
    agc.set_targets(list(range(B)), [0.1] * B)
    gains = []
    for t in range(T):
        y48 = frame(p, "f32", x[t])[0]
        det.frame(x[t])
        want = agc.frame(m.frame(det.report, y48))
        assert cm.same(frame(g, "f32", x[t])[0], want), f"frame {t}"
        assert g.rc.read_agc_report().tobytes() == agc.report.tobytes(), f"frame {t}: the level control's report"
        gains.append((bool(m.flags(0) & dcm.MUTED), agc.gains()[0].view(U32)))
    held = [v for mu, v in gains if mu]
    first = next(i for i, (mu, _) in enumerate(gains) if mu)
    assert len(held) >= TONE_N // 480 and all(v == gains[first - 1][1] for v in held), "the gain in front of the digit is held through it"
    assert len({int(v) for _, v in gains}) > 3, "the gain does move elsewhere"
    p.close()
    g.close()


# ---------------------------------------------------------------------------------------------------------------- 4: off, resets, refusals
@pytest.mark.parametrize("B", (5,))
def test_nothing_new_while_removal_is_on_for_nobody(model, B):
    x, _ = key_inputs(B)
    det_on = [True] * B
    never, off = Pair(model, [48000] * B, detect=det_on), Pair(model, [48000] * B, detect=det_on)
    off.rc.set_stream_dtmf_clamp(list(range(B)), 1)                      # on, then off again for everybody
    off.rc.set_stream_dtmf_clamp(list(range(B)), 0)
    off.rc.set_dtmf_clamp_report(True)
    det = Det(B)
    for t in range(12):
        want = frame(never, "f32", x[t])
        got = frame(off, "f32", x[t])
        assert same(got[0], want[0]) and same(got[1], want[1]), f"frame {t}"
        det.frame(x[t])
        for q in (never, off):
            td.assert_same_as_model(q, det, f"frame {t}: detection alone gives what it gives today")
    for q in (never, off):
        assert q.rc.kernel_times(("rate_clamp",))["rate_clamp"] == (0.0, 0), "nobody on, no launch"
    for name in FAMILIES:
        assert launches(never, name) == launches(off, name) == (12 if name in ("rate_up", "rate_down", "rate_dtmf") else 0), name
    assert not never.rc.dtmf_clamp_state().any() and not off.rc.dtmf_clamp_state().any() and not off.rc.read_dtmf_clamp_report().view(U32).any()
    assert never.rc.stream_dtmf_clamp().tolist() == off.rc.stream_dtmf_clamp().tolist() == [0] * B
    never.close()
    off.close()


@pytest.mark.parametrize("form", ("host", "dev"))
def test_the_resets_zero_the_removal_state(model, form):
    import torch
    B = 9
    rates = [8000, 8000, 8000, 16000, 48000, 48000, 24000, 48000, 32000]
    p = Pair(model, rates, remove=[True] * B)
    m = Clamp(B)
    busy = np.tile(np.array([det_word(dm.ON | dm.HIT, "7"), 9, 1, ord("7")], U32), (B, 1))
    t = 0

    def tick(ids=None):
        nonlocal t
        rows = np.full((B, 480), 0.25, F32)
        p.rc.set_dtmf_report_rows(busy)
        d = to_dev(rows)
        p.rc.dtmf_clamp_f32_dev(d.data_ptr(), ids=ids)
        want = m.frame(busy, rows, ids=ids)
        assert cm.same(to_host(p.ctx, d), want), f"tick {t}"
        assert_same_as_model(p.rc, m, f"tick {t}")
        t += 1

    for _ in range(8):
        tick()
    assert m.state.all(axis=0)[[0, 1, 2, 3]].all(), "marks, cut, muted rows and an event's dur everywhere"
    p.rc.reset_streams([1, 4])
    m.reset([1, 4])
    assert not p.rc.dtmf_clamp_state()[[1, 4]].any() and p.rc.dtmf_clamp_state()[0].all()
    tick()
    tick(ids=[0, 1, 2])                                                  # a stream that does not advance keeps its state
    p.rc.set_stream_rates([3, 7], [8000, 16000])
    m.reset([3, 7])
    tick()
    if form == "host":
        p.rc.import_streams([1, 2], p.rc.export_streams([0] * 2))
    else:
        stride = p.rc.record_stride()
        d_rec, d_st = dev_full((2, stride), torch.uint8, 0), dev_full((2,), torch.int32, 99)
        p.rc.export_streams_dev([0] * 2, d_rec.data_ptr())
        p.rc.import_streams_dev([1, 2], d_rec.data_ptr(), d_st.data_ptr())
        assert to_host(p.ctx, d_st).tolist() == [api.SS_OK] * 2
    m.reset([1, 2])
    assert not p.rc.dtmf_clamp_state()[[1, 2]].any() and p.rc.dtmf_clamp_state()[0].all(), "the slot that was only exported keeps its state"
    tick()
    p.rc.set_stream_dtmf_clamp([5, 6], [0, 1])                           # off keeps the state; on for a stream that is on keeps it too
    m.set([5, 6], [0, 1])
    tick()
    p.rc.set_stream_dtmf_clamp([5], [1])                                 # on for a stream that was off: a fresh state
    m.set([5], [1])
    assert not p.rc.dtmf_clamp_state()[5].any() and p.rc.dtmf_clamp_state()[6].all()
    tick()
    p.rc.reset()
    m.reset()
    assert not p.rc.dtmf_clamp_state().any()
    tick()
    assert p.rc.stream_dtmf_clamp().tolist() == [1] * B and np.array_equal(p.rc.dtmf_clamp_params(), C), "switches and parameters are settings: they survive"
    p.close()


def test_refusals_change_nothing(model):
    B = 3
    p = Pair(model, [48000] * B)
    assert np.array_equal(p.rc.dtmf_clamp_params(), C) and p.rc.stream_dtmf_clamp().tolist() == [0] * B
    with pytest.raises(api.PercepNetError, match="pn_rate_set_dtmf_clamp_report"):
        p.rc.read_dtmf_clamp_report()
    # the guard must be in time for the detector's on_frames: all three setters refuse what breaks it, naming the values
    for on_frames, pre in ((5, 1), (6, 0)):
        d, c = D.copy(), C.copy()
        d[dm.ON_FRAMES], c[dcm.PRE] = on_frames, pre
        word = f"on_frames {on_frames} \\+ pre {pre} > 5"
        if pre != 1:                                                     # the parameters first, nobody on: the switch is refused
            p.rc.set_dtmf_clamp_params(c)
        p.rc.set_dtmf_params(d)
        with pytest.raises(api.PercepNetError, match=word):
            p.rc.set_stream_dtmf_clamp([0], [1])
        if pre == 1:
            with pytest.raises(api.PercepNetError, match=word):
                p.rc.set_dtmf_clamp_params(c)
        assert p.rc.stream_dtmf_clamp().tolist() == [0] * B
        p.rc.set_dtmf_params(D)
        p.rc.set_dtmf_clamp_params(C)
        p.rc.set_stream_dtmf_clamp([0], [1])                             # somebody on: now the detector's parameters are refused
        with pytest.raises(api.PercepNetError, match=f"on_frames {on_frames} \\+ pre 1 > 5"):
            p.rc.set_dtmf_params(d)
        c2 = C.copy()
        c2[dcm.PRE] = 3
        with pytest.raises(api.PercepNetError, match="on_frames 3 \\+ pre 3 > 5"):
            p.rc.set_dtmf_clamp_params(c2)
        assert same(p.rc.dtmf_params(), D) and np.array_equal(p.rc.dtmf_clamp_params(), C)
        p.rc.set_stream_dtmf_clamp([0], [0])
    for on_frames, pre in ((5, 0), (4, 1)):                              # ... and what is in time is accepted
        d, c = D.copy(), C.copy()
        d[dm.ON_FRAMES], c[dcm.PRE] = on_frames, pre
        p.rc.set_dtmf_clamp_params(c)
        p.rc.set_dtmf_params(d)
        p.rc.set_stream_dtmf_clamp([0, 2], [1, 1])
        p.rc.set_stream_dtmf_clamp([0, 2], [0, 0])
        p.rc.set_dtmf_params(D)
    p.rc.set_dtmf_clamp_params(C)
    for i, v in ((dcm.PRE, 5), (dcm.POST, 9), (dcm.VOLUME, 64), (dcm.TS_PER_FRAME, 0), (dcm.POST, -1)):
        c = C.copy()
        c[i] = v
        with pytest.raises(api.PercepNetError, match=f"index {i} "):
            p.rc.set_dtmf_clamp_params(c)
    for ids, on, word in (([B], [1], "out of range"), ([-1], [1], "out of range"), ([1, 1], [1, 1], "twice")):
        with pytest.raises(api.PercepNetError, match=word):
            p.rc.set_stream_dtmf_clamp(ids, on)
    d = to_dev(np.zeros((B, 480), F32))
    with pytest.raises(api.PercepNetError, match="twice"):
        p.rc.dtmf_clamp_f32_dev(d.data_ptr(), ids=[2, 2])
    with pytest.raises(api.PercepNetError, match="aligned"):
        p.rc.dtmf_clamp_f32_dev(d.data_ptr() + 4)
    with pytest.raises(api.PercepNetError, match="rate_up, rate_down, rate_mix, rate_plc, rate_agc, rate_lim, rate_dtmf, rate_clamp"):
        p.rc.kernel_times(("rate_xyz",))
    # removal on, detection on, the user's detector report off: reading it is refused as it is today, and removal works all the same
    p.rc.set_stream_dtmf([0, 1, 2], 1)
    p.rc.set_stream_dtmf_clamp([0, 1, 2], 1)
    p.rc.set_dtmf_clamp_report(True)
    x = conference_inputs()
    for t in range(14):
        frame(p, "f32", x[t])
    with pytest.raises(api.PercepNetError, match="pn_rate_set_dtmf_report"):
        p.rc.read_dtmf_report()
    rep = p.rc.read_dtmf_clamp_report()
    assert int(rep["flags"][0]) & dcm.MUTED and int(rep["muted"][0]) >= 4 and not rep["muted"][1:].any()
    p.rc.set_stream_dtmf_clamp([], [])
    assert np.array_equal(p.rc.dtmf_clamp_params(), C) and p.rc.stream_dtmf_clamp().tolist() == [1, 1, 1]
    p.close()


def test_removal_on_and_detection_off_leaves_the_stream_alone(model):
    """detection on for nobody: the detector does not run, whatever its report rows hold is not read, and marks drain"""
    B = 5
    x, _ = key_inputs(B)
    a, b = Pair(model, [48000] * B), Pair(model, [48000] * B, remove=[True] * B)
    stale = np.tile(np.array([det_word(dm.ON | dm.HIT | dm.BEGIN, "7"), 9, 1, ord("7")], U32), (B, 1))
    b.rc.set_dtmf_report_rows(stale)
    m = Clamp(B)
    for t in range(10):
        ga, gb = frame(a, "f32", x[t]), frame(b, "f32", x[t])
        assert same(ga[0], gb[0]) and same(ga[1], gb[1]), f"frame {t}"
        m.frame(None, ga[0])
        assert_same_as_model(b.rc, m, f"frame {t}")
    assert launches(b) == 10 and not m.state.any() and (m.report[:, 0] == dcm.ON).all()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_dtmf_clamp_prints_each_ended_event_and_mutes_the_digit(model, blob, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    B = 3
    x = np.rint(conference_inputs().astype(np.float64) * 32767.0).astype(np.int16)       # [T, 3, 480]: pair 0 presses '8'
    args = []
    for i in range(B):
        np.ascontiguousarray(x[:, i]).tofile(tmp_path / f"in{i}.pcm")
        args += [f"in{i}.pcm", f"out{i}.pcm"]
    base = [exe, "--model", "m.pnw", "--atten-lim", "0", "--dtmf"]
    run = subprocess.run(base + ["--dtmf-clamp", "--dtmf-guard", "1,1"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    plain = subprocess.run(base + [a.replace("out", "plain") for a in args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    p = Pair(model, [48000] * B, detect=[True] * B, remove=[True] * B)
    p.rc.set_dtmf_clamp_params([1, 1, 10, 80])
    want, outs = [], []
    for t in range(T):
        outs.append(frame(p, "i16", x[t])[0])
        rep = p.rc.read_dtmf_clamp_report()
        want += [f"dtmf-event: pair {s} frame {t} event {int(rep[s]['event_end']) >> 24} end 1 duration {int(rep[s]['event_end']) & 0xffff}"
                 for s in range(B) if int(rep[s]["flags"]) & dcm.EVENT_END]
    p.close()
    got = [ln for ln in run.stdout.splitlines() if ln.startswith("dtmf-event:")]
    assert len(want) == 1 and " event 8 end 1 " in want[0] and got == want, (got, want)
    assert [ln for ln in run.stdout.splitlines() if ln.startswith("dtmf:")] == [ln for ln in plain.stdout.splitlines() if ln.startswith("dtmf:")] != []
    out0 = np.fromfile(tmp_path / "out0.pcm", np.int16).reshape(-1, 480)
    assert out0.shape[0] >= T - 1 and np.count_nonzero(~out0.any(axis=1)) >= TONE_N // 480, "the digit's rows are silence"
    for i in (1, 2):
        assert (tmp_path / f"out{i}.pcm").read_bytes() == (tmp_path / f"plain{i}.pcm").read_bytes(), f"pair {i} pressed nothing: its audio is what it is without --dtmf-clamp"
    assert (tmp_path / "out0.pcm").read_bytes() != (tmp_path / "plain0.pcm").read_bytes()
