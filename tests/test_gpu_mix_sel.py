"""Loudest-N selection, send gains, the hold and the mix report of the conference mix (-m gpu): include/percepnet_hip.h "conferences:
loudest-N talkers, send gains, mix report"; kernel percepnet_amd/csrc/pn_rate_mix.hip pn_rate_mix_sel_kernel, host side pn_rate.cpp
(rate_mix and the setting calls), rules pn_mix_rules.h, bindings api.RateConverter.set_stream_mix_gains / set_conf_speakers /
set_mix_hold / set_mix_report / read_mix_report, CLI percepnet_run --conf-speakers / --mix-gains.

The oracle is the numpy float32 model tests/mix_sel_model.py: alone for the kernel, and for whole frames inside the composition
pn_rate_up_* -> pn_process_f32[_active] -> model -> pn_rate_down_* on a SECOND context and converter that never has a conference,
as tests/test_gpu_conf.py does it.  Every comparison is equality of bits (of NaN-ness where a value is NaN); no tolerance.

Shapes: the context of tests/test_gpu_conf.py, B = 48 streams with conferences of 32, 5, 4, 3, 2 and 1 scattered over the slots, its
id lists (which bring the big conference to 17, 16, 9, 8 and 1 advancing members, the kernel's size-class edges) and its rates and
laws."""
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import conf_model as cm
from tests import families
from tests import mix_sel_model as mm
from tests import report_model as rm
from tests import test_gpu_conf as tc
from tests import test_gpu_rate_pipe as tp
from tests.test_gpu_conf import B, CONFS, KERNEL_LISTS, LAWS, LONER, PERM, RATES, SENTINEL, T, Twin, nof, to_dev, to_host, dev_full

pytestmark = pytest.mark.gpu
F32 = np.float32
NONE = cm.NONE
BIG, FIVE, FOUR, THREE, TWO, ONE = (cm.members(CONFS, c) for c, _ in tc.SIZES)
ALL = list(range(B))


def caps_of(by_size):
    """caps [B] by conference number from {member count: N}"""
    caps = [0] * B
    for c, k in tc.SIZES:
        caps[c] = by_size[k]
    return caps


CAPS1 = caps_of({32: 3, 5: 5, 4: 1, 3: 0, 2: 1, 1: 1})               # N < k, N = k, N = 1 and "all"
MUTED = (BIG[1], BIG[20])
GAINS1 = np.ones(B, F32)
GAINS1[list(MUTED)] = 0
GAINS1[BIG[5]], GAINS1[BIG[9]] = F32(0.5), F32(1e-20)
NAN_ROW, TIE, ZERO_ROW, INF_ROW = BIG[3], (BIG[7], BIG[12], BIG[25]), BIG[15], FIVE[2]


def sel_rows():
    """[B, 480]: gaussian rows scaled per slot (distinct levels); in the big conference a muted member with +inf in its row, an
    all-NaN row (rank 1 of N = 3), the three loudest finite rows an exact tie — a row, a copy of it and its negation, at ranks 2, 3
    and 4, across the cut — a row of zeros; in the conference of five a row with one +inf sample"""
    rng = np.random.default_rng(5200)
    y = rng.standard_normal((B, 480)).astype(F32) * (F32(0.5) + F32(0.03125) * np.arange(B, dtype=F32))[:, None]
    y[MUTED[0], 10] = np.inf
    y[NAN_ROW] = np.nan
    y[TIE[0]] = rng.standard_normal(480).astype(F32) * F32(40)
    y[TIE[1]] = y[TIE[0]]
    y[TIE[2]] = -y[TIE[0]]
    y[ZERO_ROW] = 0
    y[INF_ROW, 33] = np.inf
    return y


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


def settings(tw, gains=None, caps=None, hold=None, report=None):
    if gains is not None:
        tw.rc.set_stream_mix_gains(ALL, gains)
        assert tw.rc.stream_mix_gains().tolist() == [float(g) for g in gains]
    if caps is not None:
        tw.rc.set_conf_speakers(ALL, caps)
        assert tw.rc.conf_speakers().tolist() == list(caps)
    if hold is not None:
        tw.rc.set_mix_hold(hold)
        assert tw.rc.mix_hold() == float(F32(hold))
    if report is not None:
        tw.rc.set_mix_report(report)


def kernel(tw, y, ids=None):
    """pn_rate_mix_f32 on rows y -> (out rows over a sentinel, the mix report when it is on)"""
    import torch
    d_in, d_out = to_dev(y), dev_full((B, 480), torch.float32, float(SENTINEL["f32"]))
    tw.rc.mix_f32_dev(d_in.data_ptr(), d_out.data_ptr(), ids=ids)
    got = to_host(tw.ctx, d_out)
    assert tc.same(to_host(tw.ctx, d_in), y), "the input rows are read only"
    return got


def assert_rows(got, want, ids, what):
    for s in range(B):
        assert cm.same(got[s], want[s]), f"{what}: stream {s} (conference {CONFS[s]})"
        if ids is not None and s not in ids:
            assert (got[s] == SENTINEL["f32"]).all(), f"{what}: the row of unlisted stream {s} keeps its sentinel"


def assert_report(got, want, ids, what):
    for s in (ALL if ids is None else ids):
        assert mm.same_report(got[s:s + 1], want[s:s + 1]), f"{what}: record of stream {s}: {got[s]} != {want[s]}"


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_selection_rows_hold_what_they_must():
    y = sel_rows()
    o, lv, rep = mm.mix(y, CONFS, gains=GAINS1, caps=CAPS1)
    assert len({float(v) for v in lv[[s for s in ALL if CONFS[s] != NONE and GAINS1[s] != 0 and s not in TIE and s != NAN_ROW]]}) == B - 1 - 2 - 3 - 1, "distinct levels"
    assert np.isnan(lv[NAN_ROW]) and lv[TIE[0]] == lv[TIE[1]] == lv[TIE[2]] and lv[ZERO_ROW] == 0 and lv[INF_ROW] == np.inf
    sel = [s for s in BIG if rep["flags"][s] & 1]
    assert sel == sorted([NAN_ROW, TIE[0], TIE[1]]), "NaN first, then the two lower slots of the tie; the negated row is cut"
    quiet = [s for s in BIG if s not in sel]
    assert all(np.isnan(o[s]).all() for s in quiet + list(TIE[:2])) and not np.isnan(o[NAN_ROW]).any(), "the NaN talker's listeners hear NaN, it does not"
    assert all(rep["flags"][s] == 6 and lv[s] == 0 for s in MUTED)
    x = GAINS1[BIG[9]] * y[BIG[9]]
    assert 0 < (x * x).max() < np.finfo(F32).tiny and 0 < lv[BIG[9]] == mm.level(x), "the products of the 1e-20 member are subnormal, its level is their sum"
    assert (rep["flags"][FIVE] == 5).all() and sum(rep["flags"][s] & 1 for s in FOUR) == 1 and (rep["flags"][THREE] == 5).all()
    assert np.isinf(o[FIVE[0], 33]) and not np.isinf(o[INF_ROW]).any()


@pytest.fixture(scope="module")
def sel_twin(model):
    tw = Twin(model, "mixed", CONFS)
    settings(tw, gains=GAINS1, caps=CAPS1, report=True)
    yield tw
    tw.close()


@pytest.mark.parametrize("which", list(KERNEL_LISTS))
def test_kernel_alone_against_the_model(sel_twin, which):
    tw, ids = sel_twin, KERNEL_LISTS[which]
    y = sel_rows()
    tw.rc.set_mix_hold(0.0)                                            # (zeroes every level: each list starts from nothing)
    before = tw.rc.read_mix_report()
    got = kernel(tw, y, ids)
    want, lv, rep = mm.mix(y, CONFS, ids, out=np.full((B, 480), SENTINEL["f32"], F32), gains=GAINS1, caps=CAPS1, report=before)
    assert_rows(got, want, ids, f"list {which}")
    got_rep = tw.rc.read_mix_report()
    assert_report(got_rep, rep, ids, f"list {which}")
    for s in ALL:
        if ids is not None and s not in ids:
            assert got_rep[s].tobytes() == before[s].tobytes(), f"list {which}: the record of unlisted stream {s} is left as it was"
    adv = ALL if ids is None else ids
    # the muted member's +inf reaches nobody: 0 * inf would be a NaN in every listener's column 10
    assert not any(np.isnan(got[s, 10]) for s in adv if s in BIG and NAN_ROW not in adv), f"list {which}"
    assert NAN_ROW not in adv or not np.isnan(got[NAN_ROW]).any(), f"list {which}: the NaN talker hears the others, the muted +inf not among them"


# ---------------------------------------------------------------------------------------------------------------- 2
def test_same_arithmetic_as_the_plain_kernel(model):
    tw = Twin(model, "mixed", CONFS)
    y = tc.kernel_rows()
    plain = {which: kernel(tw, y, ids) for which, ids in KERNEL_LISTS.items()}
    for caps in (None, [32] * B):
        settings(tw, caps=caps, report=True)                           # the selecting kernel, forced by the report alone; then N = 32
        for which, ids in KERNEL_LISTS.items():
            got = kernel(tw, y, ids)
            want = cm.mix(y, CONFS, ids, out=np.full((B, 480), SENTINEL["f32"], F32))
            assert_rows(got, want, ids, f"N = {caps and 32}, list {which}")
            assert_rows(got, plain[which], ids, f"N = {caps and 32}, list {which}, against the plain kernel")
            rep = tw.rc.read_mix_report()
            assert all(rep["flags"][s] == (0 if CONFS[s] == NONE else 5) for s in (ALL if ids is None else ids))
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_back_to_plain(model):
    # without a conference: a setting off its default runs the mix (every row a copy), every setting back at its default runs nothing
    a, b = Twin(model, 8000), Twin(model, 8000)
    x = tc.inputs("i16", 80, 3)
    a.rc.set_profiling(True)
    b.rc.set_profiling(True)
    settings(a, gains=GAINS1, caps=CAPS1, hold=0.5, report=True)
    for t in range(3):
        got, want = tc.frame(a, "i16", x[t]), tc.frame(b, "i16", x[t])
        assert tc.same(got[0], want[0]) and tc.same(got[1], want[1]), f"frame {t}: nobody is in a conference"
    assert a.rc.kernel_times(("rate_mix",))["rate_mix"][1] == 3 and b.rc.kernel_times(("rate_mix",))["rate_mix"][1] == 0
    rep = a.rc.read_mix_report()
    assert rep.tobytes() == bytes(16 * B), "zero records"
    for back in (dict(gains=np.ones(B, F32)), dict(caps=[0] * B), dict(hold=0.0)):
        settings(a, **back)
        tc.frame(a, "i16", x[3])
        tc.frame(b, "i16", x[3])
    assert a.rc.kernel_times(("rate_mix",))["rate_mix"][1] == 6, "the report alone keeps the selecting kernel on"
    settings(a, report=False)
    a.rc.reset_profile()
    for t in range(4, 7):
        got, want = tc.frame(a, "i16", x[t]), tc.frame(b, "i16", x[t])
        assert tc.same(got[0], want[0]) and tc.same(got[1], want[1]), f"frame {t}"
    assert a.rc.kernel_times(("rate_up", "rate_down", "rate_mix")) and a.rc.kernel_times(("rate_mix",))["rate_mix"] == (0.0, 0), "what a converter that never set anything launches"
    with pytest.raises(api.PercepNetError, match="off"):
        a.rc.read_mix_report()
    a.close()
    b.close()
    # with conferences: after the way there and back, the bits and the launch counts of a converter that never set anything
    a, b = Twin(model, "mixed", CONFS), Twin(model, "mixed", CONFS)
    settings(a, gains=GAINS1, caps=CAPS1, hold=0.5, report=True)
    y = tc.kernel_rows()
    kernel(a, y)
    settings(a, gains=np.ones(B, F32), caps=[0] * B, hold=0.0, report=False)
    for tw in (a, b):
        tw.rc.set_profiling(True)
    for which, ids in KERNEL_LISTS.items():
        assert_rows(kernel(a, y, ids), kernel(b, y, ids), ids, f"list {which}")
    ta, tb = a.rc.kernel_times(("rate_mix",)), b.rc.kernel_times(("rate_mix",))
    assert ta["rate_mix"][1] == tb["rate_mix"][1] == len(KERNEL_LISTS)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 4
LOUD, STEADY, PAUSED = BIG[4], BIG[10], BIG[6]


def hold_rows(t):
    """call t: LOUD has level ~ 480 * 64 in call 0 and is silent afterwards; STEADY ~ 480 * 2.56 in every call; PAUSED ~ 480 * 256 in call 2
    and silent otherwise; the other members of the big conference ~ 480 * 0.01"""
    rng = np.random.default_rng(5300)
    y = rng.standard_normal((B, 480)).astype(F32) * F32(0.1)
    y[STEADY] *= F32(16)
    y[LOUD] = y[LOUD] * F32(80) if t == 0 else 0
    y[PAUSED] = y[PAUSED] * F32(160) if t == 2 else 0
    return y


def test_hold(model):
    tw = Twin(model, "mixed", CONFS)
    caps = caps_of({32: 1, 5: 0, 4: 0, 3: 0, 2: 0, 1: 0})
    settings(tw, caps=caps, hold=0.5, report=True)
    lv, rep = None, None
    loud, seen = [], {}
    for t in range(8):
        ids = [s for s in ALL if s != PAUSED] if t in (3, 4, 5) else None     # PAUSED does not advance in calls 3..5
        y = hold_rows(t)
        got = kernel(tw, y, ids)
        want, lv, rep = mm.mix(y, CONFS, ids, out=np.full((B, 480), SENTINEL["f32"], F32), caps=caps, hold=0.5, levels=lv, report=rep)
        assert_rows(got, want, ids, f"call {t}")
        got_rep = tw.rc.read_mix_report()
        assert_report(got_rep, rep, None, f"call {t}")
        loud.append(int(got_rep["flags"][LOUD]) & 1)
        seen[t] = got_rep["level"].copy()
    # N = 1: LOUD's 480 * 64 halves per call — above STEADY's 480 * 2.56 through call 4, below it from call 5 on; PAUSED's 480 * 256
    # takes call 2 and, kept while it does not advance, calls 6 and 7
    assert loud == [1, 1, 0, 1, 1, 0, 0, 0], f"LOUD is held exactly as long as the model says: {loud}"
    assert seen[1][LOUD] == F32(0.5) * seen[0][LOUD] and seen[1][STEADY] == seen[0][STEADY], "a decaying hold beside a steady level"
    assert seen[5][PAUSED] == seen[2][PAUSED] and seen[6][PAUSED] == F32(0.5) * seen[2][PAUSED], "a member that does not advance keeps its level"
    zeros = np.zeros((B, 480), F32)

    def after(what, cleared):
        nonlocal lv, rep
        assert (lv[BIG] > 0).sum() > 20, "levels to clear"
        lv[cleared] = 0
        kernel(tw, zeros)
        _, lv, rep = mm.mix(zeros, CONFS, caps=caps, hold=0.5, levels=lv, report=rep)
        got_rep = tw.rc.read_mix_report()
        assert_report(got_rep, rep, None, what)
        assert (got_rep["level"][cleared] == 0).all() and (got_rep["level"][[s for s in BIG if s not in cleared]] > 0).sum() >= (0 if len(cleared) == B else 20), what

    tw.rc.reset_streams([STEADY, BIG[11]])
    after("pn_rate_reset_streams zeroes the listed levels", [STEADY, BIG[11]])
    kernel(tw, hold_rows(1))
    _, lv, rep = mm.mix(hold_rows(1), CONFS, caps=caps, hold=0.5, levels=lv, report=rep)
    tw.rc.set_stream_confs([BIG[12], BIG[13]], [40, 40])               # (the same conference: the table does not change, the levels start again)
    after("pn_rate_set_stream_confs zeroes the listed levels", [BIG[12], BIG[13]])
    kernel(tw, hold_rows(1))
    _, lv, rep = mm.mix(hold_rows(1), CONFS, caps=caps, hold=0.5, levels=lv, report=rep)
    tw.rc.set_mix_hold(0.5)
    lv_before = lv.copy()
    lv[:] = 0
    kernel(tw, zeros)
    _, lv, rep = mm.mix(zeros, CONFS, caps=caps, hold=0.5, levels=lv, report=rep)
    got_rep = tw.rc.read_mix_report()
    assert_report(got_rep, rep, None, "pn_rate_set_mix_hold zeroes all levels")
    assert (got_rep["level"] == 0).all() and (lv_before[BIG] > 0).sum() > 20
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def edge_rows(seed):
    """sums on the cast edges in their first 100 columns: 0.5 + 0.5 = 32768 / 32768 (clipped) in the conference of three; -1 and
    -1 - 1 / 32768 (the second clipped) in the conference of four; a NaN and an inf column in the conference of five; gaussian sums
    of 31 rows of rms 0.25 in the big one"""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((B, 480)).astype(F32) * F32(0.25)
    y[THREE + FOUR + TWO] = 0
    y[THREE[0], :100], y[THREE[1], :100] = F32(0.5), F32(0.5)
    y[FOUR[0], :100], y[FOUR[1], :100] = F32(-1.0), F32(-1.0 / 32768)
    y[FIVE[0], 7], y[FIVE[1], 9] = np.nan, np.inf
    return y


def test_mix_report(model):
    tw = Twin(model, "mixed", CONFS)
    settings(tw, report=True)
    y = edge_rows(5400)
    got = kernel(tw, y)
    want, lv, rep = mm.mix(y, CONFS)
    assert_rows(got, want, None, "edge rows")
    first = tw.rc.read_mix_report()
    assert_report(first, rep, None, "edge rows")
    assert np.array_equal(first["mix_peak"][[s for s in ALL if s != LONER]], rm.peak(want[[s for s in ALL if s != LONER]]))
    assert np.array_equal(first["mix_clipped"][[s for s in ALL if s != LONER]], rm.count_clipped(want[[s for s in ALL if s != LONER]]))
    assert first["mix_clipped"][THREE].tolist() == [0, 0, 100] and first["mix_peak"][THREE].tolist() == [0.5, 0.5, 1.0]
    assert first["mix_clipped"][FOUR].tolist() == [0, 0, 100, 100] and first["mix_peak"][FOUR[2]] == F32(1.0) + F32(2.0 ** -15)
    assert first["mix_clipped"][FIVE[2]] >= 2 and first["mix_peak"][FIVE[2]] == np.inf and first["mix_clipped"][FIVE[0]] >= 1
    assert first["mix_clipped"][BIG].sum() > 0 and first[LONER].tobytes() == bytes(16), "a stream without a conference has a zero record"
    assert (first["flags"][[s for s in ALL if s != LONER]] == 5).all() and cm.same(first["level"], lv) and np.isnan(lv[FIVE[0]])
    # other rows under a list: the records of the unlisted streams are the first call's
    ids = KERNEL_LISTS["9"]
    y2 = edge_rows(5401) * F32(0.5)
    got = kernel(tw, y2, ids)
    want2, lv2, rep2 = mm.mix(y2, CONFS, ids, out=np.full((B, 480), SENTINEL["f32"], F32), levels=lv, report=first)
    assert_rows(got, want2, ids, "edge rows, list")
    second = tw.rc.read_mix_report()
    assert_report(second, rep2, None, "edge rows, list")
    out = [s for s in ALL if s not in ids]
    assert second[out].tobytes() == first[out].tobytes() and sum(second[s].tobytes() != first[s].tobytes() for s in ids) >= 10
    # the device form gives the same records
    import torch
    d = dev_full((B, 4), torch.int32, 77)
    tw.rc.read_mix_report_dev(d.data_ptr())
    assert to_host(tw.ctx, d).tobytes() == second.tobytes()
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 6
CAPS2 = [2] * B


def composed(tw, kind, x, ids, st):
    """The frame by hand on a twin that has no conference: up, the engine, the model on the host under the settings st (a dict:
    gains, caps, hold, levels, report — levels and report are carried along), down"""
    import torch
    nan = float("nan")
    d_in = to_dev(np.array(x))
    x48, y48, d_gr = dev_full((B, 480), torch.float32, nan), dev_full((B, 480), torch.float32, nan), dev_full((B, 68), torch.float32, nan)
    getattr(tw.rc, f"up_{kind}_dev")(d_in.data_ptr(), x48.data_ptr(), ids=ids)
    if ids is None:
        tw.ctx.process_f32_dev(x48.data_ptr(), y48.data_ptr(), d_gr.data_ptr())
    else:
        tw.ctx.process_f32_active_dev(x48.data_ptr(), y48.data_ptr(), d_gr.data_ptr(), ids)
    y = to_host(tw.ctx, y48)
    o, st["levels"], st["report"] = mm.mix(y, CONFS, ids, out=np.full((B, 480), nan, F32), gains=st["gains"], caps=st["caps"], hold=st["hold"],
                                           levels=st["levels"], report=st["report"])
    d_out = dev_full((B, tw.w), getattr(torch, {"f32": "float32", "i16": "int16", "g711": "uint8"}[kind]), SENTINEL[kind].item())
    getattr(tw.rc, f"down_{kind}_dev")(to_dev(o).data_ptr(), d_out.data_ptr(), ids=ids)
    return to_host(tw.ctx, d_out).copy(), to_host(tw.ctx, d_gr).copy(), y


_reference = {}


def reference(model, kind, active):
    """12 frames of the composition under GAINS1, N = 2 everywhere, saturate on: computed once per (format, list or not)"""
    if (kind, active) not in _reference:
        b = Twin(model, "mixed")
        b.ctx.set_output_saturate(True)
        x = tc.inputs(kind, b.w)
        st = dict(gains=GAINS1, caps=CAPS2, hold=0.0, levels=None, report=None)
        frames, two, energy = [], 0, 0
        for t in range(T):
            ids = tc.ids_at(t) if active else None
            out, gr, y = composed(b, kind, x[t], ids, st)
            frames.append((out, gr, st["report"].copy()))
            two += int(sum(int(st["report"]["flags"][s]) & 1 for s in BIG if ids is None or s in ids) == 2)
            if t >= 7:
                energy += int(np.count_nonzero(st["report"]["level"][BIG]))
        assert two == T and energy > 0, "two of the big conference are selected in every frame, and there is signal behind the delay"
        b.close()
        _reference[(kind, active)] = frames
    return _reference[(kind, active)]


@pytest.mark.parametrize("kind,active", (("f32", False), ("i16", False), ("g711", False), ("f32", True)))
def test_whole_frame_against_the_composition(model, kind, active):
    want = reference(model, kind, active)
    a = Twin(model, "mixed", CONFS)
    a.ctx.set_output_saturate(True)
    settings(a, gains=GAINS1, caps=CAPS2, report=True)
    x = tc.inputs(kind, a.w)
    for t in range(T):
        ids = tc.ids_at(t) if active else None
        got = tc.frame(a, kind, x[t], ids)
        tc.assert_frame(a, got, want[t], ids, f"{kind} frame {t}:")
        assert_report(a.rc.read_mix_report(), want[t][2], ids, f"{kind} frame {t}")
    a.close()


def test_whole_frame_pipelined(model):
    want = reference(model, "i16", False)
    a = Twin(model, "mixed", CONFS)
    a.ctx.set_output_saturate(True)
    settings(a, gains=GAINS1, caps=CAPS2, report=True)
    x = tc.inputs("i16", 480)
    rot = tp.Rot(a.ctx, 480, "i16", B)
    res = rot.run(x, lambda t, h_in, h_out, h_gr, h_rep: a.rc.submit_host_i16(h_in, h_out, h_gr))
    for t in range(T):
        tc.assert_frame(a, res[t][:2], want[t], None, f"pipelined frame {t}:")
    assert_report(a.rc.read_mix_report(), want[T - 1][2], None, "the last frame's records")
    assert a.ctx.frames_delivered() == T
    rot.free()
    a.close()


# ---------------------------------------------------------------------------------------------------------------- 7
T_GAIN, T_CAP, T_HOLD = 8, 9, 10
GAINS2 = GAINS1.copy()
GAINS2[BIG[0]], GAINS2[MUTED[0]], GAINS2[BIG[5]] = 0, 1, 4               # one mutes, one is unmuted, one is raised
CAPS3 = caps_of({32: 1, 5: 2, 4: 0, 3: 1, 2: 2, 1: 0})


def test_changes_between_two_pipelined_frames(model):
    b = Twin(model, "mixed")
    b.ctx.set_output_saturate(True)
    x = tc.inputs("i16", 480, 1)
    st = dict(gains=GAINS1, caps=CAPS2, hold=0.0, levels=None, report=None)
    want, matters = [], {"gain": False, "cap": False}
    for t in range(T):
        if t == T_GAIN:
            st["gains"] = GAINS2
        if t == T_CAP:
            st["caps"] = CAPS3
        if t == T_HOLD:
            st["hold"], st["levels"] = 0.75, None
        old = dict(st, gains=GAINS1) if t == T_GAIN else dict(st, caps=CAPS2) if t == T_CAP else None
        lv_in = st["levels"]
        out, gr, y = composed(b, "i16", x[t], None, st)
        want.append((out, gr))
        if old is not None:
            o_old = mm.mix(y, CONFS, gains=old["gains"], caps=old["caps"], hold=old["hold"], levels=lv_in)[0]
            o_new = mm.mix(y, CONFS, gains=st["gains"], caps=st["caps"], hold=st["hold"], levels=lv_in)[0]
            matters["gain" if t == T_GAIN else "cap"] = not np.array_equal(o_old, o_new)
    assert all(matters.values()), "the changes matter to the frames behind them"
    b.close()
    a = Twin(model, "mixed", CONFS)
    a.ctx.set_output_saturate(True)
    settings(a, gains=GAINS1, caps=CAPS2, report=True)
    L, h = a.ctx.L, a.rc.h
    ids = np.array(ALL, np.int32)

    def submit(t, h_in, h_out, h_gr, h_rep):
        # arrays that are overwritten as soon as the call has returned, with no wait before or after
        if t == T_GAIN:
            g = GAINS2.copy()
            assert L.pn_rate_set_stream_mix_gains(h, ids.ctypes.data, B, g.ctypes.data) == 0, L.pn_last_error()
            g[:] = 7
        if t == T_CAP:
            n = np.array(CAPS3, np.int32)
            assert L.pn_rate_set_conf_speakers(h, ids.ctypes.data, B, n.ctypes.data) == 0, L.pn_last_error()
            n[:] = 31
        if t == T_HOLD:
            assert L.pn_rate_set_mix_hold(h, 0.75) == 0, L.pn_last_error()
        a.rc.submit_host_i16(h_in, h_out, h_gr)

    rot = tp.Rot(a.ctx, 480, "i16", B)
    res = rot.run(x, submit)
    for t in range(T):
        tc.assert_frame(a, res[t][:2], want[t], None, f"frame {t}:")
    assert_report(a.rc.read_mix_report(), st["report"], None, "the last frame's records: the hold began at frame 10 with levels of zero")
    assert a.rc.stream_mix_gains().tolist() == GAINS2.tolist() and a.rc.conf_speakers().tolist() == CAPS3 and a.rc.mix_hold() == 0.75
    rot.free()
    a.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_refusals_change_nothing(model):
    import ctypes
    a = Twin(model, "mixed", CONFS)
    settings(a, gains=GAINS1, caps=CAPS1, hold=0.25)
    a.rc.set_profiling(True)
    y = sel_rows()
    first = kernel(a, y)
    L, h = a.ctx.L, a.rc.h
    i32, f32 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, F32))
    for ids, g, word in ((i32(0, 1), f32(1, np.nan), b"at index 1:"), (i32(0, 1), f32(-1, np.nan), b"at index 0:"), (i32(2, 1, 0), f32(1, 1, np.inf), b"at index 2:"),
                         (i32(0, 0), f32(1, 1), b"twice"), (i32(0, B), f32(1, 1), b"out of range"), (i32(-1), f32(1), b"out of range")):
        assert L.pn_rate_set_stream_mix_gains(h, ids.ctypes.data, len(ids), g.ctypes.data) == -1 and word in L.pn_last_error(), word
    for confs, n, word in ((i32(40, 3), i32(2, 33), b"at index 1:"), (i32(40, 3), i32(-1, 33), b"at index 0:"), (i32(40, B), i32(2, 2), b"out of range"),
                           (i32(-1), i32(2), b"out of range"), (i32(3, 3), i32(2, 2), b"twice")):
        assert L.pn_rate_set_conf_speakers(h, confs.ctypes.data, len(confs), n.ctypes.data) == -1 and word in L.pn_last_error(), word
    for d in (1.0, -0.5, float("nan"), 2.0):
        assert L.pn_rate_set_mix_hold(h, ctypes.c_float(d)) == -1 and b"[0, 1)" in L.pn_last_error(), d
    rep = np.zeros(B, api.MIX_REPORT_DTYPE)
    assert L.pn_rate_read_mix_report(h, rep.ctypes.data) == -1 and b"off" in L.pn_last_error()
    assert L.pn_rate_read_mix_report_dev(h, rep.ctypes.data) == -1 and b"off" in L.pn_last_error()
    assert L.pn_rate_set_stream_mix_gains(h, None, 0, None) == 0 and L.pn_rate_set_conf_speakers(h, None, 0, None) == 0
    assert a.rc.stream_mix_gains().tolist() == GAINS1.tolist() and a.rc.conf_speakers().tolist() == CAPS1 and a.rc.mix_hold() == 0.25
    assert a.rc.kernel_times(("rate_mix",))["rate_mix"][1] == 1, "a refused call launches nothing"
    a.rc.set_mix_hold(0.25)                                            # (the levels of the first call go)
    assert_rows(kernel(a, y), first, None, "the call after the refusals")
    a.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_cli_speakers_and_gains(model, blob, tmp_path):
    frames, gains = 9, (1, 0.5, 0, 1)
    rng = np.random.default_rng(5500)
    x = [np.rint(rng.standard_normal(frames * 480 + 13 + i) * 4096 * (i + 1)).clip(-32768, 32767).astype(np.int16) for i in range(4)]
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    args = []
    for i, v in enumerate(x):
        v.tofile(tmp_path / f"in{i}.pcm")
        args += [f"in{i}.pcm", f"out{i}.pcm"]
    opts = ["--model", "m.pnw", "--conference", "0,0,0,0", "--conf-speakers", "2", "--mix-gains", "1,0.5,0,1", "--saturate"]
    run = subprocess.run([exe] + opts + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    got = [np.fromfile(tmp_path / f"out{i}.pcm", np.int16) for i in range(4)]
    ctx = api.Context(model, 4)
    ctx.set_output_saturate(True)
    rc = api.MixedRateConverter(ctx, (48000,) * 4)
    rc.set_stream_confs([0, 1, 2, 3], [0] * 4)
    rc.set_conf_speakers([0, 1, 2, 3], [2] * 4)
    rc.set_stream_mix_gains([0, 1, 2, 3], gains)
    inp, out = tp.Pin(ctx.L, (4, 480), np.int16), tp.Pin(ctx.L, (4, 480), np.int16)
    want = [np.zeros((frames - 1) * 480, np.int16) for _ in range(4)]
    for t in range(frames):
        for s in range(4):
            inp.a[s] = x[s][t * 480:(t + 1) * 480]
        rc.submit_host_i16(inp.p, out.p, None, ids=[0, 1, 2, 3])
        ctx.host_wait()
        if t > 0:
            for s in range(4):
                want[s][(t - 1) * 480:t * 480] = out.a[s]
    rc.close()
    ctx.close()
    inp.free()
    out.free()
    for i in range(4):
        assert got[i].size == want[i].size and np.array_equal(got[i], want[i]), f"pair {i}"
    assert all(np.count_nonzero(w[7 * 480:]) > 0 for w in want), "signal behind the delay"
    assert not np.array_equal(want[0], want[3]), "two listeners of one conference hear different sums"
