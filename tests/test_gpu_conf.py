"""Conference mixing on the rate converter (-m gpu): include/percepnet_hip.h "conferences"; kernel percepnet_amd/csrc/pn_rate_mix.hip,
host side pn_rate.cpp (the one hook in rate_frame), table rules pn_conf.h, bindings api.RateConverter.set_stream_confs /
stream_confs / mix_f32_dev, CLI percepnet_run --conference.

The oracle is the numpy float32 model tests/conf_model.py: alone for the kernel, and for whole frames inside the composition
pn_rate_up_* -> pn_process_f32[_active] -> model -> pn_rate_down_* on a SECOND context and converter of the same model that never has
a conference.  Every comparison is equality of bits (of NaN-ness where a sum is NaN: conf_model.same says why); no tolerance.

Shapes: one context of B = 48 streams — twelve blocks of the four-streams-per-block row kernels — with the conferences scattered
over the slots by s -> (29 s + 7) mod 48: one of 32 (the cap), of 5 and 4 (either side of the kernel's size-class edge 4 | 5), of
3 and 2 (either side of 2 | 3) and of 1; one stream has none.  The id lists of the kernel test bring the big conference to 17, 16,
9 and 8 advancing members, the other two class edges.  Whole-frame tests run 12 frames: six of the engine's delay, in which its
output is next to nothing, and six of signal."""
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import conf_model as cm
from tests import families
from tests import g711_model as gm
from tests import test_gpu_rate as tg
from tests import test_gpu_rate_mixed as tm
from tests import test_gpu_rate_pipe as tp

pytestmark = pytest.mark.gpu
B, T = 48, 12
F32 = np.float32
NONE = cm.NONE
PERM = [(29 * s + 7) % B for s in range(B)]
SIZES = ((40, 32), (3, 5), (47, 4), (0, 3), (17, 2), (9, 1))       # (conference, members): ids at both ends of [0, B) among them
CONFS = [NONE] * B
_at = 0
for _c, _k in SIZES:
    for _s in PERM[_at:_at + _k]:
        CONFS[_s] = _c
    _at += _k
LONER = PERM[47]                                                    # the stream without a conference
RATES = tuple((8000, 16000, 24000, 48000)[s % 4] for s in range(B))
LAWS = tuple((gm.ULAW, gm.ALAW, gm.ALAW)[s % 3] for s in range(B))
SENTINEL = {"f32": F32(777.0), "i16": np.int16(12345), "g711": np.uint8(0x5A)}
DTYPE = {"f32": np.float32, "i16": np.int16, "g711": np.uint8}
same, to_dev, to_host, dev_full, nof = tg.same, tg.to_dev, tg.to_host, tg.dev_full, tm.nof


def test_the_layout_is_what_the_docstring_says():
    assert sorted(PERM) == list(range(B)) and CONFS.count(NONE) == 1 and CONFS[LONER] == NONE
    for c, k in SIZES:
        m = cm.members(CONFS, c)
        assert len(m) == k and (k < 3 or any(b - a > 1 for a, b in zip(m, m[1:]))), "scattered, not contiguous"
    assert {RATES[s] for s in cm.members(CONFS, 40)} == {8000, 16000, 24000, 48000} and {LAWS[s] for s in cm.members(CONFS, 40)} == set(gm.LAWS)
    assert len({s // 4 for s in cm.members(CONFS, 40)}) == 12, "the big conference has members in every block of the row kernels"


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


class Twin:
    """A context of B streams and a converter beside it: mixed with RATES (case "mixed") or single-rate (case = the rate); the laws
    are LAWS; confs: set on every stream"""

    def __init__(self, model, case="mixed", confs=None):
        self.ctx = api.Context(model, B)
        self.rc = api.MixedRateConverter(self.ctx, RATES) if case == "mixed" else api.RateConverter(self.ctx, case)
        self.rates = list(RATES) if case == "mixed" else [case] * B
        self.w = self.rc.frame
        self.rc.set_stream_laws(list(range(B)), LAWS)
        assert self.rc.stream_confs().tolist() == [NONE] * B, "a new converter has no conference"
        if confs is not None:
            self.rc.set_stream_confs(list(range(B)), confs)
            assert self.rc.stream_confs().tolist() == list(confs)

    def ns(self):
        return [nof(r) for r in self.rates]

    def close(self):
        self.rc.close()
        self.ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 1
def kernel_rows():
    """[B, 480] floats: gaussian values, and in known columns the values whose sums have one right answer only in the stated order
    and arithmetic: -0.0 everywhere (col 0), subnormals (1), 1e30 / -1e30 / 1 by slot (2), one +inf per conference (3), one -inf
    (4), +inf and -inf in two members of a conference (5), one NaN (6), +0.0 and -0.0 mixed (7)"""
    rng = np.random.default_rng(4800)
    y = rng.standard_normal((B, 480)).astype(F32)
    y[:, 0] = F32(-0.0)
    y[:, 1] = (rng.integers(1, 1 << 22, B).astype(np.uint32) | (rng.integers(0, 2, B).astype(np.uint32) << 31)).view(F32)
    y[:, 2] = np.where(np.arange(B) % 3 == 0, F32(1e30), np.where(np.arange(B) % 3 == 1, F32(-1e30), F32(1.0)))
    y[:, 7] = np.where(np.arange(B) % 2 == 0, F32(0.0), F32(-0.0))
    for c, k in SIZES:
        m = cm.members(CONFS, c)
        y[m[0], 3] = F32(np.inf)
        y[m[-1], 4] = F32(-np.inf)
        y[m[0], 5], y[m[-1], 5] = F32(np.inf), F32(-np.inf)        # (a conference of one: -inf, and nobody hears it)
        y[m[k // 2], 6] = F32(np.nan)
    y[LONER, 3:7] = (F32(np.inf), F32(-np.inf), F32(np.nan), F32(np.nan))
    return y


def list_with(big, seed):
    """An id list, in no order: `big` members of the conference of 32, one member too few of every other conference (so the
    conference of 2 lists a stream whose whole conference is out, and the conference of 1 is out), and the stream without one"""
    rng = np.random.default_rng(seed)
    ids = [LONER]
    for c, k in SIZES:
        m = cm.members(CONFS, c)
        ids += [int(v) for v in rng.permutation(m)[:big if k == 32 else k - 1]]
    return [int(v) for v in rng.permutation(ids)]


KERNEL_LISTS = {"all": None, "17": list_with(17, 1), "16": list_with(16, 2), "9": list_with(9, 3), "8": list_with(8, 4), "alone": list_with(1, 5)}


@pytest.fixture(scope="module")
def kernel_twin(model):
    tw = Twin(model, "mixed", CONFS)
    yield tw
    tw.close()


def test_the_kernel_rows_hold_what_they_must():
    y = kernel_rows()
    sub = np.abs(y[:, 1])
    assert (sub > 0).all() and (sub < np.finfo(F32).tiny).all() and np.signbit(y[:, 0]).all()
    o = cm.mix(y, CONFS)
    big = cm.members(CONFS, 40)
    assert np.isnan(o[big[1], 5]) and np.isnan(o[big[1], 6]) and o[big[1], 3] == np.inf and o[big[1], 4] == -np.inf
    assert np.signbit(o[LONER, 0]) and np.signbit(o[:, 0]).sum() == 1 and (o[:, 0] == 0).all(), "-0.0 survives only as a copy"
    assert len({float(v) for v in o[big, 2]}) > 1, "the 1e30 column depends on who listens"
    for name, ids in KERNEL_LISTS.items():
        if ids is not None:
            assert len(set(ids)) == len(ids) and ids != sorted(ids)
            for c, k in SIZES:
                listed = [s for s in cm.members(CONFS, c) if s in ids]
                assert len(listed) == (int(name) if name.isdigit() and k == 32 else 1 if k == 32 else k - 1)


@pytest.mark.parametrize("which", list(KERNEL_LISTS))
def test_kernel_alone_against_the_model(kernel_twin, which):
    import torch
    tw, ids = kernel_twin, KERNEL_LISTS[which]
    y = kernel_rows()
    d_in, d_out = to_dev(y), dev_full((B, 480), torch.float32, float(SENTINEL["f32"]))
    tw.rc.mix_f32_dev(d_in.data_ptr(), d_out.data_ptr(), ids=ids)
    got = to_host(tw.ctx, d_out)
    want = cm.mix(y, CONFS, ids, out=np.full((B, 480), SENTINEL["f32"], F32))
    for s in range(B):
        assert cm.same(got[s], want[s]), f"list {which}: stream {s} (conference {CONFS[s]})"
        if ids is not None and s not in ids:
            assert (got[s] == SENTINEL["f32"]).all(), f"the row of unlisted stream {s} keeps its sentinel"
    assert same(to_host(tw.ctx, d_in), y), "the input rows are read only"
    if ids is not None:
        two = [s for s in cm.members(CONFS, 17) if s in ids]
        assert len(two) == 1 and (got[two[0]] == 0).all() and not np.signbit(got[two[0]]).any(), "the whole conference is out: +0.0"


def test_kernel_on_a_converter_that_never_had_a_conference_copies(model):
    import torch
    tw = Twin(model, 8000)
    y = kernel_rows()
    d_in, d_out = to_dev(y), dev_full((B, 480), torch.float32, float(SENTINEL["f32"]))
    tw.rc.mix_f32_dev(d_in.data_ptr(), d_out.data_ptr(), ids=[5, 0, 47])
    got = to_host(tw.ctx, d_out)
    assert all(same(got[s], y[s]) for s in (0, 5, 47)) and (np.delete(got, [0, 5, 47], 0) == SENTINEL["f32"]).all()
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 2
_inputs = {}


def inputs(kind, w, seed=0):
    """[T, B, w] seeded input rows of a sample format: gaussian noise of rms 0.25 as float or int16, random bytes for G.711"""
    key = (kind, w, seed)
    if key not in _inputs:
        if kind == "g711":
            a = np.random.default_rng(4900 + seed + w).integers(0, 256, (T, B, w)).astype(np.uint8)
            a.setflags(write=False)
            _inputs[key] = a
        else:
            _inputs[key] = tp.noise(kind, w, 40 + seed, B, T)
    return _inputs[key]


def frame(tw, kind, x, ids=None):
    """One frame through the converter's own entry point -> (out rows, g|r)"""
    import torch
    d_in = to_dev(np.array(x))
    d_out = dev_full((B, tw.w), getattr(torch, {"f32": "float32", "i16": "int16", "g711": "uint8"}[kind]), SENTINEL[kind].item())
    d_gr = dev_full((B, 68), torch.float32, float("nan"))
    getattr(tw.rc, f"process_{kind}_dev")(d_in.data_ptr(), d_out.data_ptr(), d_gr.data_ptr(), ids=ids)
    return to_host(tw.ctx, d_out).copy(), to_host(tw.ctx, d_gr).copy()


def composed(tw, kind, x, confs, ids=None):
    """The same frame by hand on a twin that has no conference: up, the engine, the numpy model on the host, down"""
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
    o = cm.mix(y, confs, ids, out=np.full((B, 480), nan, F32))
    d_out = dev_full((B, tw.w), getattr(torch, {"f32": "float32", "i16": "int16", "g711": "uint8"}[kind]), SENTINEL[kind].item())
    getattr(tw.rc, f"down_{kind}_dev")(to_dev(o).data_ptr(), d_out.data_ptr(), ids=ids)
    return to_host(tw.ctx, d_out).copy(), to_host(tw.ctx, d_gr).copy(), y


def assert_frame(tw, got, want, ids, what):
    for s, n in enumerate(tw.ns()):
        if ids is None or s in ids:
            assert same(got[0][s, :n], want[0][s, :n]), f"{what} stream {s} (conference {tw.rc.stream_confs()[s]})"
            assert same(got[1][s], want[1][s]), f"{what} g|r of stream {s}: the tap is the stream's own"
        else:
            assert (got[0][s] == SENTINEL[{np.dtype(np.float32): "f32", np.dtype(np.int16): "i16", np.dtype(np.uint8): "g711"}[got[0].dtype]]).all(), \
                f"{what} the row of unlisted stream {s} is untouched"


@pytest.mark.parametrize("case", ("mixed", 8000), ids=str)
@pytest.mark.parametrize("kind", ("f32", "i16", "g711"))
def test_whole_frame_against_the_composition(model, kind, case):
    a, b = Twin(model, case, CONFS), Twin(model, case)
    for tw in (a, b):
        tw.ctx.set_output_saturate(kind == "g711")               # int16 through the wrapping cast, G.711 through the saturating one
    x = inputs(kind, a.w)
    heard, own = 0, 0
    for t in range(T):
        got = frame(a, kind, x[t])
        want = composed(b, kind, x[t], CONFS)
        assert_frame(a, got, want, None, f"{case} {kind} frame {t}:")
        y = want[2]
        if t >= 6:                                               # (behind the engine's delay of six frames)
            big = cm.members(CONFS, 40)
            heard += int(np.count_nonzero(cm.mix(y, CONFS)[big]))
            own += int(np.count_nonzero(y[big]))
    # (the stream without a conference: the model copies its row, so it is compared with what b, which never had a conference, gives)
    assert heard > 0 and own > 0, "signal behind the delay"
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 3
SUBSETS = (list_with(17, 11), list_with(32, 12) + [cm.members(CONFS, 9)[0]], list_with(9, 13), list(range(B)))
BIG = cm.members(CONFS, 40)
FIVE = cm.members(CONFS, 3)
# the change behind frame 8: two members of the big conference leave it, one for the conference of five (6 now: another size
# class), one for none; the stream without a conference takes the freed place; the conference of two dissolves
CHANGE_IDS = [BIG[30], LONER, BIG[2], cm.members(CONFS, 17)[0], cm.members(CONFS, 17)[1]]
CHANGE_TO = [3, 40, NONE, NONE, NONE]
AFTER = list(CONFS)
for _s, _c in zip(CHANGE_IDS, CHANGE_TO):
    AFTER[_s] = _c
T_CHANGE = 9


def ids_at(t):
    return SUBSETS[t % 4]


def confs_at(t):
    return CONFS if t < T_CHANGE else AFTER


def change(tw):
    """pn_rate_set_stream_confs with arrays that are overwritten as soon as the call has returned, with no wait before or after"""
    ids, to = np.array(CHANGE_IDS, np.int32), np.array(CHANGE_TO, np.int32)
    assert tw.ctx.L.pn_rate_set_stream_confs(tw.rc.h, ids.ctypes.data, len(CHANGE_IDS), to.ctypes.data) == 0, tw.ctx.L.pn_last_error()
    ids[:] = 0
    to[:] = 40


@pytest.fixture(scope="module")
def changed_frames(model):
    """The synchronous path, int16 saturating, an id list every frame and the change in front of frame 9: per frame the out rows
    and g|r, checked against the composition under the table of that frame"""
    a, b = Twin(model, "mixed", CONFS), Twin(model, "mixed")
    for tw in (a, b):
        tw.ctx.set_output_saturate(True)
    x = inputs("i16", 480, 1)
    out, differs = [], False
    for t in range(T):
        if t == T_CHANGE:
            change(a)
        got = frame(a, "i16", x[t], ids_at(t))
        want = composed(b, "i16", x[t], confs_at(t), ids_at(t))
        assert_frame(a, got, want, ids_at(t), f"frame {t}:")
        if t >= T_CHANGE:
            old, new = cm.mix(want[2], CONFS, ids_at(t)), cm.mix(want[2], AFTER, ids_at(t))
            differs |= any(not np.array_equal(old[s], new[s]) for s in CHANGE_IDS if s in ids_at(t))
        out.append(got)
    assert a.rc.stream_confs().tolist() == AFTER and differs, "the change matters to the frames behind it"
    a.close()
    b.close()
    return out


def test_a_change_between_two_frames_synchronous(changed_frames):
    assert len(changed_frames) == T


def test_a_change_between_two_frames_pipelined(model, changed_frames):
    a = Twin(model, "mixed", CONFS)
    a.ctx.set_output_saturate(True)
    L = a.ctx.L
    x = inputs("i16", 480, 1)
    sets = [(tp.Pin(L, (B, 480), np.int16), tp.Pin(L, (B, 480), np.int16), tp.Pin(L, (B, 68), F32)) for _ in range(3)]
    res = {}

    def take(i):
        res[i] = (sets[i % 3][1].a.copy(), sets[i % 3][2].a.copy())

    for t in range(T):
        inp, out, gr = sets[t % 3]
        inp.a[...] = x[t]
        out.a[...] = SENTINEL["i16"]
        gr.a.view(np.uint8)[...] = 0xEE
        if t == T_CHANGE:
            change(a)                                             # queued behind frame 8, which is still in flight
        a.rc.submit_host_i16(inp.p, out.p, gr.p, ids=ids_at(t))
        if t >= 2:
            take(t - 2)
    a.ctx.host_wait()
    take(T - 2)
    take(T - 1)
    rates = a.rates
    for t in range(T):
        for s in ids_at(t):
            n = nof(rates[s])
            assert np.array_equal(res[t][0][s, :n], changed_frames[t][0][s, :n]), f"frame {t} stream {s}: byte for byte the synchronous path"
            assert same(res[t][1][s], changed_frames[t][1][s]), f"g|r frame {t} stream {s}"
    assert a.rc.stream_confs().tolist() == AFTER and a.ctx.frames_delivered() == T
    a.close()
    for s3 in sets:
        for p in s3:
            p.free()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_refusals_change_nothing_and_resets_keep_the_setting(model):
    import torch
    a, b = Twin(model, "mixed", CONFS), Twin(model, "mixed")
    x = inputs("i16", 480, 2)
    for t in range(8):
        assert_frame(a, frame(a, "i16", x[t]), composed(b, "i16", x[t], CONFS), None, f"frame {t}:")
    L, h = a.ctx.L, a.rc.h
    i32 = lambda *v: np.array(v, np.int32)
    for ids, confs, word in ((i32(0, 0), i32(1, 1), b"twice"), (i32(0, B), i32(1, 1), b"out of range"), (i32(0, 1), i32(1, B), b"at index 1:"),
                             (i32(0, 1), i32(-2, 1), b"at index 0:"), (i32(LONER), i32(40), b"conference 40 would have 33 members")):
        assert L.pn_rate_set_stream_confs(h, ids.ctypes.data, len(ids), confs.ctypes.data) == -1 and word in L.pn_last_error(), word
    assert L.pn_rate_set_stream_confs(h, None, 0, None) == 0
    rows = dev_full((B + 1, 480), torch.float32, 1.0)
    p = rows.data_ptr()
    for d_in, d_out in ((p, p), (p, p + 1920), (p + 1920, p), (p, p + 1920 * (B - 1))):
        assert L.pn_rate_mix_f32(h, d_in, d_out, None, 0) == -1 and b"overlap" in L.pn_last_error()
    assert L.pn_rate_mix_f32(h, p, p + 8, None, 0) == -1 and b"aligned" in L.pn_last_error()
    assert L.pn_rate_mix_f32(h, p, None, None, 0) == -1
    assert (to_host(a.ctx, rows) == 1).all(), "a refused mix launches nothing"
    assert a.rc.stream_confs().tolist() == CONFS
    assert_frame(a, frame(a, "i16", x[8]), composed(b, "i16", x[8], CONFS), None, "the frame after the refusals:")
    # resets and a rate change keep the setting (and the engine's and the converter's own state goes the way it goes without conferences)
    moved = [BIG[0], FIVE[1]]
    for tw in (a, b):
        tw.rc.reset_streams(moved)
        tw.ctx.reset_streams(moved)
        tw.rc.set_stream_rates([BIG[5]], [8000 if RATES[BIG[5]] != 8000 else 16000])
        tw.rates[BIG[5]] = 8000 if RATES[BIG[5]] != 8000 else 16000
    assert a.rc.stream_confs().tolist() == CONFS
    a.rc.reset()
    b.rc.reset()
    assert a.rc.stream_confs().tolist() == CONFS
    for t in range(9, T):
        assert_frame(a, frame(a, "i16", x[t]), composed(b, "i16", x[t], CONFS), None, f"frame {t}, behind the resets:")
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_nothing_runs_while_no_stream_is_in_a_conference(model):
    a, b = Twin(model, 8000, CONFS), Twin(model, 8000)
    x = inputs("i16", 80, 3)
    a.rc.set_profiling(True)
    for t in range(7):
        frame(a, "i16", x[t])
        frame(b, "i16", x[t])
    assert a.rc.kernel_times(("rate_mix",))["rate_mix"][1] == 7 and a.rc.kernel_times()["rate_down"][1] == 7, "one mix launch a frame while on"
    a.rc.set_stream_confs(list(range(B)), [NONE] * B)
    a.rc.reset_profile()
    energy = 0
    for t in range(7, T):
        got, want = frame(a, "i16", x[t]), frame(b, "i16", x[t])
        # the down-converter's tail still holds the last 2D = 192 samples of what it converted in frame 6, the mixes: they reach the
        # first 2T = 32 samples of frame 7 (z[m] reads the 48 kHz samples 6m - 191 .. 6m - 1) and nothing behind them
        first = 2 * 16 if t == 7 else 0
        assert same(got[0][:, first:], want[0][:, first:]) and same(got[1], want[1]), f"frame {t}: what a converter that never had a conference gives"
        assert t > 7 or not same(got[0][:, :first], want[0][:, :first]), "(and the tail does reach those 32)"
        energy += int(np.count_nonzero(got[0]))
    times = a.rc.kernel_times(("rate_up", "rate_down", "rate_mix"))
    assert times["rate_mix"] == (0.0, 0) and times["rate_up"][1] == T - 7 and times["rate_down"][1] == T - 7 and energy > 0
    with pytest.raises(api.PercepNetError, match="rate_mix"):
        a.rc.kernel_times(("rate_mux",))
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_cli_three_rates_in_one_conference(model, blob, tmp_path):
    rates, confs, frames = (8000, 16000, 48000, 24000), (2, 2, 2, NONE), (9, 12, 12, 11)      # pair 0 ends first and is then no longer listed
    rng = np.random.default_rng(5000)
    x = [np.rint(rng.standard_normal(f * nof(r) + 13 + i) * 8192).clip(-32768, 32767).astype(np.int16) for i, (r, f) in enumerate(zip(rates, frames))]
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    args = []
    for i, v in enumerate(x):
        v.tofile(tmp_path / f"in{i}.pcm")
        args += [f"in{i}.pcm", f"out{i}.pcm"]
    opts = ["--model", "m.pnw", "--rates", ",".join(map(str, rates)), "--saturate", "--conference", "2,2,2,-"]
    run = subprocess.run([exe] + opts + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    got = [np.fromfile(tmp_path / f"out{i}.pcm", np.int16) for i in range(4)]
    run = subprocess.run([exe] + opts + ["--slots", "2"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "--slots" in run.stderr
    # the Python path: the same frames through submit_host_i16 with the list of the pairs that still have input
    ctx = api.Context(model, 4)
    ctx.set_output_saturate(True)
    rc = api.MixedRateConverter(ctx, rates)
    rc.set_stream_confs([0, 1, 2, 3], confs)
    inp, out = tp.Pin(ctx.L, (4, 480), np.int16), tp.Pin(ctx.L, (4, 480), np.int16)
    want = [np.zeros((f - 1) * nof(r), np.int16) for r, f in zip(rates, frames)]
    for t in range(max(frames)):
        live = [s for s in range(4) if t < frames[s]]
        inp.a[...] = 0
        for s in live:
            n = nof(rates[s])
            inp.a[s, :n] = x[s][t * n:(t + 1) * n]
        rc.submit_host_i16(inp.p, out.p, None, ids=live)
        ctx.host_wait()
        for s in live:
            n = nof(rates[s])
            if t > 0:
                want[s][(t - 1) * n:t * n] = out.a[s, :n]
    rc.close()
    ctx.close()
    inp.free()
    out.free()
    for i in range(4):
        assert got[i].size == want[i].size and np.array_equal(got[i], want[i]), f"pair {i} ({rates[i]} Hz)"
    assert all(np.count_nonzero(w[7 * nof(r):]) > 0 for w, r in zip(want[1:], rates[1:])), "signal behind the delay"
