"""The rate converter on the pipelined host path, its device-side records and the timing of its kernels (-m gpu):
include/percepnet_hip.h pn_rate_submit_host_* / pn_rate_export_streams / pn_rate_import_streams / pn_rate_set_profiling; host side
pn_rate.cpp on pn_host_pipe.cpp's pipe_submit, kernel pn_rate_records_dev_kernel in pn_rate.hip, bindings api.RateConverter, CLI
percepnet_run --rate / --rates.

The oracle throughout is the unchanged synchronous code on a twin context and converter of the same batch size and model; every
comparison is bit equality, no tolerance anywhere.

Shapes: B = 6 (two blocks of four waves, the second one partial), 14 frames (the engine's six-frame delay, plus several reuses of
each of the two pipeline slots), PN_NN_MFMA, seeded noise at about -12 dBFS, pinned buffers in three rotating sets: the outputs of
frame t - 2 are read once the submit of frame t has returned, like percepnet_run does."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import families
from tests import rate_records_cases as cases
from tests import test_gpu_rate as tg
from tests import test_gpu_rate_mixed as tm

pytestmark = pytest.mark.gpu
B, T = 6, 14
RATES6 = (8000, 48000, 16000, 24000, 8000, 16000)
ROW = 480
F32 = np.float32
same, to_dev, to_host, nof = tg.same, tg.to_dev, tg.to_host, tm.nof
DTYPE = {"i16": np.int16, "f32": np.float32}


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


_noise = {}


def noise(kind, n, seed=0, b=B, t=T):
    """[t, b, n] seeded gaussian noise of rms 0.25 (about -12 dBFS), computed once per shape"""
    key = (kind, n, seed, b, t)
    if key not in _noise:
        g = np.random.default_rng(7000 + seed + n).standard_normal((t, b, n)) * 0.25
        a = g.clip(-1.0, 1.0 - 2.0 ** -15).astype(F32) if kind == "f32" else np.rint(g * 32768).clip(-32768, 32767).astype(np.int16)
        a.setflags(write=False)
        _noise[key] = a
    return _noise[key]


class Pin:
    """A pinned host array (pn_host_alloc)"""

    def __init__(self, L, shape, dtype):
        self.L = L
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.p = L.pn_host_alloc(n)
        assert self.p
        self.a = np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(self.p)).view(dtype).reshape(shape)

    def free(self):
        self.a = None
        self.L.pn_host_free(self.p)


class Rot:
    """Three rotating pinned sets (input rows, output rows, g|r, report records) on a pipelined path"""

    def __init__(self, ctx, n, kind, b=B):
        self.ctx, self.L = ctx, ctx.L
        self.sets = [(Pin(self.L, (b, n), DTYPE[kind]), Pin(self.L, (b, n), DTYPE[kind]), Pin(self.L, (b, 68), F32), Pin(self.L, (b, 8), np.uint32))
                     for _ in range(3)]

    def take(self, k):
        return tuple(p.a.copy() for p in self.sets[k][1:])

    def run(self, x, submit, frames=None):
        """x [T, b, n]; submit(t, h_in, h_out, h_gr, h_rep) queues frame t (and whatever goes in front of it) -> per frame
        (out, gr, report), each read after the submit of frame t + 2 has returned or after the final pn_host_wait"""
        frames = range(len(x)) if frames is None else frames
        res, order = {}, list(frames)
        for i, t in enumerate(order):
            inp, out, gr, rep = self.sets[i % 3]
            inp.a[...] = x[t]
            out.a.view(np.uint8)[...] = 0xEE
            gr.a.view(np.uint8)[...] = 0xEE
            rep.a[...] = 0xEEEEEEEE
            submit(t, inp.p, out.p, gr.p, rep.p)
            if i >= 2:
                res[order[i - 2]] = self.take((i - 2) % 3)
        self.ctx.host_wait()
        for i in range(max(len(order) - 2, 0), len(order)):
            res[order[i]] = self.take(i % 3)
        return [res[t] for t in order]

    def free(self):
        for s in self.sets:
            for p in s:
                p.free()


def dev_bytes(shape, fill=0):
    import torch
    t = torch.full(shape, fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def dev_i32(n, fill=77):
    import torch
    t = torch.full((n,), fill, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return t


def rates_of(rc):
    return rc.stream_rates().tolist() if rc.rate is None else [rc.rate] * rc.n_streams


def assert_streams_equal(got, want, rates, what):
    """(out, gr) pairs: each stream's first n_s samples and its g|r row"""
    for s, r in enumerate(rates):
        n = nof(r)
        assert same(np.ascontiguousarray(got[0][s, :n]), np.ascontiguousarray(want[0][s, :n])), f"{what} stream {s} ({r} Hz)"
        assert same(got[1][s], want[1][s]), f"g|r {what} stream {s} ({r} Hz)"


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", ("i16", "f32"))
@pytest.mark.parametrize("rate", api.RATES)
def test_single_rate_equals_the_synchronous_path(model, rate, kind):
    n = nof(rate)
    x = noise(kind, n)
    twin = tg.Pair(model, B, rate)
    want = [(twin.rc.process_i16 if kind == "i16" else twin.rc.process_f32)(x[t]) for t in range(T)]
    twin.close()
    assert np.count_nonzero(np.stack([w[0] for w in want[7:]])) > 0, "the frames past the engine's delay carry signal"
    p = tg.Pair(model, B, rate)
    rot = Rot(p.ctx, n, kind)
    sub = p.rc.submit_host_i16 if kind == "i16" else p.rc.submit_host_f32
    got = rot.run(x, lambda t, i, o, g, r: sub(i, o, g))
    for t in range(T):
        assert same(got[t][0], want[t][0]) and same(got[t][1], want[t][1]), f"{rate} Hz {kind} frame {t}"
    assert p.ctx.frames_delivered() == T
    p.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_mixed_with_a_rate_change(model):
    x = noise("i16", ROW, 1)
    after = list(RATES6)
    after[1] = 8000

    def between(p, t):
        if t == 6:                                               # before the seventh frame, with no wait in between
            p.rc.set_stream_rates([1], [8000])
            p.ctx.reset_streams([1])

    twin = tm.MixedPair(model, RATES6)
    want = []
    for t in range(T):
        between(twin, t)
        want.append(twin.rc.process_i16(x[t]))
    twin.close()
    p = tm.MixedPair(model, RATES6)
    rot = Rot(p.ctx, ROW, "i16")

    def submit(t, i, o, g, r):
        between(p, t)
        p.rc.submit_host_i16(i, o, g)

    got = rot.run(x, submit)
    assert p.rc.stream_rates().tolist() == after
    for t in range(T):
        assert_streams_equal(got[t], want[t], RATES6 if t < 6 else after, f"frame {t}")
    assert np.count_nonzero(np.stack([g[0][1, :80] for g in got[6:]])) > 0, "the slot that changed its rate carries signal again"
    p.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_active_set_and_a_refused_list(model):
    import torch
    x = noise("i16", ROW, 2)
    subsets = ([0, 2, 4, 5], [5, 1, 3], [0, 1, 2, 3, 4, 5], [3])
    twin = tm.MixedPair(model, RATES6)
    want = []
    d_out = tg.dev_full((B, ROW), torch.int16, 12345)
    d_gr = tg.dev_full((B, 68), torch.float32, float("nan"))
    for t in range(T):
        d_in = to_dev(np.array(x[t]))
        twin.rc.process_i16_dev(d_in.data_ptr(), d_out.data_ptr(), d_gr.data_ptr(), ids=subsets[t % 4])
        want.append((to_host(twin.ctx, d_out).copy(), to_host(twin.ctx, d_gr).copy()))
    twin.close()
    p = tm.MixedPair(model, RATES6)
    rot = Rot(p.ctx, ROW, "i16")
    got = rot.run(x, lambda t, i, o, g, r: p.rc.submit_host_i16(i, o, g, ids=subsets[t % 4]))
    for t in range(T):
        for s in subsets[t % 4]:
            n = nof(RATES6[s])
            assert same(np.ascontiguousarray(got[t][0][s, :n]), np.ascontiguousarray(want[t][0][s, :n])), f"frame {t} stream {s}"
            assert same(got[t][1][s], want[t][1][s]), f"g|r frame {t} stream {s}"
    assert np.count_nonzero(got[-1][0][1]) > 0 and np.count_nonzero(got[-1][0][3, :240]) > 0 and np.count_nonzero(got[-2][0][0, :80]) > 0
    assert p.ctx.frames_delivered() == T
    dup = np.array([0, 2, 0], np.int32)
    inp, out, gr, _ = rot.sets[0]
    assert p.ctx.L.pn_rate_submit_host_i16_active(p.rc.h, inp.p, out.p, gr.p, dup.ctypes.data, 3) == -1
    assert b"twice" in p.ctx.L.pn_last_error()
    far = np.array([0, B], np.int32)
    assert p.ctx.L.pn_rate_submit_host_f32_active(p.rc.h, inp.p, out.p, gr.p, far.ctypes.data, 2) == -1
    p.ctx.host_wait()
    assert p.ctx.frames_delivered() == T, "a refused list consumes no pipeline slot"
    assert p.ctx.L.pn_ctx_frames_done(p.ctx.h) == T
    p.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_frame_report_of_each_submit(model):
    x = noise("i16", ROW, 3)
    twin = tm.MixedPair(model, RATES6)
    twin.ctx.set_report(True)
    want = []
    for t in range(T):
        o, g = twin.rc.process_i16(x[t])
        want.append((o, g, twin.ctx.read_report()))
    twin.close()
    p = tm.MixedPair(model, RATES6)
    p.ctx.set_report(True)
    rot = Rot(p.ctx, ROW, "i16")
    got = rot.run(x, lambda t, i, o, g, r: p.rc.submit_host_i16(i, o, g, h_report=r))
    for t in range(T):
        assert_streams_equal(got[t], want[t], RATES6, f"frame {t}")
        assert np.array_equal(got[t][2], want[t][2].view(np.uint32).reshape(B, 8)), f"report records of frame {t}"
    assert max(w[2]["out_energy"].max() for w in want[7:]) > 0
    p.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_prepare_delivery_and_destroy_in_flight(model):
    x = noise("i16", 80, 4)
    p = tg.Pair(model, B, 8000)
    assert p.ctx.pipe_streams() == ""
    p.rc.host_pipeline_prepare()
    assert len(p.ctx.pipe_streams()) == 2, "the context's pipeline is built by the converter's prepare"
    assert p.ctx.frames_delivered() == 0
    rot = Rot(p.ctx, 80, "i16")
    rot.run(x, lambda t, i, o, g, r: p.rc.submit_host_i16(i, o, g))
    assert p.ctx.frames_delivered() == T
    p.rc.host_pipeline_prepare()                                  # again: nothing more to do
    p.rc.close()
    # a second converter on the same context: two frames in flight when it is destroyed
    rc2 = api.RateConverter(p.ctx, 8000)
    for k in range(2):
        inp, out, gr, _ = rot.sets[k]
        inp.a[...] = x[k]
        rc2.submit_host_i16(inp.p, out.p, gr.p)
    rc2.close()                                                   # completes them before it frees its staging rows
    assert p.ctx.frames_delivered() == T + 2
    p.ctx.host_wait()
    # Context.host_pipeline_prepare: the public call on a context of its own
    ctx = api.Context(model, B)
    ctx.host_pipeline_prepare()
    assert len(ctx.pipe_streams()) == 2 and ctx.frames_delivered() == 0
    ctx.close()
    p.ctx.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_interleaved_with_the_contexts_own_submits(model):
    x = noise("f32", ROW, 5)
    twin = api.Context(model, B)
    rot = Rot(twin, ROW, "f32")
    want = rot.run(x, lambda t, i, o, g, r: twin._chk(twin.L.pn_submit_host_f32(twin.h, i, o, g)))
    twin.close()
    rot.free()
    p = tm.MixedPair(model, (48000,) * B)                                 # every stream at 48000: the conversions are copies
    rot = Rot(p.ctx, ROW, "f32")

    def submit(t, i, o, g, r):
        if t % 2 == 0:
            p.rc.submit_host_f32(i, o, g)
        else:
            p.ctx._chk(p.ctx.L.pn_submit_host_f32(p.ctx.h, i, o, g))

    got = rot.run(x, submit)
    for t in range(T):
        assert same(got[t][0], want[t][0]) and same(got[t][1], want[t][1]), f"frame {t}"
    assert np.count_nonzero(want[-1][0]) > 0
    assert p.ctx.frames_delivered() == T
    p.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 7
SRC = [0, 2, 3, 4, 5]                                             # every stream of RATES6 with converter state
DST = [1, 3, 4, 5, 0]                                             # where they continue in the second converter


def test_device_records_export_and_continuation(model):
    x = noise("i16", ROW, 6)
    src_rates = [RATES6[s] for s in SRC]
    # the synchronous twin gives the records after the seventh frame, per rate group, through the host form
    twin = tm.MixedPair(model, RATES6)
    for t in range(7):
        twin.rc.process_i16(x[t])
    want_rec = {s: twin.rc.export_streams([s])[0] for s in SRC}
    twin.close()
    a = tm.MixedPair(model, RATES6)
    assert a.rc.record_stride() == api.rate_state_max_bytes() == 912
    d_rec = dev_bytes((len(SRC), 912), 0xAB)
    d_ctx = dev_bytes((len(SRC), api.STREAM_STATE_BYTES))
    rot = Rot(a.ctx, ROW, "i16")

    def submit(t, i, o, g, r):
        if t == 7:                                               # queued behind the seventh frame, in front of the eighth
            a.rc.export_streams_dev(SRC, d_rec.data_ptr())
            a.ctx.export_streams_dev(SRC, d_ctx.data_ptr())
        a.rc.submit_host_i16(i, o, g)

    stay = rot.run(x, submit)
    rec = to_host(a.ctx, d_rec)
    for i, s in enumerate(SRC):
        nb = api.rate_state_bytes(RATES6[s])
        assert np.array_equal(rec[i, :nb], want_rec[s]), f"record of stream {s} equals the host export"
        assert not rec[i, nb:].any(), f"record of stream {s}: zeros from its size up to the stride"
        assert api.rate_state_check(rec[i, :nb], RATES6[s]) == api.SS_OK
    a.close()
    rot.free()
    # into other slots of a second mixed converter whose streams start at 48000
    b = tm.MixedPair(model, (48000,) * B)
    st_ctx, st_rc = dev_i32(len(SRC)), dev_i32(len(SRC))
    b.rc.set_stream_rates(DST, src_rates)
    b.ctx.import_streams_dev(DST, d_ctx.data_ptr(), st_ctx.data_ptr())
    b.rc.import_streams_dev(DST, d_rec.data_ptr(), st_rc.data_ptr())
    xb = np.zeros_like(x)
    xb[:, DST] = x[:, SRC]
    rot = Rot(b.ctx, ROW, "i16")
    moved = rot.run(xb, lambda t, i, o, g, r: b.rc.submit_host_i16(i, o, g), frames=range(7, T))
    assert not to_host(b.ctx, st_ctx).any() and not to_host(b.ctx, st_rc).any()
    for k, t in enumerate(range(7, T)):
        for s, d in zip(SRC, DST):
            n = nof(RATES6[s])
            assert same(np.ascontiguousarray(moved[k][0][d, :n]), np.ascontiguousarray(stay[t][0][s, :n])), f"frame {t}: stream {s} continues in slot {d}"
            assert same(moved[k][1][d], stay[t][1][s]), f"g|r frame {t}: stream {s} continues in slot {d}"
    assert all(np.count_nonzero(np.stack([stay[t][0][s, :nof(RATES6[s])] for t in range(7, T)])) > 0 for s in SRC)
    b.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 8
def warm_pair(model, seed):
    """A mixed pair three synchronous frames in: every tail holds signal"""
    p = tm.MixedPair(model, RATES6)
    x = noise("i16", ROW, seed)
    for t in range(3):
        p.rc.process_i16(x[t])
    return p


def export_dev(p, ids):
    d = dev_bytes((len(ids), p.rc.record_stride()), 0xAB)
    p.rc.export_streams_dev(ids, d.data_ptr())
    return to_host(p.ctx, d)


def test_device_records_hostile_headers(model):
    import torch
    p = warm_pair(model, 7)
    before = export_dev(p, SRC)
    assert all(before[i, 16:api.rate_state_bytes(RATES6[s])].any() for i, s in enumerate(SRC))
    plan = {0: "magic", 2: "version", 3: "other_rate", 4: "size_word", 5: "good"}
    recs = before.copy()
    body = recs[:, 16:].view(F32)
    body += F32(1.0)                                             # an import that went through would change every tail
    want_status = []
    for i, s in enumerate(SRC):
        table = {name: (hdr, verdict) for name, hdr, verdict in cases.hostile_headers(RATES6[s])}
        hdr, verdict = table[plan[s]]
        recs[i, :16] = np.frombuffer(hdr, np.uint8)
        want_status.append(verdict)
        assert api.rate_state_check(recs[i, :api.rate_state_bytes(RATES6[s])], RATES6[s]) == verdict, "the host verdict for the same bytes"
    assert want_status == [cases.SS_BAD_MAGIC, cases.SS_BAD_VERSION, cases.SS_BAD_RATE, cases.SS_BAD_SIZE, cases.SS_OK]
    d_recs = torch.from_numpy(recs).to("cuda:0")
    torch.cuda.synchronize()
    d_status = dev_i32(len(SRC))
    p.rc.import_streams_dev(SRC, d_recs.data_ptr(), d_status.data_ptr())
    assert to_host(p.ctx, d_status).tolist() == want_status
    after = export_dev(p, SRC)
    for i, s in enumerate(SRC):
        nb = api.rate_state_bytes(RATES6[s])
        if want_status[i] == cases.SS_OK:
            assert np.array_equal(after[i, :nb], recs[i, :nb]) and not np.array_equal(after[i], before[i]), f"stream {s}: the good record is imported"
            assert not after[i, nb:].any()
        else:
            assert np.array_equal(after[i], before[i]), f"stream {s}: a refused record leaves both tails untouched"
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_device_records_refusals(model):
    p = warm_pair(model, 8)
    L = p.ctx.L
    before = export_dev(p, SRC)
    d_buf = dev_bytes((4, 912), 0xAB)
    d_good = dev_bytes((4, 912))
    p.rc.export_streams_dev([0, 2, 3, 4], d_good.data_ptr())
    d_status = dev_i32(4)
    ids = lambda *a: np.array(a, np.int32)

    def refused(lst, ptr, imp):
        a = ids(*lst)
        rc = L.pn_rate_import_streams(p.rc.h, a.ctypes.data, a.size, ptr, d_status.data_ptr()) if imp else \
            L.pn_rate_export_streams(p.rc.h, a.ctypes.data, a.size, ptr)
        assert rc == -1, (lst, imp)
        return L.pn_last_error()

    assert b"no converter state" in refused([0, 1], d_buf.data_ptr(), False)          # a 48000 slot
    assert b"no converter state" in refused([0, 1], d_good.data_ptr(), True)
    assert b"twice" in refused([0, 2, 0], d_good.data_ptr(), True)                    # a duplicate id on import
    assert b"out of range" in refused([0, B], d_buf.data_ptr(), False)
    assert b"aligned" in refused([0, 2], d_buf.data_ptr() + 8, False)                 # a misaligned pointer
    assert b"aligned" in refused([0, 2], d_good.data_ptr() + 8, True)
    a = ids(0, 2)
    assert L.pn_rate_import_streams(p.rc.h, a.ctypes.data, 2, d_good.data_ptr(), None) == -1, "d_status is required"
    assert L.pn_rate_export_streams(p.rc.h, a.ctypes.data, 0, None) == 0 and L.pn_rate_import_streams(p.rc.h, a.ctypes.data, 0, None, None) == 0
    assert (to_host(p.ctx, d_buf) == 0xAB).all(), "a refused export writes nothing"
    assert (to_host(p.ctx, d_status) == 77).all(), "a refused import writes no status"
    assert np.array_equal(export_dev(p, SRC), before), "every tail is unchanged"
    dup = export_dev(p, [4, 0, 4])                                                    # duplicates are legal in an export
    assert np.array_equal(dup[0], before[3]) and np.array_equal(dup[1], before[0]) and np.array_equal(dup[2], before[3])
    p.close()
    # a single-rate converter: the stride is the record, the device export is the host export
    q = tg.Pair(model, B, 16000)
    x = noise("i16", 160, 9)
    for t in range(2):
        q.rc.process_i16(x[t])
    assert q.rc.record_stride() == api.rate_state_bytes(16000) == 528
    assert np.array_equal(export_dev(q, [5, 0, 5]), q.rc.export_streams([5, 0, 5]))
    q.close()


# ---------------------------------------------------------------------------------------------------------------- 10
def test_profiling_of_the_two_kernels(model):
    x = noise("i16", 80, 10)
    plain = api.Context(model, B)
    plain_keys = set(plain.kernel_times())
    plain.close()
    p = tg.Pair(model, B, 8000)
    rot = Rot(p.ctx, 80, "i16")
    rot.run(x, lambda t, i, o, g, r: p.rc.submit_host_i16(i, o, g))
    assert p.rc.kernel_times() == {"rate_up": (0.0, 0), "rate_down": (0.0, 0)}, "off by default: nothing is recorded"
    p.rc.set_profiling(True)
    rot.run(x, lambda t, i, o, g, r: p.rc.submit_host_i16(i, o, g))
    times = p.rc.kernel_times()
    print("rate_up / rate_down over 14 frames (ms, launches):", times)
    assert set(times) == {"rate_up", "rate_down"}
    for name, (ms, launches) in times.items():
        assert launches == T and ms > 0, name
    assert set(p.ctx.kernel_times()) == plain_keys, "the context's family list is unchanged"
    p.rc.set_profiling(False)
    p.rc.reset_profile()
    rot.run(x[:2], lambda t, i, o, g, r: p.rc.submit_host_i16(i, o, g))
    assert p.rc.kernel_times() == {"rate_up": (0.0, 0), "rate_down": (0.0, 0)}
    ms, n = ctypes.c_double(), ctypes.c_int64()
    assert p.ctx.L.pn_rate_kernel_time(p.rc.h, b"backend", ctypes.byref(ms), ctypes.byref(n)) == -1
    p.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 11
def cli_through_python(model, rates, pcm, names, n_slots):
    """percepnet_run --rates .. --slots n_slots --report (percepnet_run.cpp run_shard) restated on the Python pipelined path: pairs
    queue for the slots, a slot taken over continues at the new pair's rate after a reset, three rotating pinned sets, the report
    records through h_report -> (output samples per pair, report lines in the order they are printed)"""
    P = len(rates)
    nb = min(n_slots, P)
    ctx = api.Context(model, nb)
    rc = api.MixedRateConverter(ctx, rates[:nb])
    ctx.set_report(True)
    ns = [nof(r) for r in rates]
    avail = [len(p) // n for p, n in zip(pcm, ns)]
    pos = [0] * P
    rot = Rot(ctx, ROW, "i16", nb)
    meta = [dict(pair=[None] * nb, skip=[False] * nb, last=[False] * nb) for _ in range(3)]
    out = [[] for _ in range(P)]
    stat = [dict(frames=0, clipped=0, peak=F32(0), e_in=0.0, e_out=0.0) for _ in range(P)]
    lines = []
    cur, alive, first, next_pair = list(range(nb)), [True] * nb, [True] * nb, nb

    def flush(k):
        m = meta[k]
        o, rep = rot.sets[k][1].a, rot.sets[k][3].a
        for s in range(nb):
            pr = m["pair"][s]
            if pr is None:
                continue
            ps = stat[pr]
            if not m["skip"][s]:
                out[pr].append(o[s, :ns[pr]].copy())
                f = rep[s, :4].view(F32)
                ps["frames"] += 1
                ps["clipped"] += int(rep[s, 6:7].view(np.int32)[0])
                ps["e_in"] += float(f[1])
                ps["e_out"] += float(f[3])
                ps["peak"] = max(ps["peak"], f[2])
            if m["last"][s]:
                level = "%.2f dB" % (10 * math.log10(ps["e_out"] / ps["e_in"])) if ps["e_in"] > 0 and ps["e_out"] > 0 else "n/a"
                lines.append("%s: frames %d clipped %d peak %.6f level %s" % (names[pr], ps["frames"], ps["clipped"], float(ps["peak"]), level))

    t = 0
    while True:
        m = meta[t % 3]
        inp, o, gr, rep = rot.sets[t % 3]
        restart, restart_rates = [], []
        for s in range(nb):
            m["pair"][s], m["skip"][s], m["last"][s] = None, False, False
            row = None
            if alive[s]:
                pr = cur[s]
                if pos[pr] < avail[pr]:
                    row = pcm[pr][pos[pr] * ns[pr]:(pos[pr] + 1) * ns[pr]]
                    pos[pr] += 1
                else:
                    alive[s] = False
                    prev = meta[(t + 2) % 3]
                    if t >= 1 and prev["pair"][s] == pr:
                        prev["last"][s] = True
                    while next_pair < P:
                        pr = cur[s] = next_pair
                        next_pair += 1
                        if avail[pr] >= 1:
                            row, pos[pr], alive[s], first[s] = pcm[pr][:ns[pr]], 1, True, True
                            restart.append(s)
                            restart_rates.append(rates[pr])
                            break
            inp.a[s] = 0
            if alive[s]:
                m["pair"][s], m["skip"][s] = cur[s], first[s]
                first[s] = False
                inp.a[s, :ns[cur[s]]] = row
        if not any(alive):
            break
        if restart:
            ctx.reset_streams(restart)
            rc.set_stream_rates(restart, restart_rates)
        rc.submit_host_i16(inp.p, o.p, gr.p, h_report=rep.p)
        if t >= 2:
            flush((t - 2) % 3)
        t += 1
    ctx.host_wait()
    for u in range(max(t - 2, 0), t):
        flush(u % 3)
    rc.close()
    ctx.close()
    rot.free()
    return [np.concatenate(o) if o else np.zeros(0, np.int16) for o in out], lines


def test_cli_equals_the_python_pipelined_path(model, blob, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    rates, frames = (8000, 48000, 16000, 24000), (9, 12, 8, 10)   # two slots: 8000 -> 16000 in one, 48000 -> 24000 in the other
    (tmp_path / "m.pnw").write_bytes(blob)
    pcm, args, names = [], [], []
    for i, (r, f) in enumerate(zip(rates, frames)):
        n = nof(r)
        v = noise("i16", f * n + 37 + 5 * i, 20 + i, 1, 1)[0, 0].copy()    # a partial tail frame, which is dropped
        v.tofile(tmp_path / f"in{i}.pcm")
        pcm.append(v)
        names.append(f"out{i}.pcm")
        args += [f"in{i}.pcm", f"out{i}.pcm"]
    run = subprocess.run([exe, "--model", "m.pnw", "--rates", ",".join(map(str, rates)), "--slots", "2", "--report"] + args,
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    want, lines = cli_through_python(model, list(rates), pcm, names, 2)
    for i, (r, f) in enumerate(zip(rates, frames)):
        got = np.fromfile(tmp_path / f"out{i}.pcm", np.int16)
        assert got.size == (f - 1) * nof(r) and np.count_nonzero(want[i]) > 0
        assert np.array_equal(got, want[i]), f"pair {i} ({r} Hz)"
    assert len(lines) == 4 and run.stdout.splitlines() == lines
