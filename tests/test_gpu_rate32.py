"""32000 Hz on the rate converter, on the GPU (-m gpu): the rational 3:2 rows of percepnet_amd/csrc/pn_rate.hip
(rt_up_rows<3, 2> / rt_down_rows<3, 2>) in the single-rate and the mixed kernels, through every entry point that carries a rate.

Every comparison is bit equality.  The kernels are checked against the exact float32 models of tests/rate32_model.py, fed the
LIBRARY's taps (tests/test_rate32_host.py ties those models to the shipped integer-factor arithmetic and checks the taps); a
mixed converter against single-rate converters of each stream's rate; the pipelined path against the synchronous one.

Sizes: B = 5 (one full block of four waves and a partial one) and B = 1; the mixed batch is B = 6 at
(32000, 48000, 16000, 32000, 8000, 24000), so block 0 runs four different branches and block 1 is partial.  The kernel tests run
4 frames, so that both tails cross frame boundaries; the whole-frame tests run 10, past the engine's 6 frames of delay."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import conf_model as cm
from tests import families
from tests import g711_model as gm
from tests import rate32_model as r32
from tests import rate_model as rmod

pytestmark = pytest.mark.gpu
F32 = np.float32
RATE, N, TD = 32000, 320, 48
RATES6 = (32000, 48000, 16000, 32000, 8000, 24000)
T_KERNEL, T_CHAIN = 4, 10
DTYPE = {"f32": np.float32, "i16": np.int16, "g711": np.uint8}
SENTINEL = {"f32": F32(777.0), "i16": np.int16(12345), "g711": np.uint8(0x5A)}


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


def nof(rate):
    return api.rate_mixed_frame_samples(rate)


_taps = {}


def taps(rate):
    if rate not in _taps:
        _taps[rate] = (api.rate_taps(rate, False), api.rate_taps(rate, True))
    return _taps[rate]


def models(rate, B):
    """(up, down) float32 models of B streams at `rate` with the library's taps; 48000 is a copy"""
    if rate == 48000:
        return (lambda x: np.array(x, F32)), (lambda o: np.array(o, F32))
    L, M = r32.LM[rate]
    h, g = taps(rate)
    return r32.Up(B, L, M, h), r32.Down(B, L, M, g)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


_keep = []


@pytest.fixture(autouse=True)
def keep_device_rows():
    """the converter's launches are asynchronous on the context's stream: every row handed to one stays allocated to the test's end"""
    yield
    _keep.clear()


def to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()                   # the context runs on its own non-blocking stream
    _keep.append(t)
    return t


def to_host(ctx, t):
    ctx.synchronize()
    return t.cpu().numpy()


def dev_full(shape, dtype, fill):
    import torch
    t = torch.full(shape, fill, dtype={np.float32: torch.float32, np.int16: torch.int16, np.uint8: torch.uint8, np.int32: torch.int32}[dtype], device="cuda:0")
    torch.cuda.synchronize()
    _keep.append(t)
    return t


def dev_out(shape, kind):
    return dev_full(shape, DTYPE[kind], SENTINEL[kind].item())


class Pair:
    """A context and a converter beside it: single-rate (rate an int) or mixed (a tuple of rates)"""

    def __init__(self, model, B, rate, nn_mode=api.NN_MFMA):
        self.ctx = api.Context(model, B, nn_mode=nn_mode)
        self.mixed = not isinstance(rate, int)
        self.rc = api.MixedRateConverter(self.ctx, rate) if self.mixed else api.RateConverter(self.ctx, rate)
        self.B, self.rate, self.n = B, rate, self.rc.frame

    def up(self, kind, d_in, d_out, ids=None):
        getattr(self.rc, f"up_{kind}_dev")(d_in.data_ptr(), d_out.data_ptr(), ids=ids)

    def down(self, kind, d_in, d_out, ids=None):
        getattr(self.rc, f"down_{kind}_dev")(d_in.data_ptr(), d_out.data_ptr(), ids=ids)

    def tails(self, ids):
        """the two tails of the listed streams as the host export gives them, one row per stream"""
        return [self.rc.export_streams([s])[0] for s in ids]

    def close(self):
        self.rc.close()
        self.ctx.close()


def samples(kind, shape, seed, law=gm.ULAW):
    """seeded rows of a format over its whole range, and the float32 samples they stand for"""
    rng = np.random.default_rng(32000 + seed)
    if kind == "f32":
        x = rng.uniform(-1.0, 1.0, shape).astype(F32)
        return x, x
    if kind == "i16":
        x = rng.integers(-32768, 32768, shape).astype(np.int16)
        x[0, 3], x[0, 4] = -32768, 32767
        return x, rmod.from_i16(x)
    x = rng.integers(0, 256, shape).astype(np.uint8)
    return x, rmod.from_i16(gm.decode(law, x))


def leave(kind, z, saturate, law=gm.ULAW):
    """what the down kernel writes for the float32 row z in a format"""
    if kind == "f32":
        return z
    c = rmod.to_i16(z, saturate)
    return c if kind == "i16" else gm.encode(law, c)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", ("f32", "i16", "g711"))
def test_kernels_alone_against_the_model(model, kind):
    """Single-rate at 32000: up and down, 4 frames with carried tails, B = 5 and 1; G.711 goes up under A-law and down under mu-law."""
    for B in (5, 1):
        p = Pair(model, B, RATE)
        assert p.n == N and p.rc.state_bytes == 336 and p.rc.record_stride() == 336
        up_law, down_law = gm.ALAW, gm.ULAW
        x, xf = samples(kind, (B, T_KERNEL * N), B, up_law)
        o = (np.random.default_rng(3232 + B).uniform(-1.0, 1.0, (B, T_KERNEL * 480)) * 1.5).astype(F32)
        up, down = models(RATE, B)
        over = 0
        for t in range(T_KERNEL):
            if kind == "g711":
                p.rc.set_stream_laws(list(range(B)), [up_law] * B)
            d_y = dev_full((B, 480), np.float32, float("nan"))
            p.up(kind, to_dev(x[:, t * N:(t + 1) * N]), d_y)
            y = to_host(p.ctx, d_y)
            assert same(y, up(xf[:, t * N:(t + 1) * N])), f"up B={B} {kind} frame {t}"
            assert np.count_nonzero(y[:, 1::3]) > 0
            if kind == "g711":
                p.rc.set_stream_laws(list(range(B)), [down_law] * B)
            d_z = dev_out((B, N), kind)
            p.down(kind, to_dev(o[:, t * 480:(t + 1) * 480]), d_z)
            z = down(o[:, t * 480:(t + 1) * 480])
            over += int(rmod.rm.clipped_t(z * F32(32768)).sum())
            assert same(to_host(p.ctx, d_z), leave(kind, z, False, down_law)), f"down B={B} {kind} frame {t}"
        assert over > 0, "precondition: the cast sees out-of-range values"
        p.close()


@pytest.mark.parametrize("kind", ("f32", "i16", "g711"))
def test_kernels_with_an_id_list_touch_nothing_else(model, kind):
    B, ids = 5, [3, 1]
    rest = [s for s in range(B) if s not in ids]
    p = Pair(model, B, RATE)
    up, down = models(RATE, B)
    x, xf = samples(kind, (B, 2 * N), 11)
    o = np.random.default_rng(7).uniform(-1.0, 1.0, (B, 2 * 480)).astype(F32)
    d_y, d_z = dev_full((B, 480), np.float32, 777.0), dev_out((B, N), kind)
    p.up(kind, to_dev(x[:, :N]), d_y)                            # frame 0 for everybody: every tail holds signal
    p.down(kind, to_dev(o[:, :480]), d_z)
    up(xf[:, :N]); down(o[:, :480])
    before, before_listed = p.tails(rest), p.tails(ids)
    d_y, d_z = dev_full((B, 480), np.float32, 777.0), dev_out((B, N), kind)
    p.up(kind, to_dev(x[:, N:]), d_y, ids=ids)
    p.down(kind, to_dev(o[:, 480:]), d_z, ids=ids)
    y, z = to_host(p.ctx, d_y), to_host(p.ctx, d_z)
    want_y, want_z = up(xf[:, N:]), leave(kind, down(o[:, 480:]), False)
    assert same(y[ids], want_y[ids]) and same(z[ids], want_z[ids])
    assert (y[rest] == F32(777.0)).all() and (z[rest] == SENTINEL[kind]).all(), "unlisted rows are not written"
    assert all(np.array_equal(a, b) for a, b in zip(p.tails(rest), before)), "unlisted tails are not written"
    assert all(not np.array_equal(a, b) for a, b in zip(p.tails(ids), before_listed)), "listed tails advance"
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def singles(model):
    """one single-rate pair of B = 6 per rate with a filter: what a mixed stream is compared against, slot for slot"""
    ps = {r: Pair(model, 6, r) for r in sorted(set(RATES6) - {48000})}
    yield ps
    for p in ps.values():
        p.close()


@pytest.mark.parametrize("kind", ("f32", "i16", "g711"))
def test_mixed_equals_single_rate_converters_slot_for_slot(model, singles, kind):
    B = len(RATES6)
    p = Pair(model, B, RATES6)
    laws = [(gm.ULAW, gm.ALAW)[s % 2] for s in range(B)]
    for q in [p] + list(singles.values()):
        q.rc.reset()
        q.rc.set_stream_laws(list(range(B)), laws)
    rng = np.random.default_rng(66)
    for t in range(T_KERNEL):
        x = samples(kind, (B, 480), 100 + t)[0]
        o = rng.uniform(-1.0, 1.0, (B, 480)).astype(F32)
        d_y, d_z = dev_full((B, 480), np.float32, 777.0), dev_out((B, 480), kind)
        p.up(kind, to_dev(x), d_y)
        p.down(kind, to_dev(o), d_z)
        y, z = to_host(p.ctx, d_y), to_host(p.ctx, d_z)
        for r, q in singles.items():
            n = nof(r)
            s_y, s_z = dev_full((B, 480), np.float32, 777.0), dev_out((B, n), kind)
            q.up(kind, to_dev(x[:, :n]), s_y)
            q.down(kind, to_dev(o), s_z)
            s_y, s_z = to_host(q.ctx, s_y), to_host(q.ctx, s_z)
            for s in [s for s in range(B) if RATES6[s] == r]:
                assert same(y[s], s_y[s]), f"up {kind} frame {t} stream {s} ({r} Hz)"
                assert same(z[s, :n], s_z[s]), f"down {kind} frame {t} stream {s} ({r} Hz)"
                assert (z[s, n:] == SENTINEL[kind]).all(), f"frame {t} stream {s}: the rest of the output row is untouched"
        assert same(z[1], leave(kind, o[1], False, laws[1]))     # the 48000 stream: a copy through the format
    # the 32000 rows against the model too, one frame from zeroed tails
    p.rc.reset()
    x, xf = samples(kind, (B, 480), 200)
    xf = np.stack([rmod.from_i16(gm.decode(laws[s], x[s])) for s in range(B)]) if kind == "g711" else xf
    d_y = dev_full((B, 480), np.float32, 777.0)
    p.up(kind, to_dev(x), d_y)
    up, _ = models(RATE, 2)
    assert same(to_host(p.ctx, d_y)[[0, 3]], up(xf[[0, 3], :N]))
    p.close()


def test_mixed_with_one_stream_at_32000(model):
    p = Pair(model, 1, (RATE,))
    up, down = models(RATE, 1)
    rng = np.random.default_rng(1)
    for t in range(2):
        x, o = rng.uniform(-1, 1, (1, 480)).astype(F32), rng.uniform(-1, 1, (1, 480)).astype(F32)
        d_y, d_z = dev_full((1, 480), np.float32, 777.0), dev_out((1, 480), "f32")
        p.up("f32", to_dev(x), d_y)
        p.down("f32", to_dev(o), d_z)
        z = to_host(p.ctx, d_z)
        assert same(to_host(p.ctx, d_y), up(x[:, :N])) and same(z[:, :N], down(o)) and (z[:, N:] == F32(777.0)).all()
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_rate_changes_leave_no_stale_tail_words(model):
    """8000 -> 32000 -> 16000 on slot 1 between frames: after each change the slot equals a fresh converter of the new rate.  The
    8000 tail is 192 words, the 32000 tail 48, the 16000 tail 96: words 48..95 written at 8000 must be zero again at 16000."""
    B, s = 3, 1
    p = Pair(model, B, (24000, 8000, 48000))
    rng = np.random.default_rng(832)
    for rate in (8000, RATE, 16000):
        if rate != 8000:
            p.rc.set_stream_rates([s], [rate])
        assert p.rc.stream_rates().tolist() == [24000, rate, 48000]
        fresh = Pair(model, 1, rate)
        n = nof(rate)
        for t in range(2):
            x, o = rng.uniform(-1, 1, (B, 480)).astype(F32), rng.uniform(-1, 1, (B, 480)).astype(F32)
            d_y, d_z = dev_full((B, 480), np.float32, 777.0), dev_out((B, 480), "f32")
            p.up("f32", to_dev(x), d_y)
            p.down("f32", to_dev(o), d_z)
            f_y, f_z = dev_full((1, 480), np.float32, 777.0), dev_out((1, n), "f32")
            fresh.up("f32", to_dev(x[s:s + 1, :n]), f_y)
            fresh.down("f32", to_dev(o[s:s + 1]), f_z)
            assert same(to_host(p.ctx, d_y)[s], to_host(fresh.ctx, f_y)[0]), f"up at {rate} Hz frame {t}"
            assert same(to_host(p.ctx, d_z)[s, :n], to_host(fresh.ctx, f_z)[0]), f"down at {rate} Hz frame {t}"
        assert np.array_equal(p.rc.export_streams([s]), fresh.rc.export_streams([0]))
        fresh.close()
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 4
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


def chain_noise(kind, B, n, seed):
    g = np.random.default_rng(9000 + seed).standard_normal((T_CHAIN, B, n)) * 0.25
    return g.clip(-1.0, 1.0 - 2.0 ** -15).astype(F32) if kind == "f32" else np.rint(g * 32768).clip(-32768, 32767).astype(np.int16)


def pipelined(p, kind, x, ctx_frames=()):
    """x [T, B, n] through submit_host_*, one frame in flight behind the other -> per frame (out, gr); frames listed in
    ctx_frames go through the CONTEXT's own pn_submit_host_* instead, as 48 kHz frames (row length 480 only)"""
    B, n = x.shape[1:]
    sets = [(Pin(p.ctx.L, (B, n), DTYPE[kind]), Pin(p.ctx.L, (B, n), DTYPE[kind]), Pin(p.ctx.L, (B, 68), F32)) for _ in range(3)]
    res = []
    for t in range(len(x)):
        i, o, g = sets[t % 3]
        i.a[...] = x[t]
        o.a.view(np.uint8)[...] = 0xEE
        if t in ctx_frames:
            p.ctx._chk(getattr(p.ctx.L, f"pn_submit_host_{kind}")(p.ctx.h, i.p, o.p, g.p))
        else:
            getattr(p.rc, f"submit_host_{kind}")(i.p, o.p, g.p)
        if t >= 2:
            res.append((sets[(t - 2) % 3][1].a.copy(), sets[(t - 2) % 3][2].a.copy()))
    p.ctx.host_wait()
    for t in range(max(len(x) - 2, 0), len(x)):
        res.append((sets[t % 3][1].a.copy(), sets[t % 3][2].a.copy()))
    assert p.ctx.frames_delivered() == len(x)
    for s in sets:
        for q in s:
            q.free()
    return res


@pytest.mark.parametrize("kind", ("i16", "f32"))
def test_whole_frames_single_rate(model, kind):
    """10 frames at 32000, B = 5: the host form, the device form, the active form with a skipped stream and the pipelined
    form give the same bits."""
    B, skip = 5, 2
    x = chain_noise(kind, B, N, 1)
    a = Pair(model, B, RATE)
    want = [getattr(a.rc, f"process_{kind}")(x[t]) for t in range(T_CHAIN)]
    a.close()
    assert np.count_nonzero(np.stack([w[0] for w in want[7:]])) > 0, "the frames past the engine's delay carry signal"
    b, c = Pair(model, B, RATE), Pair(model, B, RATE)
    ids = [s for s in range(B) if s != skip]
    for t in range(T_CHAIN):
        d_in = to_dev(x[t])
        o1, o2 = dev_out((B, N), kind), dev_out((B, N), kind)
        g1 = dev_full((B, 68), np.float32, float("nan"))
        getattr(b.rc, f"process_{kind}_dev")(d_in.data_ptr(), o1.data_ptr(), g1.data_ptr())
        getattr(c.rc, f"process_{kind}_dev")(d_in.data_ptr(), o2.data_ptr(), None, ids=ids)
        r1, r2 = to_host(b.ctx, o1), to_host(c.ctx, o2)
        assert same(r1, want[t][0]) and same(to_host(b.ctx, g1), want[t][1]), f"{kind} frame {t}: device form"
        assert same(r2[ids], want[t][0][ids]) and (r2[skip] == SENTINEL[kind]).all(), f"{kind} frame {t}: active form"
    b.close(); c.close()
    d = Pair(model, B, RATE)
    got = pipelined(d, kind, x)
    for t in range(T_CHAIN):
        assert same(got[t][0], want[t][0]) and same(got[t][1], want[t][1]), f"{kind} frame {t}: pipelined form"
    d.close()


def test_whole_frames_mixed_interleaved_with_the_contexts_own_submits(model):
    """A mixed converter at RATES6, float rows of 480: frames 3 and 6 go through the context's own pn_submit_host_f32 as 48 kHz
    frames, the others through the converter.  The pipelined run equals the synchronous one, each stream's own n samples."""
    B = len(RATES6)
    x = chain_noise("f32", B, 480, 2)
    own = (3, 6)
    a = Pair(model, B, RATES6)
    want = [a.ctx.process_f32(x[t]) if t in own else a.rc.process_f32(x[t]) for t in range(T_CHAIN)]
    a.close()
    b = Pair(model, B, RATES6)
    got = pipelined(b, "f32", x, own)
    b.close()
    for t in range(T_CHAIN):
        for s, r in enumerate(RATES6):
            n = 480 if t in own else nof(r)
            assert same(got[t][0][s, :n], want[t][0][s, :n]), f"frame {t} stream {s} ({r} Hz)"
            assert same(got[t][1][s], want[t][1][s]), f"g|r frame {t} stream {s}"
            if t not in own:
                assert not want[t][0][s, n:].any(), "the host form returns the rest of a row as zeros"
    assert all(np.count_nonzero(want[-1][0][s, :nof(r)]) > 0 for s, r in enumerate(RATES6))


# ---------------------------------------------------------------------------------------------------------------- 5
def burst(rate, f_rel, n_samples):
    """a sine at f_rel * rate under a Hann envelope over the middle quarter of the length, zeros around it (so that the
    correlation peak is unique: one period off costs 1e-3 of it), peak 0.5"""
    t = np.arange(n_samples)
    env = np.zeros(n_samples)
    w = n_samples // 4
    env[(n_samples - w) // 2:(n_samples - w) // 2 + w] = np.hanning(w)
    return (0.5 * np.sin(2 * np.pi * f_rel * t) * env).astype(F32)


def lag_of(x, z):
    K = 1 << int(np.ceil(np.log2(2 * x.size)))
    c = np.fft.irfft(np.fft.rfft(z.astype(np.float64), K) * np.conj(np.fft.rfft(x.astype(np.float64), K)), K)
    return int(np.argmax(c[:x.size]))


def test_delay_and_fidelity_at_a_0_db_limit(model):
    """A sine burst at 0.05 of the rate through the whole chain (up, the engine at a 0 dB attenuation limit, down) in one mixed
    converter at (32000, 24000).  The lag of the correlation peak is 1952 samples at 32000 (1472 at 24000), and the maximum error
    against the float64 model of the same chain (rate32_model.chain_f64), past the first 8 frames, is at most twice what the
    24 kHz stream of the same run shows against its own model.
    Measured on an MI355X: 32 kHz 1.99e-07, 24 kHz 1.68e-07 (ratio 1.18): both are fp32 rounding of a signal of peak 0.5."""
    T = 40
    rates = (RATE, 24000)
    p = Pair(model, 2, rates)
    p.ctx.set_atten_limit([0, 1], 0.0)
    x = [burst(r, 0.05, T * nof(r)) for r in rates]
    z = [np.zeros(T * nof(r), F32) for r in rates]
    row = np.zeros((2, 480), F32)
    for t in range(T):
        for s, r in enumerate(rates):
            row[s, :nof(r)] = x[s][t * nof(r):(t + 1) * nof(r)]
        out = p.rc.process_f32(row, want_gr=False)[0]
        for s, r in enumerate(rates):
            z[s][t * nof(r):(t + 1) * nof(r)] = out[s, :nof(r)]
    p.close()
    err = []
    for s, r in enumerate(rates):
        L, M = r32.LM[r]
        ref = r32.chain_f64(x[s], L, M)
        lag, mlag = lag_of(x[s], z[s]), lag_of(x[s], ref)
        err.append(float(np.abs(z[s] - ref)[8 * nof(r):].max()))
        print(f"{r} Hz: lag {lag} (model {mlag}), max |GPU - float64 model| {err[-1]:.3e}")
        assert lag == mlag == api.rate_mixed_delay_samples(r) == r32.delay_samples(r)
    assert api.rate_delay_samples(RATE) == 1952
    assert err[0] <= 2 * err[1]


# ---------------------------------------------------------------------------------------------------------------- 6
def test_host_records_move_between_a_mixed_and_a_single_rate_converter(model):
    K = 8
    x = chain_noise("f32", 2, 480, 3)
    a = Pair(model, 2, (8000, RATE))
    stay = [a.rc.process_f32(x[t]) for t in range(T_CHAIN)]
    a.close()
    a = Pair(model, 2, (8000, RATE))
    for t in range(K):                                           # past the engine's 6 frames of delay: both tails hold signal
        a.rc.process_f32(x[t])
    rec_ctx, rec = a.ctx.export_streams([1]), a.rc.export_streams([1])
    assert rec.shape == (1, 336) and api.rate_state_check(rec[0], RATE) == api.SS_OK
    assert struct.unpack_from("<4sIIi", rec[0].tobytes()) == (b"PNRS", 1, 336, RATE)
    body = rec[0, 16:].view("<f4")
    assert same(body[:32], x[K - 1, 1, N - 32:N]), "the up tail: the last 32 input samples, oldest first"
    assert body[32:].any(), "the down tail: 48 samples at 48 kHz"
    with pytest.raises(api.PercepNetError):
        a.rc.import_streams([0], rec)                            # an 8000 slot refuses it
    b = Pair(model, 1, RATE)
    b.ctx.import_streams([0], rec_ctx)
    b.rc.import_streams([0], rec)
    assert np.array_equal(b.rc.export_streams([0]), rec)
    for t in range(K, T_CHAIN):
        z, gr = b.rc.process_f32(x[t, 1:2, :N])
        assert same(z[0], stay[t][0][1, :N]) and same(gr[0], stay[t][1][1]), f"frame {t}"
    # and back into a mixed slot
    back = b.rc.export_streams([0])
    a.rc.import_streams([1], back)
    assert np.array_equal(a.rc.export_streams([1]), back)
    assert np.count_nonzero(stay[-1][0][1, :N]) > 0
    a.close(); b.close()


def test_device_records_at_the_fixed_stride(model):
    rates = (8000, RATE, 48000, 24000, RATE)
    p = Pair(model, len(rates), rates)
    x = chain_noise("i16", len(rates), 480, 4)
    for t in range(8):                                           # past the engine's delay: the down tails hold signal
        p.rc.process_i16(x[t])
    ids, sizes = [0, 1, 3], [912, 336, 400]
    assert p.rc.record_stride() == 912
    d_rec = dev_full((3, 912), np.uint8, 0xAB)
    p.rc.export_streams_dev(ids, d_rec.data_ptr())
    rec = to_host(p.ctx, d_rec)
    for i, (s, nb) in enumerate(zip(ids, sizes)):
        assert struct.unpack_from("<4sIIi", rec[i].tobytes()) == (b"PNRS", 1, nb, rates[s])
        assert np.array_equal(rec[i, :nb], p.rc.export_streams([s])[0]) and rec[i, 16:nb].any()
        assert not rec[i, nb:].any(), "zeros from the record's size up to the stride"
    # import: the 32000 record into slot 4 (good), a 16000 record into slot 1 (refused)
    before = p.tails([1, 4])
    recs = np.zeros((2, 912), np.uint8)
    recs[0, :336] = rec[1, :336]
    recs[0, 16:336].view("<f4")[...] += F32(1.0)
    q = Pair(model, 1, 16000)
    q.rc.process_f32(chain_noise("f32", 1, 160, 5)[0])
    recs[1, :528] = q.rc.export_streams([0])[0]
    q.close()
    want = [api.rate_state_check(recs[0, :336], RATE), api.rate_state_check(recs[1, :528], RATE)]
    assert want == [api.SS_OK, api.SS_BAD_RATE]
    d_status = dev_full((2,), np.int32, 77)
    d_recs = to_dev(recs)
    p.rc.import_streams_dev([4, 1], d_recs.data_ptr(), d_status.data_ptr())
    assert to_host(p.ctx, d_status).tolist() == want
    after = p.tails([1, 4])
    assert np.array_equal(after[0], before[0]), "the refused slot's tails are untouched"
    assert np.array_equal(after[1], recs[0, :336]) and not np.array_equal(after[1], before[1])
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_conference_of_three_rates_and_three_formats(model):
    """Streams 0 (32000, int16), 1 (8000, G.711 A-law) and 2 (48000, float) in one conference, stream 3 (32000, float) in none:
    up per format with id lists, the mix, down per format — against conf_model.mix fed the per-stream models."""
    rates, confs = (RATE, 8000, 48000, RATE), [2, 2, 2, cm.NONE]
    fmt = ("i16", "g711", "f32", "f32")
    B = 4
    p = Pair(model, B, rates)
    p.rc.set_stream_laws([1], [gm.ALAW])
    p.rc.set_stream_confs(list(range(B)), confs)
    ups, downs = zip(*(models(r, 1) for r in rates))
    for t in range(3):
        rows = {k: samples(k, (B, 480), 300 + 10 * t + i, gm.ALAW) for i, k in enumerate(DTYPE)}
        d_y, d_o = dev_full((B, 480), np.float32, 777.0), dev_full((B, 480), np.float32, 555.0)
        for k in DTYPE:
            p.up(k, to_dev(rows[k][0]), d_y, ids=[s for s in range(B) if fmt[s] == k])
        p.rc.mix_f32_dev(d_y.data_ptr(), d_o.data_ptr())
        y = np.concatenate([ups[s](rows[fmt[s]][1][s:s + 1, :nof(rates[s])]) for s in range(B)])
        assert same(to_host(p.ctx, d_y), y), f"frame {t}: the 48 kHz rows"
        o = cm.mix(y, confs)
        assert cm.same(to_host(p.ctx, d_o), o), f"frame {t}: the mix"
        for k in DTYPE:
            d_z = dev_out((B, 480), k)
            ids = [s for s in range(B) if fmt[s] == k]
            p.down(k, d_o, d_z, ids=ids)
            z = to_host(p.ctx, d_z)
            for s in ids:
                n = nof(rates[s])
                want = leave(k, downs[s](o[s:s + 1])[0], False, gm.ALAW)
                assert same(z[s, :n], want), f"frame {t} stream {s} ({rates[s]} Hz, {k})"
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_saturating_edge_at_32000(model):
    B = 5
    o = (np.random.default_rng(99).uniform(-1.0, 1.0, (B, 480)) * 1.5).astype(F32)
    for saturate in (False, True):
        p = Pair(model, B, RATE)
        p.ctx.set_output_saturate(saturate)
        _, down = models(RATE, B)
        z = down(o)
        assert rmod.rm.clipped_t(z * F32(32768)).any(axis=1).all(), "every row leaves the int16 range"
        d_z = dev_out((B, N), "i16")
        p.down("i16", to_dev(o), d_z)
        got = to_host(p.ctx, d_z)
        assert same(got, rmod.to_i16(z, saturate)), f"saturate={saturate}"
        p.close()
    assert not np.array_equal(rmod.to_i16(z, True), rmod.to_i16(z, False))


# ---------------------------------------------------------------------------------------------------------------- 9
def test_cli_rate_32000_and_rates(model, blob, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    rates, frames = (RATE, 8000), (10, 9)
    rng = np.random.default_rng(3200)
    pcm = [np.rint(rng.standard_normal(f * nof(r) + 17 + i) * 8192).clip(-32768, 32767).astype(np.int16) for i, (r, f) in enumerate(zip(rates, frames))]
    for i, v in enumerate(pcm):
        v.tofile(tmp_path / f"in{i}.pcm")
    r = subprocess.run([exe, "--model", "m.pnw", "--rate", "32000", "in0.pcm", "out0.pcm"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    p = Pair(model, 1, RATE)
    want = p.rc.run_pcm(pcm[0][None, :frames[0] * N])[0]
    p.close()
    got = np.fromfile(tmp_path / "out0.pcm", np.int16)
    assert got.size == (frames[0] - 1) * N and np.count_nonzero(want[7 * N:]) > 0 and np.array_equal(got, want)
    r = subprocess.run([exe, "--model", "m.pnw", "--rates", "32000,8000", "in0.pcm", "mix0.pcm", "in1.pcm", "mix1.pcm"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    p = Pair(model, 2, rates)
    want = p.rc.run_pcm(pcm)
    p.close()
    for i in range(2):
        got = np.fromfile(tmp_path / f"mix{i}.pcm", np.int16)
        assert got.size == (frames[i] - 1) * nof(rates[i]) and np.array_equal(got, want[i]), f"pair {i}"
    bad = subprocess.run([exe, "--model", "m.pnw", "--rate", "32001", "in0.pcm", "x.pcm"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    # refused with what was expected and the usage text, which names the new rate
    assert bad.returncode == 1 and "--rate: expected" in bad.stderr and "got '32001'" in bad.stderr and not (tmp_path / "x.pcm").exists()
    assert "usage:" in bad.stderr and "--rate 8000|16000|24000|32000" in bad.stderr
