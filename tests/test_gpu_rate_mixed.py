"""The mixed rate converter on the GPU (-m gpu): include/percepnet_hip.h "mixed rates"; kernels pn_rate_up_mixed_kernel /
pn_rate_down_mixed_kernel in percepnet_amd/csrc/pn_rate.hip, host side pn_rate.cpp, binding api.MixedRateConverter, CLI
percepnet_run --rates.

Every comparison is bit equality: against the float32 models of tests/rate_model.py fed the library's taps (the kernels alone),
against slot s of a single-rate converter of the same batch size fed the same input (a whole frame), and against the plain
context (a 48000 stream, whose conversion is a copy).  No tolerance anywhere.

Batches: B = 5 at (8000, 48000, 16000, 24000, 8000) — one block whose four waves run four different factors, and a partial block
— and B = 1 at each of the four rates.  Inputs are seeded by tests/test_gpu_rate.py's generators: stream s at rate R is row s of
that rate's batch.  Kernel tests run 4 frames, whole-frame tests 10 (the engine's delay is 6)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import families
from tests import rate_model as rmod
from tests import test_gpu_rate as tg

pytestmark = pytest.mark.gpu
RATES5 = (8000, 48000, 16000, 24000, 8000)
CASES = (RATES5,) + tuple((r,) for r in api.MIXED_RATES)
T_KERNEL, T_CHAIN = tg.T_KERNEL, tg.T_CHAIN
MODES = tg.MODES
F32 = np.float32
ROW = 480
same, to_dev, to_host, dev_full = tg.same, tg.to_dev, tg.to_host, tg.dev_full


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
    return 480 // rmod.factor(rate)


def case_id(rates):
    return "-".join(str(r // 1000) for r in rates)


def inputs(kind, rates, T, seed=0):
    """-> per stream s its [T * n_s] samples: row s of test_gpu_rate's seeded batch of that stream's rate and this batch size"""
    gen = tg.noise_f32 if kind == "f32" else tg.noise_i16
    return [gen(r, len(rates), T, seed)[s] for s, r in enumerate(rates)]


def rows(xs, rates, t, fill):
    """Frame t of every stream at the front of a [B, 480] row filled with `fill`"""
    a = np.full((len(rates), ROW), fill, xs[0].dtype)
    for s, r in enumerate(rates):
        n = nof(r)
        a[s, :n] = xs[s][t * n:(t + 1) * n]
    return a


def fill_of(kind):
    return F32(np.nan) if kind == "f32" else np.int16(12345)


def is_fill(a, kind):
    return np.isnan(a).all() if kind == "f32" else (a == 12345).all()


class UpModel:
    """rate_model's up kernel of one stream at any of the four rates (48000: the copy)"""

    def __init__(self, rate):
        self.L = rmod.factor(rate)
        self.m = rmod.Up(1, self.L, tg.taps(rate)[0]) if self.L > 1 else None

    def __call__(self, x):
        x = np.asarray(x, F32)
        return self.m(x[None])[0] if self.m else x.copy()


class DownModel:
    def __init__(self, rate):
        self.L = rmod.factor(rate)
        self.m = rmod.Down(1, self.L, tg.taps(rate)[1]) if self.L > 1 else None

    def __call__(self, o):
        o = np.asarray(o, F32)
        return self.m(o[None])[0] if self.m else o.copy()


class MixedPair:
    """A context and a mixed converter beside it."""

    def __init__(self, model, rates, nn_mode=api.NN_MFMA):
        self.ctx = api.Context(model, len(rates), nn_mode=nn_mode)
        self.rc = api.MixedRateConverter(self.ctx, rates)
        self.B = len(rates)

    def reset(self):
        self.ctx.reset()
        self.rc.reset()

    def close(self):
        self.rc.close()
        self.ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("rates", CASES, ids=case_id)
def test_up_kernel_alone(model, rates):
    import torch
    B = len(rates)
    p = MixedPair(model, rates)
    assert p.rc.stream_rates().tolist() == list(rates) and p.rc.frame == ROW
    assert p.ctx.L.pn_rate_is_mixed(p.rc.h) == 1 and p.ctx.L.pn_rate_row_samples(p.rc.h) == ROW
    for kind in ("f32", "i16"):
        p.rc.reset()
        xs = inputs(kind, rates, T_KERNEL)
        if kind == "i16":
            assert min(x.min() for x in xs) == -32768 and max(x.max() for x in xs) == 32767, "both ends of the int16 range"
        up = [UpModel(r) for r in rates]
        for t in range(T_KERNEL):
            x = rows(xs, rates, t, fill_of(kind))                # the unused remainder: NaN / 12345, and it must not matter
            d_in, d_out = to_dev(x), dev_full((B, 480), torch.float32, float("nan"))
            (p.rc.up_f32_dev if kind == "f32" else p.rc.up_i16_dev)(d_in.data_ptr(), d_out.data_ptr())
            y = to_host(p.ctx, d_out)
            for s, r in enumerate(rates):
                xf = x[s, :nof(r)] if kind == "f32" else rmod.from_i16(x[s, :nof(r)])
                assert same(y[s], up[s](xf)), f"{case_id(rates)} {kind} frame {t} stream {s} ({r} Hz)"
                if r == 48000:
                    assert same(y[s], np.ascontiguousarray(xf, F32)), "48000 is the copy"
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def down_rows(rates):
    """[B][T_KERNEL * 480]: stream s at rate R is row s of test_gpu_rate's down-kernel rows of R (48000: the same recipe)"""
    return [(np.random.default_rng(3003 + r).uniform(-1.0, 1.0, (5, T_KERNEL * 480)).astype(F32) * F32(1.5))[s].astype(F32)
            for s, r in enumerate(rates)]


@pytest.mark.parametrize("rates", CASES, ids=case_id)
def test_down_kernel_alone(model, rates):
    import torch
    B = len(rates)
    o = down_rows(rates)
    # precondition, from the numpy model alone: after the filter the rows leave the int16 range at every rate of the batch
    over = {r: 0 for r in rates}
    for s, r in enumerate(rates):
        dm = DownModel(r)
        for t in range(T_KERNEL):
            over[r] += int(rmod.rm.clipped_t(dm(o[s][t * 480:(t + 1) * 480]) * F32(32768)).sum())
    assert all(v > 0 for v in over.values()), over
    p = MixedPair(model, rates)
    for kind in ("f32", "wrap", "saturate"):
        p.rc.reset()
        p.ctx.set_output_saturate(kind == "saturate")
        down = [DownModel(r) for r in rates]
        for t in range(T_KERNEL):
            d_in = to_dev(np.stack([v[t * 480:(t + 1) * 480] for v in o]))
            if kind == "f32":
                d_out = dev_full((B, ROW), torch.float32, float("nan"))
                p.rc.down_f32_dev(d_in.data_ptr(), d_out.data_ptr())
            else:
                d_out = dev_full((B, ROW), torch.int16, 12345)
                p.rc.down_i16_dev(d_in.data_ptr(), d_out.data_ptr())
            got = to_host(p.ctx, d_out)
            for s, r in enumerate(rates):
                n = nof(r)
                z = down[s](o[s][t * 480:(t + 1) * 480])
                want = z if kind == "f32" else rmod.to_i16(z, kind == "saturate")
                assert same(np.ascontiguousarray(got[s, :n]), want), f"{case_id(rates)} {kind} frame {t} stream {s} ({r} Hz)"
                assert is_fill(got[s, n:], "f32" if kind == "f32" else "i16"), "the remainder of an output row keeps its sentinel"
    p.ctx.set_output_saturate(False)
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def control_run(model, rates, xs, kind, nn_mode):
    """Per stream s: (out [T, n_s], gr [T, 68]) of slot s of a single-rate pair of the same B whose slot s is fed xs[s] (the
    other slots: that rate's own seeded rows), or of the plain context for a 48000 stream.  Host entry points."""
    B, res = len(rates), {}
    for r in sorted(set(rates)):
        n = nof(r)
        T = xs[rates.index(r)].size // n
        gen = tg.noise_f32 if kind == "f32" else tg.noise_i16
        x = gen(r, B, T, 99).copy()
        for s, rs in enumerate(rates):
            if rs == r:
                x[s] = xs[s]
        if r == 48000:
            ctx = api.Context(model, B, nn_mode=nn_mode)
            run = ctx.process_f32 if kind == "f32" else ctx.process_i16
            close = ctx.close
        else:
            pair = tg.Pair(model, B, r, nn_mode)
            run = pair.rc.process_f32 if kind == "f32" else pair.rc.process_i16
            close = pair.close
        outs = [run(tg.fr(x, t, n)) for t in range(T)]
        close()
        for s, rs in enumerate(rates):
            if rs == r:
                res[s] = (np.stack([o[0][s] for o in outs]), np.stack([o[1][s] for o in outs]))
    return res


def mixed_frame(p, kind, form, x, sentinel):
    """One frame of every stream through the mixed pair -> (out [B, 480], gr [B, 68]); device forms start from sentinel rows"""
    import torch
    if form == "host":
        return (p.rc.process_f32 if kind == "f32" else p.rc.process_i16)(x)
    d_in = to_dev(x)
    d_out = dev_full((p.B, ROW), torch.float32 if kind == "f32" else torch.int16, sentinel)
    d_gr = dev_full((p.B, 68), torch.float32, float("nan"))
    (p.rc.process_f32_dev if kind == "f32" else p.rc.process_i16_dev)(d_in.data_ptr(), d_out.data_ptr(), d_gr.data_ptr())
    return to_host(p.ctx, d_out), to_host(p.ctx, d_gr)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rates", CASES, ids=case_id)
def test_mixed_equals_single_rate(model, rates, mode):
    p = MixedPair(model, rates, MODES[mode])
    for kind in ("f32", "i16"):
        xs = inputs(kind, rates, T_CHAIN, 1)
        want = control_run(model, rates, xs, kind, MODES[mode])
        assert all(np.count_nonzero(want[s][0][6:]) > 0 for s in range(len(rates))), "the frames past the engine's delay must carry signal"
        for form in ("dev", "host"):
            p.reset()
            for t in range(T_CHAIN):
                out, gr = mixed_frame(p, kind, form, rows(xs, rates, t, fill_of(kind)), 77)
                for s, r in enumerate(rates):
                    n = nof(r)
                    what = f"{case_id(rates)} {mode} {kind} {form} frame {t} stream {s} ({r} Hz)"
                    assert same(np.ascontiguousarray(out[s, :n]), want[s][0][t]), what
                    assert same(gr[s], want[s][1][t]), "g|r " + what
                    assert (out[s, n:] == (77 if form == "dev" else 0)).all(), "the remainder of an output row is not written: " + what
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_rate_change_between_frames(model):
    import torch
    rates, B = RATES5, 5
    new = {0: 16000, 1: 8000}                                     # 8000 -> 16000 and 48000 -> 8000, from frame 2 on
    after = tuple(new.get(s, r) for s, r in enumerate(rates))
    xa, xb = inputs("f32", rates, T_CHAIN, 6), inputs("f32", after, T_CHAIN, 7)

    def frame_rows(t, change):
        if t < 2 or not change:
            return rows(xa, rates, t, F32(np.nan))
        return rows([xb[s] if s in new else xa[s] for s in range(B)], after, t, F32(np.nan))

    def run(change):
        p = MixedPair(model, rates)
        d_in = [to_dev(frame_rows(t, change)) for t in range(T_CHAIN)]
        d_out = [dev_full((B, ROW), torch.float32, 77.0) for _ in range(T_CHAIN)]
        d_gr = [dev_full((B, 68), torch.float32, float("nan")) for _ in range(T_CHAIN)]
        for t in range(T_CHAIN):                                 # nothing here synchronises: the change is ordered by the stream
            if t == 2 and change:
                ids = np.array(sorted(new), np.int32)
                p.rc.set_stream_rates(ids, [new[s] for s in ids])
                p.ctx.reset_streams(ids)
                assert p.rc.stream_rates().tolist() == list(after)
            p.rc.process_f32_dev(d_in[t].data_ptr(), d_out[t].data_ptr(), d_gr[t].data_ptr())
        out, gr = [to_host(p.ctx, d) for d in d_out], [to_host(p.ctx, d) for d in d_gr]
        p.close()
        return out, gr

    got, got_gr = run(True)
    # streams 2..4 against an undisturbed run
    ctl, ctl_gr = run(False)
    for t in range(T_CHAIN):
        for s in (2, 3, 4):
            assert same(got[t][s], ctl[t][s]) and same(got_gr[t][s], ctl_gr[t][s]), f"frame {t} stream {s} is undisturbed"
    # streams 0 and 1 from frame 2 on: fresh streams of the new rate
    for s, r in new.items():
        n = nof(r)
        fresh = tg.Pair(model, 1, r)
        for t in range(2, T_CHAIN):
            z, g = fresh.rc.process_f32(xb[s][None, t * n:(t + 1) * n])
            assert same(np.ascontiguousarray(got[t][s, :n]), z[0]) and same(got_gr[t][s], g[0]), f"frame {t} stream {s}: a fresh {r} Hz stream"
            assert (got[t][s, n:] == 77).all()
        fresh.close()
        assert np.count_nonzero(np.stack([got[t][s, :n] for t in range(8, T_CHAIN)])) > 0
    # before the change they ran at the old rates (frames 0 and 1 of the undisturbed run)
    for t in range(2):
        assert same(got[t], ctl[t]) and same(got_gr[t], ctl_gr[t])


# ---------------------------------------------------------------------------------------------------------------- 5
def test_active_set(model):
    import torch
    rates, B, skipped = RATES5, 5, [1, 3, 4]                      # a 48000, a 24000 and an 8000 stream sit out frame 2
    # the two kernels alone, against rate_model fed only the frames a stream received
    p = MixedPair(model, rates)
    xs = inputs("f32", rates, T_KERNEL, 4)
    o48 = down_rows(rates)
    up, down = [UpModel(r) for r in rates], [DownModel(r) for r in rates]
    d_y = dev_full((B, 480), torch.float32, 12345.0)
    d_z = dev_full((B, ROW), torch.float32, 54321.0)
    for t in range(T_KERNEL):
        ids = [s for s in range(B) if not (t == 2 and s in skipped)]
        y0, z0 = to_host(p.ctx, d_y).copy(), to_host(p.ctx, d_z).copy()
        d_x, d_o = to_dev(rows(xs, rates, t, F32(np.nan))), to_dev(np.stack([v[t * 480:(t + 1) * 480] for v in o48]))
        p.rc.up_f32_dev(d_x.data_ptr(), d_y.data_ptr(), ids=ids)
        p.rc.down_f32_dev(d_o.data_ptr(), d_z.data_ptr(), ids=ids)
        y, z = to_host(p.ctx, d_y), to_host(p.ctx, d_z)
        for s, r in enumerate(rates):
            n = nof(r)
            if s in ids:
                assert same(y[s], up[s](xs[s][t * n:(t + 1) * n])), f"up frame {t} stream {s}"
                assert same(np.ascontiguousarray(z[s, :n]), down[s](o48[s][t * 480:(t + 1) * 480])), f"down frame {t} stream {s}"
                assert (z[s, n:] == 54321.0).all()
            else:
                assert same(y[s], y0[s]) and same(z[s], z0[s]), "rows of a skipped stream stay untouched"
    # whole frames: the skipped streams continue like the same streams alone, fed only the frames they received
    p.reset()
    xs = inputs("f32", rates, T_CHAIN, 4)
    alone = MixedPair(model, [rates[s] for s in skipped])
    d_out = dev_full((B, ROW), torch.float32, 12345.0)
    d_gr = dev_full((B, 68), torch.float32, 54321.0)
    for t in range(T_CHAIN):
        ids = [s for s in range(B) if not (t == 2 and s in skipped)]
        before = to_host(p.ctx, d_out).copy()
        x = rows(xs, rates, t, F32(np.nan))
        d_x = to_dev(x)
        p.rc.process_f32_dev(d_x.data_ptr(), d_out.data_ptr(), d_gr.data_ptr(), ids=ids)
        out, gr = to_host(p.ctx, d_out), to_host(p.ctx, d_gr)
        if t == 2:
            assert same(out[skipped], before[skipped]), "rows of skipped streams stay untouched"
            continue
        z, g = alone.rc.process_f32(x[skipped])
        for k, s in enumerate(skipped):
            n = nof(rates[s])
            assert same(np.ascontiguousarray(out[s, :n]), np.ascontiguousarray(z[k, :n])) and same(gr[s], g[k]), f"tick {t} stream {s}"
            assert (out[s, n:] == 12345.0).all()
    assert np.count_nonzero(to_host(p.ctx, d_out)[skipped][:, :80]) > 0
    assert p.ctx.L.pn_ctx_frames_done(p.ctx.h) == T_CHAIN
    alone.close()
    p.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_records_between_mixed_and_single_rate(model):
    R, B, s = 16000, 5, 1
    n = nof(R)
    lib = api.load_library()
    x = tg.noise_f32(R, B, T_CHAIN, 5)
    plain, plain_gr = tg.run_host(model, R, x)                    # [T, B, n]: the undisturbed single-rate run
    src = tg.Pair(model, B, R)
    for t in range(3):
        src.rc.process_f32(tg.fr(x, t, n))
    rec_ctx, rec_rc = src.ctx.export_streams([s]), src.rc.export_streams([s])
    src.close()
    assert rec_rc.shape == (1, api.rate_state_bytes(R))
    # into slot 1 of a mixed pair, which runs at 48000 until its rate is set
    dst = MixedPair(model, RATES5)
    ids = lambda *a: np.array(a, np.int32)
    buf = np.full(4 * 912, 0xAB, np.uint8)

    def refused_export(*lst):
        a = ids(*lst)
        assert lib.pn_rate_export_streams_host(dst.rc.h, a.ctypes.data, a.size, buf.ctypes.data) == -1
        assert (buf == 0xAB).all(), "a refused export writes nothing"
        return lib.pn_last_error()

    assert b"one rate" in refused_export(0, 2)                    # 8000 and 16000
    assert b"no converter state" in refused_export(1)             # a 48000 slot
    assert b"no converter state" in refused_export(0, 1)
    a1 = ids(s)
    assert lib.pn_rate_import_streams_host(dst.rc.h, a1.ctypes.data, 1, rec_rc.ctypes.data) == -1, "the slot still runs at 48000"
    dst.rc.set_stream_rates([s], [R])
    other = np.zeros((1, api.rate_state_bytes(8000)), np.uint8)
    other[0, :16] = np.frombuffer(struct.pack("<4sIIi", b"PNRS", 1, api.rate_state_bytes(8000), 8000), np.uint8)
    forged = rec_rc.copy()
    forged[0, 12:16] = np.frombuffer(struct.pack("<i", 24000), np.uint8)
    keep = dst.rc.export_streams([s])
    for bad in (other, forged):
        assert lib.pn_rate_import_streams_host(dst.rc.h, a1.ctypes.data, 1, bad.ctypes.data) == -1 and b"Hz" in lib.pn_last_error()
    a2 = ids(s, 2)                                                # both at 16000 now, the second record of another rate: all or nothing
    two = np.concatenate([rec_rc, forged])
    assert lib.pn_rate_import_streams_host(dst.rc.h, a2.ctypes.data, 2, two.ctypes.data) == -1
    assert np.array_equal(dst.rc.export_streams([s]), keep), "a refused import leaves the converter untouched"
    assert dst.rc.stream_rates().tolist() == [8000, R, 16000, 24000, 8000]
    dst.ctx.import_streams([s], rec_ctx)
    dst.rc.import_streams([s], rec_rc)
    row = np.zeros((B, ROW), F32)
    for t in range(3, 6):
        row[s, :n] = x[s, t * n:(t + 1) * n]
        z, gr = dst.rc.process_f32(row)
        assert same(np.ascontiguousarray(z[s, :n]), plain[t, s]) and same(gr[s], plain_gr[t, s]), f"single-rate -> mixed, frame {t}"
    # and the other way: out of the mixed slot into a single-rate converter
    back_ctx, back_rc = dst.ctx.export_streams([s]), dst.rc.export_streams([s])
    assert back_rc.shape == rec_rc.shape and api.rate_state_check(back_rc[0], R) == api.SS_OK
    dst.close()
    back = tg.Pair(model, 1, R)
    back.ctx.import_streams([0], back_ctx)
    back.rc.import_streams([0], back_rc)
    for t in range(6, T_CHAIN):
        z, gr = back.rc.process_f32(tg.fr(x, t, n)[s:s + 1])
        assert same(z[0], plain[t, s]) and same(gr[0], plain_gr[t, s]), f"mixed -> single-rate, frame {t}"
    assert np.count_nonzero(plain[6:, s]) > 0
    back.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals_change_nothing(model):
    import torch
    rates, B, T = RATES5, 5, 8
    lib = api.load_library()
    ctx = api.Context(model, B)
    with pytest.raises(api.PercepNetError):
        api.MixedRateConverter(ctx, (8000, 48000, 44100, 24000, 8000))
    bad = np.array((8000, 48000, 44100, 24000, 8000), np.int32)
    assert not lib.pn_rate_create_mixed(ctx.h, bad.ctypes.data) and b"index 2:" in lib.pn_last_error()
    single = api.RateConverter(ctx, 16000)
    one, r16 = np.zeros(1, np.int32), np.full(1, 16000, np.int32)
    assert lib.pn_rate_set_stream_rates(single.h, one.ctypes.data, 1, r16.ctypes.data) == -1
    got = np.zeros(B, np.int32)
    assert lib.pn_rate_get_stream_rates(single.h, got.ctypes.data) == 0 and (got == 16000).all()
    assert lib.pn_rate_is_mixed(single.h) == 0 and lib.pn_rate_row_samples(single.h) == 160
    single.close()
    ctx.close()

    xs = inputs("f32", rates, T, 8)

    def run(attempts):
        p = MixedPair(model, rates)
        outs = []
        for t in range(T):
            d_in = to_dev(rows(xs, rates, t, F32(np.nan)))
            d_out = dev_full((B, ROW), torch.float32, 77.0)
            d_gr = dev_full((B, 68), torch.float32, float("nan"))
            if t == 2 and attempts:
                def refused(ids, rs):
                    a, r = np.array(ids, np.int32), np.array(rs, np.int32)
                    assert lib.pn_rate_set_stream_rates(p.rc.h, a.ctypes.data, a.size, r.ctypes.data) == -1
                    assert p.rc.stream_rates().tolist() == list(rates)
                refused([0, 2, 0], [16000, 8000, 24000])          # a duplicate id
                refused([0, B], [16000, 8000])                    # an id out of range
                refused([-1], [16000])
                refused([0, 2], [16000, 44100])                   # a bad rate
                assert lib.pn_rate_set_stream_rates(p.rc.h, None, 2, r16.ctypes.data) == -1
                assert lib.pn_rate_set_stream_rates(p.rc.h, one.ctypes.data, 0, r16.ctypes.data) == 0, "n == 0 is a no-op"
                d_x48 = dev_full((B, 480), torch.float32, float("nan"))
                i, o, x48 = d_in.data_ptr(), d_out.data_ptr(), d_x48.data_ptr()                                  # misaligned rows
                assert lib.pn_rate_process_f32(p.rc.h, i + 4, o, None) == -1 and lib.pn_rate_process_f32(p.rc.h, i, o + 8, None) == -1
                assert lib.pn_rate_up_f32(p.rc.h, i + 4, x48, None, 0) == -1 and lib.pn_rate_up_f32(p.rc.h, i, x48 + 4, None, 0) == -1
                assert lib.pn_rate_down_f32(p.rc.h, x48 + 4, o, None, 0) == -1 and lib.pn_rate_down_f32(p.rc.h, x48, o + 8, None, 0) == -1
                assert b"aligned" in lib.pn_last_error()
                assert (to_host(p.ctx, d_out) == 77.0).all() and np.isnan(to_host(p.ctx, d_x48)).all()
                assert p.rc.stream_rates().tolist() == list(rates)
            p.rc.process_f32_dev(d_in.data_ptr(), d_out.data_ptr(), d_gr.data_ptr())
            outs.append((to_host(p.ctx, d_out), to_host(p.ctx, d_gr)))
        assert p.ctx.L.pn_ctx_frames_done(p.ctx.h) == T
        p.close()
        return outs

    got, ctl = run(True), run(False)
    for t in range(T):
        assert same(got[t][0], ctl[t][0]) and same(got[t][1], ctl[t][1]), f"frame {t} equals the control's"
    assert np.count_nonzero(got[-1][0][:, :80]) > 0


# ---------------------------------------------------------------------------------------------------------------- 8
def test_cli_rates_with_slot_takeover(model, blob, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    rates, frames = (8000, 48000, 16000, 24000), (9, 12, 8, 10)   # two slots: 8000 -> 16000 in one, 48000 -> 24000 in the other
    (tmp_path / "m.pnw").write_bytes(blob)
    pcm, args = [], []
    for i, (r, f) in enumerate(zip(rates, frames)):
        n = nof(r)
        v = (tg.band_limited_noise(r, 1, f * n + 37 + 5 * i, 60 + i)[0] * 32767 * 1.2).clip(-32768, 32767).astype(np.int16)
        v.tofile(tmp_path / f"in{i}.pcm")
        pcm.append(v)
        args += [f"in{i}.pcm", f"out{i}.pcm"]
    run = subprocess.run([exe, "--model", "m.pnw", "--rates", ",".join(map(str, rates)), "--strict", "--slots", "2"] + args,
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    for i, (r, f) in enumerate(zip(rates, frames)):
        n = nof(r)
        got = np.fromfile(tmp_path / f"out{i}.pcm", np.int16)
        assert got.size == (f - 1) * n
        if r == 48000:
            ctx = api.Context(model, 1, nn_mode=api.NN_STRICT)
            want = ctx.run_pcm(pcm[i][None, :f * n])[0][0]
            ctx.close()
        else:
            p = tg.Pair(model, 1, r, api.NN_STRICT)
            want = p.rc.run_pcm(pcm[i][None, :f * n])[0]
            p.close()
        assert np.count_nonzero(want) > 0 and np.array_equal(got, want), f"pair {i} ({r} Hz)"
    for bad in (["--rates", "8000,44100"], ["--rates", "8000"], ["--rate", "8000", "--rates", "8000,8000"]):
        b = subprocess.run([exe, "--model", "m.pnw"] + bad + ["in0.pcm", "x.pcm", "in1.pcm", "y.pcm"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert b.returncode == 1 and "--rates" in b.stderr and not (tmp_path / "x.pcm").exists()
