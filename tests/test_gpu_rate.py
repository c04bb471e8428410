"""The batched rate converter on the GPU (-m gpu): include/percepnet_hip.h "batched rate converter"; kernels
percepnet_amd/csrc/pn_rate.hip, host side pn_rate.cpp, binding api.RateConverter, CLI percepnet_run --rate.

The two kernels are checked bit for bit against the exact float32 models of tests/rate_model.py, which are fed the LIBRARY's
taps (api.rate_taps; tests/test_rate_host.py checks those against an independent double design).  A whole frame is checked
against the same three steps called by hand and, in NN_STRICT, against numpy up -> the CPU oracle -> numpy down.

Sizes: B = 5 (a partial last block of four) and B = 1, all three rates.  The kernel tests run 4 frames, so that both tails cross
frame boundaries.  The whole-frame tests run those 4 and 6 more: the engine's own delay is 6 frames (2880 samples), so only from
frame 6 on does anything but zeros reach the down-converter; the events the tests are about (reset, skipped tick, move) stay at
frame 2."""
import os
import struct
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import families
from tests import rate_model as rmod

pytestmark = pytest.mark.gpu
RATES = rmod.RATES
BS = (5, 1)
T_KERNEL, T_CHAIN = 4, 10
MODES = {"mfma": api.NN_MFMA, "strict": api.NN_STRICT}
F32 = np.float32


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


_taps = {}


def taps(rate):
    if rate not in _taps:
        _taps[rate] = (api.rate_taps(rate, False), api.rate_taps(rate, True))
    return _taps[rate]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def noise_f32(rate, B, T, seed=0):
    """Seeded floats in [-1, 1): [B, T * n]"""
    n = 480 // rmod.factor(rate)
    return np.random.default_rng(1000 + seed + rate).uniform(-1.0, 1.0, (B, T * n)).astype(F32)


def noise_i16(rate, B, T, seed=0):
    """Seeded int16 over the whole range, both ends included: [B, T * n]"""
    n = 480 // rmod.factor(rate)
    x = np.random.default_rng(2000 + seed + rate).integers(-32768, 32768, (B, T * n)).astype(np.int16)
    x[0, 3], x[0, 4], x[-1, n + 1], x[-1, n + 2] = -32768, 32767, 32767, -32768
    return x


def fr(x, t, n):
    return np.ascontiguousarray(x[:, t * n:(t + 1) * n])


class Pair:
    """A context and a converter beside it."""

    def __init__(self, model, B, rate, nn_mode=api.NN_MFMA):
        self.ctx = api.Context(model, B, nn_mode=nn_mode)
        self.rc = api.RateConverter(self.ctx, rate)
        self.B, self.rate, self.L, self.n = B, rate, rmod.factor(rate), 480 // rmod.factor(rate)

    def reset(self):
        self.ctx.reset()
        self.rc.reset()

    def close(self):
        self.rc.close()
        self.ctx.close()


def to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()                   # the context runs on its own non-blocking stream
    return t


def to_host(ctx, t):
    ctx.synchronize()
    return t.cpu().numpy()


def dev_full(shape, dtype, fill):
    import torch
    t = torch.full(shape, fill, dtype=dtype, device="cuda:0")
    torch.cuda.synchronize()
    return t


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("rate", RATES)
def test_up_kernel_alone(model, rate):
    import torch
    h, _ = taps(rate)
    for B in BS:
        p = Pair(model, B, rate)
        L, n = p.L, p.n
        for kind in ("f32", "i16"):
            p.rc.reset()
            x = noise_f32(rate, B, T_KERNEL) if kind == "f32" else noise_i16(rate, B, T_KERNEL)
            xf = x if kind == "f32" else rmod.from_i16(x)
            up = rmod.Up(B, L, h)
            rows = []
            for t in range(T_KERNEL):
                d_in, d_out = to_dev(fr(x, t, n)), dev_full((B, 480), torch.float32, float("nan"))
                (p.rc.up_f32_dev if kind == "f32" else p.rc.up_i16_dev)(d_in.data_ptr(), d_out.data_ptr())
                y = to_host(p.ctx, d_out)
                assert same(y, up(fr(xf, t, n))), f"{rate} Hz B={B} {kind} frame {t}"
                rows.append(y)
            y = np.concatenate(rows, axis=1)
            delayed = np.concatenate([np.zeros((B, rmod.T), F32), xf], axis=1)[:, :T_KERNEL * n]
            assert same(np.ascontiguousarray(y[:, ::L]), delayed), "phase 0 carries the bits of the input 16 samples earlier"
            assert np.count_nonzero(y[:, 1::L]) > 0
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("rate", RATES)
def test_down_kernel_alone(model, rate):
    import torch
    _, g = taps(rate)
    for B in BS:
        p = Pair(model, B, rate)
        L, n = p.L, p.n
        # (the seed is one whose rows, by the numpy model alone, leave the int16 range after the filter at every rate, also in row 0)
        o = (np.random.default_rng(3003 + rate).uniform(-1.0, 1.0, (5, T_KERNEL * 480)).astype(F32) * F32(1.5))[:B].astype(F32)
        for kind in ("f32", "wrap", "saturate"):
            p.rc.reset()
            p.ctx.set_output_saturate(kind == "saturate")
            down = rmod.Down(B, L, g)
            over = 0
            for t in range(T_KERNEL):
                d_in = to_dev(fr(o, t, 480))
                if kind == "f32":
                    d_out = dev_full((B, n), torch.float32, float("nan"))
                    p.rc.down_f32_dev(d_in.data_ptr(), d_out.data_ptr())
                else:
                    d_out = dev_full((B, n), torch.int16, 12345)
                    p.rc.down_i16_dev(d_in.data_ptr(), d_out.data_ptr())
                got, z = to_host(p.ctx, d_out), down(fr(o, t, 480))
                over += int(rmod.rm.clipped_t(z * F32(32768)).sum())
                want = z if kind == "f32" else rmod.to_i16(z, kind == "saturate")
                assert same(got, want), f"{rate} Hz B={B} {kind} frame {t}"
            assert over > 0, "precondition: both casts see out-of-range values"
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rate", RATES)
def test_whole_frame_is_the_three_steps_by_hand(model, rate, mode):
    import torch
    for B in BS:
        a, b = Pair(model, B, rate, MODES[mode]), Pair(model, B, rate, MODES[mode])
        n = a.n
        for kind in ("f32", "i16"):
            a.reset(); b.reset()
            x = noise_f32(rate, B, T_CHAIN, 1) if kind == "f32" else noise_i16(rate, B, T_CHAIN, 1)
            dt = torch.float32 if kind == "f32" else torch.int16
            energy = 0.0
            for t in range(T_CHAIN):
                d_in = to_dev(fr(x, t, n))
                o1, o2 = dev_full((B, n), dt, 77), dev_full((B, n), dt, 99)
                g1, g2 = dev_full((B, 68), torch.float32, float("nan")), dev_full((B, 68), torch.float32, float("nan"))
                x48, y48 = dev_full((B, 480), torch.float32, float("nan")), dev_full((B, 480), torch.float32, float("nan"))
                if kind == "f32":
                    a.rc.process_f32_dev(d_in.data_ptr(), o1.data_ptr(), g1.data_ptr())
                    b.rc.up_f32_dev(d_in.data_ptr(), x48.data_ptr())
                else:
                    a.rc.process_i16_dev(d_in.data_ptr(), o1.data_ptr(), g1.data_ptr())
                    b.rc.up_i16_dev(d_in.data_ptr(), x48.data_ptr())
                b.ctx.process_f32_dev(x48.data_ptr(), y48.data_ptr(), g2.data_ptr())
                (b.rc.down_f32_dev if kind == "f32" else b.rc.down_i16_dev)(y48.data_ptr(), o2.data_ptr())
                r1, r2 = to_host(a.ctx, o1), to_host(b.ctx, o2)
                assert same(r1, r2), f"{rate} Hz {mode} B={B} {kind} frame {t}"
                assert same(to_host(a.ctx, g1), to_host(b.ctx, g2)), f"g|r {rate} Hz {mode} B={B} {kind} frame {t}"
                energy += float((r1.astype(np.float64) ** 2).sum())
            assert energy > 0, "the frames past the engine's delay must carry signal"
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def oracle_chain(oracle, rate, x):
    """x [B, T * n] fp32 -> (z [B, T * n], gr [B, T, 68]): numpy up, the CPU oracle's float entry point, numpy down."""
    h, g = taps(rate)
    B, L = x.shape[0], rmod.factor(rate)
    n = 480 // L
    T = x.shape[1] // n
    up, down = rmod.Up(B, L, h), rmod.Down(B, L, g)
    x48 = np.concatenate([up(fr(x, t, n)) for t in range(T)], axis=1)
    res = [oracle.run_float(x48[s]) for s in range(B)]
    y48 = np.stack([r[0] for r in res])
    z = np.concatenate([down(fr(y48, t, 480)) for t in range(T)], axis=1)
    return z, np.stack([r[1] for r in res])


@pytest.mark.parametrize("rate", RATES)
def test_strict_chain_against_the_oracle(model, oracle, rate):
    for B in BS:
        x = noise_f32(rate, B, T_CHAIN, 2)
        want, want_gr = oracle_chain(oracle, rate, x)
        assert np.count_nonzero(want[:, 6 * (480 // rmod.factor(rate)):]) > 0
        p = Pair(model, B, rate, api.NN_STRICT)
        for t in range(T_CHAIN):
            z, gr = p.rc.process_f32(fr(x, t, p.n))
            assert same(z, fr(want, t, p.n)), f"{rate} Hz B={B} frame {t}"
            assert same(gr, np.ascontiguousarray(want_gr[:, t])), f"g|r {rate} Hz B={B} frame {t}"
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def run_host(model, rate, x, nn_mode=api.NN_MFMA, before=None):
    """x [B, T * n] fp32 through a fresh pair, host entry point -> z [T, B, n], gr [T, B, 68]; before(t, pair) runs first."""
    p = Pair(model, x.shape[0], rate, nn_mode)
    zs, grs = [], []
    for t in range(x.shape[1] // p.n):
        if before:
            before(t, p)
        z, gr = p.rc.process_f32(fr(x, t, p.n))
        zs.append(z); grs.append(gr)
    p.close()
    return np.stack(zs), np.stack(grs)


@pytest.mark.parametrize("rate", RATES)
def test_reset_streams(model, rate):
    for B in BS:
        s = 2 if B > 2 else 0
        x = noise_f32(rate, B, T_CHAIN, 3)
        n = 480 // rmod.factor(rate)
        plain, plain_gr = run_host(model, rate, x)

        def reset_at_2(t, p):
            if t == 2:
                p.ctx.reset_streams([s]); p.rc.reset_streams([s])
        got, got_gr = run_host(model, rate, x, before=reset_at_2)
        fresh, fresh_gr = run_host(model, rate, np.ascontiguousarray(x[s:s + 1, 2 * n:]))
        keep = np.arange(B) != s
        assert same(got[:, keep], plain[:, keep]) and same(got_gr[:, keep], plain_gr[:, keep]), "the other streams are undisturbed"
        assert same(got[:2, s], plain[:2, s])
        assert same(got[2:, s], fresh[:, 0]) and same(got_gr[2:, s], fresh_gr[:, 0]), "a reset stream continues like a fresh one"
        assert np.count_nonzero(fresh[6:]) > 0 and not same(got[2:, s], plain[2:, s])


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("rate", RATES)
def test_active_set(model, rate):
    import torch
    for B in BS:
        skipped = [1, 3] if B > 3 else [0]
        x = noise_f32(rate, B, T_CHAIN, 4)
        n = 480 // rmod.factor(rate)
        plain, _ = run_host(model, rate, x)
        # the skipped streams alone, fed only the frames they receive
        recv = [t for t in range(T_CHAIN) if t != 2]
        xs = np.concatenate([fr(x, t, n)[skipped] for t in recv], axis=1)
        alone, _ = run_host(model, rate, xs)
        p = Pair(model, B, rate)
        d_out = dev_full((B, n), torch.float32, 12345.0)
        d_gr = dev_full((B, 68), torch.float32, 54321.0)
        k = 0
        for t in range(T_CHAIN):
            ids = [s for s in range(B) if not (t == 2 and s in skipped)]
            before = to_host(p.ctx, d_out).copy()
            d_in = to_dev(fr(x, t, n))
            p.rc.process_f32_dev(d_in.data_ptr(), d_out.data_ptr(), d_gr.data_ptr(), ids=ids)
            out = to_host(p.ctx, d_out)
            if t == 2:
                assert same(out[skipped], before[skipped]), "rows of skipped streams stay untouched"
            else:
                assert same(out[skipped], alone[k]), f"{rate} Hz B={B} tick {t}: skipped streams continue from what they received"
                k += 1
            listed = [s for s in range(B) if s not in skipped]
            assert same(out[listed], plain[t][listed]), f"{rate} Hz B={B} tick {t}: listed streams match an all-active run"
        # an id list is refused under the context's rules, and nothing runs
        before = to_host(p.ctx, d_out).copy()
        d_x48 = dev_full((B, 480), torch.float32, float("nan"))
        for bad in ([0, 0], [B], [-1]):
            with pytest.raises(api.PercepNetError):
                p.rc.process_f32_dev(d_in.data_ptr(), d_out.data_ptr(), None, ids=bad)
            with pytest.raises(api.PercepNetError):
                p.rc.up_f32_dev(d_in.data_ptr(), d_x48.data_ptr(), ids=bad)
        assert same(to_host(p.ctx, d_out), before) and np.isnan(to_host(p.ctx, d_x48)).all()
        assert p.ctx.L.pn_ctx_frames_done(p.ctx.h) == T_CHAIN
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("rate", RATES)
def test_moving_a_stream(model, rate):
    B, s = 5, 1
    x = noise_f32(rate, B, T_CHAIN, 5)
    plain, plain_gr = run_host(model, rate, x)
    src, dst = Pair(model, B, rate), Pair(model, 1, rate)
    n = src.n
    for t in range(3):                                           # frames 0..2 in the source
        src.rc.process_f32(fr(x, t, n))
    rec_ctx, rec_rc = src.ctx.export_streams([s]), src.rc.export_streams([s])
    assert rec_rc.shape == (1, api.rate_state_bytes(rate)) and api.rate_state_check(rec_rc[0], rate) == api.SS_OK
    assert struct.unpack_from("<4sIIi", rec_rc[0].tobytes()) == (b"PNRS", 1, api.rate_state_bytes(rate), rate)
    tail = rec_rc[0, 16:].view("<f4")
    assert same(np.ascontiguousarray(tail[:32]), np.ascontiguousarray(x[s, 3 * n - 32:3 * n])), "the up tail: the last 32 input samples, oldest first"
    # a record of another rate is refused and the target is left untouched: first feed the target something to lose
    dst.rc.process_f32(fr(x, 0, n)[:1])
    keep = dst.rc.export_streams([0])
    other = RATES[(RATES.index(rate) + 1) % 3]
    po = Pair(model, 1, other)
    rec_other = po.rc.export_streams([0])
    po.close()
    with pytest.raises(api.PercepNetError):
        dst.rc.import_streams([0], rec_other)
    forged = rec_rc.copy()
    forged[0, 12:16] = np.frombuffer(struct.pack("<i", other), np.uint8)         # this rate's size, another rate's name
    with pytest.raises(api.PercepNetError):
        dst.rc.import_streams([0], forged)
    lib = dst.ctx.L                                              # Pair.L is the rate factor; the library hangs off the context
    assert lib.pn_rate_import_streams_host(dst.rc.h, np.zeros(1, np.int32).ctypes.data, 1, forged.ctypes.data) == -1
    assert b"Hz" in lib.pn_last_error()
    assert np.array_equal(dst.rc.export_streams([0]), keep)
    # the move
    dst.ctx.import_streams([0], rec_ctx)
    dst.rc.import_streams([0], rec_rc)
    for t in range(3, T_CHAIN):
        z, gr = dst.rc.process_f32(fr(x, t, n)[s:s + 1])
        assert same(z[0], plain[t, s]) and same(gr[0], plain_gr[t, s]), f"{rate} Hz frame {t}"
    assert np.count_nonzero(plain[6:, s]) > 0
    src.close(); dst.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def band_limited_noise(rate, B, n_samples, seed):
    """Aperiodic noise below 0.6 of the low-rate Nyquist (an FFT mask over the whole length), peak 0.5: [B, n_samples] fp32"""
    w = np.random.default_rng(seed).standard_normal((B, n_samples))
    W = np.fft.rfft(w, axis=1)
    W[:, np.fft.rfftfreq(n_samples, 1.0 / rate) >= 0.6 * rate / 2] = 0
    W[:, 0] = 0
    v = np.fft.irfft(W, n_samples, axis=1)
    return (0.5 * v / np.abs(v).max(axis=1, keepdims=True)).astype(F32)


def lag_and_residual(x, z, n, delay_hint=None):
    """-> (lag of the maximum cross-correlation of z against x, residual-to-signal power ratio in dB after aligning by that
    lag, over the output samples past the first 8 frames)"""
    N = x.size
    M = 1 << int(np.ceil(np.log2(2 * N)))
    c = np.fft.irfft(np.fft.rfft(z.astype(np.float64), M) * np.conj(np.fft.rfft(x.astype(np.float64), M)), M)
    lag = int(np.argmax(c[:N]))
    zz, xx = z[max(lag, 8 * n):].astype(np.float64), x[max(lag, 8 * n) - lag:N - lag].astype(np.float64)
    return lag, 10 * np.log10(((zz - xx) ** 2).sum() / (xx ** 2).sum())


@pytest.mark.parametrize("rate", RATES)
def test_delay_and_fidelity_at_a_0_db_limit(model, rate):
    """The lag of the maximum cross-correlation is exactly the documented delay, and past the first 8 frames the residual after
    that alignment is at most 1 dB above what the float64 model of the same chain leaves (both are printed, per rate and stream;
    the model alone gives -88.8 | -89.2 | -90.0 dB at 8 | 16 | 24 kHz for stream 0 of the B = 1 case)."""
    T, L = 40, rmod.factor(rate)
    n = 480 // L
    for B in BS:
        x = band_limited_noise(rate, B, T * n, 7 + rate)

        def bypass(t, p):
            if t == 0:
                p.ctx.set_atten_limit(np.arange(B), 0.0)
        z = run_host(model, rate, x, before=bypass)[0]               # [T, B, n]
        z = np.ascontiguousarray(z.transpose(1, 0, 2)).reshape(B, T * n)
        for s in range(B):
            lag, gpu_db = lag_and_residual(x[s], z[s], n)
            mlag, model_db = lag_and_residual(x[s], rmod.chain_f64(x[s], L), n)
            print(f"{rate} Hz B={B} stream {s}: lag {lag} (model {mlag}), residual GPU {gpu_db:.2f} dB, float64 model {model_db:.2f} dB")
            assert lag == api.rate_delay_samples(rate) == mlag
            assert gpu_db <= model_db + 1.0


# ---------------------------------------------------------------------------------------------------------------- 9
def test_cli_rate_16000(model, blob, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    rate, n = 16000, 160
    frames = (12, 9)
    (tmp_path / "m.pnw").write_bytes(blob)
    pcm = []
    for i, f in enumerate(frames):
        v = (band_limited_noise(rate, 1, f * n + 37 + 50 * i, 50 + i)[0] * 32767 * 1.2).clip(-32768, 32767).astype(np.int16)
        v.tofile(tmp_path / f"in{i}.pcm")
        pcm.append(v)
    r = subprocess.run([exe, "--model", "m.pnw", "--rate", "16000", "--strict", "--slots", "1", "in0.pcm", "out0.pcm", "in1.pcm", "out1.pcm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for i, f in enumerate(frames):
        got = np.fromfile(tmp_path / f"out{i}.pcm", np.int16)
        assert got.size == (f - 1) * n
        p = Pair(model, 1, rate, api.NN_STRICT)
        want = p.rc.run_pcm(pcm[i][None, :f * n])[0]
        p.close()
        assert np.count_nonzero(want) > 0 and np.array_equal(got, want), f"pair {i}"
    bad = subprocess.run([exe, "--model", "m.pnw", "--rate", "44100", "in0.pcm", "x.pcm"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--rate" in bad.stderr and not (tmp_path / "x.pcm").exists()
