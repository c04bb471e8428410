"""G.711 rows on the rate converter (-m gpu): include/percepnet_hip.h "G.711 streams"; kernels percepnet_amd/csrc/pn_rate.hip (the
8-bit staging and leaving of the four row kernels), host side pn_rate.cpp, arithmetic pn_g711.h, bindings api.RateConverter /
api.MixedRateConverter, CLI percepnet_run --g711.

The oracle throughout is the unchanged int16 path on a twin context and converter of the same batch size and model, fed the
model-decoded samples (tests/g711_model.py), and the model's encoding of what it gives: a G.711 stream must give, bit for bit, the
encoding of what the _i16 path gives on the decoded samples.  Every comparison is equality; there is no tolerance anywhere.

Shapes: B = 5 (one full block of four waves and a block with one live wave), id lists such as [4, 0, 2], laws mixed across the
streams; the kernel tests run 3 frames (both tails cross frame boundaries), the whole-frame tests 14 (the engine's six-frame delay
plus both filter tails).  Cases: the three single-rate converters and a mixed one with every one of the four rates."""
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api
from tests import families
from tests import g711_model as gm
from tests import test_gpu_rate as tg
from tests import test_gpu_rate_mixed as tm
from tests import test_gpu_rate_pipe as tp

pytestmark = pytest.mark.gpu
B, T_KERNEL, T = 5, 3, 14
RATES5 = (8000, 48000, 16000, 24000, 8000)
CASES = (8000, 16000, 24000, RATES5)
LAWS5 = (gm.ALAW, gm.ULAW, gm.ULAW, gm.ALAW, gm.ULAW)
IDS = [4, 0, 2]
SENTINEL = 0x5A
F32 = np.float32
same, to_dev, to_host, dev_full, nof = tg.same, tg.to_dev, tg.to_host, tg.dev_full, tm.nof


def case_id(case):
    return tm.case_id(case) if isinstance(case, tuple) else str(case // 1000)


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
    """A context and a converter beside it, single-rate (case = the rate) or mixed (case = the rates); laws: set on every stream"""

    def __init__(self, model, case, laws=None, nn_mode=api.NN_MFMA):
        self.mixed = isinstance(case, tuple)
        self.p = tm.MixedPair(model, case, nn_mode) if self.mixed else tg.Pair(model, B, case, nn_mode)
        self.ctx, self.rc = self.p.ctx, self.p.rc
        self.rates = list(case) if self.mixed else [case] * B
        self.ns = [nof(r) for r in self.rates]
        self.w = self.rc.frame
        assert self.rc.stream_laws().tolist() == [gm.ULAW] * B, "a new converter is mu-law everywhere"
        if laws is not None:
            self.rc.set_stream_laws(list(range(B)), laws)
            assert self.rc.stream_laws().tolist() == list(laws)

    def records(self):
        """the converter's state record of every stream that has one"""
        return {s: self.rc.export_streams([s])[0].copy() for s, r in enumerate(self.rates) if r != 48000}

    def close(self):
        self.p.close()


_codes = {}


def codes(w, frames, seed=0):
    """[frames, B, w] seeded random bytes; the first 52 samples of stream s in frame t are the block (s + t) % 5 of the 256 codes
    (five blocks of 52 cover them), so that within three frames every code occurs under both laws of LAWS5"""
    key = (w, frames, seed)
    if key not in _codes:
        a = np.random.default_rng(9000 + seed + w).integers(0, 256, (frames, B, w)).astype(np.uint8)
        for t in range(frames):
            for s in range(B):
                a[t, s, :52] = ((s + t) % 5 * 52 + np.arange(52)) % 256
        a.setflags(write=False)
        _codes[key] = a
    return _codes[key]


def test_the_input_rows_hold_every_code_under_both_laws():
    x = codes(80, T_KERNEL)
    for law in gm.LAWS:
        seen = np.unique(np.concatenate([x[:, s, :80].ravel() for s in range(B) if LAWS5[s] == law]))
        assert seen.size == 256, gm.NAMES[law]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_up_kernel_against_the_int16_kernel(model, case):
    import torch
    a, b = Twin(model, case, LAWS5), Twin(model, case)
    x = codes(a.w, T_KERNEL)
    for t in range(T_KERNEL):
        ids = IDS if t == 1 else None
        lin = gm.decode_rows(LAWS5, x[t])                         # (the rest of a mixed row is decoded too, and ignored like the bytes)
        d_a, d_b = dev_full((B, 480), torch.float32, float("nan")), dev_full((B, 480), torch.float32, float("nan"))
        a.rc.up_g711_dev(to_dev(np.array(x[t])).data_ptr(), d_a.data_ptr(), ids=ids)
        b.rc.up_i16_dev(to_dev(lin).data_ptr(), d_b.data_ptr(), ids=ids)
        ya, yb = to_host(a.ctx, d_a), to_host(b.ctx, d_b)
        for s in range(B):
            if ids is None or s in ids:
                assert same(ya[s], yb[s]) and not np.isnan(ya[s]).any(), f"{case_id(case)} frame {t} stream {s}"
            else:
                assert np.isnan(ya[s]).all(), f"frame {t}: the row of unlisted stream {s} is untouched"
    ra, rb = a.records(), b.records()
    assert ra.keys() == rb.keys() and len(ra) == sum(r != 48000 for r in a.rates)
    for s in ra:
        assert np.array_equal(ra[s], rb[s]) and ra[s][16:16 + 128].any(), f"converter record of stream {s}"
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def down_rows48():
    """[T_KERNEL, B, 480] floats: uniform in +-1.5 (so beyond +-1), with exactly +-1, runs of zeros and one NaN planted"""
    o = (np.random.default_rng(9100).uniform(-1.0, 1.0, (T_KERNEL, B, 480)).astype(F32) * F32(1.5)).astype(F32)
    o[:, :, 7], o[:, :, 8] = F32(1.0), F32(-1.0)
    o[:, :, 100:140] = F32(0)
    o[1, 2, :] = F32(0)                                            # a whole frame of zeros in one stream
    o[0, 0, 300] = F32(np.nan)
    return o


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_down_kernel_against_the_int16_kernel(model, case):
    import torch
    o = down_rows48()
    assert (np.abs(o[np.isfinite(o)]) > 1).any() and (o == 1).any() and (o == -1).any() and np.isnan(o).sum() == 1 and (o == 0).any()
    a, b = Twin(model, case, LAWS5), Twin(model, case)
    lin = {}
    for sat in (False, True):
        a.rc.reset()
        b.rc.reset()
        a.ctx.set_output_saturate(sat)
        b.ctx.set_output_saturate(sat)
        for t in range(T_KERNEL):
            ids = IDS if t == 1 else None
            d_in = to_dev(o[t])
            d_a, d_b = dev_full((B, a.w), torch.uint8, SENTINEL), dev_full((B, a.w), torch.int16, 12345)
            a.rc.down_g711_dev(d_in.data_ptr(), d_a.data_ptr(), ids=ids)
            b.rc.down_i16_dev(d_in.data_ptr(), d_b.data_ptr(), ids=ids)
            ya, yb = to_host(a.ctx, d_a), to_host(b.ctx, d_b)
            lin[sat, t] = yb
            for s, n in enumerate(a.ns):
                if ids is None or s in ids:
                    assert np.array_equal(ya[s, :n], gm.encode(LAWS5[s], yb[s, :n])), f"{case_id(case)} saturate={sat} frame {t} stream {s}"
                    assert (ya[s, n:] == SENTINEL).all(), "the bytes behind a stream's own samples keep their sentinel"
                else:
                    assert (ya[s] == SENTINEL).all(), f"frame {t}: the row of unlisted stream {s} is untouched"
    assert any(not np.array_equal(lin[False, t], lin[True, t]) for t in range(T_KERNEL)), "the rows clip: both casts are exercised"
    ra, rb = a.records(), b.records()
    assert ra.keys() == rb.keys() and all(np.array_equal(ra[s], rb[s]) for s in ra), "the down tails are the int16 path's"
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def run_frames(tw, fmt, x, laws_at, ids_at=lambda t: None, between=lambda tw, t: None):
    """x [T, B, w] bytes (fmt g711) through process_g711_dev, or their decoding under laws_at(t) through process_i16_dev (fmt i16);
    every frame has its own device rows and nothing waits between the frames -> per frame (out rows, g|r)"""
    import torch
    keep, outs = [], []
    for t in range(len(x)):
        between(tw, t)
        if fmt == "g711":
            d_in, d_out = to_dev(np.array(x[t])), dev_full((B, tw.w), torch.uint8, SENTINEL)
            call = tw.rc.process_g711_dev
        else:
            d_in, d_out = to_dev(gm.decode_rows(laws_at(t), x[t])), dev_full((B, tw.w), torch.int16, 12345)
            call = tw.rc.process_i16_dev
        d_gr = dev_full((B, 68), torch.float32, float("nan"))
        call(d_in.data_ptr(), d_out.data_ptr(), d_gr.data_ptr(), ids=ids_at(t))
        keep.append(d_in)
        outs.append((d_out, d_gr))
    return [(to_host(tw.ctx, o).copy(), to_host(tw.ctx, g).copy()) for o, g in outs]


def assert_frames(tw, got, want, laws_at, ids_at=lambda t: None):
    for t, ((ya, ga), (yb, gb)) in enumerate(zip(got, want)):
        ids = ids_at(t)
        for s, n in enumerate(tw.ns):
            if ids is None or s in ids:
                assert np.array_equal(ya[s, :n], gm.encode(laws_at(t)[s], yb[s, :n])), f"frame {t} stream {s}"
                assert same(ga[s], gb[s]), f"g|r frame {t} stream {s}"
                assert (ya[s, n:] == SENTINEL).all()
            else:
                assert (ya[s] == SENTINEL).all(), f"frame {t}: the row of unlisted stream {s} is untouched"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_whole_frame_against_the_int16_path(model, case):
    a, b = Twin(model, case, LAWS5), Twin(model, case)
    x = codes(a.w, T, 1)
    got = run_frames(a, "g711", x, lambda t: LAWS5)
    want = run_frames(b, "i16", x, lambda t: LAWS5)
    assert_frames(a, got, want, lambda t: LAWS5)
    assert all(np.count_nonzero(np.stack([w[0][s, :n] for w in want[8:]])) > 0 for s, n in enumerate(a.ns)), "signal behind the delay"
    a.close()
    b.close()


def test_active_lists_and_a_law_change_between_two_frames(model):
    subsets = ([0, 2, 4], [4, 1, 3], [0, 1, 2, 3, 4], [3])
    ids_at = lambda t: subsets[t % 4]
    after = list(LAWS5)
    after[0], after[1] = gm.ULAW, gm.ALAW
    laws_at = lambda t: LAWS5 if t < 9 else tuple(after)

    def between(tw, t):
        if t == 9:                                               # queued behind frame 8, with no wait: frame 8 runs under the old laws
            tw.rc.set_stream_laws([1, 0], [gm.ALAW, gm.ULAW])

    a, b = Twin(model, RATES5, LAWS5), Twin(model, RATES5)
    x = codes(a.w, T, 2)
    got = run_frames(a, "g711", x, laws_at, ids_at, between)
    want = run_frames(b, "i16", x, laws_at, ids_at)
    assert a.rc.stream_laws().tolist() == after
    assert_frames(a, got, want, laws_at, ids_at)
    # the change matters: under the old laws frame 10 (every stream listed) would not be what it is
    assert not np.array_equal(got[10][0][0, :80], gm.encode(LAWS5[0], want[10][0][0, :80]))
    assert np.count_nonzero(want[10][0][0, :80]) > 0 and np.count_nonzero(want[13][0][1]) > 0
    # resets and rate changes keep the laws; a refused list changes and launches nothing
    a.rc.reset()
    a.rc.reset_streams([0, 1])
    a.rc.set_stream_rates([1], [8000])
    assert a.rc.stream_laws().tolist() == after
    L, h = a.ctx.L, a.rc.h
    i32 = lambda *v: np.array(v, np.int32)
    for ids, laws, word in ((i32(0, 0), i32(1, 1), b"twice"), (i32(0, B), i32(1, 1), b"out of range"), (i32(0, 1), i32(1, 2), b"at index 1:")):
        assert L.pn_rate_set_stream_laws(h, ids.ctypes.data, 2, laws.ctypes.data) == -1 and word in L.pn_last_error()
    assert L.pn_rate_set_stream_laws(h, None, 0, None) == 0
    assert a.rc.stream_laws().tolist() == after
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 4
class Rot8:
    """Three rotating pinned sets of raw bytes, wide enough for int16 rows, for frames of either width on one converter"""

    def __init__(self, ctx, w):
        self.ctx, self.L, self.w = ctx, ctx.L, w
        self.sets = [(tp.Pin(self.L, (B * w * 2,), np.uint8), tp.Pin(self.L, (B * w * 2,), np.uint8), tp.Pin(self.L, (B, 68), F32),
                      tp.Pin(self.L, (B, 8), np.uint32)) for _ in range(3)]

    def rows(self, pin, dtype):
        return pin.a[:B * self.w * np.dtype(dtype).itemsize].view(dtype).reshape(B, self.w)

    def run(self, frames, submit):
        """frames: per frame (dtype, rows); submit(t, h_in, h_out, h_gr, h_rep) -> per frame (out rows, g|r, report), each read
        after the submit of frame t + 2 has returned or after the final pn_host_wait"""
        res = {}

        def take(i):
            _, out, gr, rep = self.sets[i % 3]
            res[i] = (self.rows(out, frames[i][0]).copy(), gr.a.copy(), rep.a.copy())

        for i, (dtype, x) in enumerate(frames):
            inp, out, gr, rep = self.sets[i % 3]
            self.rows(inp, dtype)[...] = x
            out.a[...] = 0xEE
            gr.a.view(np.uint8)[...] = 0xEE
            rep.a[...] = 0xEEEEEEEE
            submit(i, inp.p, out.p, gr.p, rep.p)
            if i >= 2:
                take(i - 2)
        self.ctx.host_wait()
        for i in range(max(len(frames) - 2, 0), len(frames)):
            take(i)
        return [res[i] for i in range(len(frames))]

    def free(self):
        for s in self.sets:
            for p in s:
                p.free()


def test_pipelined_path_equals_the_synchronous_one(model):
    """G.711 frames, every third one an int16 frame on the same converter, two of them with an id list; a law change and a rate
    change between submits with no wait; the report of every frame"""
    import torch
    x8 = codes(480, T, 3)
    x16 = tp.noise("i16", 480, 30, B, T)
    kind_at = lambda t: "i16" if t % 3 == 2 else "g711"
    ids_at = lambda t: IDS if t in (3, 10) else None
    rates_after = list(RATES5)
    rates_after[1] = 8000

    def between(tw, t):
        if t == 5:
            tw.rc.set_stream_laws([0, 1], [gm.ULAW, gm.ALAW])
        if t == 9:
            tw.rc.set_stream_rates([1], [8000])
            tw.ctx.reset_streams([1])

    # the synchronous twin: pn_rate_process_host_g711 / _i16, and the device form for the frames with a list
    b = Twin(model, RATES5, LAWS5)
    b.ctx.set_report(True)
    want = []
    for t in range(T):
        between(b, t)
        if ids_at(t) is None:
            o, g = b.rc.process_g711(x8[t]) if kind_at(t) == "g711" else b.rc.process_i16(x16[t])
        else:
            assert kind_at(t) == "g711"
            d_out, d_gr = dev_full((B, 480), torch.uint8, SENTINEL), dev_full((B, 68), torch.float32, float("nan"))
            b.rc.process_g711_dev(to_dev(np.array(x8[t])).data_ptr(), d_out.data_ptr(), d_gr.data_ptr(), ids=ids_at(t))
            o, g = to_host(b.ctx, d_out), to_host(b.ctx, d_gr)
        want.append((o.copy(), g.copy(), b.ctx.read_report().view(np.uint32).reshape(B, 8).copy()))
    b.close()
    a = Twin(model, RATES5, LAWS5)
    a.ctx.set_report(True)
    rot = Rot8(a.ctx, 480)

    def submit(t, i, o, g, r):
        between(a, t)
        (a.rc.submit_host_g711 if kind_at(t) == "g711" else a.rc.submit_host_i16)(i, o, g, h_report=r, ids=ids_at(t))

    got = rot.run([(np.uint8, x8[t]) if kind_at(t) == "g711" else (np.int16, x16[t]) for t in range(T)], submit)
    for t in range(T):
        rates = RATES5 if t < 9 else rates_after
        for s in (range(B) if ids_at(t) is None else ids_at(t)):
            n = nof(rates[s])
            assert np.array_equal(got[t][0][s, :n], want[t][0][s, :n]), f"frame {t} ({kind_at(t)}) stream {s}"
            assert same(got[t][1][s], want[t][1][s]), f"g|r frame {t} stream {s}"
            assert np.array_equal(got[t][2][s], want[t][2][s]), f"report record frame {t} stream {s}"
    assert all(np.count_nonzero(want[t][0][:, :80] != gm.SILENCE[gm.ULAW]) > 0 for t in (12, 13))
    assert max(w[2].view(F32)[:, 3].max() for w in want[8:]) > 0, "the reports carry output energy"
    assert a.ctx.frames_delivered() == T
    # a refused list consumes no slot
    L = a.ctx.L
    inp, out, gr, _ = rot.sets[0]
    dup, far = np.array([0, 2, 0], np.int32), np.array([0, B], np.int32)
    assert L.pn_rate_submit_host_g711_active(a.rc.h, inp.p, out.p, gr.p, dup.ctypes.data, 3) == -1 and b"twice" in L.pn_last_error()
    assert L.pn_rate_submit_host_g711_active(a.rc.h, inp.p, out.p, gr.p, far.ctypes.data, 2) == -1
    a.ctx.host_wait()
    assert a.ctx.frames_delivered() == T and L.pn_ctx_frames_done(a.ctx.h) == T, "a refused list consumes no pipeline slot"
    a.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_moved_stream_continues_byte_for_byte(model):
    src, dst = [0, 3], [2, 4]
    x = codes(80, T, 4)
    a = Twin(model, 8000, LAWS5)
    for t in range(7):
        a.rc.process_g711(x[t], want_gr=False)
    rec_ctx, rec_rc = a.ctx.export_streams(src), a.rc.export_streams(src)
    assert all(api.rate_state_check(r, 8000) == api.SS_OK for r in rec_rc), "the records are the existing ones"
    stay = [a.rc.process_g711(x[t])[0] for t in range(7, T)]
    a.close()
    b = Twin(model, 8000)
    assert [LAWS5[s] for s in src] != [b.rc.stream_laws()[d] for d in dst], "the records do not carry the law: the importer sets it"
    b.rc.set_stream_laws(dst, [LAWS5[s] for s in src])
    b.ctx.import_streams(dst, rec_ctx)
    b.rc.import_streams(dst, rec_rc)
    xb = np.full_like(x, gm.SILENCE[gm.ULAW])
    xb[:, dst] = x[:, src]
    for k, t in enumerate(range(7, T)):
        o, _ = b.rc.process_g711(xb[t])
        for s, d in zip(src, dst):
            assert np.array_equal(o[d], stay[k][s]), f"frame {t}: stream {s} continues in slot {d}"
    assert all(np.count_nonzero(np.stack([f[s] for f in stay]) != gm.SILENCE[LAWS5[s]]) > 0 for s in src)
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def run_cli(tmp_path, blob, opts, files):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    args = []
    for i, v in enumerate(files):
        v.tofile(tmp_path / f"in{i}.g711")
        args += [f"in{i}.g711", f"out{i}.g711"]
    run = subprocess.run([exe, "--model", "m.pnw"] + opts + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    return [np.fromfile(tmp_path / f"out{i}.g711", np.uint8) for i in range(len(files))]


def test_cli_single_rate_alaw(model, blob, tmp_path):
    frames = 9
    x = np.random.default_rng(9200).integers(0, 256, (2, frames * 80 + 37)).astype(np.uint8)     # a partial tail frame, which is dropped
    got = run_cli(tmp_path, blob, ["--rate", "8000", "--g711", "alaw", "--saturate"], [x[0], x[1]])
    ctx = api.Context(model, 2)
    ctx.set_output_saturate(True)
    rc = api.RateConverter(ctx, 8000)
    rc.set_stream_laws([0, 1], [gm.ALAW, gm.ALAW])
    want = rc.run_g711(x[:, :frames * 80])
    rc.close()
    ctx.close()
    for i in range(2):
        assert got[i].size == (frames - 1) * 80 and np.array_equal(got[i], want[i]), f"pair {i}"
    assert np.count_nonzero(want[:, 7 * 80:] != gm.SILENCE[gm.ALAW]) > 0


def test_cli_mixed_rates_ulaw_with_slot_takeover(model, blob, tmp_path):
    rates, frames = (8000, 48000, 16000), (5, 12, 6)              # two slots: the 16000 pair takes over the slot of the 8000 pair
    rng = np.random.default_rng(9300)
    x = [rng.integers(0, 256, f * nof(r) + 11 + i).astype(np.uint8) for i, (r, f) in enumerate(zip(rates, frames))]
    got = run_cli(tmp_path, blob, ["--rates", ",".join(map(str, rates)), "--g711", "ulaw", "--slots", "2"], x)

    def through_python(pair_rates, pairs):
        ctx = api.Context(model, 2)
        rc = api.MixedRateConverter(ctx, pair_rates)
        out = rc.run_g711(pairs)
        rc.close()
        ctx.close()
        return out

    # a stream's bytes depend on nothing but its own samples, so the pair that takes over a reset slot gives what it gives from
    # the start of a fresh two-slot context
    first = through_python(rates[:2], x[:2])
    third = through_python((rates[2], rates[1]), [x[2], x[1]])
    for i, want in enumerate((first[0], first[1], third[0])):
        assert got[i].size == (frames[i] - 1) * nof(rates[i]) and np.array_equal(got[i], want), f"pair {i} ({rates[i]} Hz)"
    assert np.count_nonzero(first[1][7 * 480:] != gm.SILENCE[gm.ULAW]) > 0
