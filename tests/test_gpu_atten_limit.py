"""Per-stream attenuation limit on the GPU (-m gpu): include/percepnet_hip.h pn_ctx_set_atten_limit.

The back end is bit-exact for a given g|r, so the engine's PCM is checked bit for bit against the numpy back-end model
(tests/backend_model.py, pinned to the CPU oracle by tests/test_atten_limit_host.py) fed the oracle's X / P / silence and
the GPU's own g|r tap, in every network mode.  Rows without a limit must not change at all, the 0 dB bypass must be the
delayed input, and the limit must follow the documented ordering and lifecycle rules."""
import math
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, synth
from tests import backend_model as bm
from tests import families

pytestmark = pytest.mark.gpu
MODES = {"strict": api.NN_STRICT, "mfma": api.NN_MFMA, "x3": api.NN_MFMA_X3, "f16": api.NN_MFMA_F16}
LIMITS = [math.inf, 0.0, 1.5, 6.0, 12.0, 24.0, 60.0, 1000.0]
DELAY = 2880          # output frame t vs input frame t; 2400 between the CLI's input and output files


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def backend(oracle):
    return bm.BackendModel(oracle)


def fr(pcm, t):
    return np.ascontiguousarray(pcm[:, t * 480:(t + 1) * 480])


def rotated_pool(n_streams, n_frames):
    """n_streams distinct rows: pool stream r % 256, rotated by a per-row amount."""
    pool = synth.synth_batch(256, n_frames)
    n = n_frames * 480
    shift = (np.arange(n_streams) // 256) * 997
    idx = (np.arange(n)[None, :] + shift[:, None]) % n
    return pool[np.arange(n_streams) % 256][np.arange(n_streams)[:, None], idx]


# ---------------------------------------------------------------------------------------------------------------- 3
B3, T3 = 64, 40
# frame -> {stream: dB} set before that frame; stream 5: off -> 12 dB -> off.  The loud streams 3, 23, 43, 63 change on
# frames the oracle calls non-silent (3: 6..18, 23: 6..11, 43: 26..39, 63: 8..38), the others on silent ones
SCHEDULE = {0: {s: LIMITS[s % 8] for s in range(B3)},
            8: {5: 12.0, 3: 0.0, 10: 60.0},
            10: {23: 1.5},
            14: {11: math.inf, 12: 0.0, 3: 6.0},
            21: {7: 1000.0, 63: 24.0},
            27: {5: math.inf, 17: 12.0, 43: 24.0, 23: math.inf}}


@pytest.fixture(scope="module")
def sched_inputs(oracle):
    pcm = synth.synth_batch(B3, T3)
    stages = [oracle.stages(pcm[s].astype(np.float32) / np.float32(32768)) for s in range(B3)]
    lam = np.zeros((B3, T3), np.float32)
    cur = np.zeros(B3, np.float32)
    for t in range(T3):
        for s, db in SCHEDULE.get(t, {}).items():
            cur[s] = bm.factor(db)[0]
        lam[:, t] = cur
    return pcm, stages, lam


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
def test_exact_against_the_model(model, oracle, backend, sched_inputs, mode):
    pcm, stages, lam = sched_inputs
    sil = np.stack([st["silence"] for st in stages])
    changed = [(s, t) for t in SCHEDULE if t > 0 for s in SCHEDULE[t]]
    assert {int(sil[s, t]) for s, t in changed} == {0, 1}, "the schedule must change limits on silent and non-silent frames"
    ctx = api.Context(model, B3, nn_mode=MODES[mode])
    out = np.zeros((B3, T3, 480), np.int16)
    gr = np.zeros((B3, T3, 68), np.float32)
    for t in range(T3):
        if t in SCHEDULE:
            ids = list(SCHEDULE[t])
            ctx.set_atten_limit(ids, [SCHEDULE[t][s] for s in ids])
        out[:, t], gr[:, t] = ctx.process_i16(fr(pcm, t))
    final = ctx.atten_limit()
    ctx.close()
    want = {s: LIMITS[s % 8] for s in range(B3)}
    for t in sorted(SCHEDULE):
        want.update(SCHEDULE[t])
    assert np.array_equal(final, np.array([want[s] for s in range(B3)], np.float32))
    for s in range(B3):
        st = stages[s]
        ref = bm.f2s(backend.run(st["X"], st["P"], st["silence"], gr[s], lam[s]) * np.float32(32768))
        bad = np.flatnonzero((ref != out[s]).any(axis=1))
        assert bad.size == 0, f"{mode}: stream {s} differs from the model first at frame {bad[:1]}, lam {lam[s, bad[:1]]}"
    if mode == "strict":
        _, ogr, _, _ = oracle.run_batch(pcm, want_feat=False)
        assert np.array_equal(gr.view(np.uint32), ogr.view(np.uint32)), "the g|r tap must not depend on the limit"


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n_streams", [1024, 32768])
def test_unlimited_rows_are_untouched(model, n_streams):
    T = 6
    pcm = rotated_pool(n_streams, T)
    lim = np.arange(0, n_streams, 3)
    plain, limited = api.Context(model, n_streams), api.Context(model, n_streams)
    limited.set_atten_limit(lim, np.array(LIMITS, np.float32)[np.arange(lim.size) % 7 + 1])    # finite values, 0 dB included
    other = np.setdiff1d(np.arange(n_streams), lim)
    diff = 0
    for t in range(T):
        f = fr(pcm, t)
        (a, ga), (b, gb) = plain.process_i16(f), limited.process_i16(f)
        bad = other[(a[other] != b[other]).any(axis=1)]
        assert bad.size == 0, f"{n_streams} streams, frame {t}: unlimited rows {bad[:8]} changed"
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), "g|r depends on the limit"
        diff += int((a[lim] != b[lim]).any(axis=1).sum())
    assert diff > 0, "no limited row changed: the variant did not run"
    plain.close(); limited.close()


def test_set_then_cleared_is_the_plain_engine(model):
    B, T = 1024, 5
    pcm = rotated_pool(B, T)
    plain, cleared = api.Context(model, B), api.Context(model, B)
    cleared.set_atten_limit(np.arange(B), 6.0)
    cleared.set_atten_limit(np.arange(0, B, 2), math.inf)
    cleared.set_atten_limit(np.arange(1, B, 2), [math.inf] * (B // 2))
    assert np.all(np.isinf(cleared.atten_limit()))
    for t in range(T):
        (a, ga), (b, gb) = plain.process_i16(fr(pcm, t)), cleared.process_i16(fr(pcm, t))
        assert np.array_equal(a, b) and np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), t
    plain.close(); cleared.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def bandlimited(n_streams, n_frames, seed=3):
    """Sum of sinusoids plus noise band-limited to 1..18 kHz: nothing near the 20 kHz edge of the kept bins."""
    rng = np.random.default_rng(seed)
    n = n_frames * 480
    tt = np.arange(n) / 48000
    out = np.zeros((n_streams, n))
    for s in range(n_streams):
        x = sum(rng.uniform(0.02, 0.12) * np.sin(2 * np.pi * f * tt + rng.uniform(0, 6)) for f in rng.uniform(80, 17000, 5))
        spec = np.fft.rfft(rng.standard_normal(n))
        fq = np.fft.rfftfreq(n, 1 / 48000)
        spec[(fq < 1000) | (fq > 18000)] = 0
        out[s] = x + 0.05 * np.fft.irfft(spec, n) / np.std(np.fft.irfft(spec, n))
    return out


def test_bypass_is_the_delayed_input(model, backend, oracle):
    B, T = 8, 30
    x = bandlimited(B, T)
    pcm = np.clip(np.round(x * 32767 * 0.8), -32768, 32767).astype(np.int16)
    outs = {}
    for pf in (0, 1):
        ctx = api.Context(model, B)
        ctx.set_postfilter(pf)
        ctx.set_atten_limit(np.arange(B), 0.0)
        outs[pf] = np.stack([ctx.process_i16(fr(pcm, t))[0] for t in range(T)], axis=1).reshape(B, -1)
        ctx.close()
    assert np.array_equal(outs[0], outs[1]), "at 0 dB the output cannot depend on the gains (post-filter on / off)"
    y = outs[0].astype(np.float64)
    xin = pcm.astype(np.float64)
    for s in range(B):
        err = y[s, DELAY + 960:] - xin[s, 960:xin.shape[1] - DELAY]
        sig = np.sqrt(np.mean(xin[s] ** 2))
        assert 20 * np.log10(np.sqrt(np.mean(err ** 2)) / sig) < -40, s
    # the fp32-output variant against the model, bit for bit (the model's 1/32768 convention is the f32 API's)
    xf = (pcm.astype(np.float32) / np.float32(32768))
    ctx = api.Context(model, B)
    ctx.set_atten_limit(np.arange(B), [0.0, 3.0, 6.0, 12.0, 24.0, 60.0, 1000.0, math.inf])
    got, gr = zip(*[ctx.process_f32(fr(xf, t)) for t in range(T)])
    ctx.close()
    got, gr = np.stack(got, axis=1), np.stack(gr, axis=1)
    for s, db in enumerate([0.0, 3.0, 6.0, 12.0, 24.0, 60.0, 1000.0, math.inf]):
        st = oracle.stages(xf[s])
        ref = backend.run(st["X"], st["P"], st["silence"], gr[s], bm.factor(db)[0])
        assert np.array_equal(ref.view(np.uint32), got[s].view(np.uint32)), (s, db)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_reset_streams_clears_the_limit(model):
    B, T = 16, 12
    pcm = synth.synth_batch(B, T)
    a, b = api.Context(model, B), api.Context(model, B)
    a.set_atten_limit([0, 1, 2, 3], [6.0, 12.0, 0.0, 24.0])
    for t in range(T):
        if t == 5:
            a.reset_streams([1, 2, 1]); b.reset_streams([1, 2, 1])
            assert np.array_equal(a.atten_limit()[:4], np.array([6.0, math.inf, math.inf, 24.0], np.float32))
        oa, _ = a.process_i16(fr(pcm, t)); ob, _ = b.process_i16(fr(pcm, t))
        if t >= 5:
            assert np.array_equal(oa[1:3], ob[1:3]), t        # fresh, unlimited streams
            assert np.array_equal(oa[4:], ob[4:]), t
    assert not np.array_equal(oa[[0, 3]], ob[[0, 3]])
    a.set_atten_limit([0], 1.5)
    a.reset()
    assert np.all(np.isinf(a.atten_limit()))
    a.close(); b.close()


def test_skipped_ticks_keep_the_limit(model):
    import torch
    dev = torch.device("cuda:0")
    B, T, r = 16, 14, 5
    skips = {3, 4, 9}
    pcm = synth.synth_batch(B, T)
    ctx = api.Context(model, B)
    ctx.set_atten_limit([r, 6], [12.0, 6.0])
    d_out = torch.zeros((B, 480), dtype=torch.int16, device=dev)
    d_gr = torch.zeros((B, 68), dtype=torch.float32, device=dev)
    got = []
    for t in range(T):
        d_in = torch.from_numpy(fr(pcm, t)).to(dev)
        torch.cuda.synchronize()
        active = [s for s in range(B) if not (s == r and t in skips)]
        ctx.process_i16_active_dev(d_in.data_ptr(), d_out.data_ptr(), d_gr.data_ptr(), active)
        ctx.synchronize()
        if t not in skips:
            got.append(d_out[r].cpu().numpy().copy())
    ctx.close()
    # the same stream fed only the frames it received
    solo = api.Context(model, 1)
    solo.set_atten_limit([0], 12.0)
    frames = [t for t in range(T) if t not in skips]
    want = [solo.process_i16(pcm[r:r + 1, t * 480:(t + 1) * 480])[0][0] for t in frames]
    solo.close()
    assert np.array_equal(np.stack(got), np.stack(want))


def test_pipelined_host_path_orders_the_set(model):
    B, T, k = 32, 10, 4
    pcm = synth.synth_batch(B, T)
    ids, dbs = [1, 4, 9, 30], [0.0, 6.0, 12.0, 1000.0]
    dev = api.Context(model, B)
    want = []
    for t in range(T):
        if t == k + 1:
            dev.set_atten_limit(ids, dbs)
        want.append(dev.process_i16(fr(pcm, t))[0])
    dev.close()
    pipe = api.Context(model, B)
    ins = [fr(pcm, t) for t in range(T)]
    outs = [np.zeros((B, 480), np.int16) for _ in range(T)]
    for t in range(T):
        pipe.submit_host_i16(ins[t].ctypes.data, outs[t].ctypes.data)
        if t == k:                                            # between the submits of frames k and k + 1
            pipe.set_atten_limit(ids, dbs)
    pipe.host_wait()
    pipe.close()
    for t in range(T):
        assert np.array_equal(outs[t], want[t]), t


def test_export_import_under_the_target_setting(model):
    B, T0, T1 = 16, 9, 8
    pcm = synth.synth_batch(B, T0 + T1)
    pcm_b = synth.synth_batch(B, 5, first_stream=100)
    a, a_off = api.Context(model, B), api.Context(model, B)
    for c in (a, a_off):
        c.set_atten_limit([2], 6.0)
        for t in range(T0):
            c.process_i16(fr(pcm, t))
    a_off.set_atten_limit([2], math.inf)                      # same state as a, limit off from here on
    rec = a.export_streams([2])
    assert rec.shape == (1, api.STREAM_STATE_BYTES) and api.STREAM_STATE_BYTES == 54688
    assert np.array_equal(rec, a_off.export_streams([2])), "a record must not carry the limit"
    tgt = api.Context(model, B)
    tgt.set_atten_limit([7, 9], [6.0, math.inf])
    for t in range(5):
        tgt.process_i16(fr(pcm_b, t))
    tgt.import_streams([7, 9], np.concatenate([rec, rec]))
    assert tgt.atten_limit()[7] == 6.0 and np.isinf(tgt.atten_limit()[9])
    for t in range(T0, T0 + T1):
        f = fr(pcm, t)
        g = np.ascontiguousarray(fr(pcm_b, 0))
        g[7] = g[9] = f[2]
        ot, _ = tgt.process_i16(g)
        oa, _ = a.process_i16(f)
        oo, _ = a_off.process_i16(f)
        assert np.array_equal(ot[7], oa[2]), t                # limited -> limited: continues bit for bit
        assert np.array_equal(ot[9], oo[2]), t                # imported into a slot that is off: unlimited
    for c in (a, a_off, tgt):
        c.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals_change_nothing(model):
    ctx = api.Context(model, 16)
    ctx.set_atten_limit([0, 1], [6.0, 12.0])
    before = ctx.atten_limit()
    for ids, db in (([16], [3.0]), ([-1], [3.0]), ([3, 3], [3.0, 4.0]), ([4], [-1.0]), ([4, 5], [2.0, math.nan]),
                    ([0, 1], [-0.5, 3.0])):
        with pytest.raises(api.PercepNetError):
            ctx.set_atten_limit(ids, db)
        assert np.array_equal(ctx.atten_limit(), before), (ids, db)
    ctx.set_atten_limit([], [])
    assert np.array_equal(ctx.atten_limit(), before)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_cli_atten_lim_with_slot_reuse(model, blob, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    a, b = synth.synth_stream(3, 14), synth.synth_stream(8, 11)
    a.tofile(tmp_path / "a.pcm"); b.tofile(tmp_path / "b.pcm")
    (tmp_path / "m.pnw").write_bytes(blob)
    r = subprocess.run([exe, "--model", "m.pnw", "--atten-lim", "6", "--slots", "1", "a.pcm", "a.out", "b.pcm", "b.out"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for name, x in (("a", a), ("b", b)):
        ctx = api.Context(model, 1)
        ctx.set_atten_limit([0], 6.0)
        want, _ = ctx.run_pcm(x[None])
        ctx.close()
        assert (tmp_path / f"{name}.out").read_bytes() == want[0].tobytes(), name
    plain = subprocess.run([exe, "--model", "m.pnw", "a.pcm", "p.out"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and (tmp_path / "p.out").read_bytes() != (tmp_path / "a.out").read_bytes()
    bad = subprocess.run([exe, "--model", "m.pnw", "--atten-lim", "-3", "a.pcm", "q.out"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0
