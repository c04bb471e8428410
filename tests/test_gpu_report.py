"""Per-stream frame report and saturating int16 output on the GPU (-m gpu): include/percepnet_hip.h pn_ctx_set_report,
pn_ctx_set_output_saturate; kernel percepnet_amd/csrc/pn_outstage.hip.

The reference of every check is the engine as it stands: a plain context that never enables the feature.  Its float outputs,
g|r tap, silence flags and pitch periods say what a record must hold (tests/report_model.py), and its int16 output what wrap
mode must still give, bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, synth
from tests import families
from tests import report_model as rm

pytestmark = pytest.mark.gpu
MODES = {"strict": api.NN_STRICT, "mfma": api.NN_MFMA}
D = rm.DELAY_FRAMES


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


def fr(pcm, t):
    return np.ascontiguousarray(pcm[:, t * 480:(t + 1) * 480])


def delayed(pcm, t):
    """The input frame that output frame t is about (zeros before the seventh frame)."""
    return fr(pcm, t - D) if t >= D else np.zeros((pcm.shape[0], 480), np.int16)


def to_f32(x):
    return x.astype(np.float32) / np.float32(32768)


def periods(ctx):
    return ctx.debug_copy(13, ctx.n_streams).view(np.int32).copy()


def run_plain_f32(model, pcm, n_frames, nn_mode=api.NN_MFMA, limit_db=None):
    """The plain float context over pcm / 32768 -> o [T, B, 480], gr [T, B, 68], silence [T, B], period [T, B]."""
    B = pcm.shape[0]
    ctx = api.Context(model, B, nn_mode=nn_mode)
    if limit_db is not None:
        ctx.set_atten_limit(np.arange(B), limit_db)
    o, gr, sil, per = [], [], [], []
    for t in range(n_frames):
        a, g = ctx.process_f32(to_f32(fr(pcm, t)))
        o.append(a); gr.append(g); sil.append(ctx.read_features()[1]); per.append(periods(ctx))
    ctx.close()
    return np.stack(o), np.stack(gr), np.stack(sil), np.stack(per)


def run_i16(model, pcm, n_frames, nn_mode=api.NN_MFMA, limit_db=None, report=False, saturate=False):
    """An int16 context -> PCM [T, B, 480] (and the records [T, B] with report=True)."""
    B = pcm.shape[0]
    ctx = api.Context(model, B, nn_mode=nn_mode)
    if limit_db is not None:
        ctx.set_atten_limit(np.arange(B), limit_db)
    ctx.set_report(report)
    ctx.set_output_saturate(saturate)
    out, rep = [], []
    for t in range(n_frames):
        out.append(ctx.process_i16(fr(pcm, t), want_gr=False)[0])
        if report:
            rep.append(ctx.read_report())
    ctx.close()
    return (np.stack(out), np.stack(rep)) if report else np.stack(out)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
def test_parity_with_a_plain_context(model, mode):
    B, T = 13, 20
    pcm = synth.synth_batch(B, T)
    o, gr, sil, per = run_plain_f32(model, pcm, T, MODES[mode])
    plain = run_i16(model, pcm, T, MODES[mode])
    got, rep = run_i16(model, pcm, T, MODES[mode], report=True)
    assert np.array_equal(got, plain), "wrap mode through the stage must be the fused cast, bit for bit"
    assert {0, 1} <= set(sil.ravel().tolist()), "the batch must cover silent and non-silent frames"
    for t in range(T):
        rm.check_report(rep[t], o[t], gr[t], sil[t], per[t], delayed(pcm, t), f"{mode} frame {t}")
        if t < D:
            assert not rep[t]["in_peak"].any() and not rep[t]["in_energy"].any()
    # the float entry point: output untouched, the same records
    ctx = api.Context(model, B, nn_mode=MODES[mode])
    ctx.set_report(True)
    ctx.set_output_saturate(True)                            # float samples are never altered, also in saturate mode
    for t in range(T):
        a, g = ctx.process_f32(to_f32(fr(pcm, t)))
        assert np.array_equal(a.view(np.uint32), o[t].view(np.uint32)) and np.array_equal(g.view(np.uint32), gr[t].view(np.uint32)), t
        assert ctx.read_report().tobytes() == rep[t].tobytes(), t
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 2
SQUARE_PERIODS = {0: 48, 2: 40, 4: 96}                      # rows of +-32767 square waves; rows 1 and 3 are speech
B2, T2 = 5, 12


def square(period, n):
    return np.where(np.arange(n) % period < period // 2, 32767, -32767).astype(np.int16)


def clip_pcm():
    pcm = np.zeros((B2, T2 * 480), np.int16)
    pcm[1], pcm[3] = synth.synth_stream(1, T2), synth.synth_stream(5, T2)
    for r, p in SQUARE_PERIODS.items():
        pcm[r] = square(p, T2 * 480)
    return pcm


@pytest.fixture(scope="module")
def clip_case(model):
    """0 dB attenuation limit (the bypass: the input band-limited to 20 kHz): plain float outputs and a saturating context."""
    pcm = clip_pcm()
    o = run_plain_f32(model, pcm, T2, limit_db=0.0)[0]
    sat, rep = run_i16(model, pcm, T2, limit_db=0.0, report=True, saturate=True)
    return pcm, o, sat, rep


def test_saturation_and_clip_count(model, clip_case):
    pcm, o, sat, rep = clip_case
    n_out = rm.count_clipped(o)                              # [T, B], from the plain float context alone
    sq, speech = sorted(SQUARE_PERIODS), [1, 3]
    print("out-of-range samples per frame, square rows:", n_out[:, sq].T.tolist(), "peak", np.abs(o[:, sq]).max(axis=(0, 2)) * 32768)
    assert np.all(n_out[7:, sq] >= 1) and np.all(n_out[:, sq].sum(axis=0) >= 100), "precondition: every square row leaves the int16 range"
    assert np.array_equal(sat, rm.cast(o, True)), "saturate mode: clip(trunc(o * 32768))"
    assert np.array_equal(rep["out_clipped"], n_out)
    assert not n_out[:, speech].any()
    wrap, wrep = run_i16(model, pcm, T2, limit_db=0.0, report=True)
    plain = run_i16(model, pcm, T2, limit_db=0.0)
    assert np.array_equal(wrap, plain), "wrap mode with the report on is the plain int16 context"
    assert np.array_equal(wrap, rm.cast(o, False))
    assert wrep.tobytes() == rep.tobytes(), "the records do not depend on the cast"
    assert np.array_equal(sat[:, speech], wrap[:, speech]), "rows in range are cast as before"
    assert not np.array_equal(sat[:, sq], wrap[:, sq])
    # saturation alone (no report): the same PCM
    assert np.array_equal(run_i16(model, pcm, T2, limit_db=0.0, saturate=True), sat)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_slot_and_batch_independence(model):
    T = 10
    x = synth.synth_stream(4, T)
    rows = []
    for B, slot in ((1, 0), (13, 12), (70, 69)):
        pcm = synth.synth_batch(B, T, first_stream=20)
        pcm[slot] = x
        rows.append(run_i16(model, pcm, T, report=True)[1][:, slot])
    assert rows[0]["out_energy"][D + 1:].all() and rows[0]["in_energy"][D:].all()
    assert rows[0].tobytes() == rows[1].tobytes() == rows[2].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_lifecycle(model):
    B, T, k = 13, 16, 5
    pcm = synth.synth_batch(B, T)
    plain = run_i16(model, pcm, T)
    ctx = api.Context(model, B)
    with pytest.raises(api.PercepNetError):
        ctx.read_report()                                    # off by default
    with pytest.raises(api.PercepNetError):
        ctx.submit_host_i16(0, 0, None, h_report=np.zeros(8 * B, np.uint32).ctypes.data)
    ctx.set_profiling(True)
    for t in range(T):
        if t == k:                                           # enabled mid-run: from the next frame on
            assert ctx.kernel_times()["backend"][1] == k     # one launch per frame while off
            ctx.set_report(True)
            ctx.reset_profile()
        if t == 9:
            ctx.reset_streams([3])                           # the setting survives; the slot's history is zero again
        out = ctx.process_i16(fr(pcm, t), want_gr=False)[0]
        if t == 9:
            fresh = api.Context(model, 1)
            want3 = [fresh.process_i16(fr(pcm, u)[3:4], want_gr=False)[0][0] for u in range(9, T)]
            fresh.close()
        if t < 9:
            assert np.array_equal(out, plain[t]), t
        else:
            keep = np.arange(B) != 3
            assert np.array_equal(out[keep], plain[t][keep]) and np.array_equal(out[3], want3[t - 9]), t
        if t >= k:
            want = np.abs(to_f32(delayed(pcm, t))).max(axis=1)
            if 9 <= t < 9 + D:
                want[3] = 0                                  # six frames of the zeros the reset left
            rep = ctx.read_report()
            assert t < D or (want[np.arange(B) != 3].all() and (t < 9 + D or want[3] > 0))
            assert np.array_equal(rep["in_peak"], want) and np.array_equal(rep["in_energy"] == 0, want == 0), t
    assert ctx.kernel_times()["backend"][1] == 2 * (T - k)   # two launches per frame while on
    ctx.set_report(False)
    ctx.reset_profile()
    ctx.process_i16(fr(pcm, 0), want_gr=False)
    assert ctx.kernel_times()["backend"][1] == 1
    with pytest.raises(api.PercepNetError):
        ctx.read_report()
    ctx.set_report(True)
    ctx.reset()                                              # a context reset leaves the setting on
    ctx.process_i16(fr(pcm, 0), want_gr=False)
    assert not ctx.read_report()["in_peak"].any()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_active_set(model):
    import torch
    dev = torch.device("cuda:0")
    B, T = 13, 17
    skipped, skip_at = [2, 7], (8, 9)
    pcm = synth.synth_batch(B, T)
    active = lambda t: [s for s in range(B) if not (s in skipped and t in skip_at)]
    # the frames each stream has received up to and including tick t
    received = {s: [] for s in range(B)}
    ref = api.Context(model, B)
    ctx = api.Context(model, B)
    ctx.set_report(True)
    r_in = torch.zeros((B, 480), dtype=torch.float32, device=dev)
    r_out = torch.zeros((B, 480), dtype=torch.float32, device=dev)
    r_gr = torch.zeros((B, 68), dtype=torch.float32, device=dev)
    d_in = torch.zeros((B, 480), dtype=torch.int16, device=dev)
    d_out = torch.full((B, 480), 12345, dtype=torch.int16, device=dev)
    for t in range(T):
        ids = active(t)
        for s in ids:
            received[s].append(t)
        r_in.copy_(torch.from_numpy(to_f32(fr(pcm, t)))); d_in.copy_(torch.from_numpy(fr(pcm, t)))
        torch.cuda.synchronize()
        before = d_out.cpu().numpy().copy()
        ref.process_f32_active_dev(r_in.data_ptr(), r_out.data_ptr(), r_gr.data_ptr(), ids)
        ctx.process_i16_active_dev(d_in.data_ptr(), d_out.data_ptr(), None, ids)
        sil, per = ref.read_features()[1], periods(ref)
        rep = ctx.read_report()
        o, gr, out = r_out.cpu().numpy(), r_gr.cpu().numpy(), d_out.cpu().numpy()
        x = np.zeros((B, 480), np.int16)
        for s in ids:
            if len(received[s]) > D:
                x[s] = fr(pcm, received[s][-1 - D])[s]
        if t == 12:                                          # six received frames back crosses the two skipped ticks
            assert received[2][-1 - D] == 4 and not np.array_equal(x[2], delayed(pcm, t)[2])
        rm.check_report(rep[ids], o[ids], gr[ids], sil[ids], per[ids], x[ids], f"tick {t}")
        assert np.array_equal(out[ids], rm.cast(o[ids], False)), t
        idle = [s for s in range(B) if s not in ids]
        assert np.array_equal(out[idle], before[idle]), f"tick {t}: the rows of skipped streams must stay untouched"
    ref.close(); ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_pipelined_host_path_delivers_each_frames_report(model):
    B, T = 13, 10
    pcm = synth.synth_batch(B, T)
    want_out, want_rep = run_i16(model, pcm, T, report=True)
    ctx = api.Context(model, B)
    ctx.set_report(True)
    ins = [fr(pcm, t) for t in range(T)]
    outs = [np.zeros((B, 480), np.int16) for _ in range(T)]
    reps = [np.zeros(B, api.REPORT_DTYPE) for _ in range(T)]
    for t in range(T):
        if t == 4:                                           # one-shot: a frame submitted without a request delivers none
            ctx.submit_host_i16(ins[t].ctypes.data, outs[t].ctypes.data)
        else:
            ctx.submit_host_i16(ins[t].ctypes.data, outs[t].ctypes.data, h_report=reps[t].ctypes.data)
    ctx.host_wait()
    for t in range(T):
        assert np.array_equal(outs[t], want_out[t]), t
        assert reps[t].tobytes() == (want_rep[t].tobytes() if t != 4 else bytes(32 * B)), t
    assert ctx.read_report().tobytes() == want_rep[T - 1].tobytes()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_cli_saturate_and_report(model, blob, clip_case, tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    pcm, o, sat, rep = clip_case
    pcm[0].tofile(tmp_path / "sq.pcm")
    (tmp_path / "m.pnw").write_bytes(blob)
    r = subprocess.run([exe, "--model", "m.pnw", "--atten-lim", "0", "--saturate", "--report", "sq.pcm", "sq.out"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "sq.out").read_bytes() == sat[1:, 0].tobytes()        # minus the first frame (main.cpp:37)
    m = re.search(r"sq\.out: frames (\d+) clipped (\d+) peak ([0-9.]+) level (-?[0-9.]+) dB", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == T2 - 1 and int(m.group(2)) == int(rep["out_clipped"][1:, 0].sum())
    assert abs(float(m.group(3)) - float(rep["out_peak"][1:, 0].max())) < 1e-6
    level = 10 * np.log10(rep["out_energy"][1:, 0].astype(np.float64).sum() / rep["in_energy"][1:, 0].astype(np.float64).sum())
    assert abs(float(m.group(4)) - level) < 0.006
    wrap = subprocess.run([exe, "--model", "m.pnw", "--atten-lim", "0", "sq.pcm", "wrap.out"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert wrap.returncode == 0 and wrap.stdout == "" and (tmp_path / "wrap.out").read_bytes() == rm.cast(o[1:, 0], False).tobytes()
