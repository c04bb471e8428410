"""GPU tests (-m gpu) of the batched training-feature generator at its decision edges: pn_featgen_*, pn_targets_kernel,
pn_saturate_i16_kernel and the percepnet_featgen file driver on the pairs of tests/featgen_cases.py, against the CPU oracle's
train_run (pinned to the compiled reference's train() on synth pairs by tests/test_oracle.py and on these pairs by
tests/test_featgen_cases_host.py).

The comparison (_check): fields 0:70 and 104:138 of the 138-float record bit for bit; the 34 ideal gains within
featgen_cases.gains_match (G_RTOL relative, the existing suite's, plus four half units of the smallest subnormal — derived there,
not measured — and zero exactly where the oracle is zero); test_output.pcm within +-1 LSB, and wherever the oracle sits on an
int16 rail the GPU sits on the same rail or one LSB inside it.
"""
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, synth
from tests import featgen_cases as fc

pytestmark = pytest.mark.gpu

G_RTOL = 2e-6                    # tests/test_gpu_featgen.py
PCM_TOL_LSB = 1
T = fc.T
R99 = np.float32(0.99)
EXACT = np.r_[0:70, 104:138]     # Ey_lookahead, Ephaty, T, pitch_corr | r


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(rec, pcm, orec, opcm, what=None):
    bad = np.argwhere(_bits(rec[..., EXACT]) != _bits(orec[..., EXACT]))
    assert bad.size == 0, (what, len(bad), bad[:4])
    g, og = rec[..., 70:104], orec[..., 70:104]
    ok = fc.gains_match(g, og, G_RTOL)
    assert ok.all(), (what, int((~ok).sum()), g[~ok][:4], og[~ok][:4])
    if pcm is not None:
        p, o = pcm.astype(np.int32), opcm.astype(np.int32)
        assert np.abs(p - o).max() <= PCM_TOL_LSB, (what, int(np.abs(p - o).max()))
        assert (p[o == 32767] >= 32766).all() and (p[o == -32768] <= -32767).all(), what


@pytest.fixture(scope="module")
def want(oracle):
    """The oracle's (records, PCM) of every case and of every filler pair of the batches, computed once."""
    C = fc.cases()
    case = {name: oracle.train_run(*C[name]) for name in C}
    fill = {p: oracle.train_run(*synth.synth_pair(p, T)) for p in sorted(fc.filler_pairs(0).values())}
    return case, fill


def _want_batch(want, order):
    case, fill = want
    rec = np.empty((fc.B, T, 138), np.float32); pcm = np.empty((fc.B, T, 480), np.int16)
    for name, r in fc.case_rows(order).items():
        rec[r], pcm[r] = case[name]
    for r, p in fc.filler_pairs(order).items():
        rec[r], pcm[r] = fill[p]
    return rec, pcm


@pytest.fixture(scope="module")
def gpu_batch():
    """run(order) -> (records [131, T, 138], PCM [131, T, 480]) of batch(order) through FeatGen(131).run(), each order once."""
    done = {}

    def run(order):
        if order not in done:
            sp, no, _ = fc.batch(order)
            fg = api.FeatGen(fc.B)
            try:
                done[order] = fg.run(sp, no)
            finally:
                fg.close()
        return done[order]
    return run


def _conditions(rows, rec, pcm):
    """The conditions of tests/test_featgen_cases_host.py that read outputs, on the GPU's own: the edges were exercised here."""
    g = lambda name: rec[rows[name], :, 70:104]
    r = lambda name: rec[rows[name], :, 104:138]
    for name in ("identical_loud", "square_both", "fullnoise_both"):
        p = pcm[rows[name]]
        assert (p == 32767).sum() >= 50 and (p == -32768).sum() >= 50, (name, int((p == 32767).sum()), int((p == -32768).sum()))
    for name in ("noisy_zero", "dither1/zero", "square/loud"):
        assert (r(name) == R99).mean() >= 0.5, (name, float((r(name) == R99).mean()))
    for name in ("identical", "neg", "quarter", "speech_zero"):
        assert not (r(name) == R99).any(), name
    for name in ("identical", "neg", "quarter"):
        assert (g(name) >= 0.999).mean() >= 0.7, (name, float((g(name) >= 0.999).mean()))
    for name in ("speech_zero", "noisy_zero", "zero/dither1"):
        assert (g(name) == 0).all(), name
    for name in ("dc-1/dc+1", "alt/step", "dither4/voiced", "impulse/dc1"):
        v = g(name)
        assert v[v != 0].min() < 1e-9, (name, float(v[v != 0].min()))
    assert np.isfinite(rec).all()


@pytest.mark.parametrize("order", (0, 1))
def test_cases_against_the_oracle(order, want, gpu_batch):
    """FeatGen(131).run() on batch(order): every row against train_run of its own pair; every case bit-identical between the two
    arrangements (placement and neighbours do not matter); the non-vacuity conditions hold on the GPU's own outputs."""
    rec, pcm = gpu_batch(order)
    orec, opcm = _want_batch(want, order)
    rows = fc.case_rows(order)
    at = {r: name for name, r in rows.items()}
    for r in range(fc.B):
        _check(rec[r], pcm[r], orec[r], opcm[r], (order, r, at.get(r)))
    _conditions(rows, rec, pcm)
    rec2, pcm2 = gpu_batch(1 - order)
    rows2 = fc.case_rows(1 - order)
    for name in rows:
        assert np.array_equal(_bits(rec[rows[name]]), _bits(rec2[rows2[name]])), name
        assert np.array_equal(pcm[rows[name]], pcm2[rows2[name]]), name


def test_cases_in_every_front_end_family(want, gpu_batch):
    """PERCEPNET_FE=split|mono|g2 around creation only, batch(0): split against the oracle, mono and g2 against split bit for bit,
    records and PCM."""
    sp, no, _ = fc.batch(0)
    res = {}
    for fam in ("split", "mono", "g2"):
        os.environ["PERCEPNET_FE"] = fam
        try:
            fg = api.FeatGen(fc.B)
        finally:
            del os.environ["PERCEPNET_FE"]
        try:
            res[fam] = fg.run(sp, no)
        finally:
            fg.close()
    orec, opcm = _want_batch(want, 0)
    _check(res["split"][0], res["split"][1], orec, opcm, "split")
    for fam in ("mono", "g2"):
        assert np.array_equal(_bits(res[fam][0]), _bits(res["split"][0])), fam
        assert np.array_equal(res[fam][1], res["split"][1]), fam


def _case_batch():
    """The cases alone, in table order: 26 pairs, ragged for every group size (16, 4, 64)."""
    C = fc.cases()
    names = list(C)
    assert len(names) % 4 and len(names) % 16
    return names, np.stack([C[n][0] for n in names]), np.stack([C[n][1] for n in names])


def _frame_major(x):
    """[B, T * 480] -> contiguous [T][B][480]"""
    return np.ascontiguousarray(x.reshape(x.shape[0], -1, 480).transpose(1, 0, 2))


def test_frame_api_with_and_without_the_test_pcm(gpu_batch):
    """pn_featgen_process_i16 frame by frame on device tensors, d_test_pcm on even frames and NULL on odd ones: the records are
    those of the batch run bit for bit, and so is the PCM of the even frames — the synthesis memory advanced on the frames that
    dropped their PCM (pn_featgen.cpp, fg_frame).  The PCM buffers of the odd frames are not written."""
    import torch
    names, sp, no = _case_batch()
    B = len(names)
    rec0, pcm0 = gpu_batch(0)
    rows = fc.case_rows(0)
    fg = api.FeatGen(B)
    try:
        d_sp, d_no = torch.from_numpy(_frame_major(sp)).cuda(), torch.from_numpy(_frame_major(no)).cuda()
        rec = torch.empty((T, B, 138), dtype=torch.float32, device="cuda")
        pcm = torch.full((T, B, 480), 12345, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()                              # inputs resident before the generator's stream reads them
        for t in range(T):
            fg.process_dev(d_sp[t].data_ptr(), d_no[t].data_ptr(), rec[t].data_ptr(), pcm[t].data_ptr() if t % 2 == 0 else None)
        fg.synchronize(); torch.cuda.synchronize()
    finally:
        fg.close()
    rec, pcm = rec.cpu().numpy().transpose(1, 0, 2), pcm.cpu().numpy().transpose(1, 0, 2)
    for i, name in enumerate(names):
        assert np.array_equal(_bits(rec[i]), _bits(rec0[rows[name]])), name
        assert np.array_equal(pcm[i, 0::2], pcm0[rows[name], 0::2]), name
    assert (pcm[:, 1::2] == 12345).all()


def test_on_a_callers_stream(gpu_batch):
    """A generator on a caller's HIP stream: pn_featgen_process_i16_files on device tensors issued on that stream equals, bit for
    bit, a generator with its own stream (and the batch run).  reset() in the middle of a run, then the same frames again: the
    first frames' records and PCM again."""
    import torch
    names, sp, no = _case_batch()
    B, H = len(names), T // 2
    rec0, pcm0 = gpu_batch(0)
    rows = fc.case_rows(0)

    def run(stream):
        ts = stream or torch.cuda.current_stream()
        with torch.cuda.stream(ts):
            fg = api.FeatGen(B, stream=stream.cuda_stream if stream else None)
            try:
                d_sp, d_no = torch.from_numpy(sp).cuda(), torch.from_numpy(no).cuda()
                d_sp_h, d_no_h = d_sp[:, :H * 480].contiguous(), d_no[:, :H * 480].contiguous()
                rec = torch.empty((B, T, 138), dtype=torch.float32, device="cuda")
                pcm = torch.empty((B, T, 480), dtype=torch.int16, device="cuda")
                half = [(torch.empty((B, H, 138), dtype=torch.float32, device="cuda"), torch.empty((B, H, 480), dtype=torch.int16, device="cuda"))
                        for _ in range(2)]
                if not stream:                                # an own-stream generator does not wait for the caller's copies;
                    ts.synchronize()                          # one on the caller's stream is ordered behind them
                fg.process_files_dev(d_sp.data_ptr(), d_no.data_ptr(), T, rec.data_ptr(), pcm.data_ptr())
                fg.reset()
                fg.process_files_dev(d_sp_h.data_ptr(), d_no_h.data_ptr(), H, half[0][0].data_ptr(), half[0][1].data_ptr())
                fg.reset()                                    # in the middle of a run
                fg.process_files_dev(d_sp_h.data_ptr(), d_no_h.data_ptr(), H, half[1][0].data_ptr(), half[1][1].data_ptr())
                if stream:
                    stream.synchronize()                      # the work was issued on the caller's stream: it alone is waited for
                else:
                    fg.synchronize()
                return [x.cpu().numpy() for x in (rec, pcm, half[0][0], half[0][1], half[1][0], half[1][1])]
            finally:
                fg.close()

    mine = run(torch.cuda.Stream())
    own = run(None)
    for a, b in zip(mine, own):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    rec, pcm, ra, pa, rb, pb = mine
    for i, name in enumerate(names):
        assert np.array_equal(_bits(rec[i]), _bits(rec0[rows[name]])), name
        assert np.array_equal(pcm[i], pcm0[rows[name]]), name
    for r, p in ((ra, pa), (rb, pb)):
        assert np.array_equal(_bits(r), _bits(rec[:, :H])) and np.array_equal(p, pcm[:, :H])


def test_file_driver_across_its_chunk_edge(oracle, tmp_path):
    """percepnet_featgen --test-pcm, four jobs of 1030, 1025, 1024 and 0 frames from files of 7 and 5 whole frames (coprime) plus
    a partial tail that is never used: pn_featgen_run_files cycles them with (f0 + f) % n across its 1024-frame chunk edge and
    keeps counts[j] - f0 frames of the second chunk (6, 1, 0, 0).  Against train_run on the cycled arrays; the count-0 job leaves
    empty files; the inputs are loud enough for the long run to cross both rails."""
    C = fc.cases()
    A = 3                                                     # first frame taken from each case
    jobs = [("identical_loud", 7, 5, 1030), ("loud/square", 5, 7, 1025), ("peak1+dither1", 7, 5, 1024), ("square_both", 5, 7, 0)]
    tail = np.arange(100, dtype=np.int16)
    args, expect = [os.path.join(os.path.dirname(api.LIB_PATH), "percepnet_featgen"), "--test-pcm"], []
    for j, (name, ns, nn, count) in enumerate(jobs):
        s, n = C[name][0][A * 480:(A + ns) * 480], C[name][1][A * 480:(A + nn) * 480]
        a, b, o = tmp_path / f"s{j}.pcm", tmp_path / f"n{j}.pcm", tmp_path / f"o{j}.f32"
        np.concatenate([s, tail]).tofile(a); np.concatenate([n, tail]).tofile(b)
        args += [str(a), str(b), str(count), str(o)]
        cyc = lambda x, k: x.reshape(k, 480)[np.arange(count) % k].reshape(-1)
        expect.append((o, count, cyc(s, ns), cyc(n, nn)))
    subprocess.run(args, check=True, timeout=300)
    rails = [0, 0]
    for o, count, s, n in expect:
        rec = np.fromfile(o, np.float32); pcm = np.fromfile(str(o) + ".test_output.pcm", np.int16)
        tin = np.fromfile(str(o) + ".test_input.pcm", np.int16)
        assert rec.size == count * 138 and pcm.size == count * 480
        assert np.array_equal(tin, n)
        if count:
            orec, opcm = oracle.train_run(s, n)
            _check(rec.reshape(count, 138), pcm.reshape(count, 480), orec, opcm, str(o))
            rails[0] += int((pcm[1024 * 480:] == 32767).sum()); rails[1] += int((pcm[1024 * 480:] == -32768).sum())
    assert rails[0] >= 20 and rails[1] >= 20, rails           # behind the chunk edge; the oracle: 59 and 57, all in job 0
