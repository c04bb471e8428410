"""GPU parity tests (-m gpu) of the batched training-feature generator: the HIP
path through the C-ABI (pn_featgen_*, the mangled train(), the percepnet_featgen CLI) against the CPU
oracle and against the committed records of the compiled reference's train().

Tolerance: every field of the 138-float record is bit-exact EXCEPT the 34 ideal gains g, which pass
through post_filtering's sinf (denoise.cpp:227): libm's sinf on the CPU, OCML's on the GPU, each
within 1 ULP of sin but not of each other.  g is therefore compared with a relative bound
(G_RTOL, a few float ULPs after the two 34-term sums and the sqrt that follow) down to the subnormal range:
the absolute term is four half units of the smallest subnormal, for the last roundings into a subnormal word
(derived in tests/featgen_cases.py, gains_match; the reference's gains go down to 1e-28).  test_output.pcm,
which is synthesised with those gains, is compared within +-1 LSB.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, synth

pytestmark = pytest.mark.gpu

G_RTOL = 2e-6
G_ATOL = 4 * 2.0 ** -149
PCM_TOL_LSB = 1


def _oracle_pairs(oracle, sp, no):
    recs, pcms = [], []
    for p in range(sp.shape[0]):
        r, q = oracle.train_run(sp[p], no[p])
        recs.append(r); pcms.append(q)
    return np.stack(recs), np.stack(pcms)


def _check(rec, pcm, orec, opcm):
    exact = np.r_[0:70, 104:138]                        # Ey_lookahead, Ephaty, T, pitch_corr, r
    assert np.array_equal(rec[..., exact].view(np.uint32), orec[..., exact].view(np.uint32))
    g, og = rec[..., 70:104], orec[..., 70:104]
    assert np.all(np.abs(g - og) <= G_RTOL * np.abs(og) + G_ATOL), np.abs(g - og).max()
    assert np.array_equal(g == 0, og == 0)
    if pcm is not None:
        d = np.abs(pcm.astype(np.int32) - opcm.astype(np.int32))
        assert d.max() <= PCM_TOL_LSB, d.max()


def test_featgen_matches_oracle(oracle):
    """12 pairs incl. silence pairs (3, 7, 11), 60 frames: records and test_output.pcm."""
    B, T = 12, 60
    sp, no = synth.synth_pairs(B, T)
    fg = api.FeatGen(B)
    rec, pcm = fg.run(sp, no)
    orec, opcm = _oracle_pairs(oracle, sp, no)
    _check(rec, pcm, orec, opcm)
    assert (rec[3, 14:25, 70:104] == 0).all() and (rec[:, :, 104:] == np.float32(0.99)).any()
    fg.close()


def test_featgen_front_end_families_agree_bit_for_bit(oracle):
    """The generator runs the front-end family of its plan, like a context: PERCEPNET_FE=split|mono|g2 at creation.  19 pairs
    (a ragged second block of the 16-streams-per-block g4 kernel, a partial group of the g2 and pitch kernels; silence pairs
    3, 7, 11) x 14 frames (a wrap of the 12-slot history ring and of the 6-slot spectrum ring).  split against the oracle;
    mono and g2 against split bit for bit, records (the target kernel is the same, so its inputs — both sides' band energies,
    side outputs and periods — were equal) and PCM.  A pair costs 98 408 device bytes whatever the family."""
    B, T = 19, 14
    sp, no = synth.synth_pairs(B, T)
    res = {}
    for fam in ("split", "mono", "g2"):
        os.environ["PERCEPNET_FE"] = fam
        try:
            fg = api.FeatGen(B)
        finally:
            del os.environ["PERCEPNET_FE"]
        res[fam] = fg.run(sp, no)
        fg.close()
    orec, opcm = _oracle_pairs(oracle, sp, no)
    _check(res["split"][0], res["split"][1], orec, opcm)
    for fam in ("mono", "g2"):
        assert np.array_equal(res[fam][0].view(np.uint32), res["split"][0].view(np.uint32)), fam
        assert np.array_equal(res[fam][1], res["split"][1]), fam
    a, b = api.FeatGen(B), api.FeatGen(1)
    assert a.device_bytes() - b.device_bytes() == 18 * 98408
    a.close(); b.close()


def test_featgen_golden_records_of_compiled_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "featgen_golden.npz"))
    sp = np.stack([g["speech_0"], g["speech_2"], g["speech_3"]]); no = np.stack([g["noisy_0"], g["noisy_2"], g["noisy_3"]])
    fg = api.FeatGen(3)
    rec, pcm = fg.run(sp, no)
    _check(rec, pcm, np.stack([g["rec_0"], g["rec_2"], g["rec_3"]]), np.stack([g["pcm_0"], g["pcm_2"], g["pcm_3"]]))
    fg.close()


def test_featgen_chunked_calls_continue_state_and_reset(oracle):
    """Two calls of 20 frames == one call of 40 (state carried); reset() == fresh."""
    B, T = 5, 40
    sp, no = synth.synth_pairs(B, T)
    fg = api.FeatGen(B)
    full, _ = fg.run(sp, no, want_test_pcm=False)
    fg.reset()
    a, _ = fg.run(sp[:, :20 * 480], no[:, :20 * 480], want_test_pcm=False)
    b, _ = fg.run(sp[:, 20 * 480:], no[:, 20 * 480:], want_test_pcm=False)
    assert np.array_equal(np.concatenate([a, b], axis=1).view(np.uint32), full.view(np.uint32))
    fg.close()


def test_featgen_frame_api_on_device_buffers(oracle):
    """pn_featgen_process_i16 frame by frame on torch device tensors."""
    import torch
    B, T = 6, 24
    sp, no = synth.synth_pairs(B, T)
    fg = api.FeatGen(B)                                   # its own non-blocking HIP stream
    d_sp = torch.from_numpy(np.ascontiguousarray(sp.reshape(B, T, 480).transpose(1, 0, 2))).cuda()   # [T][B][480]
    d_no = torch.from_numpy(np.ascontiguousarray(no.reshape(B, T, 480).transpose(1, 0, 2))).cuda()
    rec = torch.empty((T, B, 138), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                              # inputs resident before the other stream reads them
    for t in range(T):
        fg.process_dev(d_sp[t].data_ptr(), d_no[t].data_ptr(), rec[t].data_ptr(), None)
    fg.synchronize(); torch.cuda.synchronize()
    orec, _ = _oracle_pairs(oracle, sp, no)
    _check(rec.cpu().numpy().transpose(1, 0, 2), None, orec, None)
    fg.close()


def test_featgen_large_batch_placement_invariance():
    """4099 pairs (ragged vs the 16-streams-per-block tiling) built from 7 distinct pairs: identical
    pairs must give identical records wherever they sit in the batch."""
    B, T, K = 4099, 12, 7
    bsp, bno = synth.synth_pairs(K, T)
    idx = np.arange(B) % K
    fg = api.FeatGen(B)
    rec, pcm = fg.run(bsp[idx], bno[idx])
    for k in range(K):
        sel = rec[idx == k]
        assert np.array_equal(sel.view(np.uint32), np.broadcast_to(sel[0], sel.shape).view(np.uint32)), k
        ps = pcm[idx == k]
        assert np.array_equal(ps, np.broadcast_to(ps[0], ps.shape)), k
    fg.close()


def test_train_symbol_and_cli_file_semantics(oracle, tmp_path):
    """The mangled train() (rnnoise.h:66) for one job, and percepnet_featgen for three jobs with
    different counts; inputs shorter than count are cycled over their whole frames, a partial tail
    frame is never used (denoise.cpp:693-715)."""
    lib = ctypes.CDLL(api.LIB_PATH)
    T = 30
    sp, no = synth.synth_pairs(3, T)
    paths = []
    for p in range(3):
        a, b = tmp_path / f"s{p}.pcm", tmp_path / f"n{p}.pcm"
        tail = np.arange(100, dtype=np.int16)                  # partial trailing frame: ignored
        np.concatenate([sp[p], tail]).tofile(a); np.concatenate([no[p][:20 * 480], tail]).tofile(b)   # noisy: 20 frames, cycled
        paths.append((str(a), str(b)))
    counts = [30, 25, 12]

    def expect(p, count):
        n_cyc = np.concatenate([no[p][:20 * 480]] * 2)[:count * 480]
        return oracle.train_run(sp[p][:count * 480], n_cyc), n_cyc

    # train(): cwd by-products like the reference
    cwd = os.getcwd(); os.chdir(tmp_path)
    try:
        argv = (ctypes.c_char_p * 5)(b"percepNet", paths[0][0].encode(), paths[0][1].encode(), b"30", b"out0.f32")
        assert getattr(lib, "_Z5trainiPPc")(5, argv) == 0
        assert getattr(lib, "_Z5trainiPPc")(3, argv) == 1                  # usage error -> 1 like the reference
    finally:
        os.chdir(cwd)
    (orec, opcm), n_cyc = expect(0, 30)
    rec = np.fromfile(tmp_path / "out0.f32", np.float32).reshape(30, 138)
    _check(rec, np.fromfile(tmp_path / "test_output.pcm", np.int16).reshape(30, 480), orec, opcm)
    assert np.array_equal(np.fromfile(tmp_path / "test_input.pcm", np.int16), n_cyc)

    exe = os.path.join(os.path.dirname(api.LIB_PATH), "percepnet_featgen")
    args = [exe, "--test-pcm"]
    for p in range(3):
        args += [paths[p][0], paths[p][1], str(counts[p]), str(tmp_path / f"cli{p}.f32")]
    subprocess.run(args, check=True, timeout=300)
    for p in range(3):
        (orec, opcm), n_cyc = expect(p, counts[p])
        rec = np.fromfile(tmp_path / f"cli{p}.f32", np.float32).reshape(counts[p], 138)
        pcm = np.fromfile(str(tmp_path / f"cli{p}.f32") + ".test_output.pcm", np.int16).reshape(counts[p], 480)
        _check(rec, pcm, orec, opcm)
    assert subprocess.run([exe, "a", "b"], capture_output=True).returncode == 1
    # multi-device host (SURVEY 8(f)1 / run.sh:95-117's fan-out): --devices shards the jobs over one host thread + one
    # generator per listed device; the same device twice on this 1-GPU box = two threads, ragged shards of 2 + 1 jobs.
    # The records must be byte-identical to the single-device run.
    args2 = [exe, "--devices", "0,0", "--test-pcm"]
    for p in range(3):
        args2 += [paths[p][0], paths[p][1], str(counts[p]), str(tmp_path / f"md{p}.f32")]
    subprocess.run(args2, check=True, timeout=300)
    for p in range(3):
        assert (tmp_path / f"md{p}.f32").read_bytes() == (tmp_path / f"cli{p}.f32").read_bytes(), p
        assert (tmp_path / f"md{p}.f32.test_output.pcm").read_bytes() == (tmp_path / f"cli{p}.f32.test_output.pcm").read_bytes(), p
    for bad in ("0,,0", "0,", "x", "0,99"):              # an empty element is not device 0; an ordinal must be visible
        r = subprocess.run([exe, "--devices", bad] + args2[4:], capture_output=True, text=True)
        assert r.returncode == 1 and "--devices" in r.stderr, (bad, r.stderr)

