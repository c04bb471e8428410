"""Comfort noise on the rate converter: the host-only surface, no GPU (include/percepnet_hip.h "comfort noise"; the rule lives in the
HIP-free percepnet_amd/csrc/pn_cng_rules.h): pn_cng_sid_decode and pn_cng_frame against the numpy model (tests/cng_model.py) bit for
bit, the level table, the level and the stability of the model's noise, the refusals that need no device, the CLI's argument errors,
and the rules under the address and undefined-behaviour sanitizers in a stand-alone program (tests/c/cng_sanitize.cpp).

Measured on the model, for the seeds used here (DESIGN.md "Numerics of comfort noise"):
  white noise, M = 0, 100 rows of 80 samples, slots 0..3: level errors -0.079, +0.046, +0.060, -0.104 dB at L = 0, 20, 60, 127 (bound
    0.3 dB = 5 sigma of an rms over 8000 iid triangular samples, relative sd sqrt(1.4 / 32000) = 0.0066 = 0.057 dB);
  shaped noise, M = 12, SHAPED below (poles near the unit circle: k_1 = -0.945, k_2 = 0.732), L = 30, 100 rows of 160 samples, slots
    0..7: level errors -0.003 -0.118 +0.045 +0.184 +0.021 +0.141 -0.127 +0.105 dB, the largest 0.184 dB; the test asserts twice that,
    0.37 dB — the estimate's variance grows with the filter's correlation length and cannot be derived in general;
  all twelve N_i at 0, and at 254, L = 30, 200 rows of 80: every sample finite, the largest |sample| 1.7e-4 and 0.025 — under the 1.0
    the test asserts; no bound is derived in the rule."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import cng_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32
SHAPED_BOUND_DB = 0.37                                   # twice the 0.184 dB measured on the model (above)
SHAPED = (7, 220, 90, 150, 110, 140, 120, 135, 125, 130, 127, 128)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def db(x):
    return 20.0 * np.log10(x)


def model_rows(sids, n_rows, ns, seed=cm.DEFAULT_SEED):
    """n_rows rows of ns samples of the streams 0 .. len(sids) - 1, one run each -> float32 [len(sids)][n_rows * ns]"""
    sids = np.stack(sids)
    n = len(sids)
    st = np.zeros((n, 16), U32)
    return np.concatenate([cm.rows(st, sids, cm.key(seed, np.arange(n)), [t > 0] * n, [ns] * n)[0][:, :ns] for t in range(n_rows)], axis=1)


def library_rows(sids, n_rows, ns, seed=cm.DEFAULT_SEED):
    """the same from pn_cng_frame, a stream at a time"""
    out = []
    for slot, sid in enumerate(sids):
        st = np.zeros(16, U32)
        out.append(np.concatenate([api.cng_frame(sid, st, seed, slot, t > 0, ns)[0] for t in range(n_rows)]))
    return np.stack(out)


def test_constants():
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    for name, val in (("PN_CNG_MAX_ORDER", "12"), ("PN_CNG_SID_BYTES", "14"), ("PN_CNG_DEFAULT_LEVEL", "60"), ("PN_CNG_DEFAULT_SEED", "0x434e4731u"),
                      ("PN_CNG_REPORT_WORDS", "4")):
        assert f"#define {name} {val}\n" in hdr, name
    assert (api.CNG_MAX_ORDER, api.CNG_SID_BYTES, api.CNG_DEFAULT_LEVEL, api.CNG_DEFAULT_SEED) == (cm.MAX_ORDER, cm.SID_BYTES, cm.DEFAULT_LEVEL, cm.DEFAULT_SEED)
    assert api.CNG_REPORT_WORDS == 4 and api.CNG_REPORT_DTYPE == cm.REPORT_DTYPE and api.CNG_REPORT_DTYPE.itemsize == 16
    rules = open(os.path.join(ROOT, "percepnet_amd", "csrc", "pn_cng_rules.h")).read()
    assert "#define PN_CNG_STATE_WORDS 16\n" in rules and "0x381cc471" in rules
    assert same(api.cng_sid(60), cm.sid(60)) and same(api.cng_sid(3, [1, 2]), cm.sid(3, [1, 2]))
    assert abs(float(cm.C) * np.sqrt((2.0 ** 32 - 1) / 6.0) - 1.0) < 6e-8, "c is the fp32 nearest 1 / sigma_u"


def test_the_level_table_is_within_one_ulp():
    for L in range(128):
        got, want = api.cng_level(L), F32(10.0 ** (-L / 20.0))
        assert same(got, cm.LEVEL[L]) and abs(int(got.view(U32)) - int(want.view(U32))) <= 1, L
    assert np.isnan(api.cng_level(-1)) and np.isnan(api.cng_level(128))


@pytest.mark.parametrize("M", (0, 1, 2, 12))
def test_decode_is_the_models_bit_for_bit(M):
    rng = np.random.default_rng(9100 + M)
    cases = [[v] * M for v in (0, 127, 254)] + [rng.integers(0, 255, M).tolist() for _ in range(8)]
    for N in cases:
        for L in (0, 1, 126, 127, 60):
            g, k, m = api.cng_sid_decode(cm.sid(L, N))
            wg, wk, wm = cm.decode(cm.sid(L, N))
            assert m == wm == M and same(g, wg) and same(k, wk), (L, N)
            assert same(k[:M], ((np.array(N, np.float64) - 127) * 258 / 32768).astype(F32)) and not k[M:].any()
            assert g > 0 and np.isfinite(g)
    assert api.cng_sid_decode(cm.sid(20))[0] == F32(0.1) and api.cng_sid_decode(cm.sid(0, [127] * 12))[0] == 1.0


def test_bytes_behind_the_order_are_not_looked_at():
    s = cm.sid(40, [3, 250])
    t = s.copy()
    t[4:] = 255
    assert [same(a, b) for a, b in zip(api.cng_sid_decode(s)[:2], api.cng_sid_decode(t)[:2])] == [True, True]


def test_refusals():
    L = api.load_library()
    for bad, words in ((cm.sid(128), "level 128"), (np.array([13, 0] + [0] * 12, np.uint8), "order 13"), (cm.sid(5, [0, 255]), "N_2 = 255")):
        with pytest.raises(api.PercepNetError, match=words):
            api.cng_sid_decode(bad)
        with pytest.raises(api.PercepNetError, match=words):
            api.cng_frame(bad, np.zeros(16, U32), 0, 0, False, 80)
    with pytest.raises(api.PercepNetError, match="14"):
        api.cng_sid_decode(np.zeros(13, np.uint8))
    for n in (0, 79, 81, 400, 481):
        with pytest.raises(api.PercepNetError, match="80, 160, 240, 320 or 480"):
            api.cng_frame(cm.sid(60), np.zeros(16, U32), 0, 0, False, n)
    g, M, k, st, row = F32(0), np.zeros(1, np.int32), np.zeros(12, F32), np.zeros(16, U32), np.zeros(80, F32)
    sid = cm.sid(60)
    assert L.pn_cng_sid_decode(None, k.ctypes.data, k.ctypes.data, M.ctypes.data) == -1
    assert L.pn_cng_sid_decode(sid.ctypes.data, None, k.ctypes.data, M.ctypes.data) == -1
    assert L.pn_cng_frame(None, st.ctypes.data, 0, 0, 0, 80, row.ctypes.data, None) == -1
    assert L.pn_cng_frame(sid.ctypes.data, None, 0, 0, 0, 80, row.ctypes.data, None) == -1
    assert L.pn_cng_frame(sid.ctypes.data, st.ctypes.data, 0, 0, 0, 80, None, None) == -1
    assert L.pn_cng_frame(sid.ctypes.data, st.ctypes.data, 0, -1, 0, 80, row.ctypes.data, None) == -1
    # the converter's calls refuse a NULL converter before anything else; marks with the switch off need a device (tests/test_gpu_cng.py)
    for name, args in (("pn_rate_set_cng", (None, 1)), ("pn_rate_set_silent", (None, None, 0)), ("pn_rate_set_stream_sid", (None, None, 0, None, 14)),
                       ("pn_rate_get_stream_sid", (None, None)), ("pn_rate_cng_f32", (None, None, None, 0)), ("pn_rate_set_cng_report", (None, 1)),
                       ("pn_rate_read_cng_report", (None, None)), ("pn_rate_set_cng_seed", (None, 1)), ("pn_rate_get_cng_seed", (None, None))):
        assert getattr(L, name)(*args) == -1 and b"NULL" in L.pn_last_error(), name


@pytest.mark.parametrize("ns", cm.ROWS)
@pytest.mark.parametrize("M", (0, 1, 2, 12))
def test_frame_is_the_models_bit_for_bit(M, ns):
    """three rows of a run with the counter wrapping through 2^32 inside the first, a SID change in front of the third (the ramp), a
    received frame (the run ends), then a run of two"""
    rng = np.random.default_rng(9200 + 13 * M + ns)
    cases = [(N, L0, L1) for N in [[0] * M, [127] * M, [254] * M, rng.integers(0, 255, M).tolist(), rng.integers(100, 155, M).tolist()]
             for L0, L1 in ((0, 127), (1, 126), (126, 1), (127, 0))]
    n = len(cases)                                       # the cases are the streams of ONE model call per row; the library runs them one by one
    sids = [np.stack([cm.sid((L0, L0, L1, L1, L0)[t], N if t in (0, 1, 4) else N[::-1]) for N, L0, L1 in cases]) for t in range(5)]
    conts = [False, True, True, False, True]
    st = np.zeros((n, 16), U32)
    st[:, cm.W_CTR] = 2 ** 32 - ns // 2
    ms = st.copy()
    slots = 41 + np.arange(n)
    for t in range(5):
        mrow, mrep = cm.rows(ms, sids[t], cm.key(0xDEADBEEF, slots), [conts[t]] * n, [ns] * n)
        for i in range(n):
            row, rep = api.cng_frame(sids[t][i], st[i], 0xDEADBEEF, int(slots[i]), conts[t], ns)
            assert same(row, mrow[i, :ns]) and same(st[i], ms[i]) and same(rep, mrep[i]), (M, ns, cases[i], t)
            assert np.isfinite(row).all()
    assert (st[:, cm.W_CTR] == 5 * ns - ns // 2).all() and (st[:, cm.W_RUN] == 2).all() and (st[:, cm.W_TOTAL] == 5).all()
    assert all(st[i, cm.W_PREV] == api.cng_sid_decode(sids[4][i])[0].view(U32) for i in range(n))


def test_the_gain_of_a_run_and_of_a_sid_change():
    """M = 0: the row is gain(n) e(n).  An unchanged SID keeps g exactly; a changed one ramps from the old g to the new across one row;
    a new run starts at g"""
    ns, seed, slot = 160, 7, 3
    e = (cm.u_of(np.arange(4 * ns, dtype=np.int64).astype(U32), cm.key(seed, [slot])).astype(F32) * cm.C).astype(F32)
    g20, g40 = api.cng_level(20), api.cng_level(40)
    st = np.zeros(16, U32)
    r0, _ = api.cng_frame(cm.sid(20), st, seed, slot, False, ns)
    r1, _ = api.cng_frame(cm.sid(20), st, seed, slot, True, ns)
    r2, _ = api.cng_frame(cm.sid(40), st, seed, slot, True, ns)
    r3, rep = api.cng_frame(cm.sid(20), st, seed, slot, False, ns)
    assert same(r0, g20 * e[:ns]) and same(r1, g20 * e[ns:2 * ns])
    w = (np.arange(1, ns + 1).astype(F32) / F32(ns)).astype(F32)
    assert same(r2, (g20 + w * (g40 - g20)).astype(F32) * e[2 * ns:3 * ns])
    assert same(r3, g20 * e[3 * ns:]) and rep.tolist() == [1, 4, int(g20.view(U32)), 4 * ns]
    assert np.abs(e).max() <= 65535 * float(cm.C) and abs(e.std() - 1) < 0.1


def test_streams_and_seeds_have_their_own_noise():
    rows = [api.cng_frame(cm.sid(10), np.zeros(16, U32), seed, slot, False, 480)[0] for seed, slot in ((1, 0), (1, 1), (2, 0))]
    for a in range(3):
        for b in range(a + 1, 3):
            assert abs(np.corrcoef(rows[a], rows[b])[0, 1]) < 0.2 and not same(rows[a], rows[b])
    for lag in (1, 2, 7):
        assert abs(np.corrcoef(rows[0][lag:], rows[0][:-lag])[0, 1]) < 0.2, "white"


def test_the_level_of_white_noise():
    levels = (0, 20, 60, 127)
    got = library_rows([cm.sid(L) for L in levels], 100, 80)
    assert same(got, model_rows([cm.sid(L) for L in levels], 100, 80)), "the library's rows are the model's"
    x = got.astype(np.float64)
    for i, L in enumerate(levels):
        err = db(np.sqrt((x[i] * x[i]).mean())) + L
        print(f"L = {L}: level error {err:+.4f} dB")
        assert abs(err) <= 0.3, L


def test_the_level_of_shaped_noise():
    got = library_rows([cm.sid(30, SHAPED)] * 8, 100, 160)
    assert same(got, model_rows([cm.sid(30, SHAPED)] * 8, 100, 160)), "the library's rows are the model's"
    x = got.astype(np.float64)
    err = db(np.sqrt((x * x).mean(axis=1))) + 30
    print("level errors of slots 0..7 in dB:", " ".join(f"{e:+.4f}" for e in err))
    k = cm.decode(cm.sid(30, SHAPED))[1]
    assert abs(k[0]) > 0.9 and abs(k[1]) > 0.7, "poles near the unit circle"
    assert np.abs(err).max() <= SHAPED_BOUND_DB, "twice the deviation measured on the model (the docstring)"


def test_the_extreme_filters_stay_finite():
    sids = [cm.sid(30, [0] * 12), cm.sid(30, [254] * 12)]
    x = model_rows(sids, 200, 80)
    print("the largest |sample| with N_i = 0, 254:", np.abs(x).max(axis=1))
    assert np.isfinite(x).all() and np.abs(x).max() < 1.0
    # ... and the library's rows are the model's there too
    assert same(library_rows(sids, 200, 80), x)


def test_cli_refuses_bad_dtx_and_sid_arguments(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    for i in range(2):
        (tmp_path / f"in{i}.pcm").write_bytes(bytes(1920))
    files = ["in0.pcm", "out0.pcm", "in1.pcm", "out1.pcm"]
    for opts, words in ((["--sid", "30"], ("--sid", "needs --dtx")),
                        (["--dtx", "2:1"], ("--dtx", "pair 2")),
                        (["--dtx", "0:3-1"], ("--dtx", "expected")),
                        (["--dtx", "x"], ("--dtx", "expected")),
                        (["--dtx", "0:1,"], ("--dtx", "expected")),
                        (["--dtx", "0:1", "--sid", "128"], ("--sid", "level 128")),
                        (["--dtx", "0:1", "--sid", "30:255"], ("--sid", "N_1 = 255")),
                        (["--dtx", "0:1", "--sid", "30:256"], ("--sid", "expected")),
                        (["--dtx", "0:1", "--sid", "30:"], ("--sid", "expected")),
                        (["--dtx", "0:1", "--sid", ":".join(["30"] + ["1"] * 13)], ("--sid", "at most 12")),
                        (["--rate", "8000", "--dtx", "0:1", "--sid", "x"], ("--sid", "expected"))):
        run = subprocess.run([exe] + opts + files, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and all(w in run.stderr for w in words), (opts, run.stderr)
        assert not (tmp_path / "out0.pcm").exists(), opts


def test_rules_under_sanitizers(tmp_path):
    """tests/c/cng_sanitize.cpp = pn_cng_rules.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: SIDs of exactly 2 + M bytes, a state of exactly 16 words, rows of exactly n_s floats at every row
    length and order, the counter through its wrap, the counts at their ceiling, the refusals."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "cng_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "cng_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
