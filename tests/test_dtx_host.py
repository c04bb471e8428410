"""The DTX send side of the rate converter: the host-only surface, no GPU (include/percepnet_hip.h "DTX send side"; the rule lives in the
HIP-free percepnet_amd/csrc/pn_dtx_rules.h): pn_dtx_frame, pn_dtx_sid_from_acorr and pn_dtx_level against the numpy model
(tests/dtx_model.py) bit for bit, the table of level edges, the sign and quantisation contract with the receive side
(pn_cng_rules.h), the estimator on the comfort-noise model's own rows, the state machine at its edges, the refusals that need no
device, the CLI's argument errors, and the rules under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/c/dtx_sanitize.cpp).  Every SID emitted anywhere here is decoded by pn_cng_sid_decode (check_sid).

Measured here, on the library's rows (which are the model's, tests/test_cng_host.py), DESIGN.md "Numerics of the DTX send side" —
the estimate's level error 10 log10 R[0] + L at 20, 100 and 300 rows behind the first, SMOOTH = 0.1:
  white noise, M = 0, L = 30, 80-sample rows:                    -0.048, -0.302, -0.064 dB; the test asserts 0.61 dB, twice the largest
  SHAPED (test_cng_host.py), L = 30, 160-sample rows:            +0.086, -0.126, +0.589 dB; the test asserts 1.18 dB
  ten random N_i in [40, 214], L = 30, 80-sample rows:           +0.471, +0.081, -0.269 dB; the test asserts 0.95 dB
(The issue's prototype saw 0.0 .. +0.8 dB; the signs differ here, the size does not.)  L itself came out 30 everywhere but once, 29
(SHAPED, 300 rows).  The reflection coefficients of the SIDs the estimator would emit at order 12 scatter around the descriptor's: the
largest |k_i - k_i(SID)| is 0.220 (SHAPED, 20 rows), 0.150 (ten) and 0.063 (white, where every k_i should be 0); reported, not asserted.
The ten-coefficient case is a draw on which the detector stays quiet: of twelve draws tried, eight fired THR = 4 on one to thirteen of
300 pure-noise rows of 80 samples — the known limit of the header, and not only on SHAPED.
The contract test (pn_dtx_sid_from_acorr on the exact autocorrelation of the process a SID describes returns that SID's N_i) leaves out
no case: all 37 come back byte for byte."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import cng_model as cm
from tests import dtx_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32
SHAPED = (7, 220, 90, 150, 110, 140, 120, 135, 125, 130, 127, 128)
LOOP_BOUND_DB = {"white": 0.61, "shaped": 1.18, "ten": 0.95}     # twice the largest deviation measured (the docstring)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def words(rep):
    return np.frombuffer(np.asarray(rep).tobytes(), U32)


def check_sid(sid14):
    """an emitted SID is one the receive side accepts"""
    g, k, M = api.cng_sid_decode(np.asarray(sid14, np.uint8))
    assert np.isfinite(g) and g > 0 and M == sid14[0] and not np.asarray(sid14)[2 + M:].any()
    return g, k, M


_pool = {}


def noise_pool():
    """model comfort noise (tests/cng_model.py), computed once: eight streams of 60 rows of 80 samples, orders 0, 2, 10 and 12"""
    if "p" not in _pool:
        rng = np.random.default_rng(9500)
        sids = np.stack([cm.sid(0, rng.integers(60, 195, (0, 2, 10, 12)[s % 4]).tolist()) for s in range(8)])
        st = np.zeros((8, 16), U32)
        keys = cm.key(0xD7, np.arange(8))
        _pool["p"] = np.concatenate([cm.rows(st, sids, keys, [t > 0] * 8, [80] * 8)[0][:, :80] for t in range(60)], axis=1)
        assert np.isfinite(_pool["p"]).all()
    return _pool["p"]


_hand = {}


def hand_rows(B, ns, T=40, seed=0):
    """float32 [T][B][ns], read-only, computed once per shape: every stream model comfort noise at a level of its own (-20 .. -55 dBov),
    with a burst on rows 6..9 of every second stream, a level step of 12 dB from row 14 on for every third, one row each of +-full
    scale, a NaN, an inf, subnormals and zeros spread over the streams, late enough that every stream has been silent before"""
    key = (B, ns, T, seed)
    if key not in _hand:
        pool = noise_pool()
        L = pool.shape[1]
        n = np.arange(ns)
        x = np.zeros((T, B, ns), F32)
        for s in range(B):
            gain = F32(10.0 ** (-(20 + 5 * ((s + seed) % 8)) / 20.0))
            for t in range(T):
                x[t, s] = pool[(s + seed) % 8, (131 * s + 17 * seed + t * ns + n) % L] * gain
        x[6:10, ::2] += (0.25 * np.sin(2 * np.pi * 0.031 * n)).astype(F32)
        x[14:, 1::3] *= F32(4)
        x[24, ::4] = np.where(n % 2, F32(-1), F32(1))
        x[26, 1::5, 3] = np.nan
        x[28, 2::5, 7] = np.inf
        x[28, 3::5, 9] = -np.inf
        x[30, 1::2] = np.where(n % 2, F32(-1e-41), F32(1e-41))
        x[33:35, 3::4] = 0
        x.setflags(write=False)
        _hand[key] = x
    return _hand[key]


# ---------------------------------------------------------------------------------------------------------------- constants, the table
def test_constants():
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    for name, val in (("PN_DTX_N_PARAMS", 9), ("PN_DTX_THR", 0), ("PN_DTX_FLOOR_UP", 1), ("PN_DTX_FLOOR_DRIFT", 2), ("PN_DTX_FLOOR_MIN", 3), ("PN_DTX_HANGOVER", 4),
                      ("PN_DTX_SMOOTH", 5), ("PN_DTX_UPDATE_DB", 6), ("PN_DTX_MAX_INTERVAL", 7), ("PN_DTX_ORDER", 8), ("PN_DTX_REPORT_WORDS", 8), ("PN_DTX_FRAME", 0),
                      ("PN_DTX_SID", 1), ("PN_DTX_NONE", 2), ("PN_DTX_ON", 1), ("PN_DTX_ACTIVE", 2), ("PN_DTX_HANGOVER_FRAME", 4), ("PN_DTX_NONFINITE", 8)):
        assert f"#define {name} {val}\n" in hdr, name
    assert (api.DTX_N_PARAMS, api.DTX_REPORT_WORDS, api.DTX_STATE_WORDS) == (dm.N_PARAMS, dm.REPORT_WORDS, dm.STATE_WORDS) == (9, 8, 24)
    assert (api.DTX_THR, api.DTX_FLOOR_UP, api.DTX_FLOOR_DRIFT, api.DTX_FLOOR_MIN, api.DTX_HANGOVER, api.DTX_SMOOTH, api.DTX_UPDATE_DB, api.DTX_MAX_INTERVAL,
            api.DTX_ORDER) == (dm.THR, dm.FLOOR_UP, dm.FLOOR_DRIFT, dm.FLOOR_MIN, dm.HANGOVER, dm.SMOOTH, dm.UPDATE_DB, dm.MAX_INTERVAL, dm.ORDER)
    assert (api.DTX_FRAME, api.DTX_SID, api.DTX_NONE) == (dm.FRAME, dm.SID, dm.NONE) == (0, 1, 2)
    assert (api.DTX_ON, api.DTX_ACTIVE, api.DTX_HANGOVER_FRAME, api.DTX_NONFINITE) == (dm.ON, dm.ACTIVE, dm.HANGOVER_FRAME, dm.NONFINITE) == (1, 2, 4, 8)
    assert api.DTX_REPORT_DTYPE == dm.REPORT_DTYPE and api.DTX_REPORT_DTYPE.itemsize == 32
    rules = open(os.path.join(ROOT, "percepnet_amd", "csrc", "pn_dtx_rules.h")).read()
    for line in ("#define PN_DTX_STATE_WORDS 24\n", "#define PN_DTX_LAGS 13\n", "#define PN_DTX_W_N 13\n", "#define PN_DTX_W_HANG 14\n", "#define PN_DTX_W_MODE 15\n",
                 "#define PN_DTX_W_SINCE 16\n", "#define PN_DTX_W_FRAMES 17\n", "#define PN_DTX_W_SID 18\n", "0x42fe03f8"):
        assert line in rules, line
    assert same(api.dtx_default_params(), dm.default_params()) and same(dm.KQ, F32(32768 / 258))
    api.dtx_params_check(api.dtx_default_params())
    assert api.dtx_default_params().tolist() == [4.0, F32(0.1), F32(1.0023), F32(1e-10), 20.0, F32(0.1), 2.0, 0.0, 10.0]


def rules_edges():
    rules = open(os.path.join(ROOT, "percepnet_amd", "csrc", "pn_dtx_rules.h")).read()
    body = re.search(r"#define PN_DTX_EDGES \{(.*?)\}", rules, re.S).group(1)
    return np.array([float(v.strip().rstrip("f")) for v in body.replace("\\", "").split(",")], np.float64).astype(F32)


def test_the_edge_table():
    edges = rules_edges()
    assert edges.shape == (127,) and same(edges, dm.EDGE) and (np.diff(edges) < 0).all(), "127 literals, the model's, strictly falling"
    for i in range(127):
        want = F32(10.0 ** (-(i + 0.5) / 10.0))
        assert abs(int(edges[i].view(U32)) - int(want.view(U32))) <= 1, i
    for L in range(128):
        ms = F32(api.cng_level(L) * api.cng_level(L))
        assert api.dtx_level(ms) == L == dm.level(ms), L
    for i in range(127):                                 # an edge itself is not under the edge; the float below it is
        below = np.nextafter(edges[i], F32(0))
        assert api.dtx_level(edges[i]) == i == dm.level(edges[i]) and api.dtx_level(below) == i + 1 == dm.level(below), i
    assert api.dtx_level(0.0) == 127 and api.dtx_level(1.0) == 0 and api.dtx_level(np.inf) == 0 and api.dtx_level(np.nan) == 0 == dm.level(np.nan)
    assert api.dtx_level(-1.0) == 127 == dm.level(-1.0)


# ---------------------------------------------------------------------------------------------------------------- the frame
@pytest.mark.parametrize("ns", dm.ROWS)
def test_frame_is_the_models_bit_for_bit(ns):
    """four streams of 60 rows: comfort noise, a burst, a level step, +-full scale, NaN, inf, subnormals, zeros; two parameter sets"""
    rows = hand_rows(20, ns, 60, seed=ns)
    quick = np.array([4.0, 0.1, 1.5, 1e-10, 3, 0.1, 1, 4, 12], F32)
    seen, flags = set(), 0
    for s, p in ((0, quick), (1, quick), (7, dm.default_params()), (13, quick), (3, quick), (11, quick)):
        if p is not quick:
            p = p.copy()
            p[dm.HANGOVER] = 2
        st, ms = np.zeros(24, U32), np.zeros(24, U32)
        for t in range(60):
            d, rep = api.dtx_frame(p, st, rows[t, s])
            md, mrep = dm.frame(p, ms, rows[t, s])
            assert d == md and same(st, ms) and same(words(rep), mrep), (ns, s, t, st, ms, words(rep), mrep)
            assert rep["decision"] == d and not st[22:].any()
            if d == dm.SID:
                check_sid(rep["sid"])
            seen.add(d)
            flags |= int(rep["word1"]) & 0xFF
        assert st[dm.W_FRAMES] >= 57
    assert seen == {dm.FRAME, dm.SID, dm.NONE} and flags == dm.ON | dm.ACTIVE | dm.HANGOVER_FRAME | dm.NONFINITE


def test_a_nonfinite_row_changes_nothing_but_the_hangover_and_the_mode():
    p = dm.default_params()
    p[dm.HANGOVER] = 1
    rng = np.random.default_rng(3)
    st = np.zeros(24, U32)
    for t in range(6):
        d, rep = api.dtx_frame(p, st, (rng.standard_normal(160) * 1e-3).astype(F32))
    assert d == dm.NONE and st[dm.W_MODE] == dm.MODE_SILENT | dm.MODE_NOISE
    for bad in (np.nan, np.inf, -np.inf, 3e19):          # (the square of 3e19 overflows)
        x = (rng.standard_normal(160) * 1e-3).astype(F32)
        x[100] = bad
        before = st.copy()
        d, rep = api.dtx_frame(p, st, x)
        assert d == dm.FRAME and int(rep["word1"]) & 0xFF == dm.ON | dm.ACTIVE | dm.NONFINITE and int(rep["word1"]) >> 16 == 1
        changed = np.nonzero(st != before)[0].tolist()
        assert set(changed) <= {dm.W_HANG, dm.W_MODE} and st[dm.W_MODE] == dm.MODE_NOISE and st[dm.W_HANG] == 1
        d, rep = api.dtx_frame(p, st, (rng.standard_normal(160) * 1e-3).astype(F32))
        assert d == dm.FRAME and int(rep["word1"]) & dm.HANGOVER_FRAME
        d, rep = api.dtx_frame(p, st, (rng.standard_normal(160) * 1e-3).astype(F32))
        assert d == dm.SID, "from VOICE the first silent frame carries a SID"
        check_sid(rep["sid"])


# ---------------------------------------------------------------------------------------------------------------- the contract
def exact_acorr(N, L):
    """float64: the autocorrelation R[0..12] of the all-pole process the SID (L, N) describes — step-up from k_i = 258 (N_i - 127) /
    32768, the impulse response of 1 / A(z) until it has died away, lag products — scaled so that R[0] is the level's mean square"""
    k = 258.0 * (np.asarray(N, np.float64) - 127.0) / 32768.0
    a = [1.0]
    for i, ki in enumerate(k, 1):
        a = [1.0] + [a[j] + ki * a[i - j] for j in range(1, i)] + [ki]
    # the recursion h[n] = -sum a_j h[n-j] in blocks of 512: the block that follows a state (the last M outputs) is linear in it, so the
    # M unit states' blocks are computed once by the plain recursion and every later block is one matrix product
    M, B = len(k), 512
    T = np.zeros((B, M))
    for i in range(M):
        past = [0.0] * M
        past[i] = 1.0                                    # past[j]: the output j + 1 steps back
        for n in range(B):
            v = -sum(a[j + 1] * past[j] for j in range(M))
            past = [v] + past[:-1]
            T[n, i] = v
    state = np.zeros(M)
    state[0] = 1.0                                       # h[0] = 1
    blocks, total = [np.array([1.0])], 1.0
    while len(blocks) < 8192:
        blk = T @ state
        blocks.append(blk)
        state = blk[::-1][:M].copy()
        e = float(blk @ blk)
        total += e
        if e < 1e-34 * total:
            break
    h = np.concatenate(blocks)
    R = np.array([np.dot(h[j:], h[:len(h) - j]) for j in range(13)])
    return R * (float(api.cng_level(L)) ** 2 / R[0])


def contract_cases():
    rng = np.random.default_rng(9300)
    cases = [list(SHAPED)]
    for M in (1, 2, 4, 8, 10, 12):
        cases += [rng.integers(40, 215, M).tolist() for _ in range(5)]
    cases += [rng.integers(0, 255, 12).tolist() for _ in range(3)]
    cases += [[127] * 12, [40] * 3, [214, 40]]
    return cases


def test_the_sign_and_quantisation_contract_with_the_receive_side():
    """the send side is the inverse of pn_cng_rules.h: from the exact autocorrelation of what a SID synthesises, the SID's own bytes"""
    left_out = []
    cases = contract_cases()
    for i, N in enumerate(cases):
        L = (30, 0, 60, 100)[i % 4]
        R = exact_acorr(N, L).astype(F32)
        got = api.dtx_sid_from_acorr(R, len(N))
        assert same(got, dm.sid_from_acorr(R, len(N))), N
        check_sid(got)
        if not same(got, cm.sid(L, N)):
            left_out.append((N, got.tolist()))
        # a lower order gives the SID's first coefficients: the recursion is nested
        assert same(api.dtx_sid_from_acorr(R, len(N) // 2)[2:2 + len(N) // 2], np.array(N[:len(N) // 2], np.uint8)) or left_out
    print(f"{len(cases)} cases, left out: {left_out}")
    assert not left_out, "measured: none (the issue allows one case in ten)"


def test_sid_from_acorr_stops_where_the_rule_says():
    R = np.zeros(13, F32)
    assert api.dtx_sid_from_acorr(R, 12).tolist() == [0, 127] + [0] * 12, "R[0] = 0: level only, the quietest"
    for bad in (np.nan, np.inf, -1.0):
        R[0] = bad
        assert api.dtx_sid_from_acorr(R, 12)[0] == 0 and same(api.dtx_sid_from_acorr(R, 12), dm.sid_from_acorr(R, 12))
    R = np.array([1.0, 1.0] + [0.0] * 11, F32)           # |k_1| = 1: no coefficient
    assert api.dtx_sid_from_acorr(R, 12).tolist() == [0, 0] + [0] * 12
    R = np.array([1.0, 0.5, np.nan] + [0.0] * 10, F32)   # k_2 is NaN: one coefficient
    got = api.dtx_sid_from_acorr(R, 12)
    assert got[0] == 1 and same(got, dm.sid_from_acorr(R, 12)) and got[2] == int(-0.5 * 32768 / 258 + 127.5)
    R = (np.float64(0.999) ** np.arange(13)).astype(F32)   # k_1 = -0.999 quantises to N = 0, |kq| = 32766 / 32768
    got = api.dtx_sid_from_acorr(R, 12)
    assert got[2] == 0 and same(got, dm.sid_from_acorr(R, 12))
    check_sid(got)
    for order, R in ((0, np.ones(13, F32)), (12, np.arange(13, 0, -1).astype(F32))):
        assert same(api.dtx_sid_from_acorr(R, order), dm.sid_from_acorr(R, order))
    for order in (-1, 13):
        with pytest.raises(api.PercepNetError, match=r"order .*\[0, 12\]"):
            api.dtx_sid_from_acorr(np.ones(13, F32), order)


# ---------------------------------------------------------------------------------------------------------------- closed loop on the model
def estimate(sid, ns, n_rows, slot=0):
    """the estimator fed n_rows + 1 comfort-noise rows of `sid` -> (R float32 [13], the SID it would emit at order 12): no row is active
    behind the first"""
    p = dm.default_params()
    p[dm.ORDER] = 12
    cst, st = np.zeros(16, U32), np.zeros(24, U32)
    for t in range(n_rows + 1):
        row, _ = api.cng_frame(sid, cst, cm.DEFAULT_SEED, slot, t > 0, ns)
        d, rep = api.dtx_frame(p, st, row)
        assert t == 0 or not int(rep["word1"]) & dm.ACTIVE, (t, "the model's own noise must not fire the detector")
    R = st[:13].copy().view(F32)
    return R, api.dtx_sid_from_acorr(R, 12)


LOOP = {"white": (cm.sid(30), 80), "shaped": (cm.sid(30, SHAPED), 160),
        "ten": (cm.sid(30, np.random.default_rng(9401).integers(40, 215, 10).tolist()), 80)}   # (a draw on which the detector stays quiet: of the seeds 9400 .. 9411 eight fire within 300 rows of 80 samples, the known limit)


@pytest.mark.parametrize("case", sorted(LOOP))
def test_closed_loop_on_the_model(case):
    sid, ns = LOOP[case]
    _, k, M = api.cng_sid_decode(sid)
    worst = 0.0
    for n_rows in (20, 100, 300):
        R, got = estimate(sid, ns, n_rows)
        err = 10.0 * np.log10(float(R[0])) + 30.0
        gk = check_sid(got)[1]
        print(f"{case}: {n_rows} rows: level error {err:+.3f} dB, L {got[1]}, M {got[0]}, the largest |k_i - k_i(SID)| {np.abs(gk - k).max():.3f}")
        worst = max(worst, abs(err))
        assert abs(int(got[1]) - 30) <= 1, "L is quantised to 1 dB"
    assert worst <= LOOP_BOUND_DB[case], "twice the deviation measured on the model (the docstring)"


# ---------------------------------------------------------------------------------------------------------------- the state machine
def run(p, rows, st=None):
    st = np.zeros(24, U32) if st is None else st
    out = []
    for r in rows:
        d, rep = api.dtx_frame(p, st, np.asarray(r, F32))
        if d == dm.SID:
            check_sid(rep["sid"])
        out.append((d, rep.copy()))
    return out, st


def tone(amp, ns=80):
    return (amp * np.where(np.arange(ns) % 2, -1.0, 1.0)).astype(F32)      # mean square amp^2 exactly


@pytest.mark.parametrize("hang", (0, 1, 20, 255))
def test_exactly_hangover_frames_behind_the_last_active_one(hang):
    p = dm.default_params()
    p[dm.HANGOVER] = hang
    rows = [tone(1e-3)] * 3 + [tone(0.5)] * 2 + [tone(1e-3)] * (hang + 4)
    out, st = run(p, rows)
    d = [o[0] for o in out]
    # row 0 is active (the first), rows 1..2 its hangover or silent, rows 3..4 active, then exactly `hang` frames, a SID, silence
    assert d[3:5] == [dm.FRAME] * 2 and d[5:5 + hang] == [dm.FRAME] * hang and d[5 + hang] == dm.SID and d[6 + hang:] == [dm.NONE] * 3
    assert all(int(o[1]["word1"]) & dm.HANGOVER_FRAME for o in out[5:5 + hang]) and not int(out[5 + hang][1]["word1"]) & (dm.HANGOVER_FRAME | dm.ACTIVE)
    assert [int(o[1]["word1"]) >> 16 for o in out[4:6 + hang]] == [hang] + list(range(hang - 1, -1, -1)) + [0]
    if hang == 0:
        assert d[:3] == [dm.FRAME, dm.SID, dm.NONE], "a SID on the first silent frame"
    assert out[-1][1]["count"] == (2 if hang < 2 else 1)


def test_a_sid_update_on_a_level_step_of_exactly_update_db():
    """SMOOTH = 1: R[0] is the row's mean square, so the level steps with the row.  UPDATE_DB = 3: a step of 2 dB sends nothing, of 3 a SID"""
    p = dm.default_params()
    p[[dm.HANGOVER, dm.SMOOTH, dm.UPDATE_DB, dm.THR]] = (0, 1.0, 3, 100.0)
    amp = lambda L: float(api.cng_level(L))
    out, st = run(p, [tone(amp(40)), tone(amp(40)), tone(amp(40)), tone(amp(38)), tone(amp(37)), tone(amp(37)), tone(amp(39)), tone(amp(40)), tone(amp(42))])
    assert [o[0] for o in out] == [dm.FRAME, dm.SID, dm.NONE, dm.NONE, dm.SID, dm.NONE, dm.NONE, dm.SID, dm.NONE]
    assert [int(o[1]["word1"]) >> 8 & 0x7F for o in out] == [0, 40, 40, 38, 37, 37, 39, 40, 42]
    assert [int(o[1]["sid"][1]) for o in out] == [0, 40, 40, 40, 37, 37, 37, 40, 40] and [int(o[1]["count"]) for o in out] == [0, 1, 1, 1, 2, 2, 2, 3, 3]


@pytest.mark.parametrize("interval, want", ((0, "FSNNNNNN"), (1, "FSSSSSSS"), (3, "FSNNSNNS")))
def test_max_interval(interval, want):
    p = dm.default_params()
    p[[dm.HANGOVER, dm.MAX_INTERVAL]] = (0, interval)
    out, st = run(p, [tone(1e-3)] * 8)
    assert "".join("FSN"[o[0]] for o in out) == want
    assert st[dm.W_SINCE] == {0: 6, 1: 0, 3: 0}[interval]


@pytest.mark.parametrize("order", (0, 12))
def test_order(order):
    p = dm.default_params()
    p[[dm.HANGOVER, dm.ORDER]] = (0, order)
    pool = noise_pool()
    out, st = run(p, [pool[7, 80 * t:80 * t + 80] * F32(0.01) for t in range(4)])
    sids = [o[1]["sid"] for o in out if o[0] == dm.SID]
    assert sids and all(s[0] == order for s in sids)


def test_all_zero_rows_give_level_only_at_the_quietest():
    p = dm.default_params()
    p[dm.HANGOVER] = 0
    out, st = run(p, [np.zeros(80, F32)] * 3)
    assert [o[0] for o in out] == [dm.FRAME] * 3 and not st[:dm.W_HANG].any() and st[dm.W_FRAMES] == 0, "zeros in front of the first other row are not analysed"
    out, st = run(p, [tone(1e-3)] + [np.zeros(80, F32)] * 3)
    assert [o[0] for o in out] == [dm.FRAME, dm.SID, dm.NONE, dm.NONE]
    assert out[1][1]["sid"].tolist() == [0, 127] + [0] * 12 and int(out[1][1]["word1"]) >> 8 & 0x7F == 127
    assert out[3][1]["floor"] == 0 and out[3][1]["energy"] == 0
    # the floor climbs back from under FLOOR_MIN at the drift's pace, and the stream sends while it does
    p[dm.FLOOR_DRIFT] = 1.9
    more, st = run(p, [tone(1e-3)] * 24, st)
    d = [o[0] for o in more]
    first_quiet = d.index(dm.SID)
    assert d[:first_quiet] == [dm.FRAME] * first_quiet and 12 <= first_quiet <= 16 and more[first_quiet - 1][1]["floor"] > 2.5e-7


def test_the_count_of_sids_wraps_and_the_counters_saturate():
    p = dm.default_params()
    p[[dm.HANGOVER, dm.MAX_INTERVAL]] = (0, 1)
    st = np.zeros(24, U32)
    run(p, [tone(1e-3)] * 2, st)
    st[dm.W_SID + 3] |= U32(0xFFFF0000)
    st[dm.W_FRAMES] = 0xFFFFFFFE
    ms = st.copy()
    for t in range(2):
        d, rep = api.dtx_frame(p, st, tone(1e-3))
        md, mrep = dm.frame(p, ms, tone(1e-3))
        assert d == md == dm.SID and same(st, ms) and same(words(rep), mrep)
        assert rep["count"] == t and st[dm.W_FRAMES] == 0xFFFFFFFF
    p[dm.MAX_INTERVAL] = 0
    st[dm.W_SINCE] = 0xFFFE
    ms = st.copy()
    for t in range(2):
        d, rep = api.dtx_frame(p, st, tone(1e-3))
        dm.frame(p, ms, tone(1e-3))
        assert d == dm.NONE and st[dm.W_SINCE] == 0xFFFF and same(st, ms)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    L = api.load_library()
    good = dm.default_params()
    for i, (name, bads) in enumerate((("thr", (1.0, 0.5, np.inf, np.nan)), ("floor_up", (0.0, 1.5, np.nan)), ("floor_drift", (0.99, 2.0, np.nan)),
                                      ("floor_min", (0.0, -1.0, np.inf)), ("hangover", (-1, 256, 2.5)), ("smooth", (0.0, 1.01)), ("update_db", (0, 128, 1.5)),
                                      ("max_interval", (-1, 65536, 0.5)), ("order", (-1, 13, 3.5, np.nan)))):
        for v in bads:
            p = good.copy()
            p[i] = v
            with pytest.raises(api.PercepNetError, match=rf"index {i} \({name}\)"):
                api.dtx_params_check(p)
            with pytest.raises(api.PercepNetError, match=rf"index {i} \({name}\)"):
                api.dtx_frame(p, np.zeros(24, U32), np.zeros(80, F32))
    for edge in ((dm.THR, 1.0001), (dm.FLOOR_UP, 1.0), (dm.FLOOR_DRIFT, 1.0), (dm.FLOOR_DRIFT, 1.99), (dm.HANGOVER, 0), (dm.HANGOVER, 255), (dm.UPDATE_DB, 1),
                 (dm.UPDATE_DB, 127), (dm.MAX_INTERVAL, 65535), (dm.ORDER, 0), (dm.ORDER, 12)):
        p = good.copy()
        p[edge[0]] = edge[1]
        api.dtx_params_check(p)
    with pytest.raises(api.PercepNetError, match="a set has 9"):
        api.dtx_params_check(np.zeros(8, F32))
    for n in (0, 79, 81, 400, 481):
        with pytest.raises(api.PercepNetError, match="80, 160, 240, 320 or 480"):
            api.dtx_frame(good, np.zeros(24, U32), np.zeros(n, F32))
    with pytest.raises(api.PercepNetError, match="24 writable"):
        api.dtx_frame(good, np.zeros(23, U32), np.zeros(80, F32))
    st, row, rep, sid = np.zeros(24, U32), np.zeros(80, F32), np.zeros(8, U32), np.zeros(14, np.uint8)
    assert L.pn_dtx_frame(None, st.ctypes.data, row.ctypes.data, 80, rep.ctypes.data) == -1 and b"NULL" in L.pn_last_error()
    assert L.pn_dtx_frame(good.ctypes.data, None, row.ctypes.data, 80, rep.ctypes.data) == -1
    assert L.pn_dtx_frame(good.ctypes.data, st.ctypes.data, None, 80, rep.ctypes.data) == -1
    assert L.pn_dtx_frame(good.ctypes.data, st.ctypes.data, row.ctypes.data, 80, None) == dm.FRAME, "the report is optional"
    assert L.pn_dtx_sid_from_acorr(None, 10, sid.ctypes.data) == -1 and L.pn_dtx_sid_from_acorr(row.ctypes.data, 10, None) == -1
    assert L.pn_dtx_default_params(None) == -1 and L.pn_dtx_params_check(None) == -1
    # the converter's calls refuse a NULL converter before anything else
    for name, args in (("pn_rate_set_stream_dtx", (None, None, 0, None)), ("pn_rate_get_stream_dtx", (None, None)), ("pn_rate_set_dtx_params", (None, good.ctypes.data)),
                       ("pn_rate_get_dtx_params", (None, None)), ("pn_rate_dtx_f32", (None, None, None, 0)), ("pn_rate_dtx_i16", (None, None, None, 0)),
                       ("pn_rate_dtx_g711", (None, None, None, 0)), ("pn_rate_set_dtx_report", (None, 1)), ("pn_rate_read_dtx_report", (None, None)),
                       ("pn_rate_read_dtx_report_dev", (None, None)), ("pn_rate_debug_dtx_state", (None, None))):
        assert getattr(L, name)(*args) == -1 and b"NULL" in L.pn_last_error(), name


def test_cli_refuses_bad_dtx_send_arguments(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "in0.pcm").write_bytes(bytes(1920))
    files = ["in0.pcm", "out0.pcm"]
    for opts, words_ in ((["--dtx-send-hangover", "5"], ("--dtx-send-hangover", "needs --dtx-send")),
                         (["--dtx-send", "--dtx-send-hangover", "256"], ("--dtx-send-hangover", "expected", "[0, 255]")),
                         (["--dtx-send", "--dtx-send-hangover", "-1"], ("--dtx-send-hangover", "expected")),
                         (["--dtx-send", "--dtx-send-hangover", "2.5"], ("--dtx-send-hangover", "expected")),
                         (["--dtx-send", "--dtx-send-hangover", "x"], ("--dtx-send-hangover", "expected")),
                         (["--rate", "8000", "--dtx-send", "--dtx-send-hangover", "3x"], ("--dtx-send-hangover", "expected"))):
        r = subprocess.run([exe] + opts + files, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stderr for w in words_), (opts, r.stderr)
        assert not (tmp_path / "out0.pcm").exists(), opts
    r = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "[--dtx-send [--dtx-send-hangover H]]" in r.stderr


def test_rules_under_sanitizers(tmp_path):
    """tests/c/dtx_sanitize.cpp = pn_dtx_rules.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: rows of exactly n_s floats at every row length, a state of exactly 24 words, a report of exactly 8,
    13 lags, a SID of exactly 14 bytes, the rows no finite arithmetic survives, the counters at their ceilings, the refusals."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "dtx_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "dtx_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
