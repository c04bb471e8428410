"""Output limiter on the rate converter: the host-only surface, no GPU (include/percepnet_hip.h "output limiter"; the rule lives in the
HIP-free percepnet_amd/csrc/pn_lim_rules.h): pn_lim_frame against the numpy model (tests/lim_model.py) bit for bit over sequences of 60
frames, the guarantee |out| <= c on every finite row, the pinned defaults and constants, every refusal, the shape of an attack and the
time line of hold and release — on the model and on the host function alike — the CLI's refusals that need no device, and the rule
under the address and undefined-behaviour sanitizers in a stand-alone program (tests/c/lim_sanitize.cpp).

Bounds.  Every comparison is exact.  The guarantee is the rule's own (pn_lim_rules.h proves it from the monotonicity of rounding).  The
sweep behind its one non-obvious step — after at most one bit down, fl(p * q) <= c — runs 2 x 10^7 peaks over five ceilings.  The time
line is the issue's: a ratio of 2 is 6.02 dB, at +0.5 dB a frame the 13th releasing frame is the first at exactly 1.0.

k = 480 with gl < g0 — an attack whose ramp runs over the whole row because no sample passes the ceiling under the OLD gain — is
reachable with real floats: where p * ulp(q) is under half an ulp of c, the float above q = fl(c / p) still gives fl(p * g0) == c.  The
test searches such a peak and starts from a state whose gain is that float."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import lim_model as lm
from tests.test_agc_host import hostile_rows, same, voice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
D = lm.DEFAULTS
ALL_FLAGS = (lm.ON, lm.ATTACK, lm.HOLDING, lm.RELEASING, lm.ACTIVE, lm.NONFINITE)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def bits(x):
    return np.array([x], F32).view(np.uint32)[0]


def spike_row(c, at, base=0.5, spike=2.0):
    y = np.full(480, F32(base) * F32(c), F32)
    if at is not None:
        y[at] = F32(spike) * F32(c)
    return y


def k480_case():
    """(c, p, g0): gl = fl(c / p) < g0 = the float above it, and fl(p * g0) <= c: the attack whose k is 480"""
    c = F32(1.0)
    for i in range(1, 200000):
        p = np.nextafter(F32(1.9), F32(2.0)) + F32(i) * F32(2.0 ** -23)
        q = lm.needed(p, c)
        g0 = np.nextafter(q, F32(2.0))
        if F32(p * g0) <= c:
            return c, p, g0
    raise AssertionError("no peak with two gains under the ceiling in 200000 candidates")


def sequences():
    """name -> (rows [60, 480], ceiling, params, the state to start from)"""
    h = hostile_rows()
    rng = np.random.default_rng(5200)
    fresh = np.zeros((), lm.STATE_DTYPE)
    seqs = {}
    for rms in (0.02, 0.1, 0.3):
        seqs[f"voice_{rms}"] = (voice(rms, 60), 0.25, D, fresh)
    # bursts: a voice whose level steps up and down, so that attacks land inside holds and inside releases
    lev = np.where((np.arange(60) // 7) % 3 == 1, 6.0, np.where(np.arange(60) % 11 == 5, 9.0, 1.0)).astype(F32)
    seqs["bursts"] = (voice(0.05, 60) * lev[:, None], 0.2, D, fresh)
    seqs["steady_loud"] = (np.tile(voice(0.3, 1), (60, 1)), 0.25, D, fresh)     # the same peak every frame: behind the hold gl == g0, the gain stays
    seqs["noise_at_full_scale"] = ((rng.standard_normal((60, 480)) * 0.5).astype(F32), 1.0, D, fresh)
    seqs["smallest_ceiling"] = (voice(0.1, 60), 1.0 / 1024.0, D, fresh)
    rows = voice(0.2, 60)
    for i, name in enumerate(h):
        rows[5 + 5 * i] = h[name]                                        # one hostile row every five frames, voice between them
    rows[52] = np.full(480, np.finfo(F32).max, F32)                       # leaves a subnormal gain, c / FLT_MAX, behind: two frames of hold, then release
    seqs["hostile"] = (rows, 0.3, D, fresh)
    seqs["hostile_first"] = (np.concatenate([np.stack(list(h.values())), voice(0.3, 60 - len(h))]), 0.5, D, fresh)
    # the attack index at 0, in the middle, at 479; each followed by quiet rows
    c = F32(0.5)
    spikes = np.stack([spike_row(c, None, 0.4)] * 60)
    spikes[3], spikes[20], spikes[40] = spike_row(c, 0), spike_row(c, 300, spike=4.0), spike_row(c, 479, spike=16.0)
    seqs["spikes"] = (spikes, c, D, fresh)
    seqs["edge_params_fast"] = (voice(0.05, 60) * lev[:, None], 0.2, np.array([2.0, 0.0], F32), fresh)
    seqs["edge_params_frozen"] = (voice(0.05, 60) * lev[:, None], 0.2, np.array([1.0, 1000.0], F32), fresh)
    ck, pk, gk = k480_case()
    st = np.zeros((), lm.STATE_DTYPE)
    st["gain"] = gk
    first = np.full(480, F32(0.25), F32)
    first[100] = -pk
    seqs["k480"] = (np.concatenate([first[None], voice(0.1, 59)]), ck, D, st)
    return seqs


def run_host(rows, c, params, st0):
    st = st0.copy()
    out, states, flags, reps = [], [], [], []
    for y in rows:
        o, f, rep = api.lim_frame(params, c, st, y, want_report=True)
        out.append(o); states.append(st.copy()); flags.append(f); reps.append(rep.copy())
    return np.stack(out), np.array(states), flags, np.array(reps)


def run_model(rows, c, params, st0):
    m = lm.Lim(1, params)
    m.set_ceilings([0], [c])
    m.state[0] = st0
    out, states, flags, reps, ks = [], [], [], [], []
    for y in rows:
        out.append(m.frame(y[None])[0])
        states.append(m.state[0].copy()); flags.append(int(m.report[0]["flags"])); reps.append(m.report[0].copy()); ks.append(int(m.k[0]))
    return np.stack(out), np.array(states), flags, np.array(reps), ks


_runs = {}


def runs(name):
    if name not in _runs:
        seq = sequences()[name]
        _runs[name] = (seq, run_host(*seq), run_model(*seq))
    return _runs[name]


def test_constants_and_defaults_are_pinned():
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    for name, val in (("PN_LIM_N_PARAMS", 2), ("PN_LIM_RELEASE", 0), ("PN_LIM_HOLD", 1), ("PN_LIM_REPORT_WORDS", 4), ("PN_LIM_ON", 1), ("PN_LIM_ATTACK", 2),
                      ("PN_LIM_HOLDING", 4), ("PN_LIM_RELEASING", 8), ("PN_LIM_ACTIVE", 16), ("PN_LIM_NONFINITE", 32)):
        assert f"#define {name} {val}\n" in hdr, name
    assert (api.LIM_RELEASE, api.LIM_HOLD) == (lm.RELEASE, lm.HOLD) == (0, 1)
    assert (api.LIM_ON, api.LIM_ATTACK, api.LIM_HOLDING, api.LIM_RELEASING, api.LIM_ACTIVE, api.LIM_NONFINITE) == ALL_FLAGS
    assert api.LIM_N_PARAMS == lm.N_PARAMS == 2 and api.LIM_REPORT_WORDS == 4 and api.LIM_REPORT_DTYPE == lm.REPORT_DTYPE and api.LIM_REPORT_DTYPE.itemsize == 16
    assert api.LIM_STATE_DTYPE == lm.STATE_DTYPE and api.LIM_STATE_DTYPE.itemsize == 16
    d = api.lim_default_params()
    assert same(d, D) and same(d, np.array([1.0592537, 2.0], F32))
    assert d[lm.RELEASE] == api.agc_default_params()[api.AGC_STEP_UP], "the release ratio is the level control's +0.5 dB constant"
    rules = open(os.path.join(ROOT, "percepnet_amd", "csrc", "pn_lim_rules.h")).read()
    assert "#define PN_LIM_STATE_BYTES 16\n" in rules and "The guarantee" in rules and "pn_agc_apply_host" in rules
    api.lim_params_check(d)
    assert lm.params_ok(D) == -1


@pytest.mark.parametrize("name", sorted(sequences()))
def test_host_frames_are_the_models_bit_for_bit(name):
    _, host, model = runs(name)
    for t in range(60):
        assert same(host[0][t], model[0][t]), f"{name}: the row of frame {t}"
        assert host[1][t].tobytes() == model[1][t].tobytes(), f"{name}: the state after frame {t}: {host[1][t]} != {model[1][t]}"
        assert host[2][t] == model[2][t], f"{name}: the flags of frame {t}"
        assert host[3][t].tobytes() == model[3][t].tobytes(), f"{name}: the report of frame {t}: {host[3][t]} != {model[3][t]}"
    assert host[1]["spare"].max() == 0


def test_the_sequences_reach_every_flag_both_envelopes_and_every_attack_index():
    seen, ks = set(), set()
    for name in sequences():
        _, host, model = runs(name)
        seen |= set(host[2])
        ks |= {k for k in model[4] if k >= 0}
    for flag in ALL_FLAGS:
        assert any(f & flag for f in seen), flag
    assert all(f & lm.ON for f in seen) and lm.ON in seen, "every frame is ON; some frame is nothing else (unity)"
    assert (lm.ON | lm.ACTIVE) in seen, "a releasing stream that a loud row keeps at its gain: neither holding nor rising"
    assert {0, 300, 479} <= ks and any(0 < k < 479 for k in ks)
    # k = 480 with gl < g0: reached with real floats (the module's docstring)
    (rows, c, _, st0), host, model = runs("k480")
    assert model[4][0] == 480 and host[2][0] == lm.ON | lm.ATTACK | lm.ACTIVE
    g0, gl = st0["gain"], host[1][0]["gain"]
    assert gl < g0 and bits(g0) - bits(gl) == 1
    assert same(host[0][0][:3], rows[0][:3] * (g0 + (np.arange(3, dtype=F32) / F32(480.0)) * (gl - g0))), "the ramp runs over the whole row: w_j = j / 480"
    assert host[0][0][100] == -c, "p * g for a gain between the two lands on the ceiling"


@pytest.mark.parametrize("name", sorted(sequences()))
def test_every_finite_row_stays_under_the_ceiling(name):
    (rows, c, params, _), host, model = runs(name)
    c = F32(c)
    finite = 0
    for out, states, flags, *_ in (host, model):
        for t in range(60):
            if flags[t] & lm.NONFINITE:
                assert same(out[t], rows[t]), f"frame {t}: a non-finite row is not touched"
                continue
            finite += 1
            a = np.abs(out[t])
            assert (a[~np.isnan(a)] <= c).all(), f"frame {t}: max |out| {np.nanmax(a)} > {c}"
            assert np.array_equal(np.isnan(out[t]), np.isnan(rows[t])), "a NaN sample stays one and makes no other"
        g = states["gain"]
        assert (g > 0).all() and (g <= 1).all() and np.isfinite(g).all(), "the gain state lies in (0, 1]"
    assert finite >= 100


def test_one_bit_down_is_enough_over_2e7_peaks():
    """fl(p * q) <= c for q = fl(c / p) stepped down once where needed: 4 x 10^6 peaks per ceiling — a dense run of consecutive floats
    right above the ceiling, then geometric steps up to FLT_MAX — over five ceilings; the one-bit step is taken somewhere"""
    n, stepped = 4_000_000, 0
    with np.errstate(all="ignore"):
        for c in (F32(1.0 / 1024.0), F32(0.1), F32(0.5), F32(32767.0 / 32768.0), F32(1.0)):
            dense = (np.arange(1, n // 2 + 1, dtype=np.uint32) + bits(c)).view(F32)
            wide = (c * np.exp(np.linspace(np.log(1.0 + 1e-6), np.log(float(lm.FLT_MAX) / float(c)) - 1e-3, n // 2))).astype(F32)
            p = np.concatenate([dense, wide])
            p = p[(p > c) & (p <= lm.FLT_MAX)]
            q = (c / p).astype(F32)
            over = (p * q).astype(F32) > c
            stepped += int(over.sum())
            q = np.where(over, (q.view(np.uint32) - np.uint32(1)).view(F32), q)
            assert ((p * q).astype(F32) <= c).all() and (q > 0).all() and (q < 1).all(), c
            for i in (0, 1, len(p) // 3, len(p) - 1):
                assert bits(lm.needed(p[i], c)) == bits(q[i]), "the model's scalar statement is this one"
    assert stepped > 0, "the sweep met peaks that need the step"


def test_unity_gain_keeps_the_rows_bits():
    c = F32(0.25)
    y = voice(0.05, 1)[0].copy()
    y[17], y[18], y[19] = c, -0.0, -c
    y[20:22] = np.array([0x7FC12345, 0xFFC00001], np.uint32).view(F32)          # NaN payloads
    for run in ("host", "model"):
        st = np.zeros((), lm.STATE_DTYPE)
        if run == "host":
            o, f, rep = api.lim_frame(D, c, st, y, want_report=True)
        else:
            m = lm.Lim(1)
            m.set_ceilings([0], [c])
            o, f, rep, st = m.frame(y[None])[0], int(m.report[0]["flags"]), m.report[0], m.state[0]
        assert f == lm.ON and same(o, y) and st["gain"] == 1.0 and st["hold"] == 0 and st["limited"] == 0
        assert rep["gain"] == 1.0 and rep["peak"] == c and rep["limited"] == 0
    # not limited at all: the row is copied and the state is not even read as a state
    for c0 in (0.0, -0.0):
        st = np.zeros((), api.LIM_STATE_DTYPE)
        st["gain"], st["hold"], st["limited"] = 0.3, 5, 9
        before = st.copy()
        o, f, rep = api.lim_frame(D, c0, st, hostile_rows()["nan_and_inf_inside"], want_report=True)
        assert f == 0 and same(o, hostile_rows()["nan_and_inf_inside"]) and st.tobytes() == before.tobytes()
        assert rep.tobytes() == np.array((1.0, 0.0, 0, 0), lm.REPORT_DTYPE).tobytes()


@pytest.mark.parametrize("who", ("model", "host"))
@pytest.mark.parametrize("g0", (1.0, 0.75))
def test_attack_shape(who, g0):
    c = F32(0.5)
    st0 = np.zeros((), lm.STATE_DTYPE)
    st0["gain"] = g0
    run = run_model if who == "model" else run_host
    y = spike_row(c, 300)
    out, states, flags, *_ = run(y[None], c, D, st0)
    o = out[0]
    assert flags[0] == lm.ON | lm.ATTACK | lm.ACTIVE and states[0]["gain"] == 0.5 and states[0]["hold"] == 2 and states[0]["limited"] == 1
    assert o[0] == y[0] * F32(g0), "the gain leaves the previous row's end value"
    gain = o / y
    assert (np.diff(gain[:301]) <= 0).all() and gain[299] > gain[300], "the gain falls monotonically over [0, 300]"
    assert o[300] <= c and o[300] == c, "2c * 0.5 is exact: the spike lands on the ceiling"
    assert same(o[300:], y[300:] * F32(0.5)), "flat behind the sample that needed it"
    y = spike_row(c, 0)
    out, states, flags, *_ = run(y[None], c, D, st0)
    assert same(out[0], y * F32(0.5)) and flags[0] == lm.ON | lm.ATTACK | lm.ACTIVE, "the spike at index 0: the whole row at gl, the one case of a step"


@pytest.mark.parametrize("who", ("model", "host"))
def test_time_line_of_hold_and_release(who):
    c = F32(0.5)
    H = int(D[lm.HOLD])
    quiet = spike_row(c, None, 0.4)
    rows = np.stack([np.full(480, 2 * c, F32)] + [quiet] * 24)
    run = run_model if who == "model" else run_host
    out, states, flags, *_ = run(rows, c, D, np.zeros((), lm.STATE_DTYPE))
    g = states["gain"]
    assert flags[0] & lm.ATTACK and g[0] == 0.5
    for t in range(1, 1 + H):
        assert g[t] == 0.5 and flags[t] == lm.ON | lm.HOLDING | lm.ACTIVE and same(out[t], quiet * F32(0.5)), t
    for i in range(1, 14):                                               # the i-th releasing frame
        t = H + i
        want = np.fmin(F32(g[t - 1] * D[lm.RELEASE]), F32(1.0))
        assert g[t] == want and flags[t] == lm.ON | lm.RELEASING | lm.ACTIVE, (t, g[t])
        assert (g[t] == 1.0) == (i == 13), f"exactly 1.0 from the 13th releasing frame on (frame {t}: {g[t]})"
        assert out[t][0] > out[t - 1][0] and np.abs(out[t]).max() <= c
    for t in range(H + 14, 25):
        assert flags[t] == lm.ON and same(out[t], quiet) and states[t]["limited"] == states[H + 13]["limited"] == 1 + H + 13, t
    # a second burst inside the hold arms the hold again
    rows = np.stack([np.full(480, 2 * c, F32), quiet, np.full(480, 4 * c, F32), quiet, quiet, quiet])
    out, states, flags, *_ = run(rows, c, D, np.zeros((), lm.STATE_DTYPE))
    assert states["hold"].tolist() == [2, 1, 2, 1, 0, 0] and states["gain"][:5].tolist() == [0.5, 0.5, 0.25, 0.25, 0.25]
    assert flags[2] & lm.ATTACK and flags[3] & lm.HOLDING and flags[4] & lm.HOLDING and flags[5] & lm.RELEASING


def test_hostile_rows_never_leave_a_bad_state_and_the_count_saturates():
    for name in ("hostile", "hostile_first"):
        (rows, c, _, _), host, _ = runs(name)
        out, states, flags, reps = host
        assert (states["gain"] > 0).all() and (states["gain"] <= 1).all() and (states["spare"] == 0).all()
        nonfinite = [t for t in range(60) if flags[t] & lm.NONFINITE]
        assert nonfinite, name
        for t in nonfinite:
            assert same(out[t], rows[t]) and np.isinf(reps[t]["peak"])
            if t > 0:
                assert states[t].tobytes() == states[t - 1].tobytes(), "a non-finite row touches no state"
        # a row of 3e38 or FLT_MAX leaves the gain at c / p, about 1e-39: the rule brings it back by R a frame and no faster, so the
        # stream stays silent for some 1500 frames; what is checked here is that the gain is live and on its way
        assert states["gain"][59] > states["gain"].min() and flags[59] & lm.RELEASING, "behind the hostile rows the gain rises again"
    st = np.zeros((), api.LIM_STATE_DTYPE)
    st["gain"], st["limited"] = 0.5, 0xFFFFFFFE
    for want in (0xFFFFFFFF, 0xFFFFFFFF):
        api.lim_frame(D, 0.5, st, voice(0.05, 1)[0])
        assert st["limited"] == want
    m = lm.Lim(1)
    m.set_ceilings([0], [0.5])
    m.state[0] = (0.5, 0, 0xFFFFFFFF, 0)
    m.frame(voice(0.05, 1))
    assert m.state["limited"][0] == 0xFFFFFFFF


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def outside(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


@pytest.mark.parametrize("i,lo,hi", ((0, 1.0, 2.0), (1, 0.0, 1000.0)))
def test_every_parameter_at_both_edges_and_one_step_outside(i, lo, hi):
    st = np.zeros((), api.LIM_STATE_DTYPE)
    y = voice(0.5, 1)[0]

    def refused(p):
        assert lm.params_ok(p) == i
        with pytest.raises(api.PercepNetError, match=rf"index {i}\b"):
            api.lim_params_check(p)
        with pytest.raises(api.PercepNetError, match=rf"index {i}\b"):
            api.lim_frame(p, 0.1, st, y)
        assert st.tobytes() == bytes(16)

    for edge in (lo, hi):
        p = D.copy()
        p[i] = edge
        api.lim_params_check(p)
        assert lm.params_ok(p) == -1
    for bad in (outside(hi, True), outside(lo, False), np.nan, np.inf, -np.inf, hi + 1):
        p = D.copy()
        p[i] = bad
        refused(p)
    if i == lm.HOLD:
        for bad in (0.5, outside(1.0, True), 999.5):
            p = D.copy()
            p[i] = bad
            refused(p)
        p = D.copy()
        p[i] = F32(-0.0)
        api.lim_params_check(p)


def test_the_first_bad_parameter_is_named_and_bad_ceilings_are_refused(lib):
    with pytest.raises(api.PercepNetError, match=r"index 0 \(release\)"):
        api.lim_params_check(np.array([3.0, np.nan], F32))
    with pytest.raises(api.PercepNetError, match=r"index 1 \(hold\)"):
        api.lim_params_check(np.array([1.5, 2.5], F32))
    with pytest.raises(api.PercepNetError, match="2"):
        api.lim_params_check(D[:1])
    st = np.zeros((), api.LIM_STATE_DTYPE)
    y = voice(0.5, 1)[0]
    lo = F32(1.0 / 1024.0)
    for bad in (np.nan, outside(1.0, True), 2.0, -0.5, np.inf, -np.inf, outside(lo, False), outside(0.0, True), outside(0.0, False), -lo):
        assert not lm.ceiling_ok(bad)
        with pytest.raises(api.PercepNetError, match="limiter ceiling"):
            api.lim_frame(D, bad, st, y)
        t = np.array([0.1, 0.0, bad, np.nan], F32)
        assert lib.pn_rate_limiter_ceilings_check(t.ctypes.data, 4) == -1 and "index 2" in api._err(lib)
    good = np.array([0.0, -0.0, 1.0, lo, 0.5], F32)
    assert all(lm.ceiling_ok(v) for v in good)
    assert lib.pn_rate_limiter_ceilings_check(good.ctypes.data, 5) == 0 and lib.pn_rate_limiter_ceilings_check(None, 0) == 0
    assert lib.pn_rate_limiter_ceilings_check(None, 1) == -1 and lib.pn_rate_limiter_ceilings_check(good.ctypes.data, -1) == -1
    with pytest.raises(api.PercepNetError, match="480"):
        api.lim_frame(D, 0.1, st, y[:479])
    assert lib.pn_lim_frame(None, 0.1, st.ctypes.data, y.ctypes.data, y.ctypes.data, None) == -1
    assert st.tobytes() == bytes(16)


# ---- CLI -----------------------------------------------------------------------------------------------------------------------
def test_cli_refuses_bad_limiter_options(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "in0.pcm").write_bytes(bytes(1920))
    files = ["in0.pcm", "out0.pcm"]
    for opts, words in ((["--limiter", "0"], ("--limiter", "[1/1024, 1]")), (["--limiter", "1.5"], ("--limiter", "[1/1024, 1]")), (["--limiter", "nan"], ("--limiter", "[1/1024, 1]")),
                        (["--limiter", "0.5x"], ("--limiter", "[1/1024, 1]")), (["--limiter", "-0.5"], ("--limiter", "[1/1024, 1]")),
                        (["--limiter", "0.0009"], ("--limiter", "[1/1024, 1]")),
                        (["--limiter-hold", "4"], ("--limiter-hold", "needs --limiter")), (["--limiter", "0.5", "--limiter-hold", "1.5"], ("--limiter-hold", "[0, 1000]")),
                        (["--limiter", "0.5", "--limiter-hold", "1001"], ("--limiter-hold", "[0, 1000]")), (["--limiter", "0.5", "--limiter-hold", "-1"], ("--limiter-hold", "[0, 1000]")),
                        (["--limiter", "0.5", "--limiter-hold", "x"], ("--limiter-hold", "[0, 1000]"))):
        run = subprocess.run([exe] + opts + files, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and all(w in run.stderr for w in words), (opts, run.stderr)
        assert not (tmp_path / "out0.pcm").exists(), opts
    run = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "[--limiter CEIL [--limiter-hold H]]" in run.stderr and "[--agc RMS [--agc-max-gain G]]" in run.stderr


def test_rules_under_sanitizers(tmp_path):
    """tests/c/lim_sanitize.cpp = pn_lim_rules.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: whole frames over rows, states and reports of exactly 480 floats and 4 words, attacks at k = 0, 300
    and 479, hold and release, the hostile rows, every parameter's edges, the ceiling list at its exact length."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "lim_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "lim_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
