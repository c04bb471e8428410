"""Automatic level control on the rate converter: the host-only surface, no GPU (include/percepnet_hip.h "automatic level control"; the rule
lives in the HIP-free percepnet_amd/csrc/pn_agc_rules.h): pn_agc_frame against the numpy model (tests/agc_model.py) bit for bit over
sequences of 60 frames, the pinned defaults and constants, every refusal, the behaviour of the rule — on the model and on the host
function alike — the CLI's refusals that need no device, and the rule under the address and undefined-behaviour sanitizers in a
stand-alone program (tests/c/agc_sanitize.cpp).

Bounds.  The convergence bound, output RMS within 1 dB of the target at frame 100, is the issue's; the model measures +0.34 dB (the
gain is sqrt(T^2 480 / lev) with lev the smoothed energy of the frames BEFORE the gain moved, and attack outweighs release, so the
level settles a little under the loudest frames' energy).  "Stationary" is taken at the scale the rule works at: a sound whose
10 ms frames have (nearly) equal energies.  A frame holds 1.3 periods of 130 Hz, so six harmonics in PULSE-like phase alignment
(amplitude 1 / k, phase k: crest factor 2.8) put one pulse into some frames and two into others; their frame energies spread from
0.83 to 1.35 of the mean, the tracker — attack 0.5 against release 0.05 — rides the loud frames, and the rule as stated then leaves the
output at -1.75 dB at frame 100 (-0.95 dB over the ten-frame pattern).  That is a property of the rule, measured on the model, and not
what this test is about; the test signal has Schroeder's phases (crest factor 1.9, frame energies within 9 % of their mean) and
measures -0.57 dB at frame 100.  The slew bound is the rule's own: g1 lies in [g0 step_down, g0 step_up]
as float32 products, so the comparison is exact, no tolerance.  Clipping: |out * 32768| >= 32768 for no sample whose row's peak is at
most c / Gmin — the limiter's guarantee, exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import agc_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
D = am.DEFAULTS


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def voice(rms, frames, f0=130.0, start=0):
    """[frames, 480]: a stationary six-harmonic sound scaled to the RMS `rms`: equal amplitudes and Schroeder's phases -pi k (k - 1) / 6,
    the construction with a flat envelope, so that the energies of its 10 ms frames stay within 9 % of their mean (see the module's docstring)"""
    t = np.arange(start * 480, (start + frames) * 480) / 48000.0
    v = sum(np.cos(2 * np.pi * k * f0 * t - np.pi * k * (k - 1) / 6.0) for k in range(1, 7))
    return (v * (rms / np.sqrt(np.mean(v ** 2)))).astype(F32).reshape(frames, 480)


def hostile_rows():
    """name -> one row of 480: what a frame must survive"""
    sq = np.where(np.arange(480) % 96 < 48, 1.0, -1.0).astype(F32)
    at_c = voice(0.2, 1)[0].copy()
    at_c[137] = D[am.CEILING]                                         # with a fresh gain of 1: p * m == c, NOT above it
    mixed = voice(0.1, 1)[0].copy()
    mixed[5], mixed[200] = np.nan, -np.inf
    return {"nan": np.full(480, np.nan, F32), "inf": np.full(480, np.inf, F32), "3e38": np.full(480, 3e38, F32), "zeros": np.zeros(480, F32),
            "-0.0": np.full(480, -0.0, F32), "subnormal": np.full(480, 1e-41, F32), "square": sq, "at_ceiling": at_c, "nan_and_inf_inside": mixed,
            "one_nan": np.where(np.arange(480) == 7, np.nan, voice(0.05, 1)[0]).astype(F32)}


def sequences():
    """name -> (rows [60, 480], concealed frames, target, params)"""
    h = hostile_rows()
    rng = np.random.default_rng(4100)
    seqs = {}
    for rms in (0.005, 0.02, 0.1, 0.5):
        seqs[f"voice_{rms}"] = (voice(rms, 60), (), 0.1, D)
    v = voice(0.05, 60)
    rows = v.copy()
    for i, name in enumerate(h):
        rows[5 + 5 * i] = h[name]                                        # one hostile row every five frames, voice between them
    seqs["hostile"] = (rows, (), 0.1, D)
    seqs["hostile_first"] = (np.concatenate([np.stack(list(h.values())), voice(0.3, 60 - len(h))]), (), 0.25, D)
    seqs["at_ceiling_first"] = (np.concatenate([h["at_ceiling"][None], voice(0.2, 59, start=1)]), (), 0.2, D)
    step_rows = voice(0.01, 60)
    step_rows[30:] = voice(0.6, 30, start=30)                           # a 60x step in level
    seqs["step_60x"] = (step_rows, (), 0.1, D)
    pause = voice(0.1, 60)
    pause[20:40] = (rng.standard_normal((20, 480)) * 1e-4).astype(F32)
    seqs["pause"] = (pause, (), 0.1, D)
    seqs["concealed"] = (voice(0.02, 60) * np.linspace(1, 8, 60, dtype=F32)[:, None], (0, 17, 18, 19, 41), 0.1, D)
    seqs["noise_loud_target"] = ((rng.standard_normal((60, 480)) * 0.3).astype(F32), (), 1.0, D)
    p2 = D.copy()
    p2[[am.MAX_GAIN, am.MIN_GAIN, am.GATE_RMS, am.ATTACK, am.RELEASE, am.STEP_UP, am.STEP_DOWN, am.CEILING]] = (1024, 1 / 1024, 0, 1, 1, 2, 0.5, 0.5)
    seqs["edge_params"] = (voice(0.0005, 60) * np.where(np.arange(60) % 7 == 3, 900, 1).astype(F32)[:, None], (), 1.0, p2)
    p3 = D.copy()
    p3[[am.MAX_GAIN, am.MIN_GAIN]] = 1.0
    seqs["unity"] = (voice(0.3, 60), (), 0.1, p3)
    return seqs


def run_host(rows, concealed, target, params):
    st = np.zeros((), api.AGC_STATE_DTYPE)
    out, states, flags = [], [], []
    for t, y in enumerate(rows):
        o, f = api.agc_frame(params, target, st, y, concealed=t in concealed)
        out.append(o); states.append(st.copy()); flags.append(f)
    return np.stack(out), np.array(states), flags


def run_model(rows, concealed, target, params):
    m = am.Agc(1, params)
    m.set_targets([0], [target])
    out, states, flags, peaks = [], [], [], []
    for t, y in enumerate(rows):
        out.append(m.frame(y[None], concealed=(0,) if t in concealed else ())[0])
        states.append(m.state[0].copy()); flags.append(int(m.report[0]["flags"])); peaks.append(m.report[0]["peak"])
    return np.stack(out), np.array(states), flags


_runs = {}


def runs(name):
    if name not in _runs:
        seq = sequences()[name]
        _runs[name] = (seq, run_host(*seq), run_model(*seq))
    return _runs[name]


def test_constants_and_defaults_are_pinned():
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    for name, val in (("PN_AGC_N_PARAMS", 8), ("PN_AGC_MAX_GAIN", 0), ("PN_AGC_MIN_GAIN", 1), ("PN_AGC_GATE_RMS", 2), ("PN_AGC_ATTACK", 3), ("PN_AGC_RELEASE", 4),
                      ("PN_AGC_STEP_UP", 5), ("PN_AGC_STEP_DOWN", 6), ("PN_AGC_CEILING", 7), ("PN_AGC_REPORT_WORDS", 4), ("PN_AGC_ON", 1), ("PN_AGC_ADAPTED", 2),
                      ("PN_AGC_LIMITED", 4), ("PN_AGC_AT_MAX", 8), ("PN_AGC_AT_MIN", 16), ("PN_AGC_HELD_LOST", 32)):
        assert f"#define {name} {val}\n" in hdr, name
    assert (api.AGC_MAX_GAIN, api.AGC_MIN_GAIN, api.AGC_GATE_RMS, api.AGC_ATTACK, api.AGC_RELEASE, api.AGC_STEP_UP, api.AGC_STEP_DOWN, api.AGC_CEILING) == tuple(range(8))
    assert (api.AGC_ON, api.AGC_ADAPTED, api.AGC_LIMITED, api.AGC_AT_MAX, api.AGC_AT_MIN, api.AGC_HELD_LOST) == (am.ON, am.ADAPTED, am.LIMITED, am.AT_MAX, am.AT_MIN, am.HELD_LOST)
    assert api.AGC_N_PARAMS == am.N_PARAMS == 8 and api.AGC_REPORT_WORDS == 4 and api.AGC_REPORT_DTYPE == am.REPORT_DTYPE and api.AGC_REPORT_DTYPE.itemsize == 16
    assert api.AGC_STATE_DTYPE == am.STATE_DTYPE and api.AGC_STATE_DTYPE.itemsize == 16
    d = api.agc_default_params()
    assert same(d, D) and same(d, np.array([16.0, 0.125, 0.001, 0.5, 0.05, 1.0592537, 0.8912509, 0.999969482421875], F32))
    assert d[am.CEILING] == F32(32767.0 / 32768.0) and abs(20 * np.log10(d[am.STEP_UP]) - 0.5) < 1e-6 and abs(20 * np.log10(d[am.STEP_DOWN]) + 1.0) < 1e-6
    rules = open(os.path.join(ROOT, "percepnet_amd", "csrc", "pn_agc_rules.h")).read()
    assert "#define PN_AGC_STATE_BYTES 16\n" in rules and "beyond rescue" in rules, "the state's size and the rows the limiter cannot save are stated in the rules header"
    api.agc_params_check(d)
    assert am.params_ok(D) == -1


@pytest.mark.parametrize("name", sorted(sequences()))
def test_host_frames_are_the_models_bit_for_bit(name):
    (rows, concealed, target, params), host, model = runs(name)
    for t in range(60):
        assert same(host[0][t], model[0][t]), f"{name}: the row of frame {t}"
        assert host[1][t].tobytes() == model[1][t].tobytes(), f"{name}: the state after frame {t}: {host[1][t]} != {model[1][t]}"
        assert host[2][t] == model[2][t], f"{name}: the flags of frame {t}"
    assert host[1]["spare"].max() == 0


def test_the_sequences_reach_every_flag_and_every_branch():
    seen = set()
    for name in sequences():
        seen |= set(runs(name)[1][2])
    for flag in (am.ON, am.ADAPTED, am.LIMITED, am.AT_MAX, am.AT_MIN, am.HELD_LOST):
        assert any(f & flag for f in seen), flag
    assert all(f & am.ON for f in seen)
    assert am.ON in seen, "a frame that holds"
    # the row with its peak exactly at the ceiling under a fresh gain is not limited; one float32 step above, it is
    (rows, _, target, params), host, _ = runs("at_ceiling_first")
    assert not host[2][0] & am.LIMITED
    up = rows[0].copy()
    up[137] = np.nextafter(D[am.CEILING], F32(2))
    st = np.zeros((), api.AGC_STATE_DTYPE)
    _, f = api.agc_frame(params, target, st, up)
    assert f & am.LIMITED
    # a concealed frame holds level, gain and count
    (_, concealed, _, _), host, _ = runs("concealed")
    for t in concealed:
        assert host[2][t] == am.ON | am.HELD_LOST or host[2][t] == am.ON | am.HELD_LOST | am.LIMITED
        if t > 0:
            assert host[1][t]["level"] == host[1][t - 1]["level"] and host[1][t]["adapted"] == host[1][t - 1]["adapted"]


def test_a_stream_that_is_not_levelled_keeps_row_and_state():
    y = hostile_rows()["nan_and_inf_inside"]
    for T in (0.0, -0.0):
        st = np.zeros((), api.AGC_STATE_DTYPE)
        st["level"], st["gain"], st["adapted"] = 3.0, 2.0, 9
        before = st.copy()
        o, f = api.agc_frame(D, T, st, y)
        assert f == 0 and same(o, y) and st.tobytes() == before.tobytes()
    m = am.Agc(2)
    m.set_targets([1], [0.1])
    out = m.frame(np.stack([y, voice(0.1, 1)[0]]))
    assert same(out[0], y) and m.report[0].tolist() == (1.0, 0.0, 0, 0.0) and not np.signbit(m.report[0]["level"]) and m.state[0].tobytes() == bytes(16)
    assert m.report[1]["flags"] == am.ON | am.ADAPTED


def test_unity_gains_keep_the_rows_bits():
    (rows, _, _, _), host, model = runs("unity")
    assert same(host[0], rows) and same(model[0], rows), "Gmax = Gmin = 1 and a peak under the ceiling: g0' == g1' == 1"
    z = np.full(480, -0.0, F32)
    st = np.zeros((), api.AGC_STATE_DTYPE)
    o, _ = api.agc_frame(D, 0.1, st, z)
    assert same(o, z), "-0.0 stays -0.0"


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def outside(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


@pytest.mark.parametrize("i", range(8))
def test_every_parameter_at_both_edges_and_one_step_outside(i):
    lo, hi, open_lo = am.RANGES[i]
    st = np.zeros((), api.AGC_STATE_DTYPE)
    y = voice(0.1, 1)[0]

    def refused(p):
        assert am.params_ok(p) == i
        with pytest.raises(api.PercepNetError, match=rf"index {i}\b"):
            api.agc_params_check(p)
        with pytest.raises(api.PercepNetError, match=rf"index {i}\b"):
            api.agc_frame(p, 0.1, st, y)
        assert st.tobytes() == bytes(16)

    p = D.copy()
    p[i] = hi
    api.agc_params_check(p)
    assert am.params_ok(p) == -1
    p[i] = outside(hi, True)
    refused(p)
    p[i] = lo
    if open_lo:
        refused(p)
        p[i] = outside(lo, True)                                         # the smallest subnormal: inside an open end
        api.agc_params_check(p)
        p[i] = F32(-0.0)
        refused(p)
    else:
        api.agc_params_check(p)
        assert am.params_ok(p) == -1
        p[i] = outside(lo, False)
        refused(p)
    for bad in (np.nan, np.inf, -np.inf):
        p[i] = bad
        refused(p)


def test_the_first_bad_parameter_is_named_and_bad_targets_are_refused(lib):
    p = D.copy()
    p[[2, 5]] = (np.nan, 3.0)
    with pytest.raises(api.PercepNetError, match=r"index 2 \(gate_rms\)"):
        api.agc_params_check(p)
    with pytest.raises(api.PercepNetError, match="8"):
        api.agc_params_check(D[:7])
    st = np.zeros((), api.AGC_STATE_DTYPE)
    y = voice(0.1, 1)[0]
    for bad in (np.nan, outside(1.0, True), 2.0, -0.5, np.inf, -np.inf, outside(0.0, False)):
        with pytest.raises(api.PercepNetError, match="AGC target"):
            api.agc_frame(D, bad, st, y)
        t = np.array([0.1, 0.0, bad, np.nan], F32)
        assert lib.pn_rate_agc_targets_check(t.ctypes.data, 4) == -1 and "index 2" in api._err(lib)
    good = np.array([0.0, -0.0, 1.0, outside(0.0, True), 0.5], F32)
    assert lib.pn_rate_agc_targets_check(good.ctypes.data, 5) == 0 and lib.pn_rate_agc_targets_check(None, 0) == 0
    assert lib.pn_rate_agc_targets_check(None, 1) == -1 and lib.pn_rate_agc_targets_check(good.ctypes.data, -1) == -1
    with pytest.raises(api.PercepNetError, match="480"):
        api.agc_frame(D, 0.1, st, y[:479])
    assert lib.pn_agc_frame(None, 0.1, st.ctypes.data, y.ctypes.data, y.ctypes.data, 0) == -1
    assert st.tobytes() == bytes(16)


# ---- behaviour, on the model and on the host function ------------------------------------------------------------------------------
@pytest.mark.parametrize("who", ("model", "host"))
@pytest.mark.parametrize("rms", (0.02, 0.1, 0.5))
def test_a_stationary_voice_settles_within_1_db_of_the_target(rms, who):
    rows = voice(rms, 130)
    out, states, flags = (run_model if who == "model" else run_host)(rows, (), 0.1, D)
    got = np.sqrt(np.mean(out[100].astype(np.float64) ** 2))
    db = 20 * np.log10(got / 0.1)
    at50 = np.sqrt(np.mean(out[50].astype(np.float64) ** 2))
    print(f"{who} input {rms}: output RMS {got:.4f} ({db:+.2f} dB) at frame 100, {at50:.4f} at frame 50, gains {states['gain'][100:110].tolist()}")
    assert abs(db) <= 1.0
    assert all(f == am.ON | am.ADAPTED for f in flags[100:]), "settled: voiced, no clamp, no limiter"


@pytest.mark.parametrize("who", ("model", "host"))
def test_a_quiet_voice_sits_at_max_gain(who):
    rows = voice(0.005, 110)
    out, states, flags = (run_model if who == "model" else run_host)(rows, (), 0.1, D)
    assert states["gain"][100] == D[am.MAX_GAIN] and flags[100] & am.AT_MAX
    assert same(out[100], rows[100] * F32(16.0)), "g0' == g1' == 16: the row times sixteen, exactly"


@pytest.mark.parametrize("name", sorted(sequences()))
def test_slew_range_and_no_clipping(name):
    (rows, concealed, target, params), host, model = runs(name)
    Gmax, Gmin, c = params[am.MAX_GAIN], params[am.MIN_GAIN], params[am.CEILING]
    for out, states, flags in (host, model):
        g = np.concatenate([[F32(1.0)], states["gain"]]).astype(F32)
        assert (g[1:] >= Gmin).all() and (g[1:] <= max(Gmax, F32(1.0))).all(), "the gain state lies in [Gmin, Gmax]"
        assert (states["gain"].view(np.uint32) != 0).all() and np.isfinite(states["level"]).all() and (states["level"] >= 0).all(), "a live state"
        for t in range(60):
            if not flags[t] & am.LIMITED:
                assert g[t] * params[am.STEP_DOWN] <= g[t + 1] <= g[t] * params[am.STEP_UP], f"frame {t}: {g[t]} -> {g[t + 1]}"
            else:
                assert g[t + 1] <= g[t] * params[am.STEP_UP]
            pk = am.peak(rows[t][None])[0]
            if pk <= c / Gmin:
                with np.errstate(all="ignore"):
                    assert not (np.abs(out[t] * F32(32768.0)) >= 32768).any(), f"frame {t} clips (peak {pk})"


@pytest.mark.parametrize("who", ("model", "host"))
def test_a_60x_step_is_caught_in_the_same_frame_and_the_gain_then_falls_at_step_down(who):
    (rows, _, _, params), host, model = runs("step_60x")
    out, states, flags = model if who == "model" else host
    assert flags[30] & am.LIMITED and not any(f & am.LIMITED for f in flags[:30])
    assert 0.99 < np.abs(out[30]).max() < 1.0, "the row's peak lands at the ceiling (to the rounding of c / p and of the product), under full scale"
    g = states["gain"]
    falling = [t for t in range(31, 60) if g[t] == F32(g[t - 1] * D[am.STEP_DOWN])]
    assert len(falling) >= 5, "behind the limiter the gain comes down by step_down a frame"


@pytest.mark.parametrize("who", ("model", "host"))
def test_a_pause_holds_the_gain_bits(who):
    _, host, model = runs("pause")
    out, states, flags = model if who == "model" else host
    g = states["gain"].view(np.uint32)
    assert len(set(g[19:40].tolist())) == 1 and all(f == am.ON for f in flags[20:40])
    assert states["adapted"][39] == states["adapted"][19] == 20 and states["level"][39] == states["level"][19]
    assert states["adapted"][59] == 40


def test_hostile_rows_never_leave_a_stuck_state():
    (rows, _, _, params), host, _ = runs("hostile_first")
    out, states, flags = host
    assert states["gain"][59] != states["gain"][len(hostile_rows())], "behind the hostile rows the gain still adapts"
    assert flags[59] & am.ADAPTED and states["adapted"][59] > states["adapted"][len(hostile_rows())] and np.isfinite(out[59]).all()


def test_the_adapted_count_saturates():
    st = np.zeros((), api.AGC_STATE_DTYPE)
    st["adapted"] = 0xFFFFFFFE
    y = voice(0.1, 1)[0]
    for want in (0xFFFFFFFF, 0xFFFFFFFF):
        api.agc_frame(D, 0.1, st, y)
        assert st["adapted"] == want
    m = am.Agc(1)
    m.set_targets([0], [0.1])
    m.state["adapted"] = 0xFFFFFFFF
    m.frame(y[None])
    assert m.state["adapted"][0] == 0xFFFFFFFF


# ---- CLI -----------------------------------------------------------------------------------------------------------------------
def test_cli_refuses_bad_agc_options(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "in0.pcm").write_bytes(bytes(1920))
    files = ["in0.pcm", "out0.pcm"]
    for opts, words in ((["--agc", "0"], ("--agc", "(0, 1]")), (["--agc", "1.5"], ("--agc", "(0, 1]")), (["--agc", "nan"], ("--agc", "(0, 1]")),
                        (["--agc", "0.1x"], ("--agc", "(0, 1]")), (["--agc", "-0.1"], ("--agc", "(0, 1]")),
                        (["--agc-max-gain", "4"], ("--agc-max-gain", "needs --agc")), (["--agc", "0.1", "--agc-max-gain", "0.5"], ("--agc-max-gain", "[1, 1024]")),
                        (["--agc", "0.1", "--agc-max-gain", "2000"], ("--agc-max-gain", "[1, 1024]"))):
        run = subprocess.run([exe] + opts + files, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and all(w in run.stderr for w in words), (opts, run.stderr)
        assert not (tmp_path / "out0.pcm").exists(), opts
    run = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "[--agc RMS [--agc-max-gain G]]" in run.stderr and "[--plc [--lose P:F0-F1,P:F,..]]" in run.stderr


def test_rules_under_sanitizers(tmp_path):
    """tests/c/agc_sanitize.cpp = pn_agc_rules.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: whole frames over rows, states and reports of exactly 480 floats and 4 words, the hostile rows, every
    parameter's edges, the target list at its exact length."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "agc_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "agc_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
