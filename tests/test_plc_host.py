"""Packet-loss concealment on the rate converter: the host-only surface, no GPU (include/percepnet_hip.h "packet-loss concealment"; the
rule lives in the HIP-free percepnet_amd/csrc/pn_plc_rules.h): pn_plc_gain, pn_plc_period and pn_plc_pitch against the numpy model
(tests/plc_model.py) bit for bit, the exact continuation of exactly periodic histories, the CLI's refusals that need no device, and the
rules under the address and undefined-behaviour sanitizers in a stand-alone program (tests/c/plc_sanitize.cpp).

Lags found on five harmonics (amplitude 1 / k, phase k) of f0 = 80, 110, 150 and 190 Hz: 600, 436, 640 and 253 — one, one, two and one
period; any multiple of the period is an equally good lag."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import plc_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PERIODS = (240, 241, 263, 300, 301, 359, 360, 417, 480, 555, 600, 719, 720)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def periodic_history(per, seed=0):
    """-> (hist [1920], the 480 samples that continue it): eight harmonics of a period of `per` samples, random amplitudes and phases,
    sampled ONCE over a period and repeated, so the history is periodic to the bit"""
    rng = np.random.default_rng(7000 + 10 * per + seed)
    i = np.arange(per)
    base = (sum(rng.uniform(0.2, 1.0) * np.cos(2 * np.pi * k * i / per + rng.uniform(0, 2 * np.pi)) for k in range(1, 9)) * 0.1).astype(F32)
    return base[np.arange(pm.HIST) % per], base[(pm.HIST + np.arange(480)) % per]


def harmonic_history(f0):
    t = np.arange(pm.HIST)
    return (sum(np.cos(2 * np.pi * k * f0 * t / 48000 + k) / k for k in range(1, 6)) * 0.1).astype(F32)


def test_constants():
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    for name, val in (("PN_PLC_HIST", 1920), ("PN_PLC_P_MIN", 240), ("PN_PLC_P_MAX", 720), ("PN_PLC_REPORT_WORDS", 4), ("PN_PLC_CONCEALED", 1),
                      ("PN_PLC_CROSSFADE", 2), ("PN_PLC_SILENT", 4)):
        assert f"#define {name} {val}\n" in hdr, name
    assert (api.PLC_HIST, api.PLC_P_MIN, api.PLC_P_MAX) == (pm.HIST, pm.P_MIN, pm.P_MAX) == (1920, 240, 720)
    assert api.PLC_REPORT_WORDS == 4 and api.PLC_REPORT_DTYPE.itemsize == 16 and api.PLC_REPORT_DTYPE == pm.REPORT_DTYPE
    assert (api.PLC_CONCEALED, api.PLC_CROSSFADE, api.PLC_SILENT) == (pm.CONCEALED, pm.CROSSFADE, pm.SILENT) == (1, 2, 4)
    rules = open(os.path.join(ROOT, "percepnet_amd", "csrc", "pn_plc_rules.h")).read()
    assert "PN_PLC_STATE_BYTES == 10576" in rules, "the bytes of state per stream are stated in the rules header"


def test_gain_at_its_edges():
    for m, want in ((0, 1.0), (479, 1.0), (480, 1.0), (2879, F32(1.0) / F32(2400.0)), (2880, 0.0)):
        got = api.plc_gain(m)
        assert same(got, pm.gain(m)) and got == F32(want), m
    assert not np.signbit(api.plc_gain(2880)) and api.plc_gain(1 << 40) == 0
    ms = np.arange(0, 3000)
    assert same(np.array([api.plc_gain(int(m)) for m in ms]), pm.gain(ms))
    assert api.plc_gain(960) == F32(0.8) and api.plc_gain(1920) == F32(0.4), "20 % per 10 ms"


@pytest.mark.parametrize("P", (240, 720, 241, 719, 483))
def test_period_is_the_models_bit_for_bit(P):
    hist = np.random.default_rng(7100 + P).standard_normal(pm.HIST).astype(F32)
    q = api.plc_period(hist, P)
    assert q.size == P and same(q, pm.period(hist, P))
    O = P // 4
    assert same(q[:P - O], hist[pm.HIST - P:pm.HIST - O]), "the head of the period is the history's own bits"
    assert not same(q[P - O:], hist[pm.HIST - O:]), "the tail is cross-faded into the period before"


def test_period_of_equal_periods_is_exact_and_bad_lags_are_refused():
    hist, _ = periodic_history(300)
    assert same(api.plc_period(hist, 600), hist[pm.HIST - 600:]), "a == b gives a exactly"
    for P in (239, 721, 0, -1):
        with pytest.raises(api.PercepNetError, match=r"\[240, 720\]"):
            api.plc_period(hist, P)
    with pytest.raises(api.PercepNetError, match="1920"):
        api.plc_pitch(np.zeros(1919, F32))


def test_pitch_of_silence_is_the_smallest_lag():
    assert api.plc_pitch(np.zeros(pm.HIST, F32)) == pm.pitch(np.zeros(pm.HIST, F32)) == 240
    assert api.plc_pitch(np.full(pm.HIST, -0.0, F32)) == 240
    assert api.plc_pitch(np.full(pm.HIST, np.nan, F32)) == pm.pitch(np.full(pm.HIST, np.nan, F32)) == 240, "NaN scores nothing"


@pytest.mark.parametrize("seed", range(6))
def test_pitch_on_white_noise_is_the_models(seed):
    hist = (np.random.default_rng(7200 + seed).standard_normal(pm.HIST) * 10.0 ** (seed - 3)).astype(F32)
    P = api.plc_pitch(hist)
    assert P == pm.pitch(hist) and 240 <= P <= 720
    assert abs(P - 6 * pm.coarse(hist)) <= 5, "the fine lag lies around the coarse one"


@pytest.mark.parametrize("f0", (80, 110, 150, 190))
def test_pitch_on_harmonic_signals(f0):
    hist = harmonic_history(f0)
    P = api.plc_pitch(hist)
    assert P == pm.pitch(hist)
    periods = P * f0 / 48000.0
    assert round(periods) >= 1 and abs(periods - round(periods)) * 48000.0 / f0 <= 1.0, f"{P} samples is a whole number of periods of {f0} Hz to a sample"


def test_the_lags_of_the_harmonic_signals_stay_what_the_stated_orders_give():
    """The rule's summation orders are fixed in pn_plc_rules.h; these are the lags they give.  Host and model changing an order
    TOGETHER would still agree with each other and, most likely, still find whole periods: the recorded lags are what would notice."""
    assert [api.plc_pitch(harmonic_history(f0)) for f0 in (80, 110, 150, 190)] == [600, 436, 640, 253]


@pytest.mark.parametrize("per", PERIODS)
def test_an_exactly_periodic_history_is_continued_bit_for_bit(per):
    """Whichever multiple of the period the search takes: the first concealed row is the true continuation."""
    hist, want = periodic_history(per)
    P = api.plc_pitch(hist)
    assert P == pm.pitch(hist) and P % per == 0 and 240 <= P <= 720
    q = api.plc_period(hist, P)
    assert same(q, pm.period(hist, P)) and same(pm.syn(q, P, 0), want)
    # the same through the model's whole frame, from four received rows
    m = pm.Plc(1)
    for t in range(4):
        m.frame(hist[None, 480 * t:480 * (t + 1)].copy())
    row = m.frame(np.full((1, 480), np.nan, F32), lost=(0,))
    assert same(row[0], want) and m.report[0].tolist() == (pm.CONCEALED, P, 1, 1)


def test_the_model_over_a_loss_of_seven_frames_is_the_host_functions_composed():
    """the model's whole frames against the closed form g(m) q[m mod P] with P, q and g from the LIBRARY's host functions"""
    hist, _ = periodic_history(417)
    m = pm.Plc(2)
    for t in range(4):
        m.frame(np.stack([hist[480 * t:480 * (t + 1)]] * 2))
    P = api.plc_pitch(hist)
    q = api.plc_period(hist, P)
    for r in range(7):
        x = m.frame(np.full((2, 480), np.nan, F32), lost=(1,), ids=[1])
        mm = 480 * r + np.arange(480)
        g = np.array([api.plc_gain(int(v)) for v in mm], F32)
        want = (g * q[mm % P]).astype(F32) if r < 6 else np.zeros(480, F32)
        assert same(x[1], want) and np.isnan(x[0]).all(), r
        assert m.report[1].tolist() == (pm.CONCEALED | (pm.SILENT if r == 6 else 0), P, r + 1, r + 1)
    assert not x[1].any() and not np.signbit(x[1]).any() and same(m.hist[1, -480:], x[1])
    real = np.random.default_rng(3).standard_normal((2, 480)).astype(F32)
    x = m.frame(real.copy(), ids=[1])
    w = (2 * np.arange(240) + 1).astype(F32) / F32(480)
    assert same(x[1, :240], F32(0) + w * (real[1, :240] - F32(0))) and same(x[1, 240:], real[1, 240:])
    assert m.report[1].tolist() == (pm.CROSSFADE, P, 0, 7) and m.report[0].tolist() == (0, 0, 0, 0)
    assert same(m.hist[0], hist), "the stream off the list kept its history"


def test_cli_refuses_lose_without_plc_and_bad_lists(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    for i in range(2):
        (tmp_path / f"in{i}.pcm").write_bytes(bytes(1920))
    files = ["in0.pcm", "out0.pcm", "in1.pcm", "out1.pcm"]
    for opts, words in ((["--rate", "8000", "--lose", "0:1"], ("--lose", "needs --plc")),
                        (["--plc", "--lose", "2:1"], ("--lose", "pair 2")),
                        (["--plc", "--lose", "0:3-1"], ("--lose", "expected")),
                        (["--plc", "--lose", "x"], ("--lose", "expected")),
                        (["--plc", "--lose", "0:1,"], ("--lose", "expected"))):
        run = subprocess.run([exe] + opts + files, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and all(w in run.stderr for w in words), (opts, run.stderr)
        assert not (tmp_path / "out0.pcm").exists(), opts


def test_rules_under_sanitizers(tmp_path):
    """tests/c/plc_sanitize.cpp = pn_plc_rules.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: the search over a history of exactly 1920 floats, the period at every lag with a q of exactly P
    floats (P = 720 reads two periods back), the gain, the score and the cross-fade at their edges."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "plc_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "plc_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
