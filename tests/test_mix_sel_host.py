"""Loudest-N selection, send gains and the hold of the conference mix: the host-only surface, no GPU (include/percepnet_hip.h
"conferences: loudest-N talkers, send gains, mix report"; the rules live in the HIP-free percepnet_amd/csrc/pn_mix_rules.h): the
numpy model (tests/mix_sel_model.py) against tests/conf_model.py at the defaults, pn_mix_level and pn_mix_select against the model
bit for bit, pn_rate_mix_gains_check naming the first bad index, the CLI's refusals that need no device, and the rules under the
address and undefined-behaviour sanitizers in a stand-alone program (tests/c/mix_sel_sanitize.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import conf_model as cm
from tests import mix_sel_model as mm
from tests import test_gpu_conf as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
B = tc.B


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def test_constants():
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    assert "#define PN_MIX_REPORT_WORDS 4" in hdr and api.MIX_REPORT_WORDS == 4 and api.MIX_REPORT_DTYPE.itemsize == 16
    assert api.MIX_REPORT_DTYPE.names == ("level", "flags", "mix_peak", "mix_clipped")
    assert (api.MIX_SELECTED, api.MIX_MUTED, api.MIX_IN_CONF) == (1, 2, 4)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("which", list(tc.KERNEL_LISTS))
def test_model_at_the_defaults_is_the_plain_mix(which):
    y, ids = tc.kernel_rows(), tc.KERNEL_LISTS[which]
    sentinel = np.full((B, 480), 777, F32)
    want = cm.mix(y, tc.CONFS, ids, out=sentinel)
    sizes = dict(tc.SIZES)
    for caps in (None, [0] * B, [32] * B, [sizes.get(c, 0) for c in range(B)]):       # N = 0, 32, and exactly the member count
        o, lv, rep = mm.mix(y, tc.CONFS, ids, out=sentinel, caps=caps)
        assert all(cm.same(o[s], want[s]) for s in range(B)), (which, caps and caps[40])
        adv = range(B) if ids is None else ids
        assert all(rep["flags"][s] == (0 if tc.CONFS[s] == cm.NONE else 5) for s in adv), "everybody is selected"
        assert all(rep["flags"][s] == 0 and lv[s] == 0 for s in range(B) if s not in adv)


def test_model_mutes_scales_and_selects():
    y = np.zeros((6, 480), F32)
    y[0], y[1], y[2], y[3], y[4] = F32(0.5), F32(0.25), F32(np.inf), F32(0.125), F32(1.0)
    confs = [2, 2, 2, 2, cm.NONE, 2]
    gains = np.array([1, 2, 0, 1, 3, 1], F32)
    o, lv, rep = mm.mix(y, confs, gains=gains, caps=[0, 0, 2, 0, 0, 0])
    # talkers 0 (x = 0.5), 1 (0.5), 3 (0.125), 5 (0): levels 120, 120, 7.5, 0 -> the tie 0 | 1 fills N = 2
    assert lv.tolist() == [120.0, 120.0, 0.0, 7.5, 0.0, 0.0] and rep["flags"].tolist() == [5, 5, 6, 4, 0, 4]
    assert (o[0] == 0.5).all() and (o[1] == 0.5).all() and (o[2] == 1.0).all() and (o[3] == 1.0).all() and (o[5] == 1.0).all()
    assert cm.same(o[4], y[4]) and rep[4].tolist() == (0.0, 0, 0.0, 0), "no conference: its own row whatever its gain, a zero record"
    assert rep["mix_peak"].tolist() == [0.5, 0.5, 1.0, 1.0, 0.0, 1.0] and rep["mix_clipped"].tolist() == [0, 0, 480, 480, 0, 480]
    # the hold keeps talker 3 ahead of a louder newcomer for as long as d^t * 7.5 > its level
    y[0], y[1] = F32(0), F32(0)
    y[5] = F32(0.0625)                                                  # level 1.875
    sel3 = []
    for t in range(4):
        o, lv, rep = mm.mix(y if t else np.where(np.arange(6)[:, None] == 3, F32(1.0), y).astype(F32), confs, gains=gains, caps=[0, 0, 1, 0, 0, 0],
                            hold=0.5, levels=lv if t else None)
        sel3.append(int(rep["flags"][3]) & 1)
    assert sel3 == [1, 1, 1, 1] and lv[3] == 60.0, "480 -> 240 -> 120 -> 60 stays above 1.875 and above its own 7.5"


# ---------------------------------------------------------------------------------------------------------------- the level
def level_rows():
    rng = np.random.default_rng(5100)
    rows = {f"gauss{i}": rng.standard_normal(480).astype(F32) * F32(10.0 ** (i - 3)) for i in range(6)}
    rows["subnormal"] = (rng.integers(1, 1 << 22, 480).astype(np.uint32)).view(F32)
    rows["nan"] = rows["gauss3"].copy()
    rows["nan"][137] = np.nan
    rows["inf"] = rows["gauss3"].copy()
    rows["inf"][400] = -np.inf
    rows["fltmax"] = np.full(480, np.finfo(F32).max, F32)
    rows["negzero"] = np.full(480, -0.0, F32)
    rows["order"] = np.ones(480, F32)
    rows["order"][0] = 4096
    return rows


@pytest.mark.parametrize("name", list(level_rows()))
def test_level_is_the_models_bit_for_bit(name):
    x = level_rows()[name]
    got, want = api.mix_level(x), mm.level(x)
    assert cm.same(got, want), (name, got, want)
    if name == "subnormal":
        assert got == 0 and not np.signbit(got)
    if name == "nan":
        assert np.isnan(got)
    if name in ("inf", "fltmax"):
        assert got == np.inf
    if name == "negzero":
        assert got == 0 and not np.signbit(got)


def test_level_order_is_pinned_by_a_hand_worked_row():
    # 4096 at sample 0 (square 2^24), 1 elsewhere: group 0 is ((2^24 + 1) + 1) + 1 = 2^24, each add rounding back to even; the other
    # 119 groups are 4 and fold exactly: 2^24 + 476.  The plain sequential sum never leaves 2^24.
    x = level_rows()["order"]
    assert api.mix_level(x) == F32(2 ** 24 + 476) == mm.level(x) and mm.level_sequential(x) == F32(2 ** 24)
    rng = np.random.default_rng(5101)
    g = rng.standard_normal((32, 480)).astype(F32)
    assert sum(mm.level(r) != mm.level_sequential(r) for r in g) > 16, "gaussian rows tell the two orders apart too"
    assert all(cm.same(api.mix_level(r), mm.level(r)) for r in g)
    assert np.array_equal(mm.level(g), np.array([mm.level(r) for r in g])), "the model is the same by rows and batched"
    with pytest.raises(api.PercepNetError, match="480"):
        api.mix_level(np.zeros(479, F32))


# ---------------------------------------------------------------------------------------------------------------- the selection
def selection_cases():
    rng = np.random.default_rng(5102)
    row = rng.standard_normal(480).astype(F32)
    tie = mm.level(row)
    assert tie == mm.level(-row)
    return {"distinct": rng.permutation(np.arange(1, 13)).astype(F32), "ties": np.array([1, tie, 3, tie, tie, 2], F32),
            "negated": np.array([tie, -tie, 0.5], F32), "zeros": np.zeros(9, F32), "nan": np.array([1, np.inf, np.nan, 2], F32),
            "one": np.array([4], F32), "full": rng.permutation(32).astype(F32)}


@pytest.mark.parametrize("name", list(selection_cases()))
def test_select_is_the_models(name):
    lv = selection_cases()[name]
    k = len(lv)
    for n in sorted({0, 1, 2, max(k - 1, 0), k, 32}):
        got, want = api.mix_select(lv, n), mm.select(lv, n)
        assert np.array_equal(got, want), (name, n)
        assert got.sum() == (k if n == 0 else min(n, k))
    if name == "ties":
        assert api.mix_select(lv, 2).tolist() == [False, True, False, True, False, False], "the lower slots of the tie"
    if name == "negated":
        assert api.mix_select(lv, 1).tolist() == [True, False, False], "a level and its negation tie: the sign is no part of the key"
    if name == "zeros":
        assert api.mix_select(lv, 3).tolist() == [True] * 3 + [False] * 6
    if name == "nan":
        assert api.mix_select(lv, 1).tolist() == [False, False, True, False], "NaN ranks above +inf"


def test_select_refuses_bad_counts(lib):
    lv = np.zeros(33, F32)
    sel = np.zeros(33, np.uint8)
    for k, n in ((33, 0), (-1, 0), (4, 33), (4, -1)):
        assert lib.pn_mix_select(lv.ctypes.data, k, n, sel.ctypes.data) == -1
    assert lib.pn_mix_select(None, 0, 0, None) == 0 and api.mix_select([], 3).size == 0


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_gains_check_names_the_first_bad_index(lib):
    good = np.array([1, 0, -0.0, 1e-20, np.finfo(F32).max, 0.5], F32)
    assert lib.pn_rate_mix_gains_check(good.ctypes.data, 6) == 0
    assert lib.pn_rate_mix_gains_check(good.ctypes.data, 0) == 0 and lib.pn_rate_mix_gains_check(None, 0) == 0
    assert lib.pn_rate_mix_gains_check(None, 3) == -1 and lib.pn_rate_mix_gains_check(good.ctypes.data, -1) == -1
    for at in range(6):
        for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-40):
            t = good.copy()
            t[at] = bad
            if at < 5:
                t[5] = np.nan                                      # a later bad one is not the one named
            assert lib.pn_rate_mix_gains_check(t.ctypes.data, 6) == -1
            assert b"at index %d:" % at in lib.pn_last_error(), lib.pn_last_error()
    api.rate_mix_gains_check(good)
    with pytest.raises(api.PercepNetError, match="at index 1:"):
        api.rate_mix_gains_check([1, -2, np.nan])


def test_cli_refuses_the_mix_options_without_a_conference_and_bad_values(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    for i in range(2):
        (tmp_path / f"in{i}.pcm").write_bytes(bytes(1920))
    files = ["in0.pcm", "out0.pcm", "in1.pcm", "out1.pcm"]
    for opts, words in ((["--conf-speakers", "2"], ("--conf-speakers", "needs --conference")), (["--mix-gains", "1,1"], ("--mix-gains", "needs --conference")),
                        (["--conference", "0,0", "--conf-speakers", "33"], ("--conf-speakers", "[0, 32]")),
                        (["--conference", "0,0", "--conf-speakers", "x"], ("--conf-speakers", "expected")),
                        (["--conference", "0,0", "--mix-gains", "1"], ("--mix-gains", "1 gains for 2 pairs")),
                        (["--conference", "0,0", "--mix-gains", "1,-1"], ("--mix-gains", "at index 1")),
                        (["--conference", "0,0", "--mix-gains", "nan,1"], ("--mix-gains", "at index 0")),
                        (["--conference", "0,0", "--mix-gains", "1;2"], ("--mix-gains", "expected"))):
        run = subprocess.run([exe] + opts + files, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and all(w in run.stderr for w in words), (opts, run.stderr)
        assert not (tmp_path / "out0.pcm").exists(), opts


def test_rules_under_sanitizers(tmp_path):
    """tests/c/mix_sel_sanitize.cpp = pn_mix_rules.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: the level at its edge values and the hand-worked row, the hold, the selection at k = 0, 1, 32,
    the value checks."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "mix_sel_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "mix_sel_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
