"""The mixed rate converter's host-only surface, no GPU (include/percepnet_hip.h "mixed rates"; the rules live in the HIP-free
percepnet_amd/csrc/pn_rate_mixed.h): the four-rate table, refusals, the list check that names the first bad index, the single-rate
surface unchanged, and the same rules under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/c/rate_mixed_sanitize.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = {8000: (6, 80, 512), 16000: (3, 160, 992), 24000: (2, 240, 1472), 48000: (1, 480, 2880)}      # rate: L, n, delay
REFUSED = (44100, 12000, 0, -1)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def test_four_rate_table_and_refusals(lib):
    assert api.MIXED_RATES == tuple(TABLE) and api.RATE_MIXED_ROW == 480
    for rate, (L, n, delay) in TABLE.items():
        assert api.rate_mixed_frame_samples(rate) == n == 480 // L
        assert api.rate_mixed_delay_samples(rate) == delay == 2880 // L + (2 * api.RATE_TAPS if L > 1 else 0)
    for rate in api.RATES:
        assert api.rate_mixed_frame_samples(rate) == api.rate_frame_samples(rate)
        assert api.rate_mixed_delay_samples(rate) == api.rate_delay_samples(rate)
    for rate in REFUSED:
        assert api.rate_mixed_frame_samples(rate) == -1 and b"48000" in lib.pn_last_error()
        assert api.rate_mixed_delay_samples(rate) == -1 and b"48000" in lib.pn_last_error()


def test_single_rate_surface_is_unchanged(lib):
    assert api.RATES == (8000, 16000, 24000)
    assert lib.pn_rate_frame_samples(48000) == -1
    assert api.rate_frame_samples(48000) == -1 and api.rate_delay_samples(48000) == -1 and api.rate_state_bytes(48000) == 0
    assert api.rate_state_check(bytes(912), 48000) == api.SS_BAD_RATE
    with pytest.raises(api.PercepNetError):
        api.rate_taps(48000)


def check(lib, rates):
    a = np.asarray(rates, np.int32)
    return lib.pn_rate_mixed_rates_check(a.ctypes.data if a.size else None, int(a.size))


def test_rates_check_names_the_first_bad_index(lib):
    assert check(lib, []) == 0
    assert check(lib, [8000, 48000, 16000, 24000, 8000]) == 0
    assert lib.pn_rate_mixed_rates_check(None, 2) == -1
    assert lib.pn_rate_mixed_rates_check(np.zeros(1, np.int32).ctypes.data, -1) == -1
    for bad in REFUSED:
        assert check(lib, [bad]) == -1 and b"index 0:" in lib.pn_last_error()
        assert check(lib, [8000, 48000, bad, 24000]) == -1
        assert b"index 2:" in lib.pn_last_error() and str(bad).encode() in lib.pn_last_error()
    assert check(lib, [48000, 44100, 16000, 12000]) == -1
    assert b"index 1:" in lib.pn_last_error() and b"44100" in lib.pn_last_error() and b"12000" not in lib.pn_last_error()


def test_rules_under_sanitizers(tmp_path):
    """tests/c/rate_mixed_sanitize.cpp = pn_rate_mixed.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++
    with -fsanitize=address,undefined: hostile rate lists and id lists (NULL, n < 0, duplicates, out of range, lists spanning two
    rates, 48000 slots) in exactly-sized copies, each with its expected verdict."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "rate_mixed_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "rate_mixed_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
