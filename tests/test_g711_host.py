"""The G.711 companding's host-only surface, no GPU (include/percepnet_hip.h "G.711 streams"; the formulas live in the HIP-free
percepnet_amd/csrc/pn_g711.h): pn_g711_decode over all 256 codes and pn_g711_encode over all 65 536 values against the numpy
model (tests/g711_model.py), the known answers and properties the header states, the relations to CPython's audioop where it
imports, the refusals, and the same functions under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/c/g711_sanitize.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import g711_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = np.arange(256, dtype=np.uint8)
VALUES = np.arange(-32768, 32768).astype(np.int16)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def test_constants():
    assert (api.G711_ULAW, api.G711_ALAW) == (gm.ULAW, gm.ALAW) == (0, 1)


@pytest.mark.parametrize("law", gm.LAWS, ids=gm.NAMES.get)
def test_every_code_and_every_value_equal_the_model(law):
    dec = api.g711_decode(law, CODES)
    enc = api.g711_encode(law, VALUES)
    assert dec.dtype == np.int16 and enc.dtype == np.uint8
    assert np.array_equal(dec, gm.decode(law, CODES))
    assert np.array_equal(enc, gm.encode(law, VALUES))
    # shapes pass through
    assert api.g711_decode(law, CODES.reshape(4, 64)).shape == (4, 64) and api.g711_encode(law, np.zeros(0, np.int16)).size == 0


@pytest.mark.parametrize("law", gm.LAWS, ids=gm.NAMES.get)
def test_known_answers_and_properties(law):
    for v, b in gm.ENC_KNOWN[law].items():
        assert int(api.g711_encode(law, [v])[0]) == b, (v, hex(b))
    dec = api.g711_decode(law, CODES).astype(np.int32)
    assert dec.max() == gm.DEC_RANGE[law] and dec.min() == -gm.DEC_RANGE[law]
    if law == gm.ULAW:
        assert dec[0xFF] == 0 and dec[0x7F] == 0 and np.count_nonzero(dec == 0) == 2
    else:
        assert dec[0xD5] == 8 and dec[0x55] == -8 and not (dec == 0).any()
    # enc(dec(b)) == b for every b, except mu-law 0x7F -> 0xFF
    back = api.g711_encode(law, dec.astype(np.int16))
    want = CODES.copy()
    if law == gm.ULAW:
        want[0x7F] = 0xFF
    assert np.array_equal(back, want)
    # dec(enc(v)) is non-decreasing in v and at most the law's largest step away from it
    rt = api.g711_decode(law, api.g711_encode(law, VALUES)).astype(np.int32)
    assert (np.diff(rt) >= 0).all()
    assert int(np.abs(rt - VALUES.astype(np.int32)).max()) == gm.MAX_ROUND_TRIP_ERROR[law]


def test_relations_to_audioop():
    audioop = pytest.importorskip("audioop")
    codes = CODES.tobytes()
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2"), api.g711_decode(gm.ULAW, CODES))
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(codes, 2), "<i2"), api.g711_decode(gm.ALAW, CODES))
    assert np.array_equal(np.frombuffer(audioop.lin2alaw(VALUES.astype("<i2").tobytes(), 2), np.uint8), api.g711_encode(gm.ALAW, VALUES))
    # mu-law: audioop for v >= 0; for v < 0 audioop of the one's complement with the sign bit turned (audioop itself negates
    # after shifting and so differs for some negative values, which is not a bug of either)
    enc = api.g711_encode(gm.ULAW, VALUES)
    neg = VALUES < 0
    pos_ref = np.frombuffer(audioop.lin2ulaw(VALUES[~neg].astype("<i2").tobytes(), 2), np.uint8)
    neg_ref = np.frombuffer(audioop.lin2ulaw((~VALUES[neg]).astype("<i2").tobytes(), 2), np.uint8) ^ 0x80
    assert np.array_equal(enc[~neg], pos_ref) and np.array_equal(enc[neg], neg_ref)


def test_refusals(lib):
    b, v = np.full(4, 0xAB, np.uint8), np.full(4, 1234, np.int16)
    for bad in (-1, 2, 255, 8000):
        assert lib.pn_g711_decode(bad, b.ctypes.data, v.ctypes.data, 4) == -1 and b"law" in lib.pn_last_error()
        assert lib.pn_g711_encode(bad, v.ctypes.data, b.ctypes.data, 4) == -1 and b"law" in lib.pn_last_error()
        with pytest.raises(api.PercepNetError):
            api.g711_decode(bad, b)
        with pytest.raises(api.PercepNetError):
            api.g711_encode(bad, v)
    for law in gm.LAWS:
        assert lib.pn_g711_decode(law, None, v.ctypes.data, 4) == -1 and b"NULL" in lib.pn_last_error()
        assert lib.pn_g711_decode(law, b.ctypes.data, None, 4) == -1
        assert lib.pn_g711_encode(law, None, b.ctypes.data, 4) == -1
        assert lib.pn_g711_encode(law, v.ctypes.data, None, 4) == -1
        assert lib.pn_g711_decode(law, b.ctypes.data, v.ctypes.data, 0) == 0 and lib.pn_g711_encode(law, v.ctypes.data, b.ctypes.data, 0) == 0
    assert (b == 0xAB).all() and (v == 1234).all(), "a refused call and n == 0 write nothing"


def test_laws_check_names_the_first_bad_index(lib):
    good = np.array([0, 1, 1, 0, 1], np.int32)
    assert lib.pn_rate_laws_check(good.ctypes.data, 5) == 0
    assert lib.pn_rate_laws_check(good.ctypes.data, 0) == 0 and lib.pn_rate_laws_check(None, 0) == 0
    assert lib.pn_rate_laws_check(None, 3) == -1 and lib.pn_rate_laws_check(good.ctypes.data, -1) == -1
    for at in range(5):
        for bad in (2, -1, 8000):
            t = good.copy()
            t[at] = bad
            if at < 4:
                t[4] = 7                                           # a later bad one is not the one named
            assert lib.pn_rate_laws_check(t.ctypes.data, 5) == -1
            err = lib.pn_last_error()
            assert b"at index %d:" % at in err and str(bad).encode() in err, err


def test_cli_refuses_g711_without_a_converter(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "in.g711").write_bytes(bytes(960))
    for opts in (["--g711", "ulaw"], ["--rate", "8000", "--g711", "mulaw"]):
        run = subprocess.run([exe] + opts + ["in.g711", "out.g711"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and "g711" in run.stderr and not (tmp_path / "out.g711").exists(), opts
    assert "usage" in subprocess.run([exe, "--g711", "alaw", "in.g711", "out.g711"], cwd=tmp_path, capture_output=True, text=True, timeout=60).stderr


def test_companding_under_sanitizers(tmp_path):
    """tests/c/g711_sanitize.cpp = pn_g711.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: every code and every value through the header's functions into exactly-sized buffers, n = 0,
    and hostile lists of laws and ids."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "g711_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "g711_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
