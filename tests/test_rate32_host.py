"""32000 Hz on the rate converter's host-only surface, no GPU (include/percepnet_hip.h "batched rate converter" and "mixed rates";
percepnet_amd/csrc/pn_rate_design.h, pn_rate_mixed.h): the numpy model of the rational row arithmetic (tests/rate32_model.py)
tied to the shipped integer arithmetic (tests/rate_model.py) bit for bit, the sizes and taps through the C-ABI, the state-record
check, the float64 round-trip accuracy beside the other rates', and the HIP-free pieces under the address and
undefined-behaviour sanitizers in a stand-alone program (tests/c/rate32_sanitize.cpp)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import rate32_model as r32
from tests import rate_model as rmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
RATE, N, DELAY, REC = 32000, 320, 1952, 336


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("L", (6, 3, 2))
def test_model_at_M_1_is_the_shipped_arithmetic(L):
    """(L, 1) rows of the generalised model equal rate_model.up_f32 / down_f32 bit for bit on seeded noise, 3 frames, tails carried."""
    B, n = 3, 480 // L
    rng = np.random.default_rng(32 + L)
    h, g = r32.taps_f32(L, 1, False), r32.taps_f32(L, 1, True)
    assert same(h, rmod.taps_f32(L, False)) and same(g, rmod.taps_f32(L, True))
    up_a, up_b, dn_a, dn_b = r32.Up(B, L, 1, h), rmod.Up(B, L, h), r32.Down(B, L, 1, g), rmod.Down(B, L, g)
    for t in range(3):
        x = rng.uniform(-1, 1, (B, n)).astype(F32)
        o = rng.uniform(-1, 1, (B, 480)).astype(F32)
        assert same(up_a(x), up_b(x)) and same(up_a.tail, up_b.tail), f"up L={L} frame {t}"
        assert same(dn_a(o), dn_b(o)) and same(dn_a.tail, dn_b.tail), f"down L={L} frame {t}"
    x = rng.standard_normal(800)
    assert np.allclose(r32.chain_f64(x, L, 1), rmod.chain_f64(x, L), rtol=0, atol=1e-12)


def test_model_structure_at_3_2():
    """What the kernels' static asserts state, from the model's own index sets: 47 | 48 terms, no tap at +-D, nothing older than
    47 samples, nothing of the next frame.  Phase 0 copies the input's bits 16 samples late, and the up rows are every second
    output of the plain interpolation by 3 of the same samples (the 16 kHz arithmetic, whose table 32000 shares)."""
    L, M, D = 3, 2, 48
    terms, taps_seen, oldest, newest = set(), set(), 0, 0
    for m in range(N):
        idx = [i for i in range(-60, 480) if (L * m - 2 * D) / M < i < L * m / M]
        terms.add((m % 2, len(idx)))
        taps_seen |= {L * m - D - M * i for i in idx}
        oldest, newest = min(oldest, idx[0]), max(newest, idx[-1])
    assert terms == {(0, 47), (1, 48)} and max(abs(k) for k in taps_seen) == D - 1 and oldest == -47 and newest == 478
    rng = np.random.default_rng(5)
    h = r32.taps_f32(L, M, False)
    up = r32.Up(2, L, M, h)
    x = rng.uniform(-1, 1, (2, 3 * N)).astype(F32)
    y = np.concatenate([up(x[:, t * N:(t + 1) * N]) for t in range(3)], axis=1)
    delayed = np.concatenate([np.zeros((2, 16), F32), x], axis=1)
    assert same(np.ascontiguousarray(y[:, ::3]), np.ascontiguousarray(delayed[:, 0:3 * N:2])), "output 3r is input 2r - 16, bit for bit"
    # every second output of the plain interpolation by 3 of the same samples (n = 160 per call, two calls a frame)
    up3 = rmod.Up(2, 3, h)
    y3 = np.concatenate([up3(x[:, t * 160:(t + 1) * 160]) for t in range(6)], axis=1)
    assert same(np.ascontiguousarray(y3[:, ::2]), y)


def test_sizes_taps_and_mixed_surface(lib):
    assert api.RATES == (8000, 16000, 24000) and api.MIXED_RATES == (8000, 16000, 24000, 48000)
    assert api.RATES_ALL == api.RATES + (RATE,) and api.MIXED_RATES_ALL == (8000, 16000, 24000, 32000, 48000)
    assert api.rate_frame_samples(RATE) == N and api.rate_delay_samples(RATE) == DELAY == r32.delay_samples(RATE)
    assert api.rate_state_bytes(RATE) == REC == 16 + 4 * (32 + 48) and REC <= api.rate_state_max_bytes() == 912
    assert api.rate_mixed_frame_samples(RATE) == N and api.rate_mixed_delay_samples(RATE) == DELAY
    h, g = api.rate_taps(RATE, False), api.rate_taps(RATE, True)
    assert h.size == g.size == 97
    assert same(h, api.rate_taps(16000, False)), "the prototype is the 16 kHz up table, bit for bit"
    # (float)(h_double * 2 / 3), computed in double as written and narrowed once: every tap, bit for bit.  (The double rounding
    # (float)h * (float)(2 / 3) differs from it in 30 of the 97 taps, by one ulp each: an absolute bound would not see it.)
    want = (rmod.design(3) * 2 / 3).astype(F32)
    assert same(want, r32.taps_f32(3, 2, True))
    twice = h * F32(2.0 / 3.0)
    assert np.count_nonzero(want.view(np.uint32) != twice.view(np.uint32)) >= 20, "the check tells the two roundings apart"
    diff = np.flatnonzero(g.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, f"taps {diff - 48} differ from (float)(h * 2 / 3): {g[diff]} != {want[diff]}"
    assert same(g, np.ascontiguousarray(g[::-1])), "symmetric bit for bit"
    assert g[48] == F32(2.0 / 3.0) and np.all(g[np.arange(97) % 3 == 0][np.arange(33) != 16] == 0)
    assert np.count_nonzero(g) == 97 - 32, "zero at the multiples of 3 away from the centre, and nowhere else"
    t = np.full(96, 7, F32)
    assert lib.pn_rate_taps(RATE, 1, t.ctypes.data, 96) == -1 and (t == 7).all()
    # the mixed list check takes 32000 and still names the first bad index
    chk = lambda r: lib.pn_rate_mixed_rates_check(np.asarray(r, np.int32).ctypes.data, len(r))
    assert chk([32000]) == 0 and chk([8000, 32000, 48000, 16000, 24000, 32000]) == 0
    assert chk([32000, 48000, 44100, 32000]) == -1
    assert b"index 2:" in lib.pn_last_error() and b"44100" in lib.pn_last_error() and b"32000" in lib.pn_last_error()
    for bad in (32001, 31999, 64000, 44100, 12000, 96000, 7999):
        assert api.rate_frame_samples(bad) == -1 and b"32000" in lib.pn_last_error()
        assert api.rate_mixed_frame_samples(bad) == -1 and api.rate_state_bytes(bad) == 0


def test_state_record_check():
    body = np.random.default_rng(RATE).standard_normal((REC - 16) // 4).astype("<f4").tobytes()
    good = struct.pack("<4sIIi", b"PNRS", 1, REC, RATE) + body
    assert len(good) == REC and api.rate_state_check(good, RATE) == api.SS_OK
    assert api.rate_state_check(b"PNSS" + good[4:], RATE) == api.SS_BAD_MAGIC
    assert api.rate_state_check(good[:4] + struct.pack("<I", 2) + good[8:], RATE) == api.SS_BAD_VERSION
    assert api.rate_state_check(good[:8] + struct.pack("<I", 528) + good[12:], RATE) == api.SS_BAD_SIZE, "a 528-byte size word"
    assert api.rate_state_check(good[:-4], RATE) == api.SS_BAD_SIZE and api.rate_state_check(good + bytes(4), RATE) == api.SS_BAD_SIZE
    assert api.rate_state_check(good[:8], RATE) == api.SS_BAD_SIZE and api.rate_state_check(b"", RATE) == api.SS_BAD_ARG
    assert api.rate_state_check(good[:12] + struct.pack("<i", 16000) + good[16:], RATE) == api.SS_BAD_RATE, "rate word 16000 in a 32000 slot"
    assert api.rate_state_check(good, 16000) == api.SS_BAD_RATE
    rec16 = struct.pack("<4sIIi", b"PNRS", 1, 528, 16000) + bytes(512)
    assert api.rate_state_check(rec16, 16000) == api.SS_OK and api.rate_state_check(rec16, RATE) == api.SS_BAD_RATE
    assert api.rate_state_check(rec16[:12] + struct.pack("<i", RATE) + rec16[16:], 16000) == api.SS_BAD_RATE, "rate word 32000 in a 16000 slot"
    assert api.rate_state_check(rec16[:12] + struct.pack("<i", RATE) + rec16[16:], RATE) == api.SS_BAD_SIZE
    for other in (8000, 24000, 48000):
        assert api.rate_state_check(good, other) == api.SS_BAD_RATE


@pytest.mark.parametrize("f_rel", (0.02, 0.25, 0.40))
def test_roundtrip_accuracy_beside_the_other_rates(f_rel):
    """Up then down in float64, no engine: max error against the input delayed by 32 samples, after 200 samples.  32 kHz may
    cost at most 2x the worst of 8 / 16 / 24 kHz from the same function (an index error costs orders of magnitude)."""
    others = {r: r32.roundtrip_error(r, f_rel) for r in (8000, 16000, 24000)}
    e32 = r32.roundtrip_error(RATE, f_rel)
    print(f"f / rate = {f_rel}: 32 kHz {e32:.3e}; others {', '.join(f'{r}: {e:.3e}' for r, e in others.items())}; ratio {e32 / max(others.values()):.2f}")
    assert e32 <= 2 * max(others.values())
    assert max(others.values()) < 1e-3


def test_design_records_and_lists_under_sanitizers(tmp_path):
    """tests/c/rate32_sanitize.cpp = pn_rate_mixed.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: the 32000 design into exactly-sized tables and a cap one short, the record check over every
    truncation and header corruption, hostile rate lists holding 32000."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "rate32_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "rate32_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
