"""The rate converter's host-only surface, no GPU (include/percepnet_hip.h "batched rate converter"; the design and the record
check live in the HIP-free percepnet_amd/csrc/pn_rate_design.h): refusals and sizes, the fp32 tap tables against an independent
double design (tests/rate_model.py), the frequency response those tables give, the state-record check, and the same pieces under
the address and undefined-behaviour sanitizers in a stand-alone program (tests/c/rate_sanitize.cpp)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import rate_model as rmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = {8000: (6, 80, 512, 912), 16000: (3, 160, 992, 528), 24000: (2, 240, 1472, 400)}      # rate: L, n, delay, record bytes
REFUSED = (48000, 44100, 0, -1)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def test_sizes_delays_and_refusals(lib):
    assert api.RATES == tuple(TABLE) == rmod.RATES
    for rate, (L, n, delay, rec) in TABLE.items():
        assert api.rate_frame_samples(rate) == n == 480 // L
        assert api.rate_delay_samples(rate) == delay == 2880 // L + 2 * api.RATE_TAPS == rmod.delay_samples(rate)
        assert api.rate_state_bytes(rate) == rec == 16 + 4 * (32 + 2 * api.RATE_TAPS * L)
        for down in (False, True):
            assert api.rate_taps(rate, down).size == 2 * api.RATE_TAPS * L + 1
        # a destination one float short is refused, and nothing is written
        t = np.full(2 * api.RATE_TAPS * L, 7, np.float32)
        assert lib.pn_rate_taps(rate, 0, t.ctypes.data, int(t.size)) == -1 and (t == 7).all()
    for rate in REFUSED:
        assert api.rate_frame_samples(rate) == -1 and b"8000" in lib.pn_last_error()
        assert api.rate_delay_samples(rate) == -1
        assert api.rate_state_bytes(rate) == 0
        t = np.zeros(256, np.float32)
        assert lib.pn_rate_taps(rate, 0, t.ctypes.data, 256) == -1
        with pytest.raises(api.PercepNetError):
            api.rate_taps(rate)
        assert api.rate_state_check(bytes(912), rate) == api.SS_BAD_RATE


@pytest.mark.parametrize("rate", list(TABLE))
def test_taps_against_an_independent_double_design(rate):
    L = TABLE[rate][0]
    D = api.RATE_TAPS * L
    want = rmod.design(L)
    for down in (False, True):
        t = api.rate_taps(rate, down)
        assert t.dtype == np.float32
        assert np.array_equal(t.view(np.uint32), t[::-1].view(np.uint32)), "symmetric bit for bit"
        k = np.arange(-D, D + 1)
        at_zero = (k % L == 0) & (k != 0)
        assert np.all(t[at_zero] == 0) and np.count_nonzero(t == 0) == at_zero.sum(), "h[jL] == 0 exactly, and nowhere else"
        ref = want / L if down else want
        err = np.abs(t.astype(np.float64) - ref).max()
        print(f"{rate} Hz down={down}: max |taps - double design| = {err:.3e}")
        assert err <= 2.0 ** -24
        if not down:
            assert t[D] == np.float32(1) and t.view(np.uint32)[D] == 0x3F800000
        else:
            assert t[D] == np.float32(1.0 / L)


@pytest.mark.parametrize("rate", list(TABLE))
def test_frequency_response_of_the_library_taps(rate):
    """Computed in double from the LIBRARY's fp32 taps, 131 072-point FFT at 48 kHz.  h carries the up-converter's gain of L
    (zero-stuffing divides the spectrum by L), g = h / L is unity in the pass band: both are judged as |H| / L resp. |G|.
    Pass band up to 0.8 of the low-rate Nyquist within +-0.01 dB, stop band from 1.2 of it at most -80 dB."""
    L = TABLE[rate][0]
    nfft = 1 << 17
    f = np.fft.rfftfreq(nfft, 1.0 / 48000)
    nyq = rate / 2.0
    for down in (False, True):
        t = api.rate_taps(rate, down).astype(np.float64)
        mag = np.abs(np.fft.rfft(t, nfft)) / (1.0 if down else L)
        db = 20 * np.log10(np.maximum(mag, 1e-300))
        ripple = np.abs(db[f <= 0.8 * nyq]).max()
        stop = db[f >= 1.2 * nyq].max()
        print(f"{rate} Hz down={down}: pass-band ripple {ripple:.5f} dB, stop band {stop:.2f} dB")
        assert ripple <= 0.01
        assert stop <= -80.0


@pytest.mark.parametrize("rate", list(TABLE))
def test_state_record_check(rate):
    L, n, delay, nbytes = TABLE[rate]
    body = np.random.default_rng(rate).standard_normal((nbytes - 16) // 4).astype("<f4").tobytes()
    good = struct.pack("<4sIIi", b"PNRS", 1, nbytes, rate) + body
    assert len(good) == nbytes and api.rate_state_check(good, rate) == api.SS_OK
    assert api.rate_state_check(b"PNSS" + good[4:], rate) == api.SS_BAD_MAGIC
    assert api.rate_state_check(good[:4] + struct.pack("<I", 2) + good[8:], rate) == api.SS_BAD_VERSION
    assert api.rate_state_check(good[:8] + struct.pack("<I", nbytes + 4) + good[12:], rate) == api.SS_BAD_SIZE
    assert api.rate_state_check(good[:-4], rate) == api.SS_BAD_SIZE
    assert api.rate_state_check(good + bytes(4), rate) == api.SS_BAD_SIZE
    assert api.rate_state_check(good[:8], rate) == api.SS_BAD_SIZE
    assert api.rate_state_check(b"", rate) == api.SS_BAD_ARG
    for other in TABLE:
        if other != rate:
            assert api.rate_state_check(good, other) == api.SS_BAD_RATE, "a record of another rate"
            # ... also when its header claims this rate's size, or its rate field is rewritten but the size is the other's
            assert api.rate_state_check(good[:12] + struct.pack("<i", other) + good[16:], rate) == api.SS_BAD_RATE
            assert api.rate_state_check(good[:12] + struct.pack("<i", other) + good[16:], other) == api.SS_BAD_SIZE
    assert api.rate_state_check(good[:12] + struct.pack("<i", 48000) + good[16:], rate) == api.SS_BAD_RATE


@pytest.mark.parametrize("rate", list(TABLE))
def test_cast_edge_rows_cover_every_class_of_the_down_cast(rate):
    """The precondition of tests/test_gpu_cast_edges.py's rate tests, from the numpy model and the library's taps alone: in every
    row of rate_model.cast_edge_rows the model's own t = z * 32768 holds a value of every class of rate_model.t_classes, the
    samples are at least 2D + L apart, and the frame of zeros behind them still carries NaN through the tail."""
    L = TABLE[rate][0]
    D = api.RATE_TAPS * L
    g = api.rate_taps(rate, True)
    for B in (5, 1):
        o = rmod.cast_edge_rows(B, L, g)
        assert o.shape[1:] == (B, 480) and not o[-1].any() and o.shape[0] <= 6
        flat = o.transpose(1, 0, 2).reshape(B, -1)
        for r in range(B):
            at = np.flatnonzero(flat[r])
            assert at.size == len(rmod.EDGE_IMPULSES) and np.diff(at).min() >= 2 * D + L
            assert at[-1] >= flat.shape[1] - 480 - 2 * D, "the last sample's window must reach the frame of zeros"
        down = rmod.Down(B, L, g)
        with np.errstate(all="ignore"):
            z = np.stack([down(f) for f in o])
            t = z * np.float32(32768)
        for name, mask in rmod.t_classes(t).items():
            per_row = mask.sum(axis=(0, 2))
            print(f"{rate} Hz B={B} {name}: {per_row.tolist()}")
            assert np.all(per_row >= 1), name
        assert np.isnan(z[-1]).any(axis=1).all() and np.isfinite(z[-1]).any(axis=1).all()
        # NaN is 0 in both casts, and the wrap gives 0 for whatever is not finite
        assert (rmod.to_i16(z, True)[np.isnan(z)] == 0).all() and (rmod.to_i16(z, False)[~np.isfinite(t)] == 0).all()


def test_design_and_record_check_under_sanitizers(tmp_path):
    """tests/c/rate_sanitize.cpp = pn_rate_design.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: the design for each rate into exactly-sized tables, the record check over every truncation
    and every single-bit corruption of the header in exactly-sized copies."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "rate_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "rate_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])


def test_state_table_under_sanitizers(tmp_path):
    """tests/c/rate_layout_sanitize.cpp = pn_rate_layout.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: which event clears which of the converter's ten per-stream state buffers against the matrix
    written out there, the call-state sections against pn_call_rules.h, every width against its stage's constant."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "rate_layout_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "rate_layout_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
