"""In-band DTMF detection on the rate converter: the host-only surface, no GPU (include/percepnet_hip.h "DTMF detection"; the rule lives
in the HIP-free percepnet_amd/csrc/pn_dtmf_rules.h): the tables against numpy's, pn_dtmf_frame against the numpy model
(tests/dtmf_model.py) bit for bit in state and report over sequences of 40 frames, the pinned defaults, every refusal, the behaviour of
the rule at the default parameters, the CLI's refusals that need no device, and the rule under the address and undefined-behaviour
sanitizers in a stand-alone program (tests/c/dtmf_sanitize.cpp).

Offsets.  The behaviour tests start their tones at eight offsets across a frame, 60 + 50 i samples (60 .. 410).  The frame's edges
are left out on purpose.  A window of n tone samples and 960 - n of silence has P[r] + P[c] = (n / 2) E, so at the default purity of
0.5 it hits from n = 480 on, give or take the leakage between the two tones.  A 20 ms tone that starts o samples into a frame fills
its four windows with 480 - o, 960 - o, 480 + o and o samples: two hits, and nothing reported at on_frames = 3, unless o or 480 - o is
so small that a third window is half full.  At o = 0 that window sits ON the threshold (240 E against 240 E) and the last bit
decides; measured on this model, some digit's 20 ms tone is reported for o <= 5 and for o >= 440, none for 10 <= o <= 435.  That a
20 ms tone can be reported when it starts within a millisecond of a frame edge is a property of the rule as stated (a 20 ms window,
three hits, half the energy), recorded in DESIGN.md; the offsets here keep every decision at least 30 samples from it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import dtmf_model as dm
from tests import g711_model, rate_model
from tests.test_agc_host import hostile_rows, voice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32
D = dm.DEFAULTS
OFFSETS = tuple(60 + 50 * i for i in range(8))


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    L = api.load_library()
    sync_tables()
    return L


def sync_tables():
    """The model computes with its own tables unless an entry differs from the library's; then it takes the library's.  -> the entries
    that differ, as (table, k, j, library, numpy)"""
    ct, st, rot = api.dtmf_tables()
    mine = dm.make_tables()
    diff = [(name, int(i) // a.shape[-1] if a.ndim > 1 else 0, int(i) % a.shape[-1], float(a.ravel()[i]), float(b.ravel()[i]))
            for name, a, b in (("ct", ct, mine[0]), ("st", st, mine[1]), ("rot", rot, mine[2])) for i in np.flatnonzero(a.view(U32).ravel() != b.view(U32).ravel())]
    if diff:
        dm.use_tables(ct, st, rot)
    return diff


def frames_of(x):
    x = np.asarray(x, np.float64).ravel()
    return np.concatenate([x, np.zeros((-x.size) % 480)]).astype(F32).reshape(-1, 480)


def model_digits(x, params=D):
    """-> (the digits begun, the frames that hit) of one stream over the samples x"""
    reps, _ = dm.run_stream(params, frames_of(x))
    return dm.digits_begun(reps), int(np.count_nonzero(reps[:, 0] & dm.HIT))


def one_tone(digit, n, offset, **kw):
    return np.concatenate([np.zeros(offset), dm.dual_tone(digit, n, **kw), np.zeros(1920)])


def run_host(rows, concealed=(), params=D):
    st = np.zeros(dm.STATE_WORDS, U32)
    states, reps = [], []
    for t, x in enumerate(rows):
        flags, rep = api.dtmf_frame(params, st, x, concealed=t in concealed)
        assert flags == int(rep["word0"]) & 0xff
        states.append(st.copy()); reps.append(np.array([rep["word0"], rep["dur"], rep["count"], rep["last4"]], U32))
    return np.stack(states), np.stack(reps)


def run_model(rows, concealed=(), params=D):
    st = dm.fresh(1)
    sums = dm.half_sums(rows)
    states, reps = [], []
    for t in range(len(rows)):
        st, rep = dm.step(params, st, sums[t:t + 1], np.array([t in concealed]))
        states.append(st[0].copy()); reps.append(rep[0])
    return np.stack(states), np.stack(reps)


def sequences():
    """name -> (rows [40, 480], concealed frames, params)"""
    h = hostile_rows()
    rng = np.random.default_rng(4733)
    seqs = {}
    k40 = lambda digits, **kw: dm.keypad(digits, tail=19200, **kw)[:40]
    for off in (0, 30, 257):
        seqs[f"digits_{off}"] = (k40("159D", lead=off), (), D)
        seqs[f"digits_tail_{off}"] = (k40("A#07", lead=off, amp=0.02), (), D)
    for rms in (0.005, 0.1, 0.5):
        seqs[f"voice_{rms}"] = (voice(rms, 40), (), D)
    rows = k40("2468", lead=100).copy()
    for i, name in enumerate(h):
        rows[2 + 3 * i] = h[name]                                       # one hostile row every three frames, digits between them
    seqs["hostile"] = (rows, (), D)
    seqs["hostile_first"] = (np.concatenate([np.stack(list(h.values())), dm.keypad("3B", lead=7, tail=19200)])[:40], (), D)
    noisy = k40("*0#", lead=77) + (rng.standard_normal((40, 480)) * 0.02).astype(F32)
    seqs["noisy"] = (noisy, (), D)
    seqs["concealed"] = (k40("5C", lead=31, on=4800), (0, 5, 6, 7, 21), D)
    p1 = D.copy()
    p1[[dm.ON_FRAMES, dm.OFF_FRAMES]] = 1
    seqs["on1_off1"] = (frames_of(np.concatenate([np.zeros(240), dm.dual_tone("8", 2400), dm.dual_tone("2", 2400), np.zeros(16800)]))[:40], (), p1)
    p2 = np.array([0.0, 1e-3, 100, 100, 1, 100, 100], F32)
    seqs["edge_params"] = (k40("1", on=48000, lead=3), (), p2)
    return seqs


def test_defaults_and_constants():
    assert np.array_equal(api.dtmf_default_params().view(U32), D.view(U32)) and D.size == api.DTMF_N_PARAMS == 7
    assert (api.DTMF_ON, api.DTMF_HIT, api.DTMF_BEGIN, api.DTMF_END, api.DTMF_HELD_LOST) == (dm.ON, dm.HIT, dm.BEGIN, dm.END, dm.HELD_LOST) == (1, 2, 4, 8, 16)
    assert api.DTMF_STATE_WORDS == dm.STATE_WORDS == 24 and api.DTMF_REPORT_WORDS == dm.REPORT_WORDS == 4 and api.DTMF_REPORT_DTYPE.itemsize == 16


def test_tables_against_numpy():
    """The library's tables are numpy's: any entry that differs — two libraries rounding cos or sin of a double the other way — differs
    by one fp32 ulp at most, and the failure names them."""
    ct, st, rot = api.dtmf_tables()
    assert ct.shape == st.shape == (8, 480) and rot.shape == (16,)
    assert np.all(ct[:, 0] == 1.0) and np.all(st[:, 0] == 0.0)
    diff = sync_tables()
    for name, k, j, a, b in diff:
        assert abs(a - b) <= np.spacing(F32(max(abs(a), abs(b)))), ("more than one ulp apart", name, k, j, a, b)
    print("table entries that differ from numpy's:", diff)
    # exact entries: 48000 / 1209 etc. never land on a quarter turn except at j = 0, but 770 Hz * 480 = 7.7 turns: the rotation's angle is 0.7 turns
    assert rot[1] == F32(np.cos(6.283185307179586 * ((770 * 480) % 48000) / 48000.0))


@pytest.mark.parametrize("name", sorted(sequences()))
def test_host_equals_model_bit_for_bit(name):
    rows, concealed, params = sequences()[name]
    assert rows.shape == (40, 480)
    hs, hr = run_host(rows, concealed, params)
    ms, mr = run_model(rows, concealed, params)
    for t in range(40):
        assert np.array_equal(hs[t], ms[t]), (name, t, np.flatnonzero(hs[t] != ms[t]))
        assert np.array_equal(hr[t], mr[t]), (name, t, hr[t], mr[t])
    assert np.all(hs[:, 22:] == 0)


def test_sequences_exercise_the_rule():
    """The bit-for-bit sequences are not idle: digits begin and end in them, hostile rows never hit."""
    s = sequences()
    _, rep = run_model(*s["digits_30"])
    assert dm.digits_begun(rep) == "159D" and np.count_nonzero(rep[:, 0] & dm.END) >= 3
    _, rep = run_model(*s["hostile_first"])
    assert not np.any(rep[:len(hostile_rows()), 0] & dm.HIT) and dm.digits_begun(rep) == "3B"
    _, rep = run_model(*s["voice_0.1"])
    assert not np.any(rep[:, 0] & dm.HIT)


def test_params_check_refuses_each_index_at_both_ends_and_nan():
    api.dtmf_params_check(D)
    for i, (lo, hi, open_lo, whole) in enumerate(dm.RANGES):
        ok_lo = np.nextafter(F32(lo), F32(np.inf)) if open_lo else F32(lo)
        bad_lo = F32(lo) if open_lo else np.nextafter(F32(lo), F32(-np.inf))
        for v, ok in ((F32(hi), True), (np.nextafter(F32(hi), F32(np.inf)), False), (ok_lo, not whole or ok_lo == np.floor(ok_lo)), (bad_lo, False), (F32(np.nan), False)) + \
                (((F32(2.5), False), (F32(7.0), True)) if whole else ()):
            p = D.copy()
            p[i] = v
            assert (dm.params_ok(p) == -1) == ok, (i, v)
            if ok:
                api.dtmf_params_check(p)
            else:
                with pytest.raises(api.PercepNetError, match=f"index {i} "):
                    api.dtmf_params_check(p)
    # the FIRST bad index is named
    p = D.copy()
    p[[2, 5]] = (0.5, 0.0)
    with pytest.raises(api.PercepNetError, match="index 2 "):
        api.dtmf_params_check(p)
    with pytest.raises(api.PercepNetError):
        api.dtmf_params_check(D[:6])
    st = np.zeros(24, U32)
    with pytest.raises(api.PercepNetError):
        api.dtmf_frame(p, st, np.zeros(480, F32))
    with pytest.raises(api.PercepNetError):
        api.dtmf_frame(D, st, np.zeros(479, F32))
    with pytest.raises(api.PercepNetError):
        api.dtmf_frame(D, np.zeros(23, U32), np.zeros(480, F32))
    assert not st.any()


# ---- the behaviour of the rule at the default parameters, on the model ------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS)
def test_every_digit_once_in_order(offset):
    rows = dm.keypad(lead=offset)                                    # all 16, amplitude 0.1 a tone, 40 ms on, 40 ms off
    reps, st = dm.run_stream(D, rows)
    assert dm.digits_begun(reps) == dm.DIGITS
    assert int(st[20]) == 16 and int(st[21]) == int.from_bytes(b"*0#D", "big")
    ended = "".join(chr(int(w >> 16) & 0xff) for w in reps[:, 0] if int(w) & dm.END)
    assert ended == dm.DIGITS
    # the same through the host function
    _, hr = run_host(rows[:24])
    assert dm.digits_begun(hr) == dm.DIGITS[:3]


@pytest.mark.parametrize("offset", OFFSETS)
def test_every_digit_once_in_noise(offset):
    rng = np.random.default_rng(offset)
    x = dm.keypad(lead=offset).astype(np.float64).ravel()
    sigma = 0.1 * 10 ** (-15 / 20)                                   # white noise 15 dB under the tones
    assert model_digits(x + rng.standard_normal(x.size) * sigma)[0] == dm.DIGITS


def test_short_tones_are_never_reported():
    for offset in OFFSETS:
        for digit in dm.DIGITS:
            assert model_digits(one_tone(digit, 960, offset))[0] == "", (offset, digit)


def test_frequency_offset():
    for sr in (1, -1):
        for sc in (1, -1):
            for digit in dm.DIGITS:
                assert model_digits(one_tone(digit, 2880, 30, df_row=sr * 0.015, df_col=sc * 0.015))[0] == digit, (sr, sc, digit)
                assert model_digits(one_tone(digit, 2880, 30, df_row=sr * 0.035, df_col=sc * 0.035))[0] == "", (sr, sc, digit)


def test_twist():
    for digit in dm.DIGITS:
        for db, want in ((6, digit), (-6, digit), (10, ""), (-10, "")):
            assert model_digits(one_tone(digit, 2880, 30, amp_row=0.1, amp_col=0.1 * 10 ** (db / 20)))[0] == want, (digit, db)


def test_level():
    for digit in dm.DIGITS:
        for amp, want in ((0.5, digit), (0.008, digit), (0.0025, "")):
            assert model_digits(one_tone(digit, 2880, 30, amp_row=amp))[0] == want, (digit, amp)


def test_no_false_digits():
    t = np.arange(48000) / 48000.0
    for f in dm.FREQS:
        assert model_digits(0.1 * np.sin(2 * np.pi * f * t[:9600])) == ("", 0), f
    assert model_digits(0.1 * np.sin(2 * np.pi * 697 * t[:9600]) + 0.1 * np.sin(2 * np.pi * 770 * t[:9600])) == ("", 0)
    assert model_digits(0.1 * np.sin(2 * np.pi * 350 * t) + 0.1 * np.sin(2 * np.pi * 440 * t)) == ("", 0)       # dial tone, one second
    assert model_digits(np.random.default_rng(20).standard_normal(48000 * 20) * 0.1) == ("", 0)                 # 20 s of white noise
    for f0 in range(80, 401, 7):
        assert model_digits(voice(0.1, 30, f0=float(f0))) == ("", 0), f0


@pytest.mark.parametrize("rate", (8000, 16000, 24000))
def test_through_the_converter(rate):
    """The 16 digits sampled at the low rate, as int16 and through mu-law and A-law, at three amplitudes: nine streams through the
    up-conversion's model; each gives the 16 digits in order."""
    L = 48000 // rate
    n = 480 // L
    cases = [(coding, amp) for coding in ("i16", g711_model.ULAW, g711_model.ALAW) for amp in (0.25, 0.02, 0.008)]
    rows = []
    for coding, amp in cases:
        x = np.concatenate([np.zeros(30 // L)] + [np.concatenate([(lambda i: amp * (np.sin(2 * np.pi * dm.FREQS[i // 4] * np.arange(1920 // L) / rate) +
                                                                             np.sin(2 * np.pi * dm.FREQS[4 + i % 4] * np.arange(1920 // L) / rate)))(i),
                                                               np.zeros(1920 // L)]) for i in range(16)] + [np.zeros(2 * n)])
        x = np.concatenate([x, np.zeros((-x.size) % n)])
        v = np.round(x * 32767.0).astype(np.int16)
        if coding != "i16":
            v = g711_model.decode(coding, g711_model.encode(coding, v))
        rows.append(rate_model.from_i16(v).reshape(-1, n))
    x_low = np.stack(rows)                                            # [9, frames, n]
    up = rate_model.Up(len(cases), L, rate_model.taps_f32(L, False))
    st = dm.fresh(len(cases))
    begun = [""] * len(cases)
    for t in range(x_low.shape[1]):
        st, rep = dm.frame(D, st, up(x_low[:, t]))
        for s in range(len(cases)):
            if int(rep[s, 0]) & dm.BEGIN:
                begun[s] += chr(int(rep[s, 0] >> 8) & 0xff)
    for case, got in zip(cases, begun):
        assert got == dm.DIGITS, (rate, case, got)


def test_debounce_edges():
    p1 = D.copy()
    p1[[dm.ON_FRAMES, dm.OFF_FRAMES]] = 1
    # on_frames = off_frames = 1: '8' turns into '2' in the middle of a row, so that row's window is three quarters '8' and the next
    # one three quarters '2', both hits -> END of the old and BEGIN of the new in ONE frame.  The two share their column tone, which
    # keeps both windows pure, and their row tones lie 155 Hz apart, three times the window's 50 Hz resolution, which keeps the quarter
    # of the other digit under `rel` (neighbouring rows, 82 Hz apart, leak too much for that and end the first digit a frame early)
    x = np.concatenate([np.zeros(240), dm.dual_tone("8", 2400), dm.dual_tone("2", 2400), np.zeros(1440)])
    reps, _ = dm.run_stream(p1, frames_of(x))
    both = [t for t, w in enumerate(reps[:, 0]) if int(w) & dm.END and int(w) & dm.BEGIN]
    assert len(both) == 1 and dm.digits_begun(reps) == "82"
    w = int(reps[both[0], 0])
    assert (w >> 8) & 0xff == ord("2") and (w >> 16) & 0xff == ord("8") and int(reps[both[0], 1]) == 1 and int(reps[both[0], 2]) == 2
    assert int(reps[both[0], 3]) == (ord("8") << 8 | ord("2"))
    # ... and with on_frames = 1 the digit is reported two frames earlier than at the default of 3
    first = lambda r: next(t for t, w in enumerate(r[:, 0]) if int(w) & dm.BEGIN)
    assert first(dm.run_stream(D, frames_of(x))[0]) == first(reps) + 2
    # a one-frame dropout inside a digit does not end it at off_frames = 2; dur counts the dropout, count stays 1.  Every sample lies in
    # two windows, so the disturbance that spoils exactly ONE is a 400-sample burst of another sound (400 Hz, the dual tone's power)
    # across the boundary of rows 8 and 9: their window keeps 560 tone samples of 960, P[r] + P[c] = 2 * 280^2 = 0.68 of the 240 E it
    # needs; the windows on either side keep 760, 2 * 380^2 = 1.25 of it
    x = np.concatenate([np.zeros(60), dm.dual_tone("6", 7200)])
    cut = slice(9 * 480 - 200, 9 * 480 + 200)
    x[cut] = 0.1 * np.sqrt(2.0) * np.sin(2 * np.pi * 400.0 * np.arange(400) / 48000.0)
    reps, st = dm.run_stream(D, frames_of(x)[:14])
    assert dm.digits_begun(reps) == "6" and not np.any(reps[:, 0] & dm.END) and int(st[20]) == 1 and int(st[18]) & 0xff == ord("6")
    assert [t for t in range(3, 14) if not int(reps[t, 0]) & dm.HIT] == [9], "one window missed"
    p_off1 = D.copy()
    p_off1[dm.OFF_FRAMES] = 1
    assert dm.digits_begun(dm.run_stream(p_off1, frames_of(x)[:14])[0]) == "66", "at off_frames = 1 the same dropout ends the digit"
    t0 = first(reps)
    assert [int(reps[t, 1]) for t in range(t0, 14)] == list(range(3, 3 + 14 - t0)), "dur: the run at BEGIN, then one a frame"
    # dur of the ended digit, and last4 over more than four digits
    reps, st = dm.run_stream(D, dm.keypad("12345", lead=30))
    ends = [(chr(int(w[0] >> 16) & 0xff), int(w[1])) for w in reps if int(w[0]) & dm.END]
    assert [e[0] for e in ends] == list("12345") and all(4 <= e[1] <= 6 for e in ends), ends
    assert int(st[21]) == int.from_bytes(b"2345", "big") and int(st[20]) == 5
    # a concealed frame changes no state word and repeats cur with HELD_LOST
    rows = frames_of(np.concatenate([np.zeros(30), dm.dual_tone("9", 4800)]))
    reps, st = dm.run_stream(D, rows[:6])
    st2, rep = dm.step(D, st[None], dm.half_sums(rows[6:7]), np.array([True]))
    assert np.array_equal(st2[0], st) and int(rep[0, 0]) == dm.ON | dm.HELD_LOST | ord("9") << 8 and int(rep[0, 1]) == int(st[19])
    hst = st.copy()
    flags, hrep = api.dtmf_frame(D, hst, rows[6], concealed=True)
    assert np.array_equal(hst, st) and flags == dm.ON | dm.HELD_LOST and int(hrep["word0"]) == int(rep[0, 0])


def test_cli_refuses_bad_dtmf_options(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "in0.pcm").write_bytes(bytes(1920))
    files = ["in0.pcm", "out0.pcm"]
    for opts, words in ((["--dtmf", "--dtmf-on-frames", "0"], ("--dtmf-on-frames", "[1, 100]")), (["--dtmf", "--dtmf-on-frames", "2.5"], ("--dtmf-on-frames", "whole number")),
                        (["--dtmf", "--dtmf-on-frames", "101"], ("--dtmf-on-frames", "[1, 100]")), (["--dtmf", "--dtmf-on-frames", "nan"], ("--dtmf-on-frames",)),
                        (["--dtmf", "--dtmf-on-frames", "3x"], ("--dtmf-on-frames", "'3x'")), (["--dtmf-on-frames", "2"], ("--dtmf-on-frames needs --dtmf",))):
        run = subprocess.run([exe] + opts + files, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and all(w in run.stderr for w in words), (opts, run.stderr)
        assert not (tmp_path / "out0.pcm").exists(), opts
    run = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "[--dtmf [--dtmf-on-frames N]]" in run.stderr and "[--agc RMS [--agc-max-gain G]]" in run.stderr


def test_rules_under_sanitizers(tmp_path):
    """tests/c/dtmf_sanitize.cpp = pn_dtmf_rules.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: whole frames over a row of exactly 480 floats, a state of exactly 24 words and a report of exactly 4,
    the tables at their exact sizes, the hostile rows, every parameter's edges, the counters' saturation."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "dtmf_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "dtmf_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
