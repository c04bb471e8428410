"""DTMF removal on the rate converter: the host-only surface, no GPU (include/percepnet_hip.h "DTMF removal"; the rule lives in the
HIP-free percepnet_amd/csrc/pn_dtmf_clamp_rules.h): pn_dtmf_clamp_frame against the numpy model (tests/dtmf_clamp_model.py) bit for bit
in state, row and report; what the rule guarantees for clean tones at the default parameters; the on_frames + pre condition; the RFC
4733 payloads; every refusal; the CLI's refusals that need no device; and the rule under the address and undefined-behaviour sanitizers
in a stand-alone program (tests/c/dtmf_clamp_sanitize.cpp).

The engine is not here: the audio a frame hands to the stage is the stream's input row of six frames ago (dcm.delayed), which is what
the engine's delay of whole rows makes of it and all that the bookkeeping depends on.  The detector's reports come from its model
(tests/dtmf_model.py), whose half sums are computed once for all cases and shared by every parameter set.

The clean-tone cases: digits 1 D 5 # of 50, 80, 120, 160 and 200 ms at the 24 start offsets 0, 20, .., 460 in a row, over white noise
40 dB under the tone: 480 cases, run as 480 streams of one model."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import dtmf_clamp_model as dcm
from tests import dtmf_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32
D, C = dm.DEFAULTS, dcm.DEFAULTS
LEAD = 8                                                                 # silent rows in front of the tone's row
DIGITS, LENGTHS_MS, OFFSETS = "1D5#", (50, 80, 120, 160, 200), tuple(range(0, 480, 20))
T = LEAD + 1 + 20 + 4 + dcm.DELAY + 3                                    # the longest tone, the detector's END, the delay, the fade in


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    L = api.load_library()
    ct, st, rot = api.dtmf_tables()
    dm.use_tables(ct, st, rot)
    return L


_cases = {}


def cases():
    """-> (x [n, T, 480] float32, span [n, 2]: the tone's first sample and the one behind its last, sums [T, n, 17]: the detector's half
    sums), computed once"""
    if not _cases:
        rng = np.random.default_rng(4733)
        xs, spans = [], []
        for digit in DIGITS:
            for ms in LENGTHS_MS:
                for off in OFFSETS:
                    n = ms * 48
                    x = rng.standard_normal(T * 480) * (0.1 * 10 ** (-40 / 20))    # the dual tone's RMS is 0.1 (two sines of amplitude 0.1): noise 40 dB under it
                    a = LEAD * 480 + off
                    x[a:a + n] += dm.dual_tone(digit, n)
                    xs.append(x.astype(F32).reshape(T, 480))
                    spans.append((a, a + n))
        x = np.stack(xs)
        x.setflags(write=False)
        sums = np.stack([dm.half_sums(x[:, t]) for t in range(T)])
        sums.setflags(write=False)
        _cases.update(x=x, span=np.array(spans), sums=sums)
    return _cases["x"], _cases["span"], _cases["sums"]


_dets = {}


def detector(on_frames):
    """-> the detector model's reports [T, n, 4] over the cases at the default parameters but for on_frames"""
    if on_frames not in _dets:
        x, _, sums = cases()
        p = D.copy()
        p[dm.ON_FRAMES] = on_frames
        st, reps = dm.fresh(x.shape[0]), []
        for t in range(T):
            st, rep = dm.step(p, st, sums[t])
            reps.append(rep)
        _dets[on_frames] = np.stack(reps)
        _dets[on_frames].setflags(write=False)
    return _dets[on_frames]


_flags = {}


def clamp_flags(on_frames, params):
    """Every clean-tone case through the HOST FUNCTION pn_dtmf_clamp_frame, frame by frame from the fresh state, the audio being the
    case's input of six frames ago; state, row and report are compared with the model bit for bit on the way.  -> the host function's
    flags [T, n].  Made once per setting"""
    key = (on_frames, tuple(int(v) for v in params))
    if key not in _flags:
        x, _, _ = cases()
        det = detector(on_frames)
        prm = np.asarray(params, np.int32)
        n = det.shape[1]
        flags = np.zeros((T, n), U32)
        for s in range(n):
            rows = dcm.delayed(x[s])
            st, mst = np.zeros(dcm.STATE_WORDS, U32), [0, 0, 0, 0]
            for t in range(T):
                y = rows[t].copy()
                f, rep = api.dtmf_clamp_frame(prm, st, det[t, s], y)
                mst, mrep, kind = dcm.decide(prm, mst, det[t, s])
                assert st.tolist() == mst and [int(rep["flags"]), int(rep["event"]), int(rep["event_end"]), int(rep["muted"])] == mrep and f == mrep[0], (key, s, t)
                assert y.tobytes() == dcm.apply(kind, rows[t]).tobytes(), (key, s, t, "row")
                flags[t, s] = f
        flags.setflags(write=False)
        _flags[key] = flags
    return _flags[key]


def run_host(params, dets, rows):
    """one stream through pn_dtmf_clamp_frame from the fresh state -> (states [T, 4], rows' [T, 480], reports [T, 4])"""
    st = np.zeros(dcm.STATE_WORDS, U32)
    states, out, reps = [], [], []
    for t in range(len(rows)):
        y = np.array(rows[t], F32)
        flags, rep = api.dtmf_clamp_frame(params, st, dets[t], y)
        assert flags == int(rep["flags"])
        states.append(st.copy()); out.append(y); reps.append(np.array([rep["flags"], rep["event"], rep["event_end"], rep["muted"]], U32))
    return np.stack(states), np.stack(out), np.stack(reps)


def run_model(params, dets, rows):
    st = [0, 0, 0, 0]
    states, out, reps = [], [], []
    for t in range(len(rows)):
        st, rep, kind = dcm.decide(params, st, dets[t])
        states.append(np.array(st, U32)); out.append(dcm.apply(kind, np.asarray(rows[t], F32))); reps.append(np.array(rep, U32))
    return np.stack(states), np.stack(out), np.stack(reps)


def assert_same(name, params, dets, rows):
    hs, hy, hr = run_host(params, dets, rows)
    ms, my, mr = run_model(params, dets, rows)
    for t in range(len(rows)):
        assert np.array_equal(hs[t], ms[t]), (name, t, hs[t], ms[t])
        assert np.array_equal(hr[t], mr[t]), (name, t, hr[t], mr[t])
        assert hy[t].tobytes() == my[t].tobytes(), (name, t, "row")
    return mr


def rows_of(*parts):
    """the parts one after the other, padded with silence to whole frames -> float32 [frames, 480]"""
    x = np.concatenate(parts)
    return np.concatenate([x, np.zeros((-x.size) % 480)]).astype(F32).reshape(-1, 480)


def hostile(rows):
    """a copy of rows [T, 480] with a NaN row, an inf row, a 3e38 row and a row of -0.0 every fourth frame, so that each meets every kind of decision"""
    y = np.array(rows, F32)
    fills = (np.nan, np.inf, -np.inf, 3e38, -0.0, 1e-41)
    for t in range(1, len(y), 2):
        y[t] = F32(fills[(t // 2) % len(fills)])
    return y


# ---- constants, defaults, refusals ---------------------------------------------------------------------------------------------------
def test_defaults_and_constants():
    assert np.array_equal(api.dtmf_clamp_default_params(), C) and C.tolist() == [1, 0, 10, 80] and api.DTMF_CLAMP_N_PARAMS == 4
    assert (api.DTMF_CLAMP_ON, api.DTMF_CLAMP_MUTED, api.DTMF_CLAMP_FADE_OUT, api.DTMF_CLAMP_FADE_IN, api.DTMF_CLAMP_LATE, api.DTMF_CLAMP_EVENT, api.DTMF_CLAMP_EVENT_END) == \
        (dcm.ON, dcm.MUTED, dcm.FADE_OUT, dcm.FADE_IN, dcm.LATE, dcm.EVENT, dcm.EVENT_END) == (1, 2, 4, 8, 16, 32, 64)
    assert api.DTMF_CLAMP_STATE_WORDS == dcm.STATE_WORDS == 4 and api.DTMF_CLAMP_REPORT_WORDS == dcm.REPORT_WORDS == 4 and api.DTMF_CLAMP_REPORT_DTYPE.itemsize == 16
    assert api.DTMF_CLAMP_DELAY == dcm.DELAY == 6
    from tests import report_model
    assert report_model.DELAY_FRAMES == dcm.DELAY


def test_params_check_refuses_each_index_at_both_ends():
    api.dtmf_clamp_params_check(C)
    api.dtmf_clamp_params_check(C, D)
    for i, (lo, hi) in enumerate(dcm.RANGES):
        for v, ok in ((lo, True), (hi, True), (lo - 1, False), (hi + 1, False), (-2 ** 31, False), (2 ** 31 - 1, False)):
            p = C.copy()
            p[i] = v
            assert (dcm.params_ok(p) == -1) == ok
            if ok:
                api.dtmf_clamp_params_check(p)
            else:
                with pytest.raises(api.PercepNetError, match=f"index {i} "):
                    api.dtmf_clamp_params_check(p)
    p = C.copy()
    p[[1, 3]] = (9, 0)                                                   # the FIRST bad index is named
    with pytest.raises(api.PercepNetError, match="index 1 "):
        api.dtmf_clamp_params_check(p)
    with pytest.raises(api.PercepNetError):
        api.dtmf_clamp_params_check(C[:3])
    with pytest.raises(api.PercepNetError, match="whole"):
        api.dtmf_clamp_params_check([1.5, 0, 10, 80])
    st, y = np.zeros(4, U32), np.ones(480, F32)
    with pytest.raises(api.PercepNetError, match="index 1 "):
        api.dtmf_clamp_frame(p, st, None, y)
    with pytest.raises(api.PercepNetError):
        api.dtmf_clamp_frame(C, st, None, np.ones(479, F32))
    with pytest.raises(api.PercepNetError):
        api.dtmf_clamp_frame(C, np.zeros(3, U32), None, y)
    with pytest.raises(api.PercepNetError):
        api.dtmf_clamp_frame(C, st, np.zeros(3, U32), y)
    assert not st.any() and np.all(y == 1.0)


def test_the_in_time_condition_is_refused_naming_the_values():
    """on_frames + pre <= 5 is accepted, anything beyond refused with both values in the message: the check the converter's three
    setters share (pn_dtmf_clamp_params_check with the detector's parameters)"""
    for on_frames in range(1, 9):
        for pre in range(0, 5):
            p, d = C.copy(), D.copy()
            p[dcm.PRE], d[dm.ON_FRAMES] = pre, on_frames
            assert dcm.in_time(on_frames, pre) == (on_frames + pre <= 5)
            if on_frames + pre <= 5:
                api.dtmf_clamp_params_check(p, d)
            else:
                with pytest.raises(api.PercepNetError, match=f"on_frames {on_frames} \\+ pre {pre} > 5"):
                    api.dtmf_clamp_params_check(p, d)
            api.dtmf_clamp_params_check(p)                               # without the detector's parameters only the ranges count
    bad = D.copy()
    bad[dm.ON_FRAMES] = 2.5
    with pytest.raises(api.PercepNetError, match="index 5 "):
        api.dtmf_clamp_params_check(C, bad)


# ---- payloads --------------------------------------------------------------------------------------------------------------------------
def test_payloads():
    for ev, ch in enumerate("0123456789*#ABCD"):
        for end in (False, True):
            want = ev << 24 | (1 << 23 if end else 0) | 10 << 16 | 5 * 80
            assert api.dtmf_event_payload(ch, end, 10, 5, 80) == dcm.payload(ord(ch), end, 10, 5, 80) == want, (ch, end)
            assert want.to_bytes(4, "big") == bytes([ev, (0x80 if end else 0) | 10, 400 >> 8, 400 & 0xff]), "event, E R volume, duration in network order"
    for dur, ts, want in ((819, 80, 65520), (820, 80, 65535), (1, 65535, 65535), (2, 65535, 65535), (0xffffffff, 65535, 65535), (0x80000000, 1, 65535), (65535, 1, 65535), (65534, 1, 65534)):
        assert api.dtmf_event_payload("0", False, 0, dur, ts) == dcm.payload(ord("0"), False, 0, dur, ts) == want, (dur, ts)
    assert api.dtmf_event_payload("0", False, 0, 1, 1) == 1, "the least real payload is not 0"
    for digit in (0, ord("E"), ord("a"), ord(" "), 255):
        assert api.dtmf_event_payload(digit, False, 10, 3, 80) == dcm.payload(digit, False, 10, 3, 80) == 0
    assert api.dtmf_event_payload("5", False, 64, 3, 80) == 0 and api.dtmf_event_payload("5", False, 10, 3, 0) == 0 and api.dtmf_event_payload("5", False, 10, 3, 65536) == 0


def test_events_follow_the_detector():
    """Through a digit: the ongoing payload with E = 0 and the detector's dur, repeated by a concealed frame; in the END frame the ended
    payload with E = 1 and the dur of the previous frame's ongoing event; 0 when idle"""
    x = rows_of(np.zeros(500), dm.dual_tone("7", 4800), np.zeros(4800))[:20]
    concealed = np.zeros(20, bool)
    concealed[[6, 7]] = True
    det, _ = dm.run_stream(D, x, concealed)
    p = np.array([1, 0, 33, 160], np.int32)
    _, _, rep = run_host(p, det, dcm.delayed(x))
    ends = 0
    for t in range(20):
        cur, dur = int(det[t, 0]) >> 8 & 0xff, int(det[t, 1])
        if cur:
            assert cur == ord("7") and int(rep[t, 0]) & dcm.EVENT and int(rep[t, 1]) == 7 << 24 | 33 << 16 | dur * 160
        else:
            assert not int(rep[t, 0]) & dcm.EVENT and int(rep[t, 1]) == 0
        if int(det[t, 0]) & dm.END:
            ends += 1
            assert int(rep[t, 0]) & dcm.EVENT_END and int(rep[t, 2]) == 7 << 24 | 1 << 23 | 33 << 16 | int(det[t - 1, 1]) * 160 and int(det[t, 1]) == int(det[t - 1, 1])
        else:
            assert not int(rep[t, 0]) & dcm.EVENT_END and int(rep[t, 2]) == 0
    assert ends == 1 and int(det[7, 0]) & dm.HELD_LOST and int(rep[7, 1]) == int(rep[6, 1]) == int(rep[5, 1]) != 0, "a concealed frame repeats the event"


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------------
def test_host_equals_model_on_the_clean_tone_cases():
    """all 480 cases, every frame: state, row and report (the comparison is inside clamp_flags)"""
    flags = clamp_flags(3, C)
    assert flags.shape == (T, 480)
    assert int(np.bitwise_or.reduce(flags.ravel())) == dcm.ON | dcm.MUTED | dcm.FADE_OUT | dcm.FADE_IN | dcm.EVENT | dcm.EVENT_END


_seqs = {}
SEQUENCES = ("back_to_back_0_8", "back_to_back_1_0", "back_to_back_2_3", "back_to_back_4_0", "back_to_back_hostile", "concealed_head", "concealed_inside",
             "concealed_tail", "detection_off", "from_frame_0", "hostile", "late_5_1", "late_6_0")


def sequences():
    """name -> (clamp params, detector reports [T, 4], audio rows [T, 480]), made once and inside a test: behind the `lib` fixture, so
    the detector's model computes with the library's tables"""
    seqs = _seqs
    if seqs:
        return seqs
    # two different digits back to back at on_frames = off_frames = 1: END and BEGIN in one frame (tests/test_dtmf_host.py test_debounce_edges)
    p1 = D.copy()
    p1[[dm.ON_FRAMES, dm.OFF_FRAMES]] = 1
    x = rows_of(np.zeros(240), dm.dual_tone("8", 2400), dm.dual_tone("2", 2400), np.zeros(7200))
    det, _ = dm.run_stream(p1, x)
    assert any(int(w) & dm.END and int(w) & dm.BEGIN for w in det[:, 0])
    for pre, post in ((1, 0), (4, 0), (0, 8), (2, 3)):
        seqs[f"back_to_back_{pre}_{post}"] = (np.array([pre, post, 10, 80], np.int32), det, dcm.delayed(x))
    seqs["back_to_back_hostile"] = (C, det, hostile(dcm.delayed(x)))
    # concealed frames inside a digit, and among its first hits (the known limit)
    x = rows_of(np.zeros(700), dm.dual_tone("C", 7200), np.zeros(6500))
    for name, lost in (("inside", (8, 9, 12)), ("head", (2, 3)), ("tail", (16, 17, 18))):
        c = np.zeros(len(x), bool)
        c[list(lost)] = True
        det, _ = dm.run_stream(D, x, c)
        seqs[f"concealed_{name}"] = (C, det, dcm.delayed(x))
    seqs["hostile"] = (C, det, hostile(dcm.delayed(x)))
    # the first frames of a fresh state: a digit that is already there in frame 0, and detection off all along
    x = rows_of(dm.dual_tone("0", 3000), np.zeros(5160))
    det, _ = dm.run_stream(D, x)
    seqs["from_frame_0"] = (np.array([2, 8, 0, 1], np.int32), det, hostile(dcm.delayed(x)))      # (pre = 2: the longest guard in time at on_frames = 3)
    seqs["detection_off"] = (C, np.zeros((len(x), 4), U32), x)
    # forced past the condition: a verdict that comes late
    for on_frames, pre in ((5, 1), (6, 0)):
        p = D.copy()
        p[dm.ON_FRAMES] = on_frames
        x = rows_of(np.zeros(1000), dm.dual_tone("#", 7200), np.zeros(6200))
        det, _ = dm.run_stream(p, x)
        seqs[f"late_{on_frames}_{pre}"] = (np.array([pre, 0, 10, 80], np.int32), det, dcm.delayed(x))
    assert sorted(seqs) == sorted(SEQUENCES)
    return seqs


@pytest.mark.parametrize("name", SEQUENCES)
def test_host_equals_model_bit_for_bit(name):
    params, det, rows = sequences()[name]
    rep = assert_same(name, params, det, rows)
    flags = int(np.bitwise_or.reduce(rep[:, 0]))
    if name.startswith("late"):
        assert flags & dcm.LATE
    elif name == "detection_off":
        assert flags == dcm.ON and not rep[:, 1:].any()
    else:
        assert flags & dcm.MUTED and not flags & dcm.LATE
    if name.startswith("back_to_back"):
        both = [t for t in range(len(det)) if int(det[t, 0]) & dm.END and int(det[t, 0]) & dm.BEGIN]
        t = both[0]
        assert int(rep[t, 0]) & dcm.EVENT and int(rep[t, 0]) & dcm.EVENT_END
        assert int(rep[t, 2]) == dcm.payload(ord("8"), True, 10, int(det[t - 1, 1]), 80) and int(rep[t, 1]) == dcm.payload(ord("2"), False, 10, int(det[t, 1]), 80)


def test_a_nan_in_a_removed_row_is_gone_and_a_row_at_unity_is_not_touched():
    params, det, rows = sequences()["hostile"]
    _, y, rep = run_host(params, det, rows)
    for t in range(len(rows)):
        f = int(rep[t, 0])
        if f & dcm.MUTED or f & (dcm.FADE_IN | dcm.FADE_OUT) == dcm.FADE_IN | dcm.FADE_OUT:
            assert y[t].tobytes() == bytes(1920), t
        elif not f & (dcm.FADE_IN | dcm.FADE_OUT):
            assert y[t].tobytes() == rows[t].tobytes(), t
    assert any(np.isnan(rows[t]).all() and int(rep[t, 0]) & dcm.MUTED for t in range(len(rows))), "a NaN row met a muted frame"


# ---- what the rule guarantees for clean tones ------------------------------------------------------------------------------------------
def assert_covered(flags, det, label):
    """every input row that holds a tone sample is muted six frames later; nothing is LATE; a fade out in front, a fade in behind.  A
    tone the detector does not report (one shorter than on_frames hits) stays, untouched.  -> the digits found"""
    _, span, _ = cases()
    found = 0
    for s in range(flags.shape[1]):
        first, last = span[s, 0] // 480, (span[s, 1] - 1) // 480          # the input rows that hold a tone sample
        muted = [t for t in range(T) if int(flags[t, s]) & dcm.MUTED]
        if not np.any(det[:, s, 0] & dm.BEGIN):
            assert np.all(flags[:, s] == dcm.ON), (label, s, "no digit, no removal")
            continue
        found += 1
        assert muted, (label, s)
        assert not np.any(flags[:, s] & dcm.LATE), (label, s, "late")
        assert muted == list(range(muted[0], muted[-1] + 1)), (label, s, "one stretch")
        for r in range(first, last + 1):
            assert r + dcm.DELAY in muted, (label, s, r, "a tone sample outside the muted rows")
        assert int(flags[muted[0] - 1, s]) & dcm.FADE_OUT and int(flags[muted[-1] + 1, s]) & dcm.FADE_IN, (label, s)
        assert [t for t in range(T) if int(flags[t, s]) & (dcm.FADE_OUT | dcm.FADE_IN)] == [muted[0] - 1, muted[-1] + 1], (label, s)
    return found


def test_clean_tones_are_removed_whole_at_the_defaults():
    """the guarantees, read off the HOST FUNCTION's reports over all 480 cases"""
    _, span, _ = cases()
    det = detector(3)
    assert np.all(np.count_nonzero(det[:, :, 0] & dm.BEGIN, axis=0) == 1), "every digit is found, once"
    flags = clamp_flags(3, C)
    assert assert_covered(flags, det, "defaults") == flags.shape[1]
    # rows wholly inside a tone, said once more on their own: muted six frames later
    for s in range(flags.shape[1]):
        for r in range(-(-span[s, 0] // 480), span[s, 1] // 480):
            assert int(flags[r + dcm.DELAY, s]) & dcm.MUTED
    beyond = np.array([480 * np.count_nonzero(flags[:, s] & dcm.MUTED) - (span[s, 1] - span[s, 0]) for s in range(flags.shape[1])])
    print("samples muted beyond the tone: min", beyond.min(), "max", beyond.max())
    # the figures the documents quote (DESIGN.md 4.8 "DTMF removal"): a guard row, the unfilled part of the first and last row and the
    # detector's gap frame make 1440 where nothing sits on a threshold; a tone that starts or ends within samples of a row edge
    # gains or loses one row
    assert (int(beyond.min()), int(beyond.max())) == (960, 1920)


@pytest.mark.parametrize("on_frames,pre", ((5, 0), (4, 1), (3, 2), (1, 4), (1, 1)))
def test_in_time_settings_are_never_late(on_frames, pre):
    p, d = C.copy(), D.copy()
    p[dcm.PRE], d[dm.ON_FRAMES] = pre, on_frames
    api.dtmf_clamp_params_check(p, d)
    det = detector(on_frames)
    found = assert_covered(clamp_flags(on_frames, p), det, (on_frames, pre))
    print(f"on_frames {on_frames} pre {pre}: {found} of {det.shape[1]} digits found")
    # the shortest tones are 50 ms, five rows: they give four or five hits in a row, so only five hits in a row can miss a digit: two
    # of the 480 (the figure DESIGN.md quotes)
    assert found == (478 if on_frames == 5 else det.shape[1])


@pytest.mark.parametrize("on_frames,pre", ((5, 1), (6, 0)))
def test_past_the_condition_the_host_function_reports_late(on_frames, pre):
    p, d = C.copy(), D.copy()
    p[dcm.PRE], d[dm.ON_FRAMES] = pre, on_frames
    with pytest.raises(api.PercepNetError, match=f"on_frames {on_frames} \\+ pre {pre} > 5"):
        api.dtmf_clamp_params_check(p, d)
    flags = clamp_flags(on_frames, p)                                    # through the host function itself, which does not check the condition
    n_late = int(np.count_nonzero(np.any(flags & dcm.LATE, axis=0)))
    print(f"on_frames {on_frames} pre {pre}: LATE in {n_late} of {flags.shape[1]} cases")
    assert n_late == {(5, 1): 478, (6, 0): 385}[on_frames, pre], "the figures DESIGN.md quotes"


# ---- the CLI's refusals that need no device --------------------------------------------------------------------------------------------
def test_cli_refuses_bad_dtmf_clamp_options(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "in0.pcm").write_bytes(bytes(1920))
    files = ["in0.pcm", "out0.pcm"]
    for opts, words in ((["--dtmf-clamp"], ("--dtmf-clamp needs --dtmf",)), (["--dtmf", "--dtmf-guard", "1,0"], ("--dtmf-guard needs --dtmf-clamp",)),
                        (["--dtmf", "--dtmf-clamp", "--dtmf-guard", "5,0"], ("--dtmf-guard", "'5,0'")), (["--dtmf", "--dtmf-clamp", "--dtmf-guard", "1,9"], ("--dtmf-guard", "'1,9'")),
                        (["--dtmf", "--dtmf-clamp", "--dtmf-guard", "1"], ("--dtmf-guard", "'1'")), (["--dtmf", "--dtmf-clamp", "--dtmf-guard", "1,0x"], ("--dtmf-guard", "'1,0x'")),
                        (["--dtmf", "--dtmf-clamp", "--dtmf-guard", "3,0"], ("on_frames 3", "pre 3")),
                        (["--dtmf", "--dtmf-on-frames", "5", "--dtmf-clamp"], ("on_frames 5", "pre 1"))):
        run = subprocess.run([exe] + opts + files, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and all(w in run.stderr for w in words), (opts, run.stderr)
        assert not (tmp_path / "out0.pcm").exists(), opts
    run = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "[--dtmf [--dtmf-on-frames N]] [--dtmf-clamp [--dtmf-guard PRE,POST]]" in run.stderr


def test_rules_under_sanitizers(tmp_path):
    """tests/c/dtmf_clamp_sanitize.cpp = pn_dtmf_clamp_rules.h and pn_dtmf_rules.h (+ pn_model.cpp for the error string) built WITHOUT
    HIP by plain g++ with -fsanitize=address,undefined, a stand-alone program with its own main: the detector's rule drives the stage
    over a keypad sequence through a delay line of six exactly-sized rows; every row kind, hostile rows, every parameter's edges, the
    shifts at their ends, the saturations."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "dtmf_clamp_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "dtmf_clamp_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
