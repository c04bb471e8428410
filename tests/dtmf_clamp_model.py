"""The numpy model of the rate converter's DTMF removal (include/percepnet_hip.h "DTMF removal"; the rule:
percepnet_amd/csrc/pn_dtmf_clamp_rules.h; kernel percepnet_amd/csrc/pn_rate_dtmf_clamp.hip).  The decision is integer work; the two ramps
are one float32 quotient and one float32 product per sample, so the host function (pn_dtmf_clamp_frame) and the kernel's rows, states and
reports are compared with it bit for bit.  It is vectorised over streams: state [n, 4] uint32 words, detector report rows [n, 4],
audio rows [n, 480], report [n, 4].

The rule, for one frame of a stream with removal on; det = the detector's report row of this frame (tests/dtmf_model.py), x its row of
y48, which is the stream's input row of DELAY = 6 frames ago:
    marks     marks <<= 1; det all zero (detection off): nothing; else BEGIN: bits 0..min(dur, 31) set; else cur != 0: bit 0 set
    decision  M(k) = any bit of marks in [k - pre, k + post] clipped to 0..31; m = M(6), m_next = M(5); e0 = m or m_next: the gain is 0
              at the row's end; s0 = cut: it is 0 at its start
    the row   m: +0.0 everywhere, MUTED, muted += 1 (saturating), LATE unless s0
              not m, not s0, e0: x[j] * (float32(479 - j) / float32(480)), FADE_OUT
              not m, s0, not e0: x[j] * (float32(j + 1) / float32(480)), FADE_IN
              not m, s0, e0: +0.0 everywhere, FADE_OUT | FADE_IN
              otherwise the row stays
              cut = e0
    events    payload = event << 24 | E << 23 | volume << 16 | min(dur * ts_per_frame, 65535); cur != 0: ongoing (E = 0), EVENT;
              END: the ended digit with E = 1 and the dur of the previous frame's ongoing event (w3, or 1 where that is 0), EVENT_END;
              w3 = dur if cur else 0
Report: word 0 flags, word 1 the ongoing payload, word 2 the ended payload, word 3 rows muted so far; a stream that is not on: zeros."""
import numpy as np

from tests import dtmf_model as dm

F32 = np.float32
U32 = np.uint32
FRAME = 480
DELAY = 6
N_PARAMS = 4
PRE, POST, VOLUME, TS_PER_FRAME = range(4)
ON, MUTED, FADE_OUT, FADE_IN, LATE, EVENT, EVENT_END = 1, 2, 4, 8, 16, 32, 64
STATE_WORDS, REPORT_WORDS = 4, 4
DEFAULTS = np.array([1, 0, 10, 80], np.int32)
RANGES = ((0, 4), (0, 8), (0, 63), (1, 65535))
KEEP, ZERO, DOWN, UP = range(4)
WD = (np.arange(FRAME - 1, -1, -1).astype(F32) / F32(480.0)).astype(F32)      # float32(479 - j) / float32(480): one rounding
WU = (np.arange(1, FRAME + 1).astype(F32) / F32(480.0)).astype(F32)
# ... which is also the double quotient narrowed once
assert np.array_equal(WD, (np.arange(FRAME - 1, -1, -1) / 480.0).astype(F32)) and np.array_equal(WU, (np.arange(1, FRAME + 1) / 480.0).astype(F32))
EVENT_CODES = {ord(ch): i for i, ch in enumerate("0123456789*#ABCD")}


def params_ok(p):
    """-> the first bad index, or -1"""
    for i, (lo, hi) in enumerate(RANGES):
        if not lo <= int(p[i]) <= hi:
            return i
    return -1


def in_time(on_frames, pre):
    return int(on_frames) + int(pre) <= DELAY - 1


def payload(digit, end, volume, dur, ts_per_frame):
    """digit: the ASCII code -> the 32-bit payload, 0 for no digit"""
    ev = EVENT_CODES.get(int(digit))
    if ev is None:
        return 0
    return ev << 24 | (1 << 23 if end else 0) | (int(volume) & 63) << 16 | min(int(dur) * int(ts_per_frame), 65535)


def _any(marks, k, pre, post):
    lo, hi = max(k - pre, 0), min(k + post, 31)
    return (int(marks) & ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)) != 0


def decide(params, st, det):
    """One stream: st [4] and det [4] as Python ints -> (st', report [4], kind)"""
    pre, post, vol, ts = (int(v) for v in params)
    d0, d1 = int(det[0]), int(det[1])
    det_on = any(int(v) for v in det)
    cur, ended, dur = d0 >> 8 & 0xff, d0 >> 16 & 0xff, d1
    marks = (int(st[0]) << 1) & 0xffffffff
    if det_on:
        if d0 & dm.BEGIN:
            marks |= 0xffffffff if dur >= 31 else (1 << (dur + 1)) - 1
        elif cur:
            marks |= 1
    m, m_next = _any(marks, DELAY, pre, post), _any(marks, DELAY - 1, pre, post)
    e0, s0 = m or m_next, bool(int(st[1]) & 1)
    flags, muted = ON, int(st[2])
    if m:
        kind, flags, muted = ZERO, flags | MUTED | (0 if s0 else LATE), min(muted + 1, 0xffffffff)
    elif not s0 and e0:
        kind, flags = DOWN, flags | FADE_OUT
    elif s0 and not e0:
        kind, flags = UP, flags | FADE_IN
    elif s0 and e0:
        kind, flags = ZERO, flags | FADE_OUT | FADE_IN
    else:
        kind = KEEP
    ongoing = payload(cur, False, vol, dur, ts) if det_on and cur else 0
    done = payload(ended, True, vol, int(st[3]) or 1, ts) if det_on and d0 & dm.END else 0
    flags |= (EVENT if ongoing else 0) | (EVENT_END if done else 0)
    return [marks, 1 if e0 else 0, muted, dur if det_on and cur else 0], [flags, ongoing, done, muted], kind


def apply(kind, row):
    """row [480] float32 -> what the stage leaves of it"""
    with np.errstate(all="ignore"):
        if kind == ZERO:
            return np.zeros(FRAME, F32)
        if kind == DOWN:
            return (row * WD).astype(F32)
        if kind == UP:
            return (row * WU).astype(F32)
    return row


def frame(params, state, det, rows, on=None):
    """One frame of n streams.  state [n, 4] uint32, det [n, 4] detector report rows (None: detection off everywhere), rows [n, 480];
    on [n] (None: everybody) -> (state', rows', report [n, 4], kinds [n]); a stream that is not on keeps state and row and reports zeros"""
    st = np.array(state, U32).reshape(-1, STATE_WORDS)
    n = st.shape[0]
    x = np.array(rows, F32).reshape(n, FRAME)
    det = np.zeros((n, 4), U32) if det is None else np.asarray(det, U32).reshape(n, 4)
    rep = np.zeros((n, REPORT_WORDS), U32)
    kinds = np.zeros(n, np.int64)
    for s in range(n):
        if on is not None and not on[s]:
            continue
        st[s], rep[s], kinds[s] = decide(params, st[s], det[s])
        if kinds[s] != KEEP:
            x[s] = apply(kinds[s], x[s])
    return st, x, rep, kinds


def fresh(n):
    return np.zeros((n, STATE_WORDS), U32)


def run_stream(params, det_reports, rows):
    """One stream from the fresh state.  det_reports [T, 4] (frame t's detector report), rows [T, 480]: row t is what the engine puts out
    in frame t -> (rows' [T, 480], reports [T, 4], final state [4])"""
    det_reports = np.asarray(det_reports, U32).reshape(-1, 4)
    rows = np.asarray(rows, F32).reshape(-1, FRAME)
    st = [0, 0, 0, 0]
    out, reps = np.empty_like(rows), np.empty((rows.shape[0], REPORT_WORDS), U32)
    for t in range(rows.shape[0]):
        st, rep, kind = decide(params, st, det_reports[t])
        out[t], reps[t] = apply(kind, rows[t]), rep
    return out, reps, np.array(st, U32)


def delayed(rows, delay=DELAY):
    """rows [T, 480] -> what an engine that only delays puts out: row t is input row t - delay, zeros in front"""
    rows = np.asarray(rows, F32)
    return np.concatenate([np.zeros((delay,) + rows.shape[1:], F32), rows])[:rows.shape[0]]
