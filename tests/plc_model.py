"""The numpy float32 model of the rate converter's packet-loss concealment (include/percepnet_hip.h "packet-loss concealment"; the rule
with its summation orders: percepnet_amd/csrc/pn_plc_rules.h; kernel percepnet_amd/csrc/pn_rate_plc.hip).  Every operation below is
one float32 operation on float32 arrays — numpy never fuses a product into an add — and every sum runs in the header's order, so
the host functions (pn_plc_pitch, pn_plc_period, pn_plc_gain) and the kernel's rows and reports are compared with it bit for bit."""
import numpy as np

F32 = np.float32
HIST, P_MIN, P_MAX, FRAME = 1920, 240, 720, 480
LAG_LO, LAG_HI = 40, 120
FADE_START, FADE_END, XFADE = 480, 2880, 240
CONCEALED, CROSSFADE, SILENT = 1, 2, 4
REPORT_DTYPE = np.dtype([("flags", "<u4"), ("period", "<u4"), ("run", "<u4"), ("lost", "<u4")])


def score(c, e):
    """c * c / e where c > 0, e > 0 and the quotient is no NaN; +0.0 elsewhere"""
    c, e = np.asarray(c, F32), np.asarray(e, F32)
    with np.errstate(all="ignore"):
        s = (c * c) / e
    return np.where((c > 0) & (e > 0) & (s == s), s, F32(0.0)).astype(F32)


def best(scores):
    """strictly greater in ascending order, from +0.0 at index 0"""
    top, at = F32(0.0), 0
    for i, v in enumerate(scores):
        if v > top:
            top, at = v, i
    return at


def coarse(hist):
    d = np.ascontiguousarray(hist, dtype=F32)[5::6]
    assert d.size == 320
    lags = np.arange(LAG_LO, LAG_HI + 1)
    c, e = np.zeros(lags.size, F32), np.zeros(lags.size, F32)
    with np.errstate(all="ignore"):
        for k in range(160, 320):
            b = d[k - lags]
            c = c + d[k] * b
            e = e + b * b
    return LAG_LO + best(score(c, e))


def fine(hist, l):
    hist = np.ascontiguousarray(hist, dtype=F32)
    lo, hi = max(P_MIN, 6 * l - 5), min(P_MAX, 6 * l + 5)
    lags = np.arange(lo, hi + 1)[:, None]
    j = np.arange(8)[None, :]
    c, e = np.zeros((lags.size, 8), F32), np.zeros((lags.size, 8), F32)
    with np.errstate(all="ignore"):
        for i in range(120):
            k = 960 + 8 * i + j
            a, b = hist[k], hist[k - lags]
            c = c + a * b
            e = e + b * b
        cc, ee = c[:, 0], e[:, 0]
        for p in range(1, 8):
            cc = cc + c[:, p]
            ee = ee + e[:, p]
    return lo + best(score(cc, ee))


def pitch(hist):
    return fine(hist, coarse(hist))


def period(hist, P):
    hist = np.ascontiguousarray(hist, dtype=F32)
    assert hist.size == HIST and P_MIN <= P <= P_MAX
    O = P // 4
    q = hist[HIST - P:].copy()
    i = np.arange(P - O, P)
    a, b = hist[HIST - P + i], hist[HIST - 2 * P + i]
    w = ((i - (P - O)).astype(F32) + F32(0.5)) / F32(O)
    with np.errstate(all="ignore"):
        q[i] = a + w * (b - a)
    return q


def gain(m):
    m = np.asarray(m, np.int64)
    with np.errstate(all="ignore"):
        ramp = (FADE_END - np.clip(m, FADE_START, FADE_END)).astype(F32) / F32(FADE_END - FADE_START)
    return np.where(m < FADE_START, F32(1.0), np.where(m >= FADE_END, F32(0.0), ramp)).astype(F32)


def syn(q, P, r, n=None):
    """the synthetic samples n of the row that is r rows into a loss"""
    n = np.arange(FRAME) if n is None else np.asarray(n)
    if r >= FADE_END // FRAME:
        return np.zeros(n.size, F32)
    m = FRAME * r + n
    with np.errstate(all="ignore"):
        return (gain(m) * q[m % P]).astype(F32)


def xfade(s, real):
    """the first XFADE samples of the first received row after a loss"""
    w = (2 * np.arange(XFADE) + 1).astype(F32) / F32(2 * XFADE)
    with np.errstate(all="ignore"):
        return (s + w * (real - s)).astype(F32)


class Plc:
    """The state of B streams and one frame of the concealer over it"""

    def __init__(self, B):
        self.B = B
        self.hist = np.zeros((B, HIST), F32)          # linear: newest at [HIST - 1]
        self.q = np.zeros((B, P_MAX), F32)
        self.P = np.zeros(B, np.int64)
        self.r = np.zeros(B, np.int64)
        self.lost = np.zeros(B, np.int64)
        self.report = np.zeros(B, REPORT_DTYPE)

    def reset(self, ids=None):
        for s in range(self.B) if ids is None else ids:
            self.hist[s], self.q[s], self.P[s], self.r[s], self.lost[s] = 0, 0, 0, 0, 0

    def frame(self, x, lost=(), ids=None):
        """x [B, 480] float32, in place: the rows of the advancing streams (ids, None = all); `lost`: the marked streams — one that
        does not advance keeps everything.  The report rows of the advancing streams are rewritten."""
        for s in range(self.B) if ids is None else ids:
            is_lost, r = s in lost, int(self.r[s])
            flags = 0
            if is_lost:
                if r == 0:
                    self.P[s] = pitch(self.hist[s])
                    self.q[s, :self.P[s]] = period(self.hist[s], int(self.P[s]))
                x[s] = syn(self.q[s], int(self.P[s]), r)
                flags = CONCEALED | (SILENT if r >= FADE_END // FRAME else 0)
                self.r[s] = min(r + 1, 0x7fffffff)
                self.lost[s] += 1
            elif r > 0:
                x[s, :XFADE] = xfade(syn(self.q[s], int(self.P[s]), r, np.arange(XFADE)), x[s, :XFADE])
                flags = CROSSFADE
                self.r[s] = 0
            self.hist[s] = np.concatenate([self.hist[s, FRAME:], x[s]])
            self.report[s] = (flags, self.P[s], self.r[s], self.lost[s])
        return x
