"""The numpy float32 model of the rate converter's output limiter (include/percepnet_hip.h "output limiter"; the rule with its roundings
and the proof of its guarantee: percepnet_amd/csrc/pn_lim_rules.h; kernel percepnet_amd/csrc/pn_rate_lim.hip).  Every operation below is
one float32 operation on float32 values — numpy never fuses a product into an add and its division is the correctly rounded one — so
the host function (pn_lim_frame) and the kernel's rows, states and reports are compared with it bit for bit.

The rule, for one frame of a limited stream (ceiling c != 0), o its 480-sample row, (gain, hold, limited) its state, gain bits 0 = fresh = 1.0:
    p        max |o[j]| from +0.0, NaN ignored
    p > FLT_MAX (NONFINITE): row and state stay
    gl       p > c: q = c / p, one bit less when p * q > c; otherwise 1.0
    gl < g0  ATTACK | ACTIVE: k = first j with |o[j]| * g0 > c, or 480; out[j] = o[j] * (g0 + (j / k) * (gl - g0)) for j < k, o[j] * gl behind;
             g1 = gl, hold = H
    else     hold > 0 (HOLDING): g1 = g0, hold - 1; hold == 0: g1 = min(min(g0 * R, 1), gl), RELEASING when g1 > g0; ACTIVE when g0 < 1 or
             g1 < 1; the row takes the level control's ramp (agc_model.apply) unless g0 == g1 == 1: then it keeps its bits
    state    g1, hold, limited + ACTIVE (saturating)
A stream with c == 0: row and state untouched, report row (1.0, +0.0, 0, 0)."""
import numpy as np

from tests import agc_model as am

F32 = np.float32
FRAME = 480
N_PARAMS = 2
RELEASE, HOLD = range(2)
ON, ATTACK, HOLDING, RELEASING, ACTIVE, NONFINITE = 1, 2, 4, 8, 16, 32
REPORT_DTYPE = np.dtype([("gain", "<f4"), ("peak", "<f4"), ("flags", "<u4"), ("limited", "<u4")])
STATE_DTYPE = np.dtype([("gain", "<f4"), ("hold", "<u4"), ("limited", "<u4"), ("spare", "<u4")])
FLT_MAX = np.finfo(F32).max
DEFAULTS = np.array([1.0592537, 2.0], F32)
C_MIN, C_MAX = F32(1.0 / 1024.0), F32(1.0)
_J = np.arange(FRAME).astype(F32)


def params_ok(p):
    """-> the first bad index, or -1"""
    p = np.asarray(p, F32)
    if not (p[RELEASE] >= F32(1.0) and p[RELEASE] <= F32(2.0)):
        return RELEASE
    if not (p[HOLD] >= F32(0.0) and p[HOLD] <= F32(1000.0) and p[HOLD] == np.floor(p[HOLD])):
        return HOLD
    return -1


def ceiling_ok(c):
    c = F32(c)
    return bool(c == 0 or (c >= C_MIN and c <= C_MAX))


def needed(p, c):
    """gl of a finite peak p under the ceiling c"""
    p, c = F32(p), F32(c)
    if not p > c:
        return F32(1.0)
    with np.errstate(all="ignore"):
        q = F32(c / p)
        if F32(p * q) > c:
            q = (np.array([q], F32).view(np.uint32) - np.uint32(1)).view(F32)[0]
    return q


def step(P, c, gain_bits, hold, limited, p):
    """the scalar half of a frame -> (g0, g1, hold', limited', flags, attack, write, keep_state)"""
    P = np.asarray(P, F32)
    c, p = F32(c), F32(p)
    g0 = F32(1.0) if int(gain_bits) == 0 else np.array([gain_bits], np.uint32).view(F32)[0]
    hold, limited = int(hold), int(limited)
    if not p <= FLT_MAX:
        return g0, g0, hold, limited, ON | NONFINITE, False, False, True
    gl = needed(p, c)
    flags = ON
    if gl < g0:
        g1, hold, attack, write, active = gl, int(P[HOLD]), True, True, True
        flags |= ATTACK
    else:
        attack, g1 = False, g0
        if hold > 0:
            hold -= 1
            flags |= HOLDING
        else:
            with np.errstate(all="ignore"):
                g1 = np.fmin(np.fmin(F32(g0 * P[RELEASE]), F32(1.0)), gl)
            if g1 > g0:
                flags |= RELEASING
        active = bool(g0 < 1 or g1 < 1)
        write = not (g0 == 1 and g1 == 1)
    if active:
        flags |= ACTIVE
        if limited != 0xFFFFFFFF:
            limited += 1
    return F32(g0), F32(g1), hold, limited, flags, attack, write, False


def first_over(o, g0, c):
    with np.errstate(all="ignore"):
        over = (np.abs(np.asarray(o, F32)) * F32(g0)) > F32(c)
    return int(np.argmax(over)) if over.any() else FRAME


def attack_row(o, g0, gl, k):
    """the ramp from g0 to gl over [0, k), gl from k on"""
    o = np.asarray(o, F32)
    with np.errstate(all="ignore"):
        out = (o * F32(gl)).astype(F32)
        if k > 0:
            w = _J[:k] / F32(k)
            d = F32(gl) - F32(g0)
            out[:k] = o[:k] * (F32(g0) + w * d)
    return out


class Lim:
    """B streams of state, ceilings and the last report; frame() is one launch of the kernel over the rows"""

    def __init__(self, B, params=None):
        self.B = B
        self.params = DEFAULTS.copy() if params is None else np.array(params, F32)
        self.ceilings = np.zeros(B, F32)
        self.state = np.zeros(B, STATE_DTYPE)
        self.report = np.zeros(B, REPORT_DTYPE)
        self.k = np.full(B, -1)                       # the attack index of a stream's last frame (-1: it did not attack): for the tests

    def reset(self, ids=None):
        self.state[slice(None) if ids is None else list(ids)] = np.zeros((), STATE_DTYPE)

    def set_ceilings(self, ids, ceilings):
        for s, c in zip(ids, ceilings):
            self.ceilings[s] = F32(0.0) if c == 0 else F32(c)

    def gains(self):
        g = self.state["gain"].copy()
        g[self.state["gain"].view(np.uint32) == 0] = 1.0
        return g

    def frame(self, rows, ids=None):
        """rows [B, 480] float32 -> a copy with the listed streams' rows limited; the others' rows, states and report rows stay"""
        out = np.array(rows, dtype=F32).reshape(self.B, FRAME)
        adv = list(range(self.B)) if ids is None else [int(s) for s in ids]
        if not adv:
            return out
        pk = am.peak(out[adv])
        for i, s in enumerate(adv):
            c = self.ceilings[s]
            self.k[s] = -1
            if c == 0:
                self.report[s] = (1.0, 0.0, 0, 0)
                continue
            st = self.state[s]
            g0, g1, hold, limited, flags, attack, write, keep = step(self.params, c, st["gain"].view(np.uint32), st["hold"], st["limited"], pk[i])
            if attack:
                self.k[s] = first_over(out[s], g0, c)
                out[s] = attack_row(out[s], g0, g1, self.k[s])
            elif write:
                out[s] = am.apply(out[s], g0, g1)
            if not keep:
                self.state[s] = (g1, hold, limited, 0)
            self.report[s] = (g1, pk[i], flags, limited)
        return out
