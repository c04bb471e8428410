"""The numpy float32 model of the conference mix with loudest-N selection, send gains, the hold and the mix report
(include/percepnet_hip.h "conferences: loudest-N talkers, send gains, mix report"; kernel percepnet_amd/csrc/pn_rate_mix.hip
pn_rate_mix_sel_kernel; the host's statement percepnet_amd/csrc/pn_mix_rules.h), imported as `from tests import mix_sel_model`.

For one frame, A = the streams that advance, y[m] the engine's row of stream m, c a conference:
    talkers of c      its members in A with gain g_m != 0; contribution x[m] = g_m * y[m], one fp32 product per sample
    level             E_m = sum of x*x in ONE order: products rounded separately; 120 groups of four summed in index order from
                      +0.0; padded with +0.0 to 128 = two halves of 64, each folded by the xor butterfly v[i] = v[i] + v[i ^ stride],
                      stride 32 .. 1; E = half0[0] + half1[0]
    hold              h = d * L_prev;  L = h if d != 0 and h is finite and h > E else E; a muted advancing member's L is +0.0
    selection         key(L) = bits(L) & 0x7fffffff; talker m is selected iff N_c == 0 or fewer than N_c talkers q have
                      key(L_q) > key(L_m) or (key(L_q) == key(L_m) and q < m)
    mix               listener s gets the sum of x[m] over the selected talkers m != s, m ascending, from +0.0, plain fp32 adds
    report            level, flags (1 selected | 2 muted | 4 in a conference), fmax-peak and clipped count of what s hears
With every gain 1, every N_c 0 and d = 0 the rows are those of tests/conf_model.mix.  Where a value is NaN, WHICH NaN is the adder's
choice (conf_model.same compares NaN-ness there); everything else is bits."""
import numpy as np

from percepnet_amd import api
from tests import conf_model as cm
from tests import report_model as rm

F32 = np.float32
NONE = cm.NONE
_XOR = {s: np.arange(64) ^ s for s in (32, 16, 8, 4, 2, 1)}


def level(x):
    """x [..., 480] float32 contributions -> E [...] float32, in the kernel's order"""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = (x * x).reshape(x.shape[:-1] + (120, 4))
        e = np.zeros(p.shape[:-1], F32)
        for i in range(4):
            e = e + p[..., i]
        v = np.zeros(x.shape[:-1] + (128,), F32)
        v[..., :120] = e
        halves = []
        for half in range(2):
            h = v[..., 64 * half:64 * half + 64]
            for stride in (32, 16, 8, 4, 2, 1):
                h = h + h[..., _XOR[stride]]
            halves.append(h[..., 0])
        return (halves[0] + halves[1]).astype(F32)


def level_sequential(x):
    """the plain left-to-right sum of the same products: what the level is NOT"""
    x = np.asarray(x, F32)
    e = F32(0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for v in x * x:
            e = F32(e + v)
    return e


def hold_level(d, prev, e):
    d, prev, e = F32(d), F32(prev), F32(e)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        h = F32(d * prev)
        return h if (d != 0 and np.isfinite(h) and h > e) else e


def key(lv):
    return np.asarray(lv, F32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def select(levels, n_max):
    """levels [k] of one conference's talkers, ascending slot order -> bool [k]"""
    k = key(np.ascontiguousarray(levels, dtype=F32))
    out = np.zeros(len(k), bool)
    for i in range(len(k)):
        ahead = sum(1 for q in range(len(k)) if k[q] > k[i] or (k[q] == k[i] and q < i))
        out[i] = n_max == 0 or ahead < n_max
    return out


def mix(y, confs, ids=None, out=None, gains=None, caps=None, hold=0.0, levels=None, report=None):
    """y [B, 480] float32, confs [B]; ids: the streams that advance (None: all); gains [B] (None: 1); caps [B] by conference number
    (None: 0); hold d; levels [B]: L of the frame before (None: 0); report: MIX_REPORT_DTYPE [B] as it was (None: zeros)
    -> (o, levels, report): copies with the rows of the advancing streams written"""
    y = np.asarray(y)
    B = y.shape[0]
    assert y.dtype == F32 and y.ndim == 2 and len(confs) == B
    adv = set(range(B) if ids is None else (int(i) for i in ids))
    gains = np.ones(B, F32) if gains is None else np.asarray(gains, F32)
    caps = np.zeros(B, np.int32) if caps is None else np.asarray(caps, np.int32)
    o = np.zeros_like(y) if out is None else np.array(out, dtype=F32, copy=True)
    lv = np.zeros(B, F32) if levels is None else np.array(levels, dtype=F32, copy=True)
    rep = np.zeros(B, api.MIX_REPORT_DTYPE) if report is None else np.array(report, copy=True)
    prev = lv.copy()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for s in sorted(adv):
            if confs[s] == NONE:
                o[s] = y[s]
                rep[s] = (0, 0, 0, 0)
        for c in sorted({confs[s] for s in adv if confs[s] != NONE}):
            mem = [m for m in cm.members(confs, c) if m in adv]
            talk = [m for m in mem if gains[m] != 0]
            x = {m: gains[m] * y[m] for m in talk}
            for m in mem:
                lv[m] = hold_level(hold, prev[m], level(x[m])) if m in x else F32(0)
            sel = dict(zip(talk, select([lv[m] for m in talk], int(caps[c]))))
            for s in mem:
                acc = np.zeros(y.shape[1], F32)
                for m in talk:
                    if m != s and sel[m]:
                        acc = acc + x[m]
                o[s] = acc
                flags = (api.MIX_SELECTED if sel.get(s, False) else 0) | (0 if s in x else api.MIX_MUTED) | api.MIX_IN_CONF
                rep[s] = (lv[s], flags, rm.peak(acc), rm.count_clipped(acc))
    return o, lv, rep


def same_report(got, want):
    """records equal: level and peak by conf_model.same (NaN-ness where NaN), flags and counts exactly"""
    return bool(cm.same(got["level"], want["level"]) and cm.same(got["mix_peak"], want["mix_peak"]) and
                np.array_equal(got["flags"], want["flags"]) and np.array_equal(got["mix_clipped"], want["mix_clipped"]))
