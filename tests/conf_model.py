"""The numpy float32 model of the conference mix (include/percepnet_hip.h "conferences"; kernel percepnet_amd/csrc/pn_rate_mix.hip):

    stream s that advances, conference c:  o[s][j] = sum of y[m][j] over the members m of c with m != s that advance, m ascending,
                                           acc = +0.0f, acc = acc + y[m][j] in fp32; a lone member hears +0.0
    stream s that advances, NONE:          o[s] = y[s], bit for bit
    stream that does not advance:          contributes nothing, its output row is left as it was

Every add is one IEEE fp32 add, so the model gives the kernel's bits for finite values, infinities and signed zeros.  Where a sum
is NaN (a NaN member, or +inf with -inf) both give a NaN; WHICH NaN (sign and payload) is the adder's choice and differs between
an x86 host and the GPU, so `same` compares NaN-ness there and bits everywhere else."""
import numpy as np

NONE = -1
MAX_MEMBERS = 32
F32 = np.float32


def members(confs, c):
    """The streams of conference c, ascending"""
    return [s for s, v in enumerate(confs) if v == c and c != NONE]


def mix(y, confs, ids=None, out=None):
    """y [B, 480] float32, confs [B]; ids: the streams that advance (None: all) -> o [B, 480] float32, a copy of `out` (zeros
    when None) with the rows of the advancing streams written"""
    y = np.asarray(y)
    assert y.dtype == F32 and y.ndim == 2 and len(confs) == y.shape[0]
    adv = set(range(y.shape[0]) if ids is None else (int(i) for i in ids))
    o = np.zeros_like(y) if out is None else np.array(out, dtype=F32, copy=True)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in sorted(adv):
            if confs[s] == NONE:
                o[s] = y[s]
                continue
            acc = np.zeros(y.shape[1], F32)
            for m in members(confs, confs[s]):
                if m != s and m in adv:
                    acc = acc + y[m]
            o[s] = acc
    return o


def same(a, b):
    """equal shapes; NaN exactly where the other has NaN; the same bits everywhere else"""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
