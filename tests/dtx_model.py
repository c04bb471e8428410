"""The DTX send side of the rate converter, restated in numpy — float32 for every sum, product and quotient, integers for the state
machine, every operation rounded once, in the order of percepnet_amd/csrc/pn_dtx_rules.h.  The autocorrelation is vectorised across
streams and lanes; the scalar rule runs a stream at a time.

State of a stream: 24 uint32 words — R[13] (float bits), N (float bits), hang, the mode, since, the analysed frames, the last emitted SID
(14 bytes, then a 16-bit count) in four words, two zeros.  Report: 8 words — the decision, flags | L << 8 | hang << 16, the bits of e, the
bits of N, state words 18..21."""
import numpy as np

F32 = np.float32
U32 = np.uint32
N_PARAMS, STATE_WORDS, REPORT_WORDS, LAGS = 9, 24, 8, 13
THR, FLOOR_UP, FLOOR_DRIFT, FLOOR_MIN, HANGOVER, SMOOTH, UPDATE_DB, MAX_INTERVAL, ORDER = range(9)
FRAME, SID, NONE = 0, 1, 2
ON, ACTIVE, HANGOVER_FRAME, NONFINITE = 1, 2, 4, 8
W_N, W_HANG, W_MODE, W_SINCE, W_FRAMES, W_SID = 13, 14, 15, 16, 17, 18
MODE_SILENT, MODE_NOISE = 1, 2
ROWS = (80, 160, 240, 320, 480)
KQ = np.array([0x42FE03F8], U32).view(F32)[0]            # the fp32 nearest 32768 / 258
EDGE = np.array([10.0 ** (-(i + 0.5) / 10) for i in range(127)], np.float64).astype(F32)
REPORT_DTYPE = np.dtype([("decision", "<u4"), ("word1", "<u4"), ("energy", "<f4"), ("floor", "<f4"), ("sid", "u1", (14,)), ("count", "<u2")])


def default_params():
    return np.array([4.0, 0.1, 1.0023, 1e-10, 20, 0.1, 2, 0, 10], F32)


def bits(f):
    return int(np.array([f], F32).view(U32)[0])


def flt(u):
    return np.array([u], U32).view(F32)[0]


def acorr(x, lags=LAGS):
    """x: float32 [n][ns] -> float32 [n][lags]: lane l of 64 sums its terms n = l, l + 64, .. with n >= j from +0.0 in ascending order,
    the 64 partial sums fold by the xor butterfly 32, 16, .., 1"""
    x = np.ascontiguousarray(x, F32)
    if x.ndim == 1:
        return acorr(x[None], lags)[0]
    n, ns = x.shape
    K = (ns + 63) // 64
    idx = np.arange(K * 64).reshape(K, 64)               # term n of lane l at step k
    lane = np.arange(64)
    out = np.zeros((n, lags), F32)
    with np.errstate(all="ignore"):
        for j in range(lags):
            acc = np.zeros((n, 64), F32)
            for k in range(K):
                m = (idx[k] >= j) & (idx[k] < ns)
                a = np.where(m, idx[k], 0)
                b = np.where(m, idx[k] - j, 0)
                p = (x[:, a] * x[:, b]).astype(F32)
                acc = np.where(m[None], (acc + p).astype(F32), acc)
            for s in (32, 16, 8, 4, 2, 1):
                acc = (acc + acc[:, lane ^ s]).astype(F32)
            out[:, j] = acc[:, 0]
    return out


def level(ms):
    """L of a mean square: the number of edges above it"""
    with np.errstate(all="ignore"):
        return int(np.count_nonzero(F32(ms) < EDGE))


def levinson(R, order):
    """R: float32 [13] -> (M, [N_1..N_M])"""
    R = np.asarray(R, F32)
    N = []
    with np.errstate(all="ignore"):
        if not (R[0] > 0 and np.isfinite(R[0])):
            return 0, N
        a = np.zeros(LAGS, F32)
        E = R[0]
        for i in range(1, order + 1):
            acc = R[i]
            for j in range(1, i):
                acc = F32(acc + F32(a[j] * R[i - j]))
            k = F32(F32(-acc) / E)
            if not (abs(k) < 1):
                break
            u = F32(F32(k * KQ) + F32(127.5))
            Ni = min(max(int(u), 0), 254)
            kq = F32(F32(258 * (Ni - 127)) * F32(1.0 / 32768.0))
            En = F32(E * F32(F32(1) - F32(kq * kq)))
            if not (En > 0):
                break
            c = a.copy()
            for j in range(1, i):
                a[j] = F32(c[j] + F32(kq * c[i - j]))
            a[i] = kq
            E = En
            N.append(Ni)
    return len(N), N


def sid_from_acorr(R, order):
    """-> uint8 [14]: M, the level of R[0], N_1..N_M, zeros"""
    M, N = levinson(R, order)
    s = np.zeros(14, np.uint8)
    s[0], s[1] = M, level(np.asarray(R, F32)[0])
    s[2:2 + M] = N
    return s


def classify(p, N, frames, e):
    if not np.isfinite(e):
        return ACTIVE | NONFINITE
    if frames == 0:
        return ACTIVE
    Nc = N if N > p[FLOOR_MIN] else p[FLOOR_MIN]
    return ACTIVE if e > F32(p[THR] * Nc) else 0


def update(p, st, r, ns):
    """one frame of one enabled stream behind its sums.  p: float32 [9]; st: uint32 [24], updated in place; r: float32 [13] -> (the
    decision, uint32 [8] report)"""
    p = np.asarray(p, F32)
    r = np.asarray(r, F32)
    with np.errstate(all="ignore"):
        fns = F32(ns)
        e = F32(r[0] / fns)
        N = flt(st[W_N])
        frames, hang, mode, since = int(st[W_FRAMES]), int(st[W_HANG]), int(st[W_MODE]), int(st[W_SINCE])
        cls = classify(p, N, frames, e)
        active = bool(cls & ACTIVE)
        if not cls & NONFINITE and not (frames == 0 and e == 0):
            Nc = N if N > p[FLOOR_MIN] else p[FLOOR_MIN]
            if frames == 0 or e < N:
                N = e
            elif not active:
                N = F32(N + F32(p[FLOOR_UP] * F32(e - N)))
            else:
                N = F32(Nc * p[FLOOR_DRIFT])
            frames = min(frames + 1, 0xFFFFFFFF)
        flags = ON | cls
        if active:
            hang = int(p[HANGOVER])
        send = active or hang > 0
        if not active and hang > 0:
            hang -= 1
            flags |= HANGOVER_FRAME
        if not active:
            q = (r / fns).astype(F32)
            if not mode & MODE_NOISE:
                st[:LAGS] = q.view(U32)
            else:
                R = st[:LAGS].copy().view(F32)
                st[:LAGS] = (R + (p[SMOOTH] * (q - R).astype(F32)).astype(F32)).astype(F32).view(U32)
            mode |= MODE_NOISE
        decision, L = FRAME, 0
        if send:
            mode &= ~MODE_SILENT
        else:
            R = st[:LAGS].copy().view(F32)
            L = level(R[0])
            Ls = (int(st[W_SID]) >> 8) & 0xFF
            mi = int(p[MAX_INTERVAL])
            emit = True
            if mode & MODE_SILENT:
                emit = abs(L - Ls) >= int(p[UPDATE_DB]) or (mi > 0 and since + 1 >= mi)
            mode |= MODE_SILENT
            if emit:
                count = ((int(st[W_SID + 3]) >> 16) + 1) & 0xFFFF
                M, Ni = levinson(R, int(p[ORDER]))
                b = np.zeros(16, np.uint8)
                b[0], b[1] = M, L
                b[2:2 + M] = Ni
                b[14], b[15] = count & 0xFF, count >> 8
                st[W_SID:W_SID + 4] = b.view("<u4")
                since, decision = 0, SID
            else:
                since, decision = min(since + 1, 0xFFFF), NONE
        st[W_N], st[W_FRAMES], st[W_HANG], st[W_MODE], st[W_SINCE] = bits(N), frames, hang, mode, since
        rep = np.zeros(REPORT_WORDS, U32)
        rep[0], rep[1], rep[2], rep[3] = decision, flags | L << 8 | hang << 16, bits(e), bits(N)
        rep[4:] = st[W_SID:W_SID + 4]
    return decision, rep


def frame(p, st, row):
    """one float row of one enabled stream: the twin of pn_dtx_frame"""
    row = np.asarray(row, F32)
    assert row.size in ROWS
    return update(p, st, acorr(row), row.size)


def samples(rows, fmt="f32", laws=None):
    """output rows of a call's format as the floats the stage sees: int16 times 2^-15; G.711 (uint8, laws per row: 0 mu-law, 1 A-law)
    decoded by tests/g711_model.py first"""
    if fmt == "f32":
        return np.asarray(rows, F32)
    if fmt == "g711":
        from tests import g711_model
        rows = np.stack([g711_model.decode(int(law), r) for law, r in zip(laws, np.asarray(rows, np.uint8))])
    return (np.asarray(rows, np.int16).astype(F32) * F32(1.0 / 32768.0)).astype(F32)


class Dtx:
    """The stage of a converter of B streams: switches, parameters, state and report."""

    def __init__(self, B, ns, params=None):
        self.B = B
        self.ns = np.broadcast_to(np.asarray(ns, np.int64), (B,)).copy()
        self.params = default_params() if params is None else np.asarray(params, F32).copy()
        self.on = np.zeros(B, bool)
        self.state = np.zeros((B, STATE_WORDS), U32)
        self.report = np.zeros((B, REPORT_WORDS), U32)

    def set_on(self, ids, on):
        ids = np.asarray(ids, np.int64).reshape(-1)
        on = np.broadcast_to(np.asarray(on, bool), ids.shape)
        for s, v in zip(ids, on):
            if v and not self.on[s]:
                self.state[s] = 0
            self.on[s] = v

    def clear(self, ids=None):
        self.state[np.arange(self.B) if ids is None else np.asarray(ids, np.int64)] = 0

    def frame(self, rows, ids=None):
        """one launch over the float rows [B][>= ns] (see samples) of the streams `ids` (None: all)"""
        ids = np.arange(self.B) if ids is None else np.asarray(ids, np.int64).reshape(-1)
        rows = np.asarray(rows, F32)
        for n in np.unique(self.ns[ids]) if ids.size else ():
            sel = [int(s) for s in ids if self.ns[s] == n and self.on[s]]
            if not sel:
                continue
            r = acorr(rows[sel][:, :int(n)])
            for i, s in enumerate(sel):
                _, self.report[s] = update(self.params, self.state[s], r[i], int(n))
        for s in ids:
            if not self.on[s]:
                self.report[s] = 0

    def report_records(self):
        return self.report.copy().view(REPORT_DTYPE).reshape(self.B)
