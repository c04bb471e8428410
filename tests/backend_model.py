"""numpy model of the frame engine's back end, for the attenuation-limit tests (include/percepnet_hip.h,
pn_ctx_set_atten_limit).  From one stream's per-frame analysis spectrum X, comb-filtered spectrum P, silence flag,
g|r tap and mix factor lam it rebuilds the output: pitch_filter, the gain stage and the attenuation-limit mix in the
reference's operation order (denoise.cpp:436-485, 536-544), every step rounded to fp32 separately, then the inverse
transform through the oracle's own 960-point FFT (pno_fft960, 1/960 scale included), the window, the overlap-add
(denoise.cpp:306-359) and the CLI's truncating int16 cast (main.cpp:36).

With lam = 0 for every frame it is the unlimited engine: fed Oracle.stages() and the g|r of Oracle.run_pcm() it gives
Oracle.run_pcm()'s PCM bit for bit (tests/test_atten_limit_host.py pins that).
"""
import ctypes

import numpy as np

F32 = np.float32
SPEC_BINS = 400          # bins the engine keeps (PN_SPEC_BINS): 400..480 are exactly 0 after the gain stage


def factor(db):
    """lam, mu of an attenuation limit of `db` dB as the header defines them (double pow, one fp32 rounding, below FLT_MIN -> 0)."""
    lam = F32(10.0 ** (-float(db) / 20.0))
    if lam < np.finfo(np.float32).tiny:
        lam = F32(0)
    return lam, F32(F32(1) - lam)


class BackendModel:
    def __init__(self, oracle):
        self.lib = oracle.lib
        self.lib.pno_fft960.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        self.lib.pno_fft960.restype = None
        _, _, hw, _, border = oracle.tables()
        self.win = hw.astype(np.float32)
        self.border = [int(b) for b in border]
        band, frac = [], []
        for i in range(len(self.border) - 1):
            bs = self.border[i + 1] - self.border[i]
            band += [i] * bs
            frac.append(np.arange(bs, dtype=np.float32) / F32(bs))        # (float)j / band_size
        self.band = np.array(band)
        self.frac = np.concatenate(frac)
        self.one_m_frac = F32(1) - self.frac
        self.nk = len(band)
        assert self.border[0] == 0 and self.nk == SPEC_BINS

    def interp(self, e):
        """interp_band_gain (denoise.cpp:162-182) into a zeroed [481]: bins >= 400 stay 0.  Bin k of band b at fraction f:
        (1 - f) * e[b] + f * e[b + 1], fp32 throughout."""
        e = np.asarray(e, np.float32)
        out = np.zeros(481, np.float32)
        out[:self.nk] = self.one_m_frac * e[self.band] + self.frac * e[self.band + 1]
        return out

    def fft960(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.empty_like(x)
        fp = ctypes.POINTER(ctypes.c_float)
        self.lib.pno_fft960(x.ctypes.data_as(fp), y.ctypes.data_as(fp))
        return y

    def frame(self, X, P, silent, gr, lam, mem):
        """One frame: X, P complex [>= 481] (bins 0..480 used), gr [68], lam (fp32 factor, 0 = off), mem [480] overlap memory
        (updated in place) -> float output [480]."""
        xr = np.ascontiguousarray(np.real(X[:481]), dtype=np.float32)
        xi = np.ascontiguousarray(np.imag(X[:481]), dtype=np.float32)
        ar, ai = xr.copy(), xi.copy()
        g = np.asarray(gr[:34], np.float32)
        r = np.asarray(gr[34:68], np.float32)
        if not silent:
            pr = np.real(P[:481]).astype(np.float32)
            pi = np.imag(P[:481]).astype(np.float32)
            rf = self.interp(F32(1) - r)
            xr = rf * xr
            xi = rf * xi
            rf = self.interp(r)
            xr = xr + rf * pr
            xi = xi + rf * pi
        gf = self.interp(g)
        xr = xr * gf
        xi = xi * gf
        lam = F32(lam)
        if lam != 0:
            mu = F32(F32(1) - lam)
            k = slice(0, SPEC_BINS)
            xr[k] = (mu * xr[k]) + (lam * ar[k])
            xi[k] = (mu * xi[k]) + (lam * ai[k])
        x = np.zeros((960, 2), np.float32)
        x[:481, 0] = xr
        x[:481, 1] = xi
        x[481:, 0] = xr[479:0:-1]            # Hermitian extension: x[i] = conj(x[960 - i])
        x[481:, 1] = -xi[479:0:-1]
        y = self.fft960(x)
        t = np.empty(960, np.float32)
        t[0] = F32(960) * y[0, 0]
        t[1:] = F32(960) * y[:0:-1, 0]       # reversed read-out
        t[:480] = t[:480] * self.win
        t[480:] = t[480:] * self.win[::-1]
        out = t[:480] + mem
        mem[:] = t[480:]
        return out

    def run(self, X, P, silence, gr, lam):
        """Frames 0..n-1 of one stream: X, P [n, 481] complex, silence [n], gr [n, 68], lam scalar or [n] (fp32 factors)
        -> float output [n, 480]."""
        n = len(X)
        lam = np.broadcast_to(np.asarray(lam, np.float32), (n,))
        mem = np.zeros(480, np.float32)
        return np.stack([self.frame(X[t], P[t], bool(silence[t]), gr[t], lam[t], mem) for t in range(n)])


def f2s(v):
    """float -> int16 as the reference CLI's x86-64 build (truncate to int32, out of range / NaN -> INT32_MIN, low 16 bits)."""
    v = np.asarray(v, np.float32)
    ok = np.abs(v) < F32(2147483648.0)
    t = np.where(ok, np.trunc(np.where(ok, v, 0)).astype(np.int64), -2147483648)
    return (t & 0xFFFF).astype(np.uint16).view(np.int16)


def pcm(out_float):
    """Float frames [n, 480] -> the CLI's PCM: first frame dropped (main.cpp:37), x32768, truncating cast."""
    return f2s(out_float[1:].reshape(-1) * F32(32768))
