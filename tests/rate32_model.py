"""numpy models of the rate converter's rows for a RATIONAL factor: a rate of 48000 * M / L, up by L with every M-th output kept
and back down (include/percepnet_hip.h "batched rate converter"; kernels percepnet_amd/csrc/pn_rate.hip rt_up_rows<L, M> /
rt_down_rows<L, M>), imported as `from tests import rate32_model`.  32000 Hz is (L, M) = (3, 2); at M = 1 everything here is
tests/rate_model.py's arithmetic, which tests/test_rate32_host.py checks bit for bit.

  * EXACT float32 models with carried tails (up_f32, down_f32, Up, Down): every sum from 0.0f, oldest sample first, product and
    sum rounded separately.  The GPU tests feed them the LIBRARY's taps;
  * float64 models around the double design: the converters alone (roundtrip_f64) and the whole chain around an ideal engine
    (chain_f64), which generalise rate_model.chain_f64."""
import numpy as np

from tests import rate_model as rmod

F32 = np.float32
T = rmod.T
FRAME48 = rmod.FRAME48
LM = {8000: (6, 1), 16000: (3, 1), 24000: (2, 1), 32000: (3, 2)}
RATE32 = 32000


def frame_samples(L, M):
    assert FRAME48 * M % L == 0
    return FRAME48 * M // L


def down_tail(L, M):
    assert 2 * T * L % M == 0
    return 2 * T * L // M


def delay_samples(rate):
    L, M = LM[rate]
    return rmod.ENGINE_DELAY * M // L + 2 * T


def taps_f32(L, M, down):
    """The double design of L narrowed to fp32 once: h, or g = h * M / L computed in double as written."""
    h = rmod.design(L)
    if not down:
        return h.astype(F32)
    return (h / L if M == 1 else h * M / L).astype(F32)


def up_f32(x, tail, h, L, M=1):
    """x [B, n] fp32 (n = 480 M / L), tail [B, 32] = the 32 samples before x, h = fp32 taps [2D + 1] -> (y [B, 480], new tail).
    Output j: q = (M j) div L, p = (M j) mod L; p = 0: y[j] = x[q - 16] (a copy), else
    y[j] = sum_{i = 0..31} h[L(15 - i) + p] * x[q - 31 + i], i ascending, h indexed from its centre."""
    x, tail, h = np.asarray(x, F32), np.asarray(tail, F32), np.asarray(h, F32)
    B, n = x.shape
    D = T * L
    assert n == frame_samples(L, M) and tail.shape == (B, 2 * T) and h.shape == (2 * D + 1,)
    buf = np.concatenate([tail, x], axis=1)                      # buf[32 + q] = x[q]
    G = n // M                                                   # the pattern repeats every L outputs = M inputs
    y = np.empty((B, G, L), F32)
    for t in range(L):
        dq, p = divmod(M * t, L)                                 # output L r + t: q = M r + dq
        if p == 0:
            y[:, :, t] = buf[:, dq + T::M][:, :G]
            continue
        acc = np.zeros((B, G), F32)
        for i in range(2 * T):
            acc = acc + h[D + L * (T - 1 - i) + p] * buf[:, dq + 1 + i::M][:, :G]
        y[:, :, t] = acc
    return y.reshape(B, FRAME48), buf[:, n:].copy()


def down_f32(o, tail, g, L, M=1):
    """o [B, 480] fp32, tail [B, 2D / M] = the samples before o, g = fp32 taps [2D + 1] -> (z [B, n], new tail).
    z[m] = sum_i g[L m - D - M i] * o[i] over every integer i with (L m - 2D) / M < i < L m / M, ascending, g indexed from its
    start (its centre is D).  Taps that are exactly 0 are visited like the others."""
    o, tail, g = np.asarray(o, F32), np.asarray(tail, F32), np.asarray(g, F32)
    B = o.shape[0]
    D, n, TD = T * L, frame_samples(L, M), down_tail(L, M)
    assert o.shape == (B, FRAME48) and tail.shape == (B, TD) and g.shape == (2 * D + 1,)
    buf = np.concatenate([tail, o], axis=1)                      # buf[TD + i] = o[i]
    G = n // M
    z = np.empty((B, G, M), F32)
    for u in range(M):                                           # output M a + u reads around i = L a
        lo, hi = (L * u - 2 * D) // M + 1, -(-(L * u) // M) - 1
        assert TD + lo >= 1 and L * (G - 1) + hi < FRAME48
        acc = np.zeros((B, G), F32)
        for i in range(lo, hi + 1):
            acc = acc + g[L * u - M * i] * buf[:, TD + i::L][:, :G]
        z[:, :, u] = acc
    return z.reshape(B, n), buf[:, FRAME48:].copy()


class Up:
    """The up kernel over consecutive frames: carries the tails of B streams."""

    def __init__(self, B, L, M, h):
        self.L, self.M, self.h, self.tail = L, M, h, np.zeros((B, 2 * T), F32)

    def __call__(self, x):
        y, self.tail = up_f32(x, self.tail, self.h, self.L, self.M)
        return y


class Down:
    def __init__(self, B, L, M, g):
        self.L, self.M, self.g, self.tail = L, M, g, np.zeros((B, down_tail(L, M)), F32)

    def __call__(self, o):
        z, self.tail = down_f32(o, self.tail, self.g, self.L, self.M)
        return z


# ---- float64 ------------------------------------------------------------------------------------------------------------------
def up_f64(x, L, M):
    """x [N] at the low rate -> [N L / M] at 48 kHz: zero-stuffing to the L-times grid, the double design, every M-th sample."""
    x = np.asarray(x, np.float64)
    u = np.zeros(x.size * L)
    u[::L] = x
    return np.convolve(u, rmod.design(L))[:x.size * L:M]


def down_f64(y, L, M, N):
    """y at 48 kHz -> z [N] at the low rate: the samples M apart on the L-times grid, the double design * M / L, every L-th."""
    v = np.zeros(y.size * M)
    v[::M] = y
    return np.convolve(v, rmod.design(L) * M / L)[0:N * L:L]


def roundtrip_f64(x, L, M):
    """Up and straight back down, no engine: x delayed by 2T = 32 samples, up to the filters' error."""
    return down_f64(up_f64(x, L, M), L, M, np.asarray(x).size)


def roundtrip_error(rate, f_rel, N=2400, skip=200):
    """max |roundtrip - input delayed by 32| after `skip` samples for a sine at f_rel * rate."""
    L, M = LM[rate]
    x = np.sin(2 * np.pi * f_rel * np.arange(N))
    z = roundtrip_f64(x, L, M)
    want = np.concatenate([np.zeros(2 * T), x])[:N]
    return float(np.abs(z - want)[skip:].max())


def chain_f64(x, L, M=1):
    """float64 model of the whole chain around an ideal engine at a 0 dB attenuation limit, rate_model.chain_f64 for a rate of
    48000 M / L: up, the engine as a 2880-sample delay band-limited to 20 kHz, down.  Total delay delay_samples()."""
    x = np.asarray(x, np.float64)
    D, N = T * L, x.size
    y = up_f64(x, L, M)
    y = np.concatenate([np.zeros(rmod.ENGINE_DELAY), y])[:y.size]
    K = 1 << int(np.ceil(np.log2(y.size + 4 * D)))
    Y = np.fft.rfft(y, K)
    Y[np.fft.rfftfreq(K, 1.0 / 48000) >= 20000.0] = 0
    y = np.fft.irfft(Y, K)[:y.size]
    return down_f64(y, L, M, N)
