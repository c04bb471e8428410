"""numpy models of the batched rate converter (include/percepnet_hip.h "batched rate converter"; kernels
percepnet_amd/csrc/pn_rate.hip), imported as `from tests import rate_model`:

  * the filter design in double (design, taps_f32), the reference of tests/test_rate_host.py for the library's table;
  * EXACT float32 models of the two kernels with carried tails (up_f32, down_f32): every sum oldest sample first from 0.0f,
    the product and the sum rounded separately — numpy float32 arithmetic does exactly that, so the GPU's rows must match bit
    for bit.  The GPU tests feed them the LIBRARY's taps (api.rate_taps), so that bit-equality does not hinge on two libm
    implementations agreeing on a Bessel function;
  * the two int16 conventions at the edges (from_i16, to_i16);
  * a float64 model of the whole chain around an ideal engine (chain_f64): what the delay test measures the GPU against."""
import numpy as np

from tests import report_model as rm

F32 = np.float32
T = 16                      # PN_RATE_TAPS
FRAME48 = 480
ENGINE_DELAY = 2880         # samples at 48 kHz from input frame t to output frame t
RATES = (8000, 16000, 24000)
BETA = 8.0


def factor(rate):
    return 48000 // rate


def design(L):
    """h[k], k = -D..D in double: sinc(k / L) * I0(beta * sqrt(1 - (k / D)^2)) / I0(beta), h[0] = 1 and h[jL] = 0 exactly."""
    D = T * L
    k = np.arange(D + 1, dtype=np.float64)
    h = np.sinc(k / L) * np.i0(BETA * np.sqrt(1.0 - (k / D) ** 2)) / np.i0(BETA)
    h[0] = 1.0
    h[L::L] = 0.0
    return np.concatenate([h[:0:-1], h])


def taps_f32(L, down):
    """The design rounded to fp32 once: h, or g = h / L (divided in double) for the down-converter."""
    h = design(L)
    return (h / L if down else h).astype(F32)


def from_i16(v):
    return np.asarray(v, np.int16).astype(F32) / F32(32768)


def to_i16(z, saturate):
    """z (fp32) -> int16: trunc(z * 32768) wrapped to 16 bit, or saturated (the output stage's two casts)."""
    return rm.cast(z, saturate)


def up_f32(x, tail, h, L):
    """x [B, n] fp32 (n = 480 / L), tail [B, 32] = the 32 samples before x, h = fp32 taps [2D + 1] -> (y [B, 480], new tail).
    y[Lq] = x[q - 16] (a copy), y[Lq + p] = sum_{i = 0..31} h[L(15 - i) + p] * x[q - 31 + i], i ascending."""
    x, tail, h = np.asarray(x, F32), np.asarray(tail, F32), np.asarray(h, F32)
    B, n = x.shape
    D = T * L
    assert n * L == FRAME48 and tail.shape == (B, 2 * T) and h.shape == (2 * D + 1,)
    buf = np.concatenate([tail, x], axis=1)                      # buf[32 + q] = x[q]
    y = np.empty((B, n, L), F32)
    y[:, :, 0] = buf[:, T:T + n]
    for p in range(1, L):
        acc = np.zeros((B, n), F32)
        for i in range(2 * T):
            acc = acc + h[D + L * (T - 1 - i) + p] * buf[:, 1 + i:1 + i + n]
        y[:, :, p] = acc
    return y.reshape(B, FRAME48), buf[:, n:].copy()


def down_f32(o, tail, g, L):
    """o [B, 480] fp32, tail [B, 2D] = the 2D samples before o, g = fp32 taps [2D + 1] -> (z [B, n], new tail).
    z[m] = sum_{j = 0..2D-2} g[D - 1 - j] * o[Lm - 2D + 1 + j], j ascending."""
    o, tail, g = np.asarray(o, F32), np.asarray(tail, F32), np.asarray(g, F32)
    B = o.shape[0]
    D, n = T * L, FRAME48 // L
    assert o.shape == (B, FRAME48) and tail.shape == (B, 2 * D) and g.shape == (2 * D + 1,)
    buf = np.concatenate([tail, o], axis=1)                      # buf[2D + i] = o[i]
    acc = np.zeros((B, n), F32)
    for j in range(2 * D - 1):
        acc = acc + g[2 * D - 1 - j] * buf[:, 1 + j::L][:, :n]
    return acc, buf[:, FRAME48:].copy()


class Up:
    """The up kernel over consecutive frames: carries the tails of B streams."""

    def __init__(self, B, L, h):
        self.L, self.h, self.tail = L, h, np.zeros((B, 2 * T), F32)

    def __call__(self, x):
        y, self.tail = up_f32(x, self.tail, self.h, self.L)
        return y


class Down:
    def __init__(self, B, L, g):
        self.L, self.g, self.tail = L, g, np.zeros((B, 2 * T * L), F32)

    def __call__(self, o):
        z, self.tail = down_f32(o, self.tail, self.g, self.L)
        return z


# ---- the down kernel's int16 cast at its edges ------------------------------------------------------------------------------
# A single non-zero 48 kHz sample of amplitude A at position i, zeros around it, makes every output it reaches exactly ONE rounded
# product: z[m] = fl(g[Lm - D - i] * A), since adding zeros is exact.  Output m sees tap index Lm - i of the table (centre D), so a
# sample at a multiple of L meets only g[0] = 1 / L and the taps that are exactly 0; any other sample meets ~2T non-zero taps of
# both signs.  inf * 0 and NaN * anything are NaN, in numpy as on the GPU.
def t_classes(t):
    """t = z * 32768 (fp32) -> {class name: mask}: the ranges in which the two casts of the header behave differently.  The classes
    are disjoint: "t <= -32769" is split into (-2^31, -32769], where the wrap still truncates, and the finite t at or beyond
    -2^31, which together with those at or beyond +2^31 form "|t| >= 2^31", where the wrap gives 0."""
    t = np.asarray(t, F32)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(t)
        return {"[32767, 32768)": (t >= 32767) & (t < 32768), "[32768, 65536)": (t >= 32768) & (t < 65536),
                "(-32769, -32768)": (t > -32769) & (t < -32768), "(-2^31, -32769]": (t <= -32769) & (t > -2.0 ** 31),
                "|t| >= 2^31": fin & (np.abs(t) >= 2.0 ** 31), "+inf": t == np.inf, "-inf": t == -np.inf, "nan": np.isnan(t)}


def _amplitude(G, tau, name):
    """The first fp32 amplitude, growing in magnitude from the one that puts the largest tap of G at t = tau, at which some
    product fl(fl(G * A) * 32768) lies in class `name` (a nextafter search on the model's own arithmetic)."""
    gmax = G[np.argmax(np.abs(G))]
    A = F32(tau / 32768.0 / float(gmax))
    for _ in range(1 << 16):
        if t_classes((G * A).astype(F32) * F32(32768))[name].any():
            return A
        A = np.nextafter(A, F32(np.copysign(np.inf, A)))
    raise AssertionError(f"no amplitude puts a product into {name}")


EDGE_IMPULSES = (("[32767, 32768)", 32766.9, False), ("[32768, 65536)", 32767.9, True), ("(-32769, -32768)", -32767.9, True),
                 ("(-2^31, -32769]", -32768.9, False), ("|t| >= 2^31", 2147483000.0, False), (None, 3e38, False),
                 (None, np.inf, False), (None, -np.inf, True), (None, np.nan, False))


def cast_edge_rows(B, L, g):
    """-> o [frames + 1, B, 480] fp32: 48 kHz rows of nine well-separated single samples per stream (at least 2D + L apart, so that
    no two reach the same output), `frames` frames and one frame of zeros.  In EDGE_IMPULSES' order: five amplitudes found by _amplitude
    for the five finite classes of t_classes — (class, starting t, on a multiple of L?) — then 3e38 (z finite, z * 32768 infinite,
    both signs), +inf off the multiples of L (+inf and -inf), -inf ON a multiple of L (inf * 0: NaN) and a NaN.  Row r is shifted
    by rL samples and takes another phase.  The last sample lies in the last 6L samples of the last frame before the zeros, so its
    window reaches 2D samples into the frame of zeros through the tail."""
    g = np.asarray(g, F32)
    D = T * L
    S = 2 * D + 2 * L
    n_imp = len(EDGE_IMPULSES)
    frames = -(-((n_imp - 1) * S + 6 * L) // FRAME48)
    o = np.zeros((B, (frames + 1) * FRAME48), F32)
    for r in range(B):
        for k, (name, tau, on_multiple) in enumerate(EDGE_IMPULSES):
            phase = 0 if on_multiple else 1 + (r + k) % (L - 1)
            i = frames * FRAME48 - 6 * L - (n_imp - 1 - k) * S + r * L + phase
            G = g[np.arange(1, 2 * D)[(np.arange(1, 2 * D) + i) % L == 0]]        # the taps Lm - i that sample i meets
            o[r, i] = _amplitude(G, tau, name) if name else tau
    return np.ascontiguousarray(o.reshape(B, frames + 1, FRAME48).transpose(1, 0, 2))


def delay_samples(rate):
    return ENGINE_DELAY // factor(rate) + 2 * T


def chain_f64(x, L):
    """float64 model of the whole chain around an ideal engine at a 0 dB attenuation limit: x [N] at the low rate ->
    z [N] at the low rate.  Up (zero-stuffing and the double design), the engine as a 2880-sample delay band-limited to
    20 kHz (an FFT mask over the zero-padded signal), down (the double design / L, every L-th sample).  Zero initial state,
    like a fresh context; causal, total delay delay_samples()."""
    x = np.asarray(x, np.float64)
    D, N = T * L, x.size
    h = design(L)
    u = np.zeros(N * L)
    u[::L] = x
    # with the taps stored from k = -D, the kernel's y[j] = sum_i u[i] h[j - D - i] is element j of the full convolution: the
    # centre tap sits D samples in, which is the up-converter's delay
    y = np.convolve(u, h)[:N * L]
    y = np.concatenate([np.zeros(ENGINE_DELAY), y])[:N * L]
    M = 1 << int(np.ceil(np.log2(y.size + 4 * D)))
    Y = np.fft.rfft(y, M)
    Y[np.fft.rfftfreq(M, 1.0 / 48000) >= 20000.0] = 0
    y = np.fft.irfft(Y, M)[:y.size]
    # likewise z[m] = sum_i g[Lm - D - i] o[i] is element Lm of the full convolution with g
    return np.convolve(y, h / L)[0:N * L:L]
