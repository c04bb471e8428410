"""The training-feature generator's edge pairs, in one place (HIP-free; imported as `from tests import featgen_cases`): one table
for the host test (tests/test_featgen_cases_host.py: the oracle's train_run against the compiled reference's train(), and the
conditions that keep the GPU comparison from being vacuous) and for the GPU test (tests/test_gpu_featgen_edges.py: pn_featgen_*,
the target kernel, the saturating cast and the file driver against the oracle).

cases(T) -> {name: (speech int16 [T * 480], noisy int16 [T * 480])}, in a fixed order.  What each group is there for
(denoise.cpp:549-589, 603-787; measured per case in the docstring of tests/test_featgen_cases_host.py):

  peakN+ditherN, */dither*, dither*/*   ideal gains far below 1e-9 and Z1 pitch decisions (tests/tiny_levels.py) on both sides
  impulse/dc1, dc-1/dc+1                gains down to 1e-28; the oracle's own records change when subnormals are flushed
  alt/step, step/alt                    a level step of 90 dB on one side against an idle line on the other
  identical, identical_loud, square_both, fullnoise_both
                                        Exp == Ephaty bit for bit: `ephatp < exp_` on its equality edge, `gi > 1` everywhere,
                                        and test_output.pcm on both int16 rails
  quarter, neg                          a noisy file quieter than / opposite to its speech: the `gi > 1` clamp is the whole record
  noisy_zero, speech_zero               digital silence on one side (speech_zero is the pure-noise training pair)
  loud/square, square/loud              unrelated loud files: `ephatp < exp_` in most bands
  pulse40, saw700, missing233, jump150  the noisy side's pitch decision (rec[68], rec[69], Ephaty) at both ends of the period
                                        range, on a missing fundamental and across period jumps (the signals of
                                        test_pitch_analysis_on_periodic_signals_bit_exact)

batch(order) -> (speech, noisy, rows): 131 pairs (two full 64-thread blocks of pn_targets_kernel and a ragged one; no multiple of
the front ends' groups of 16 and 4; ragged for the saturate kernel's 256-thread blocks), every case once at rows[name], every
other row a different synth.synth_pair.
"""
import numpy as np

from percepnet_amd import synth
from tests import tiny_levels as tl

FRAME = 480
T = 20
B = 131
SQUARE_HALF_PERIOD = 120
FULLNOISE_SEED = 20261019

# case -> its row in batch(0).  The first ten sit on the rows that bound a block of the target kernel (63 | 64, 127 | 128), a
# group of 16 (15 | 16), and the batch (0, 1, 130); the others are spread over both full blocks, every place modulo 4 taken.
ROWS0 = {
    "peak1+dither1": 0, "zero/dither1": 1, "dc-1/dc+1": 15, "identical_loud": 16, "square_both": 63, "fullnoise_both": 64,
    "noisy_zero": 65, "speech_zero": 127, "impulse/dc1": 128, "square/loud": 130,
    "peak4+dither2": 5, "peak8+dither8": 10, "dither1/zero": 22, "dither1_both": 29, "alt/step": 36, "step/alt": 43,
    "voiced/dither3": 50, "dither4/voiced": 57, "identical": 70, "quarter": 77, "neg": 84, "loud/square": 91,
    "pulse40": 98, "saw700": 105, "missing233": 112, "jump150": 119,
}
NAMED_ROWS = (0, 1, 15, 16, 63, 64, 65, 127, 128, 130)
# batch(1): a row of a full block moves to the other full block and the next place modulo 4, 64 * (1 - r // 64) + (r + 1) % 64;
# the two cases of the ragged block move into the full ones, and two others take their rows
_ROWS1_EXCEPT = {"impulse/dc1": 63, "square/loud": 127, "peak4+dither2": 128, "jump150": 130}

_cache = {}


def cases(T=T):
    """-> {name: (speech, noisy)}; deterministic, the arrays are shared between calls: do not write to them."""
    if T in _cache:
        return _cache[T]
    n = T * FRAME
    t = np.arange(n)
    R = tl.rows(T)
    row = lambda name: tl.pcm_of(R[name])
    i16 = lambda v: np.clip(v, -32768, 32767).astype(np.int16)
    zero = np.zeros(n, np.int16)
    voiced, loud = synth.synth_stream(0, T), synth.synth_stream(3, T)
    square = np.where((t // SQUARE_HALF_PERIOD) % 2 == 0, 32767, -32768).astype(np.int16)
    fullnoise = np.random.default_rng(FULLNOISE_SEED).integers(-32768, 32768, n).astype(np.int16)
    out = {}
    for p, d in ((1, 1), (4, 2), (8, 8)):
        v = row(f"voiced_peak{p}")
        out[f"peak{p}+dither{d}"] = (v, i16(v.astype(np.int32) + row(f"dither{d}")))
    out["zero/dither1"] = (zero, row("dither1"))
    out["dither1/zero"] = (row("dither1"), zero)
    out["dither1_both"] = (row("dither1"), row("dither1"))
    out["impulse/dc1"] = (row("impulse"), row("dc_plus1"))
    out["dc-1/dc+1"] = (row("dc_minus1"), row("dc_plus1"))
    out["alt/step"] = (row("zero_dither_alternating"), row("loud_to_dither_step"))
    out["step/alt"] = (row("loud_to_dither_step"), row("zero_dither_alternating"))
    out["voiced/dither3"] = (voiced, row("dither3"))
    out["dither4/voiced"] = (row("dither4"), voiced)
    out["identical"] = (voiced, voiced)
    out["identical_loud"] = (loud, loud)
    out["square_both"] = (square, square)
    out["fullnoise_both"] = (fullnoise, fullnoise)
    out["quarter"] = (voiced, voiced // 4)
    out["neg"] = (voiced, i16(-voiced.astype(np.int32)))
    out["noisy_zero"] = (voiced, zero)
    out["speech_zero"] = (zero, voiced)
    out["loud/square"] = (loud, square)
    out["square/loud"] = (square, loud)
    # the formulas of tests/test_gpu_parity.py::test_pitch_analysis_on_periodic_signals_bit_exact
    out["pulse40"] = (voiced, i16(np.where(t % 40 == 0, 20000, 0)))
    out["saw700"] = (voiced, i16(((t % 700) * (24000.0 / 700) - 12000).astype(np.int64)))
    w = 2 * np.pi / 233
    out["missing233"] = (voiced, i16((6000 * np.sin(2 * w * t) + 5000 * np.sin(3 * w * t)).astype(np.int64)))
    pj = np.where((t // (3 * FRAME)) % 2 == 0, 150, 187)
    out["jump150"] = (voiced, i16(np.where(t % pj == 0, 18000, 0)))
    assert set(out) == set(ROWS0)
    for sp, no in out.values():
        assert sp.dtype == no.dtype == np.int16 and sp.shape == no.shape == (n,)
    _cache[T] = out
    return out


PITCH_CASES = ("pulse40", "saw700", "missing233", "jump150")


def case_rows(order):
    """-> {name: row} of batch(order)."""
    assert order in (0, 1)
    if order == 0:
        return dict(ROWS0)
    return {name: _ROWS1_EXCEPT.get(name, 64 * (1 - r // 64) + (r + 1) % 64) for name, r in ROWS0.items()}


def filler_pairs(order):
    """-> {row: p} for the rows no case takes: synth.synth_pair(p), p = 0 .. 104 upwards along the rows in batch(0) and
    downwards in batch(1), so that a case meets other neighbours and the oracle's records of the fillers are computed once."""
    taken = set(case_rows(order).values())
    free = [r for r in range(B) if r not in taken]
    ps = range(len(free)) if order == 0 else range(len(free) - 1, -1, -1)
    return dict(zip(free, ps))


_batches = {}


def batch(order, T=T):
    """-> (speech int16 [131, T * 480], noisy the same, {name: row})."""
    if (order, T) not in _batches:
        C, rows = cases(T), case_rows(order)
        sp = np.empty((B, T * FRAME), np.int16)
        no = np.empty_like(sp)
        for name, r in rows.items():
            sp[r], no[r] = C[name]
        for r, p in filler_pairs(order).items():
            sp[r], no[r] = synth.synth_pair(p, T)
        sp.setflags(write=False); no.setflags(write=False)
        _batches[order, T] = (sp, no, rows)
    return _batches[order, T]


def gains_match(g, og, rtol):
    """The bound of the generator's 34 ideal gains: |g - og| <= rtol * |og| + 4 * 2^-149, and zero exactly where the oracle is.
    The relative term is that of tests/test_gpu_featgen.py (libm's sinf against OCML's, each within 1 ULP of sin, then a few
    roundings).  The absolute term is derived, not measured: after sinf the path is two multiplies, two 34-term sums of
    non-negatives, a divide, a sqrt and a multiply; sinf is relatively accurate for small arguments, so the error stays relative
    down to the subnormal range, where only the last roundings into a subnormal word (g * sinf, G * gw on either side) can cost an
    absolute half unit, 2^-150, each."""
    g, og = np.asarray(g, np.float64), np.asarray(og, np.float64)
    return (np.abs(g - og) <= rtol * np.abs(og) + 4 * 2.0 ** -149) & ((g == 0) == (og == 0))
