"""The idle-line and subnormal-level rows, in one place (HIP-free; imported as `from tests import tiny_levels`): one table for the
host test (tests/test_tiny_levels_host.py: the oracle against the compiled reference and against its own flush-to-zero mutant)
and for the GPU test (tests/test_gpu_tiny_levels.py: every kernel a tiny sample passes through against the oracle).

rows(T) -> {name: Row}: float32 rows of [T * 480] with the zone each belongs to.  The zones are the levels at which a different
part of the reference's fp32 arithmetic runs through subnormals (numerics; measured per row in the docstring of
tests/test_tiny_levels_host.py):

  Z1    1e-4.5 .. 1e-6 and +-1..4 LSB of a 16-bit line: find_best_pitch's (xcorr * 1e-12)^2 numerators (pitch.cpp:46-104)
  Z2    1e-13 .. 1e-18: band energies and their products
  Z3    1e-18.5 .. 1e-22.5: the pitch correlations themselves
  Z4    1e-27 .. 1e-40.5: spectra and output samples
  Z5    <= 1e-41: the input itself
  loud  >= 1e-4, dither of +-8 LSB, the synth streams: no subnormal reaches a decision or an output
  mid   the levels between the zones and the int16-grid rows no zone condition names: compared like every other row, claimed by
        no condition

batch(order) -> the names in stream order: every wavefront of four streams of the split pitch kernel holds four different zones,
every 16-stream block a synth stream and a Z1 row.
"""
import itertools
from collections import namedtuple

import numpy as np

from percepnet_amd import synth

F32 = np.float32
FRAME = 480
T = 20
PERIOD = 217                       # samples of the base waveform's fundamental
HALF_DECADES = range(0, -92, -1)   # the float ladder: voiced * 10^(h/2)
DITHER_LSB = (1, 2, 3, 4, 8)
VOICED_PEAKS_LSB = (1, 2, 4, 8)
FILLERS = (0, 3, 7, 13)            # synth.synth_stream kinds: voiced, loud, bursts, two-tone
ZONES = ("Z1", "Z2", "Z3", "Z4", "Z5", "loud", "mid")

Row = namedtuple("Row", "x zone grid")          # x float32 [T * 480]; grid: the row is value / 32768 of an int16 row


def ladder_zone(h):
    """Zone of the ladder row voiced * 10^(h/2)."""
    if h >= -8:
        return "loud"
    if -12 <= h <= -9:
        return "Z1"
    if -36 <= h <= -26:
        return "Z2"
    if -45 <= h <= -37:
        return "Z3"
    if -81 <= h <= -54:
        return "Z4"
    if h <= -82:
        return "Z5"
    return "mid"


def ladder_name(h):
    return f"f1e{h / 2:+.1f}"


_cache = {}


def rows(T=T):
    """-> {name: Row}, in a fixed order.  One generator, default_rng(7): the noise of the base waveform first, then the dither
    rows in the order +-1, +-2, +-3, +-4, +-8 LSB (uniform integers of [-k, k])."""
    if T in _cache:
        return _cache[T]
    n = T * FRAME
    rng = np.random.default_rng(7)
    t = np.arange(n)
    voiced = sum((0.5 / k) * np.sin(2 * np.pi * k * t / PERIOD) for k in range(1, 8)) + 0.05 * rng.standard_normal(n)
    dither = {k: rng.integers(-k, k + 1, n).astype(np.int16) for k in DITHER_LSB}
    out = {}
    for h in HALF_DECADES:
        out[ladder_name(h)] = Row((voiced * 10.0 ** (h / 2)).astype(F32), ladder_zone(h), False)

    def grid(name, pcm, zone):
        pcm = np.asarray(pcm)
        assert pcm.shape == (n,) and np.array_equal(pcm, pcm.astype(np.int16))
        out[name] = Row(pcm.astype(np.int16).astype(F32) / F32(32768), zone, True)

    for k in DITHER_LSB:
        grid(f"dither{k}", dither[k], "Z1" if k <= 4 else "loud")
    for p in VOICED_PEAKS_LSB:
        grid(f"voiced_peak{p}", np.round(voiced / np.abs(voiced).max() * p), "Z1" if p == 1 else "mid")
    imp = np.zeros(n, np.int16)
    if n > 700:
        imp[700] = 1
    grid("impulse", imp, "mid")
    grid("dc_plus1", np.ones(n, np.int16), "mid")
    grid("dc_minus1", -np.ones(n, np.int16), "mid")
    grid("zero_dither_alternating", np.where((t // (3 * FRAME)) % 2 == 0, 0, dither[1]), "Z1")
    step = synth.synth_stream(3, T).copy()
    step[8 * FRAME:] = dither[1][8 * FRAME:]
    grid("loud_to_dither_step", step, "Z1")
    for s in FILLERS:
        grid(f"synth{s}", synth.synth_stream(s, T), "loud")
    _cache[T] = out
    return out


def pcm_of(row):
    """The int16 row of an int16-grid row (exact: its floats are value / 32768)."""
    assert row.grid
    v = row.x * F32(32768)
    assert np.array_equal(v, np.round(v))
    return v.astype(np.int16)


# extra copies in a batch: a synth stream for every 16-stream block, and the +-1..4 LSB dither rows a second time
_COPIES = tuple(f"synth{s}" for s in FILLERS) + tuple(f"dither{k}" for k in (1, 2, 3, 4))


_batches = {}


def batch(order=0, T=T):
    """-> list of row names, one per stream (a name may come twice).  Streams 4w .. 4w+3 share a wavefront of the split pitch
    kernel: the four rows of such a group are of four different zones.  Streams 16b .. 16b+15 share a block: each block holds a
    synth stream and a Z1 row.  len() is no multiple of 16, the last group and block are partial.  `order` 0, 1, 2: three
    arrangements; with each step every zone's rows move on to other groups (other neighbours), and within its group of four a
    row takes a place it did not have in an earlier arrangement (another 16-lane row of the wave)."""
    assert order in (0, 1, 2)
    if (order, T) in _batches:
        return list(_batches[order, T])
    R = rows(T)
    fill = [f"synth{s}" for s in FILLERS] * 2
    pools = {z: [] for z in ZONES}
    for name, r in R.items():
        if not name.startswith("synth"):
            pools[r.zone].append(name)
    pools["Z1"] += [c for c in _COPIES if c.startswith("dither")]
    rot = lambda v, k: v[k % len(v):] + v[:k % len(v)] if v else v
    fill = rot(fill, 3 * order)
    pools = {z: rot(v, 5 * order) for z, v in pools.items()}
    total = len(fill) + sum(len(v) for v in pools.values())
    assert total % 16 != 0
    n_groups = (total + 3) // 4
    n_blocks = (n_groups + 3) // 4
    assert len(fill) == n_blocks and (n_groups - 1) % 4 >= 1          # the partial last block still has its second group
    z1 = [pools["Z1"].pop(0) for _ in range(n_blocks)]                # one Z1 row reserved for each block
    used = {}                                                         # name -> places it had in the earlier arrangements
    for k in range(order):
        for i, name in enumerate(batch(k, T)):
            used.setdefault(name, set()).add(i % 4)
    names = []
    for q in range(n_groups):
        want = min(4, total - len(names))
        group, zones = [], set()
        if q % 4 == 0:
            group.append(fill.pop(0)); zones.add("loud")
        elif q % 4 == 1:
            group.append(z1.pop(0)); zones.add("Z1")
        while len(group) < want:
            z = max((z for z in ZONES if z not in zones and pools[z]), key=lambda z: len(pools[z]))   # the fullest other zone
            group.append(pools[z].pop(0)); zones.add(z)
        names += min(itertools.permutations(group), key=lambda g: sum(p in used.get(n, ()) for p, n in enumerate(g)))
    assert not fill and not z1 and not any(pools.values()) and len(names) == total
    _batches[order, T] = tuple(names)
    return names


def stack(names, T=T):
    R = rows(T)
    return np.stack([R[n].x for n in names])


def subnormal(a):
    a = np.asarray(a, F32)
    return (a != 0) & (np.abs(a) < np.finfo(F32).tiny)


def energy_matches_tiny(got, v):
    """report_model.energy_matches for finite rows at any level down to zero: the fp32 word `got` [...] against the float64 sum of
    squares `want` of the rows v [..., 480] within 3e-5 * want + 960 * 2^-150.  The relative term is the existing one (any fp32
    summation order of 480 non-negative products: gamma_481 * 2^-24 ~ 2.9e-5).  The absolute term covers what a relative bound
    cannot once the words are subnormal: 480 products and 480 additions, each of which may lose half an ulp of a subnormal,
    2^-150.  Both are derived, neither is measured."""
    got, v = np.asarray(got, F32), np.asarray(v, F32)
    assert np.isfinite(v).all()
    want = (v.astype(np.float64) ** 2).sum(axis=-1)
    return np.abs(got.astype(np.float64) - want) <= 3e-5 * want + 960 * 2.0 ** -150
