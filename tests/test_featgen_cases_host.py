"""The training-feature generator's edge pairs on the host (no GPU): is the CPU oracle's train_run a valid yardstick on the pairs
of tests/featgen_cases.py, and do those pairs reach the edges the GPU test (tests/test_gpu_featgen_edges.py) is there for?

  * the oracle is the compiled reference's train() through real files, word for word and sample for sample, on every case
    (skipped where oracle/_ref is not built);
  * the conditions below hold on the oracle alone.  They keep the GPU comparison from being vacuous; they are not measurements of
    the code under test.  The thresholds sit below what the oracle gives.

The table, condensed from what `python -m tests.test_featgen_cases_host` prints (20 frames per case; hi, lo: samples of test_output.pcm at 32767 and at
-32768; r99: share of the 680 band values with r == 0.99, i.e. where `ephatp < exp_` fired (denoise.cpp:579-589); g1: share with
g >= 0.999; ming: the smallest non-zero ideal gain, `0` where every gain is zero; dFl: record words that change when the oracle
runs with flush-to-zero and denormals-are-zero; periods: the distinct values of rec[68] * 588):

  case              hi    lo    r99     g1     ming    dFl  periods
  peak1+dither1      0     0  0.299  0.056  4.8e-06     0  211 .. 766 (10)
  peak4+dither2      0     0  0.281  0.051  3.0e-04     0  212 .. 766 (7)
  peak8+dither8      0     0  0.341  0.024  2.3e-05     0  208 .. 766 (13)
  zero/dither1       0     0  0.000  0.000        0     0  201 .. 766 (16)
  dither1/zero       0     0  0.725  0.000        0     0  766
  dither1_both       0     0  0.000  0.000  1.8e-01     0  201 .. 766 (16)
  impulse/dc1        0     0  0.093  0.000  6.3e-12    84  60, 64, 66, 766
  dc-1/dc+1          0     0  0.000  0.022  2.4e-28    91  60, 64, 66, 766
  alt/step           0     0  0.107  0.000  1.4e-26     0  220 .. 766 (15)
  step/alt           0     0  0.462  0.175  4.7e-02     0  214 .. 766 (11)
  voiced/dither3     0     0  0.141  0.609  7.7e-02     0  202 .. 766 (15)
  dither4/voiced     0     0  0.079  0.000  6.6e-19     0  294 .. 766 (14)
  identical          0     0  0.000  0.750  1-5e-07     0  294 .. 766 (14)
  identical_loud   728   705  0.000  0.750        1     0  212 .. 766 (15)
  square_both     1680  1680  0.000  0.750  1-2e-07     0  240, 766
  fullnoise_both    99    85  0.000  0.750        1     0  187 .. 766 (16)
  quarter            0     0  0.000  0.750        1     0  294 .. 766 (14)
  neg                0     0  0.000  0.750  1-5e-07     0  294 .. 766 (14)
  noisy_zero         0     0  0.731  0.000        0     0  766
  speech_zero        0     0  0.000  0.000        0     0  294 .. 766 (14)
  loud/square        0     0  0.013  0.375  2.1e-04     0  240, 766
  square/loud        0     0  0.690  0.066  3.8e-07     0  212 .. 766 (15)
  pulse40            0     0  0.141  0.241  8.5e-06     0  80, 200, 760, 766
  saw700             0     0  0.012  0.299  1.3e-08     0  181, 700, 766
  missing233         0     0  0.141  0.590  3.1e-07     0  231, 233, 766
  jump150            0     0  0.035  0.560  4.2e-03     0  150, 187, 766

g1 is 0.750 for the identical, negated and quarter-level pairs: the first five frames of a record are behind the reference's
five-frame delay, every later gain is the `gi > 1` clamp.  The four pitch cases give 10 distinct periods between them.  The
shortest is 80 (pulse40: the search doubles a period of 40, below PITCH_MIN = 60), so no pitch case reaches 70 / 588 or below; the
DC noisy files of impulse/dc1 and dc-1/dc+1 do (60, 64, 66).  The longest real ones are 700 (saw700) and 760 (pulse40); 766 is the
period of every case's first frames.
"""
import numpy as np
import pytest

from oracle.oracle import Reference, ref_available
from percepnet_amd import synth
from tests import featgen_cases as fc

R99 = np.float32(0.99)
PERIOD_SCALE = 768 - 3 * 60      # rec[68] = T / (PITCH_MAX_PERIOD - 3 * PITCH_MIN_PERIOD), denoise.cpp:767


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def runs(oracle):
    """{name: (records [T, 138], test_output.pcm [T, 480])} of the oracle, once."""
    return {name: oracle.train_run(sp, no) for name, (sp, no) in fc.cases().items()}


def _flushed(oracle, names):
    """The records of the oracle's flush-to-zero mutant; the thread's MXCSR is restored whatever happens."""
    C = fc.cases()
    prev = oracle.flush_mode(True)
    try:
        if prev == -1:
            pytest.skip("the oracle was built without SSE: no flush mode")
        return {name: oracle.train_run(*C[name])[0] for name in names}
    finally:
        if prev != -1:
            oracle.flush_mode(prev)


def _g(runs, name):
    return runs[name][0][:, 70:104]


def _r(runs, name):
    return runs[name][0][:, 104:138]


def _periods(runs, names):
    return sorted({int(round(float(v) * PERIOD_SCALE)) for name in names for v in runs[name][0][:, 68]})


def test_cases_are_what_the_table_says():
    C = fc.cases()
    assert set(C) == set(fc.ROWS0) and list(C)[:3] == ["peak1+dither1", "peak4+dither2", "peak8+dither8"]
    assert len(C) == 26 and fc.cases() is C                               # deterministic: one table
    n = fc.T * 480
    assert all(sp.dtype == no.dtype == np.int16 and sp.shape == no.shape == (n,) for sp, no in C.values())
    voiced, loud = synth.synth_stream(0, fc.T), synth.synth_stream(3, fc.T)
    for name in ("voiced/dither3", "identical", "quarter", "neg", "noisy_zero") + fc.PITCH_CASES:
        assert np.array_equal(C[name][0], voiced), name
    assert np.array_equal(C["quarter"][1], voiced // 4) and np.array_equal(C["neg"][1].astype(np.int32), np.clip(-voiced.astype(np.int32), -32768, 32767))
    assert not C["noisy_zero"][1].any() and not C["speech_zero"][0].any() and np.array_equal(C["speech_zero"][1], voiced)
    assert C["identical_loud"][0] is C["identical_loud"][1] and np.array_equal(C["identical_loud"][0], loud)
    sq = C["square_both"][0].reshape(-1, 120)
    assert (sq[0::2] == 32767).all() and (sq[1::2] == -32768).all()
    fn = C["fullnoise_both"][0]
    assert fn.min() < -32700 and fn.max() > 32700 and abs(float(fn.mean())) < 400
    assert np.abs(C["peak1+dither1"][1].astype(np.int32) - C["peak1+dither1"][0]).max() == 1
    assert np.abs(C["dc-1/dc+1"][0] + C["dc-1/dc+1"][1]).max() == 0 and (C["dc-1/dc+1"][1] == 1).all()
    p40, j150 = C["pulse40"][1], C["jump150"][1].reshape(fc.T, 480)
    assert np.array_equal(np.flatnonzero(p40), np.arange(0, n, 40)) and p40.max() == 20000
    assert np.diff(np.flatnonzero(j150[:3].reshape(-1))).tolist() == [150] * 9 and 187 in np.diff(np.flatnonzero(j150[3:6].reshape(-1)))
    assert np.abs(C["missing233"][1]).max() > 9000 and C["saw700"][1].min() == -12000


def test_batches_place_every_case_once_among_distinct_pairs():
    seen = {}
    for order in (0, 1):
        sp, no, rows = fc.batch(order)
        assert sp.shape == no.shape == (131, fc.T * 480) and sp.dtype == no.dtype == np.int16
        assert set(rows) == set(fc.cases()) and len(set(rows.values())) == len(rows)
        for name, r in rows.items():
            assert np.array_equal(sp[r], fc.cases()[name][0]) and np.array_equal(no[r], fc.cases()[name][1]), name
        pairs = {sp[r].tobytes() + no[r].tobytes() for r in range(131)}
        assert len(pairs) == 131                                          # no two rows see the same input
        fill = fc.filler_pairs(order)
        assert len(fill) == 131 - 26 and len(set(fill.values())) == len(fill) and not set(fill) & set(rows.values())
        r = next(iter(fill))
        assert np.array_equal(sp[r], synth.synth_pair(fill[r], fc.T)[0]) and np.array_equal(no[r], synth.synth_pair(fill[r], fc.T)[1])
        seen[order] = rows
    assert set(fc.NAMED_ROWS) <= set(seen[0].values()) and fc.NAMED_ROWS == (0, 1, 15, 16, 63, 64, 65, 127, 128, 130)
    assert {r // 64 for r in seen[0].values()} == {r // 64 for r in seen[1].values()} == {0, 1, 2}
    assert {r % 4 for r in seen[0].values()} == {0, 1, 2, 3}
    for name in seen[0]:                                                  # another 64-thread block, another place modulo 4
        a, b = seen[0][name], seen[1][name]
        assert a // 64 != b // 64 and a % 4 != b % 4, (name, a, b)
    assert 131 % 64 and 131 % 16 and 131 % 4 and (131 * 480) % 256


@pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built")
def test_train_oracle_is_the_compiled_reference_on_every_case(blob, runs, tmp_path):
    ref = Reference(blob)
    for k, (name, (sp, no)) in enumerate(fc.cases().items()):
        d = tmp_path / f"c{k}"; d.mkdir()
        rr, rp = ref.train(sp, no, str(d))
        orec, opcm = runs[name]
        assert np.array_equal(_bits(rr), _bits(orec)), name
        assert np.array_equal(rp, opcm), name
        assert np.array_equal(np.fromfile(d / "test_input.pcm", np.int16), no), name


def test_every_record_word_is_finite(runs):
    for name, (rec, _) in runs.items():
        assert np.isfinite(rec).all(), name


def test_both_rails_are_reached(runs):
    for name, lo_hi in (("identical_loud", 350), ("square_both", 1000), ("fullnoise_both", 50)):      # 728 / 705, 1680 / 1680, 99 / 85
        pcm = runs[name][1]
        assert (pcm == 32767).sum() >= lo_hi and (pcm == -32768).sum() >= lo_hi, (name, int((pcm == 32767).sum()), int((pcm == -32768).sum()))


def test_attenuation_branch_fires_in_most_bands_or_in_none(runs):
    for name in ("noisy_zero", "dither1/zero", "square/loud"):            # 0.731, 0.725, 0.690
        assert (_r(runs, name) == R99).mean() >= 0.5, (name, float((_r(runs, name) == R99).mean()))
    for name in ("identical", "neg", "quarter", "speech_zero"):           # the equality edge of `ephatp < exp_`, and Exp == 0
        assert not (_r(runs, name) == R99).any(), name


def test_unit_clamp_is_the_whole_record(runs):
    for name in ("identical", "neg", "quarter"):                          # 0.750: every frame behind the five-frame delay
        assert (_g(runs, name) >= 0.999).mean() >= 0.7, (name, float((_g(runs, name) >= 0.999).mean()))


def test_gains_are_zero_where_a_side_is_silent(runs):
    for name in ("speech_zero", "noisy_zero", "zero/dither1"):
        assert (_g(runs, name) == 0).all(), name


def test_smallest_gains_are_far_below_the_old_absolute_bound(runs):
    for name, below in (("dc-1/dc+1", 1e-25), ("alt/step", 1e-23), ("dither4/voiced", 1e-16), ("impulse/dc1", 1e-10)):   # 2.4e-28, 1.4e-26, 6.6e-19, 6.3e-12
        g = _g(runs, name)
        assert 0 < g[g != 0].min() < below < 1e-9, (name, float(g[g != 0].min()))


def test_flushing_subnormals_changes_the_oracles_own_records(oracle, runs):
    names = ("impulse/dc1", "dc-1/dc+1", "identical_loud")
    fl = _flushed(oracle, names)
    for name in names[:2]:                                                # 84 and 91 words of 2760
        assert (_bits(fl[name]) != _bits(runs[name][0])).sum() >= 40, name
    assert np.array_equal(_bits(fl["identical_loud"]), _bits(runs["identical_loud"][0]))      # and none of a loud pair
    assert np.float32(1e-30) * np.float32(1e-10) != 0                     # the host has its subnormals back


def test_pitch_cases_spread_the_noisy_sides_period(runs):
    """10 distinct periods: 80, 150, 181, 187, 200, 231, 233, 700, 760, 766.  The oracle delivers none at or below 70 from the pitch
    cases (pulse40 gives 80, twice its period); it does from the DC noisy files (60, 64, 66)."""
    per = _periods(runs, fc.PITCH_CASES)
    assert len(per) >= 8, per
    assert per[0] <= 80 and 700 in per and 760 in per and per[-1] >= 600, per
    assert {150, 187} <= set(_periods(runs, ("jump150",))) and 233 in _periods(runs, ("missing233",))
    assert _periods(runs, ("impulse/dc1", "dc-1/dc+1"))[0] <= 70


def table(oracle):
    runs = {name: oracle.train_run(sp, no) for name, (sp, no) in fc.cases().items()}
    fl = _flushed(oracle, list(runs))
    lines = [f"{'case':16s} {'hi':>5s} {'lo':>5s} {'r99':>6s} {'g1':>6s} {'ming':>9s} {'dFl':>5s}  periods"]
    for name, (rec, pcm) in runs.items():
        g = _g(runs, name)
        ming = g[g != 0].min() if (g != 0).any() else 0
        lines.append(f"{name:16s} {int((pcm == 32767).sum()):5d} {int((pcm == -32768).sum()):5d} {float((_r(runs, name) == R99).mean()):6.3f} "
                     f"{float((g >= 0.999).mean()):6.3f} {ming:9.3g} {int((_bits(fl[name]) != _bits(rec)).sum()):5d}  {_periods(runs, (name,))}")
    return "\n".join(lines)


if __name__ == "__main__":
    from percepnet_amd import weights
    from oracle.oracle import Oracle
    print(table(Oracle(weights.default_blob(1234))))
