"""Idle-line and subnormal signal levels on the host (no GPU): is the CPU oracle a valid yardstick there, and do the rows of
tests/tiny_levels.py tell a flushing kernel from a faithful one?

Three things, per row of tiny_levels.rows():
  * the host keeps fp32 subnormals (numpy is the model of several GPU comparisons), before and after the mutant ran;
  * the oracle is the compiled reference, bit for bit, at these levels too (skipped where oracle/_ref is not built);
  * the MUTANT: the same oracle with flush-to-zero and denormals-are-zero forced in the thread's MXCSR (pno_debug_flush_mode),
    i.e. what a kernel does if its instructions flush subnormals.  Where the mutant differs from the oracle, a GPU comparison
    against the oracle (tests/test_gpu_tiny_levels.py) can fail; where it does not, that comparison says nothing about
    subnormals.  The zone conditions below keep the GPU test from being vacuous; they are not measurements of the code under test.

The table, condensed from what `python -m tests.test_tiny_levels_host` prints (equal neighbours as one line; 20 frames per row;
dPer, dFeat, dGR: frames whose pitch period, 70 features, g|r tap differ between oracle and mutant; dOut: output words that
differ, of 9600; Ysub, Osub: subnormal words in the oracle's look-ahead spectra Y and in its output):

  row                      zone  dPer dFeat  dGR  dOut   Ysub  Osub
  f1e+0.0 .. f1e-4.0       loud     0     0    0     0      0     0      (9 rows)
  f1e-4.5                  Z1       1     1   15  7193      0     0
  f1e-5.0                  Z1      15    15   15  7199      0     0
  f1e-5.5                  Z1      15    15   15  7200      0     0
  f1e-6.0                  Z1      15    15   15  7199      0     0
  f1e-6.5 .. f1e-12.5      mid      0     0    0     0      0     0      (13 rows)
  f1e-13.0                 Z2       0     3    0     0      0     0
  f1e-13.5                 Z2       0    18    0     0      0     0
  f1e-14.0 .. f1e-18.0     Z2       0    20    0     0      0     0      (9 rows)
  f1e-18.5                 Z3       6    20   15  7030      0     0
  f1e-19.0                 Z3      15    20   15  7177      0     0
  f1e-19.5 .. f1e-21.0     Z3      15    20   15 >=7195     0     0      (4 rows)
  f1e-21.5                 Z3      15    19   15  7197      0     0
  f1e-22.0, f1e-22.5       Z3      15    15   15 >=7197     0     0
  f1e-23.0 .. f1e-26.5     mid      0     0    0     0      0     0      (8 rows; the period is 766 from here down)
  f1e-27.0                 Z4       0     0    0    76      0     0
  f1e-27.5                 Z4       0     0    0   556      2     0
  f1e-28.0                 Z4       0     0    0  3153     15     0
  f1e-28.5                 Z4       0     0    0  5764     17     0
  f1e-29.0 .. f1e-40.0     Z4       0     0    0 >=7136  17 .. 19217  1 .. 7186   (23 rows)
  f1e-40.5                 Z4       0     0    0  7011  18847  7011
  f1e-41.0                 Z5       0     0    0     0  18435     0      (the output is all zero from here down)
  f1e-41.5                 Z5       0     0    0     0  17895     0
  f1e-42.0                 Z5       0     0    0     0  16827     0
  f1e-42.5 .. f1e-45.5     Z5       0     0    0     0      0     0      (7 rows: Y is all zero)
  dither1                  Z1      15    15   15  7199      0     0
  dither2                  Z1      15    15   15  7200      0     0
  dither3                  Z1       9     9   15  7199      0     0
  dither4                  Z1       1     1   15  7176      0     0
  dither8                  loud     0     0    0     0      0     0
  voiced_peak1             Z1       1     1   15  7187      0     0
  voiced_peak2, 4, 8       mid      0     0    0     0      0     0
  impulse, dc_plus1, dc_minus1  mid 0     0    0     0      0     0
  zero_dither_alternating  Z1      10    10   12  4799      0     0
  loud_to_dither_step      Z1       4     4    4  1911      0     0
  synth0, 3, 7, 13         loud     0     0    0     0      0     0
"""
import numpy as np
import pytest

from oracle.oracle import Reference, ref_available
from tests import tiny_levels as tl

F32 = np.float32
WORDS = tl.T * 480


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _host_keeps_subnormals():
    a, b = np.array([1e-30], F32), np.array([1e-10], F32)        # arrays: the product is computed now, by this thread
    return F32(1e-30) * F32(1e-10) != 0 and (a * b)[0] != 0 and (a * b)[0] == F32(1e-40)


def _run(oracle, x):
    st = oracle.stages(x)
    out, gr = oracle.run_float(x)
    return dict(period=st["period"].copy(), feat=st["feat"].copy(), Y=st["Y"].copy(), out=out, gr=gr)


def _measure(oracle):
    """{name: (oracle, mutant)} of every row; the mutant runs last and the thread's MXCSR is restored whatever happens."""
    R = tl.rows()
    assert _host_keeps_subnormals()
    plain = {name: _run(oracle, r.x) for name, r in R.items()}
    prev = oracle.flush_mode(True)
    try:
        if prev == -1:
            pytest.skip("the oracle was built without SSE: no flush mode")
        assert not _host_keeps_subnormals(), "flush mode did not reach this thread"
        mutant = {name: _run(oracle, r.x) for name, r in R.items()}
    finally:
        if prev != -1:
            oracle.flush_mode(prev)
    assert _host_keeps_subnormals(), "the host lost its subnormals after the mutant ran"
    return {name: (plain[name], mutant[name]) for name in R}


@pytest.fixture(scope="module")
def measured(oracle):
    return _measure(oracle)


def _figures(pair):
    a, b = pair
    return dict(dPer=int((a["period"] != b["period"]).sum()),
                dFeat=int((_bits(a["feat"]) != _bits(b["feat"])).any(axis=1).sum()),
                dGR=int((_bits(a["gr"]) != _bits(b["gr"])).any(axis=1).sum()),
                dOut=int((_bits(a["out"]) != _bits(b["out"])).sum()),
                Ysub=int(tl.subnormal(a["Y"].view(F32)).sum()), Osub=int(tl.subnormal(a["out"]).sum()))


def table(measured):
    lines = [f"{'row':24s} {'zone':5s} {'dPer':>4s} {'dFeat':>5s} {'dGR':>4s} {'dOut':>5s} {'Ysub':>6s} {'Osub':>5s}"]
    for name, r in tl.rows().items():
        f = _figures(measured[name])
        lines.append(f"{name:24s} {r.zone:5s} {f['dPer']:4d} {f['dFeat']:5d} {f['dGR']:4d} {f['dOut']:5d} {f['Ysub']:6d} {f['Osub']:5d}")
    return "\n".join(lines)


def _zone(measured, zone):
    return {name: _figures(measured[name]) for name, r in tl.rows().items() if r.zone == zone}


def test_host_keeps_fp32_subnormals_before_and_after_the_mutant(measured):
    assert F32(1e-30) * F32(1e-10) != 0
    assert _host_keeps_subnormals()


def test_rows_and_batches_are_what_the_gpu_test_assumes():
    R = tl.rows()
    assert len(R) == 92 + 5 + 4 + 5 + 4 and all(r.x.dtype == F32 and r.x.shape == (WORDS,) for r in R.values())
    assert [n for n in R if n.startswith("f1e")] == [tl.ladder_name(h) for h in range(0, -92, -1)]
    for name, r in R.items():
        if r.grid:
            pcm = tl.pcm_of(r)
            assert np.array_equal(pcm.astype(F32) / F32(32768), r.x), name
    assert np.abs(tl.pcm_of(R["dither1"])).max() == 1 and set(np.unique(tl.pcm_of(R["dither4"]))) == set(range(-4, 5))
    assert [int(np.abs(tl.pcm_of(R[f"voiced_peak{p}"])).max()) for p in tl.VOICED_PEAKS_LSB] == list(tl.VOICED_PEAKS_LSB)
    imp = tl.pcm_of(R["impulse"])
    assert imp[700] == 1 and np.count_nonzero(imp) == 1
    alt = tl.pcm_of(R["zero_dither_alternating"]).reshape(tl.T, 480)
    assert not alt[0:3].any() and alt[3:6].any(axis=1).all() and not alt[6:9].any()
    step = tl.pcm_of(R["loud_to_dither_step"]).reshape(tl.T, 480)
    assert np.abs(step[:8]).max() > 20000 and np.abs(step[8:]).max() == 1
    seen = {}
    for order in (0, 1, 2):
        names = tl.batch(order)
        assert len(names) % 16 != 0 and set(names) == set(R)
        for i in range(0, len(names), 4):
            zones = [R[n].zone for n in names[i:i + 4]]
            assert len(set(zones)) == len(zones), (order, i, zones)              # a wavefront of four: four zones
        for i in range(0, len(names), 16):
            blk = names[i:i + 16]
            assert any(n.startswith("synth") for n in blk) and any(R[n].zone == "Z1" for n in blk), (order, i)
        for i, n in enumerate(names):
            seen.setdefault(n, []).append((i % 4, frozenset(names[i - i % 4:i - i % 4 + 4]) - {n}))
    once = {n: v for n, v in seen.items() if len(v) == 3}                        # (the rows a batch holds twice have 6 places)
    for n, v in once.items():
        assert len({p for p, _ in v}) >= 2 and len({nb for _, nb in v}) == 3, n   # other lane rows, other neighbours
    assert sum(len({p for p, _ in v}) == 3 for v in once.values()) >= len(once) - 2   # three different lane rows, all but two


@pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built (no /root/reference)")
def test_oracle_is_the_compiled_reference_on_every_row(blob, oracle, measured):
    ref = Reference(blob)
    for name, r in tl.rows().items():
        out, gr = measured[name][0]["out"], measured[name][0]["gr"]
        ro, rg = ref.run_float(r.x)
        assert np.array_equal(_bits(out), _bits(ro)) and np.array_equal(_bits(gr), _bits(rg)), name
        if r.grid:
            pcm = tl.pcm_of(r)
            (po, pg), (qo, qg) = oracle.run_pcm(pcm), ref.run_pcm(pcm)
            assert np.array_equal(po, qo) and np.array_equal(_bits(pg), _bits(qg)), name


def test_z1_decision_zone_the_period_depends_on_subnormals(measured):
    hit = [n for n, f in _zone(measured, "Z1").items() if f["dPer"] >= 8]
    assert len(hit) >= 5 and sum(tl.rows()[n].grid for n in hit) >= 2, hit
    assert "dither1" in hit and "dither2" in hit                      # an idle 16-bit line


def test_z2_features_depend_on_subnormals_the_period_does_not(measured):
    hit = [n for n, f in _zone(measured, "Z2").items() if f["dFeat"] >= 15 and f["dPer"] == 0]
    assert len(hit) >= 8, hit


def test_z3_the_correlations_are_subnormal(measured):
    hit = [n for n, f in _zone(measured, "Z3").items() if f["dPer"] >= 10]
    assert len(hit) >= 6, hit


def test_z4_output_words_depend_on_subnormals(measured):
    hit = [n for n, f in _zone(measured, "Z4").items() if f["dOut"] >= 7000 and f["dPer"] == 0]
    assert len(hit) >= 20, hit


def test_z5_the_spectra_hold_subnormal_words(measured):
    hit = [n for n, f in _zone(measured, "Z5").items() if f["Ysub"] >= 5000]
    assert len(hit) >= 2, hit
    assert all(tl.subnormal(tl.rows()[n].x).any() for n in hit)       # the input itself is subnormal


def test_loud_rows_flush_mode_changes_nothing(measured):
    loud = _zone(measured, "loud")
    assert len(loud) >= 14
    for n, f in loud.items():
        assert f["dPer"] == f["dFeat"] == f["dGR"] == f["dOut"] == 0, (n, f)


def test_tiny_energy_bound_is_the_existing_bound_plus_a_subnormal_term():
    from tests import report_model as rm
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, (6, 480)).astype(F32)
    e = (v * v).sum(axis=-1, dtype=F32)
    assert tl.energy_matches_tiny(e, v).all() and rm.energy_matches(e, v).all()
    assert not tl.energy_matches_tiny(e * F32(1.0001), v).any()
    tiny = (v * F32(1e-22)).astype(F32)                                # products of ~1e-44: a few subnormal ulps each
    e = (tiny * tiny).sum(axis=-1, dtype=F32)
    assert tl.subnormal(e).all() and tl.energy_matches_tiny(e, tiny).all()
    assert tl.energy_matches_tiny(np.zeros(6, F32), tiny).sum() == 0   # flushed to zero: 480 lost products are not 960 half ulps
    assert tl.energy_matches_tiny(np.zeros(6, F32), np.zeros((6, 480), F32)).all()


if __name__ == "__main__":
    from percepnet_amd import weights
    from oracle.oracle import Oracle
    print(table(_measure(Oracle(weights.default_blob(1234)))))
