"""Per-stream frame report and saturating int16 output without a GPU: the record layout (include/percepnet_hip.h
PN_REPORT_WORDS, api.REPORT_DTYPE), the refusals of the five new entry points, and the numpy model of the two casts and the clip
count (tests/report_model.py) that the GPU tests check the engine against, pinned here to hand-worked values."""
import os
import re

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import report_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("pn_ctx_set_report", "pn_ctx_set_output_saturate", "pn_ctx_read_report", "pn_ctx_read_report_dev", "pn_host_next_report")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return api.load_library()


def test_record_layout():
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    assert re.search(r"^#define PN_REPORT_WORDS 8$", hdr, re.M)
    d = api.REPORT_DTYPE
    assert api.REPORT_WORDS == 8 and d.itemsize == 32 == 4 * api.REPORT_WORDS
    want = [("in_peak", "<f4"), ("in_energy", "<f4"), ("out_peak", "<f4"), ("out_energy", "<f4"), ("gain_mean", "<f4"),
            ("pitch_period", "<i4"), ("out_clipped", "<i4"), ("flags", "<u4")]
    assert d.names == tuple(n for n, _ in want)
    for word, (name, kind) in enumerate(want):
        assert d.fields[name][1] == 4 * word and d.fields[name][0] == np.dtype(kind), name
    raw = np.arange(16, dtype="<u4")                       # two records: word k of record r is 8 r + k
    rec = raw.view(d)
    assert rec.shape == (2,) and rec["pitch_period"].tolist() == [5, 13] and rec["flags"].tolist() == [7, 15]
    assert rec["in_peak"].view("<u4").tolist() == [0, 8]


def test_new_calls_are_exported_and_refuse_null(lib):
    buf = np.zeros(8, np.uint32)
    for name in NEW_CALLS:
        assert hasattr(lib, name), name
    for rc in (lib.pn_ctx_set_report(None, 1), lib.pn_ctx_set_report(None, 0), lib.pn_ctx_set_output_saturate(None, 1),
               lib.pn_ctx_read_report(None, buf.ctypes.data), lib.pn_ctx_read_report_dev(None, buf.ctypes.data),
               lib.pn_host_next_report(None, buf.ctypes.data), lib.pn_host_next_report(None, None)):
        assert rc == -1
        assert lib.pn_last_error()
    assert not buf.any()


INF = float("inf")
DENORMAL_O = 2.0 ** -135                                    # below FLT_MIN = 2^-126; times 32768 it is the denormal 2^-120


def UP(x, toward):
    """The fp32 neighbour of x in the direction of `toward`, as a Python float."""
    return float(np.nextafter(np.float32(x), np.float32(toward)))


# t = o * 32768 ->            wrap (main.cpp:36)  saturate  counted
HAND = [(32767.9,              32767,             32767,    False),
        (-32767.9,            -32767,            -32767,    False),
        (32768.0,             -32768,             32767,    True),      # the full-scale click: +32768 wraps to -32768
        (-32768.0,            -32768,            -32768,    False),
        (-32768.5,            -32768,            -32768,    False),     # truncation toward zero still fits
        (-32769.0,             32767,            -32768,    True),
        (float("nan"),         0,                 0,        True),      # cvttss2si's 0x80000000, low 16 bits
        (0.0,                  0,                 0,        False),
        (-0.9,                 0,                 0,        False),
        (40000.0,              40000 - 65536,     32767,    True),
        (-40000.0,             65536 - 40000,    -32768,    True),
        (float("inf"),         0,                 32767,    True),
        (float("-inf"),        0,                -32768,    True),
        (3e9,                  0,                 32767,    True),
        # the thresholds and their fp32 neighbours (ulp 2^-9 just below 32768, 2^-8 just above): cvttss2si truncates toward zero
        # to int32, or gives 0x80000000 when that does not fit; the cast keeps the low 16 bits
        (32767.0,              32767,             32767,    False),
        (UP(32768.0, 0),       32767,             32767,    False),     # 32767.998...: truncates to 32767, fits
        (UP(32768.0, INF),    -32768,             32767,    True),      # 32768.0039...: 0x8000
        (UP(-32768.0, -INF),  -32768,            -32768,    False),     # -32768.0039...: truncates to -32768, fits
        (UP(-32769.0, 0),     -32768,            -32768,    False),     # -32768.996...: still -32768, both ways
        (65535.5,             -1,                 32767,    True),      # 0xffff
        (65536.0,              0,                 32767,    True),      # 0x10000
        (98304.0,             -32768,             32767,    True),      # 0x18000
        (2147483520.0,        -128,               32767,    True),      # the largest float below 2^31: 0x7fffff80
        (2147483648.0,         0,                 32767,    True),      # does not fit: 0x80000000
        (-2147483648.0,        0,                -32768,    True),      # fits, and is 0x80000000 itself
        (2.0 ** -140,          0,                 0,        False),     # a denormal t
        (DENORMAL_O * 32768.0, 0,                 0,        False)]     # a denormal o: t = 2^-120
# o whose product o * 32768 overflows fp32 ->  wrap  saturate  counted
HAND_O = [(np.finfo(np.float32).max,           0,    32767,    True),
          (-np.finfo(np.float32).max,          0,   -32768,    True),
          (DENORMAL_O,                         0,    0,        False)]


def test_cast_and_count_model_hand_worked_values():
    """The wrap column is cvttss2si's low 16 bits worked by hand.  It is not pinned against oracle/percepnet_oracle.c here:
    the oracle's cast (f2s) is a static function that only pno_run_pcm applies, to the output of a whole engine run from a
    zero state, and the oracle has no state import, so chosen values cannot be put in front of it from Python without changing
    the oracle's recipe.  tests/test_atten_limit_host.py holds the numpy wrap (backend_model.f2s) bit-equal to the oracle's PCM
    on ordinary signals."""
    t = np.array([h[0] for h in HAND], np.float32)
    assert rm.cast_t(t, False).tolist() == [h[1] for h in HAND]
    assert rm.cast_t(t, True).tolist() == [h[2] for h in HAND]
    assert rm.clipped_t(t).tolist() == [h[3] for h in HAND]
    assert rm.cast_t(t, True).dtype == np.int16 and rm.cast_t(t, False).dtype == np.int16
    assert all(float(a) == h[0] for a, h in zip(t[14:], HAND[14:])), "every threshold row is an fp32 value as written"
    assert t[14 + 1] == np.float32(32768) - np.float32(2.0 ** -9) and t[14 + 3] == np.float32(-32768) - np.float32(2.0 ** -8)
    o = np.array([h[0] for h in HAND_O], np.float32)
    assert rm.cast(o, False).tolist() == [h[1] for h in HAND_O] and rm.cast(o, True).tolist() == [h[2] for h in HAND_O]
    assert rm.clipped_t(rm.scaled(o)).tolist() == [h[3] for h in HAND_O] and np.isinf(rm.scaled(o)[:2]).all()
    # through o: the fp32 product is what is cast and counted
    o = np.zeros((2, 480), np.float32)
    o[0, :3] = [1.0, -1.0, np.float32(32767.9) / np.float32(32768)]
    o[1, 5] = np.nan
    assert rm.count_clipped(o).tolist() == [1, 1] and rm.count_clipped(o).dtype == np.int32
    assert rm.cast(o, True)[0, :3].tolist() == [32767, -32768, 32767] and rm.cast(o, False)[0, :3].tolist() == [-32768, -32768, 32767]
    # where nothing leaves the range the two casts agree
    rng = np.random.default_rng(0)
    v = rng.uniform(-1, 1, 4096).astype(np.float32) * np.float32(0.999)
    assert np.array_equal(rm.cast(v, True), rm.cast(v, False)) and rm.count_clipped(v) == 0


def test_levels_of_non_finite_rows():
    """include/percepnet_hip.h, record table: a peak is the fmax-style maximum of |v| from 0 — a NaN sample is ignored, 480 NaNs
    give 0; an energy is the fp32 sum of fp32 products — NaN as soon as one sample is NaN, +inf on overflow otherwise."""
    big, nan = np.finfo(np.float32).max, np.float32("nan")
    v = np.zeros((8, 480), np.float32)
    v[0, :] = nan                                            # 480 NaNs
    v[1, 7], v[1, 100], v[1, 479] = 0.25, nan, -0.5          # one NaN among finite samples
    v[2, 3], v[2, 4] = nan, -np.inf                          # NaN and inf: peak inf, energy NaN
    v[3, 0], v[3, 9] = np.inf, 0.5                           # inf alone
    v[4, 5], v[4, 6] = 1e30, -0.5                            # a product that overflows
    v[5, :] = 1e18                                           # 480 finite products of 1e36: the sum overflows
    v[6, 11], v[6, 12] = 0.5, -0.75                          # finite
    v[7, 0] = big
    assert rm.peak(v).tolist() == [0.0, 0.5, INF, INF, np.float32(1e30), np.float32(1e18), 0.75, big]
    assert rm.peak(v).dtype == np.float32
    want = np.array([nan, nan, nan, INF, INF, INF, 0.8125, INF], np.float32)
    assert rm.energy_matches(want, v).all()
    for wrong in (0.0, 1.0, INF, -INF, big):                 # a NaN row accepts nothing but NaN
        assert not rm.energy_matches(np.full(8, wrong, np.float32), v)[:3].any(), wrong
    for wrong in (nan, 0.0, big, -INF):                      # an overflowing row nothing but +inf
        assert not rm.energy_matches(np.full(8, wrong, np.float32), v)[[3, 4, 5, 7]].any(), wrong
    # a finite row keeps the relative 3e-5 of the float64 sum, and refuses NaN and inf
    fin = np.array([0.8125 * (1 + 2.9e-5), 0.8125 * (1 - 2.9e-5), 0.8125 * (1 + 3.2e-5), 0.8125 * (1 - 3.2e-5), nan, INF], np.float32)
    assert rm.energy_matches(fin, np.broadcast_to(v[6], (6, 480))).tolist() == [True, True, False, False, False, False]
    # check_report on such rows: what the header says passes, np.abs(o).max()'s NaN or a finite energy does not
    rep = np.zeros(8, api.REPORT_DTYPE)
    rep["out_peak"], rep["out_energy"], rep["out_clipped"] = rm.peak(v), want, rm.count_clipped(v)
    zeros = np.zeros((8, 480), np.int16)
    args = (v, np.zeros((8, 68), np.float32), np.zeros(8, np.int32), np.zeros(8, np.int32), zeros)
    rm.check_report(rep, *args)
    assert rep["out_clipped"].tolist() == [480, 1, 2, 1, 1, 480, 0, 1]
    for word, row, value in (("out_peak", 0, nan), ("out_peak", 1, nan), ("out_energy", 1, 0.3125), ("out_energy", 4, big),
                             ("out_clipped", 1, 0), ("out_peak", 6, 0.5)):
        bad = rep.copy()
        bad[word][row] = value
        with pytest.raises(AssertionError):
            rm.check_report(bad, *args)
    # the input side reads the same rules, from float rows as a float entry point stores them
    rep2 = np.zeros(8, api.REPORT_DTYPE)
    rep2["in_peak"], rep2["in_energy"] = rm.peak(v), want
    rm.check_report(rep2, np.zeros((8, 480), np.float32), *args[1:4], v)
    bad = rep2.copy()
    bad["in_peak"][1] = nan
    with pytest.raises(AssertionError):
        rm.check_report(bad, np.zeros((8, 480), np.float32), *args[1:4], v)

    # an energy is never accepted either way: a float64 sum clearly beyond FLT_MAX must be +inf, one clearly below must be near
    edge = np.zeros((2, 480), np.float32)
    edge[0, :2], edge[1, :2] = 1.3043e19, 1.3046e19         # 2 x^2 = 3.40240e38 and 3.40397e38 around FLT_MAX = 3.40282e38
    assert rm.energy_matches(np.array([3.4024e38, INF], np.float32), edge).all()
    assert not rm.energy_matches(np.array([INF, 3.4028e38], np.float32), edge).any()


def test_edge_rows_of_the_gpu_cast_tests():
    """What tests/test_gpu_cast_edges.py relies on in report_model.edge_rows, checked here without a GPU."""
    rows = rm.edge_rows([h[0] for h in HAND])
    assert set(rows) == {"E", "N", "P", "A", "C", None} and all(r.shape == (480,) and r.dtype == np.float32 for r in rows.values())
    fin = np.array([h[0] for h in HAND if np.isfinite(h[0])], np.float32)
    e = rows["E"]
    t = e * np.float32(32768)
    assert set(t.tolist()) == set(fin.tolist()) - {2.0 ** -140}, "every finite row of HAND but the denormal t, exactly (t / 32768 is exact)"
    lanes = rm.clipped_t(t).reshape(60, 8).sum(axis=1)
    assert np.all(lanes >= 1) and np.all(lanes <= 7), "every lane owns an out-of-range and an in-range sample"
    assert np.abs(e).max() == np.float32(3e9) / np.float32(32768) <= 1e5 and ((e != 0) & (np.abs(e) < np.finfo(np.float32).tiny)).any()
    assert rm.count_clipped(e) >= 60 and np.isfinite((e.astype(np.float64) ** 2).sum())
    n = rows["N"]
    assert np.isnan(n).sum() == 3 and np.isinf(n).sum() == 4 and (np.abs(n) == np.finfo(np.float32).max).sum() == 4
    assert rm.count_clipped(n) == 11 and rm.peak(n) == INF
    # quiet NaNs only
    for r in (rows["N"], rows["P"], rows["A"]):
        assert np.all(r[np.isnan(r)].view(np.uint32) & 0x00400000)
    assert np.isnan(rows["P"]).sum() == 1 and np.isnan(rows["P"][137]) and rm.count_clipped(rows["P"]) == 1 and 0 < rm.peak(rows["P"]) < 0.5
    assert np.isnan(rows["A"]).all() and rm.count_clipped(rows["A"]) == 480 and rm.peak(rows["A"]) == 0
    assert rm.count_clipped(rows["C"]) == 0 and 0.9 < rm.peak(rows["C"]) < 1 and not rows[None].any()
