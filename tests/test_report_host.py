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
        (3e9,                  0,                 32767,    True)]


def test_cast_and_count_model_hand_worked_values():
    t = np.array([h[0] for h in HAND], np.float32)
    assert rm.cast_t(t, False).tolist() == [h[1] for h in HAND]
    assert rm.cast_t(t, True).tolist() == [h[2] for h in HAND]
    assert rm.clipped_t(t).tolist() == [h[3] for h in HAND]
    assert rm.cast_t(t, True).dtype == np.int16 and rm.cast_t(t, False).dtype == np.int16
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
