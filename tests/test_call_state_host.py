"""The call-state record of the rate converter without a GPU: include/percepnet_hip.h "call-state records", the layout and the verdict
percepnet_amd/csrc/pn_call_rules.h (pn_rate_call_state_bytes / pn_rate_call_state_check), against the numpy model
tests/call_state_model.py; and the rules under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/c/call_state_sanitize.cpp).  The device side is tests/test_gpu_call_state.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import agc_model as am
from tests import call_state_model as cs
from tests import lim_model as lm
from tests import plc_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def bits(x):
    return int(np.array([x], F32).view(U32)[0])


def models(B=3, seed=5):
    """states no frame need have produced, but every one of them legal"""
    rng = np.random.default_rng(seed)
    plc, agc, lim = pm.Plc(B), am.Agc(B), lm.Lim(B)
    plc.hist[:] = rng.standard_normal((B, pm.HIST)).astype(F32) * F32(0.1)
    plc.q[:] = rng.standard_normal((B, pm.P_MAX)).astype(F32) * F32(0.1)
    plc.P[:], plc.r[:], plc.lost[:] = (480, 0, 720)[:B], (2, 0, 1)[:B], (9, 0, 4)[:B]
    agc.state[:] = [(3.5, 8.0, 17, 0), (0.0, 0.0, 0, 0), (1e-3, 1.0 / 1024.0, 0xFFFFFFFF, 0)][:B]
    lim.state[:] = [(0.25, 2, 5, 0), (0.0, 0, 0, 0), (1.0, 0, 0xFFFFFFFF, 0)][:B]
    levels = np.array([12.0, 0.0, 3e-9][:B], F32)
    return plc, agc, lim, levels


def good(mask=cs.ALL, s=0):
    plc, agc, lim, levels = models()
    return cs.pack(s, mask, plc, agc, lim, levels).copy()


def words(rec):
    return rec.view(U32)


def both(rec):
    """the host's verdict, which must be the model's"""
    v = api.rate_call_state_check(rec)
    assert v == cs.verdict(rec), (v, cs.verdict(rec))
    return v


def test_size_offsets_and_constants_are_pinned():
    assert api.rate_call_state_bytes() == api.RATE_CALL_STATE_BYTES == cs.BYTES == 10640
    assert (api.CALL_W_HIST, api.CALL_W_Q, api.CALL_W_META, api.CALL_W_AGC, api.CALL_W_LIM, api.CALL_W_MIX, api.CALL_BODY_WORDS) == (0, 1920, 2640, 2644, 2648, 2652, 2656)
    assert (cs.W_HIST, cs.W_Q, cs.W_META, cs.W_AGC, cs.W_LIM, cs.W_MIX, cs.BODY_WORDS) == (0, 1920, 2640, 2644, 2648, 2652, 2656)
    assert cs.BYTES == 16 + 4 * cs.BODY_WORDS == 16 + 4 * (pm.HIST + pm.P_MAX + 4) + am.STATE_DTYPE.itemsize + lm.STATE_DTYPE.itemsize + 16
    assert all(4 * w % 16 == 0 for w in (cs.W_Q, cs.W_META, cs.W_AGC, cs.W_LIM, cs.W_MIX, cs.BODY_WORDS)), "every section is 16-byte aligned"
    assert (api.CALL_PLC, api.CALL_AGC, api.CALL_LIM, api.CALL_MIX) == (cs.PLC, cs.AGC, cs.LIM, cs.MIX) == (1, 2, 4, 8)
    assert api.RATE_CALL_MAGIC == cs.MAGIC == int.from_bytes(b"PNCS", "little") and api.RATE_CALL_VERSION == cs.VERSION == 1
    assert api.SS_BAD_STATE == cs.BAD_STATE == -7
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    for name, v in (("PN_RATE_CALL_STATE_BYTES", 10640), ("PN_CALL_W_Q", 1920), ("PN_CALL_W_META", 2640), ("PN_CALL_W_AGC", 2644), ("PN_CALL_W_LIM", 2648),
                    ("PN_CALL_W_MIX", 2652), ("PN_CALL_BODY_WORDS", 2656), ("PN_CALL_PLC", 1), ("PN_CALL_AGC", 2), ("PN_CALL_LIM", 4), ("PN_CALL_MIX", 8)):
        assert re.search(rf"#define {name} {v}\b", hdr), name
    assert re.search(r"PN_SS_BAD_STATE = -7\b", hdr) and "#define PN_RATE_CALL_MAGIC 0x53434e50u" in hdr


def test_pack_and_unpack_are_inverse_and_lay_the_words_where_the_header_says():
    plc, agc, lim, levels = models()
    for s in range(3):
        rec = cs.pack(s, cs.ALL, plc, agc, lim, levels)
        assert rec.dtype == np.uint8 and rec.size == cs.BYTES and both(rec) == cs.OK
        w = words(rec)
        assert w[:4].tolist() == [cs.MAGIC, 1, 10640, 15]
        b = w[4:]
        assert b[cs.W_HIST:cs.W_Q].view(F32).tobytes() == plc.hist[s].tobytes() and b[cs.W_Q:cs.W_META].view(F32).tobytes() == plc.q[s].tobytes()
        assert b[cs.W_META:cs.W_AGC].tolist() == [plc.P[s], plc.r[s], plc.lost[s], 0]
        assert b[cs.W_AGC:cs.W_LIM].tobytes() == agc.state[s].tobytes() and b[cs.W_LIM:cs.W_MIX].tobytes() == lim.state[s].tobytes()
        assert b[cs.W_MIX:].tolist() == [bits(levels[s]), 0, 0, 0]
        p2, a2, l2, lv2 = pm.Plc(3), am.Agc(3), lm.Lim(3), np.zeros(3, F32)
        assert cs.unpack(rec, 2 - s, cs.ALL, p2, a2, l2, lv2) == cs.ALL
        assert cs.pack(2 - s, cs.ALL, p2, a2, l2, lv2).tobytes() == rec.tobytes()
    # a record with the AGC section alone into models that hold everything: the other three are zeroed
    rec = cs.pack(0, cs.AGC, agc=agc)
    assert both(rec) == cs.OK and not words(rec)[4:4 + cs.W_AGC].any() and not words(rec)[4 + cs.W_LIM:].any()
    cs.unpack(rec, 0, cs.ALL, plc, agc, lim, levels)
    assert not plc.hist[0].any() and plc.P[0] == 0 and lim.state[0].tobytes() == bytes(16) and levels[0] == 0 and agc.state[0]["gain"] == 8.0
    # a full record into models that hold no PLC: the section is dropped
    plc, agc, lim, levels = models()
    keep = plc.hist[1].copy()
    cs.unpack(good(cs.ALL, 0), 1, cs.ALL & ~cs.PLC, plc, agc, lim, levels)
    assert plc.hist[1].tobytes() == keep.tobytes() and agc.state[1]["gain"] == 8.0 and levels[1] == 12.0


def test_a_good_record_under_every_mask():
    for mask in range(16):
        assert both(good(mask)) == cs.OK, mask
    assert both(cs.empty().view(np.uint8)) == cs.OK


def test_every_bad_code():
    rec = good()
    assert api.rate_call_state_check(b"") == cs.verdict(None) == api.SS_BAD_ARG            # (an empty buffer travels as NULL)
    for n in (1, 15, 16, 17, 10639):
        assert both(rec[:n]) == api.SS_BAD_SIZE, n
    assert both(np.concatenate([rec, np.zeros(1, np.uint8)])) == api.SS_BAD_SIZE
    for word, v, want in ((0, 0x53524E50, api.SS_BAD_MAGIC), (1, 2, api.SS_BAD_VERSION), (1, 0, api.SS_BAD_VERSION), (2, 10624, api.SS_BAD_SIZE), (2, 912, api.SS_BAD_SIZE),
                          (3, 16, api.SS_BAD_STATE), (3, 0x8000000F, api.SS_BAD_STATE)):
        r = rec.copy()
        words(r)[word] = v
        assert both(r) == want, (word, v)
        assert api.load_library().pn_last_error(), "a refusal says why"
    # the order: magic, version, size, mask
    r = rec.copy()
    words(r)[:4] = (1, 2, 3, 16)
    assert both(r) == api.SS_BAD_MAGIC
    words(r)[0] = cs.MAGIC
    assert both(r) == api.SS_BAD_VERSION
    words(r)[1] = 1
    assert both(r) == api.SS_BAD_SIZE
    words(r)[2] = 10640
    assert both(r) == api.SS_BAD_STATE
    # a tails record is not a call-state record, and the other way round
    assert both(np.zeros(912, np.uint8)) == api.SS_BAD_MAGIC and api.rate_state_check(rec[:912], 8000) == api.SS_BAD_MAGIC


ONE_UP = lambda x: np.nextafter(F32(x), F32(np.inf))            # noqa: E731
ONE_DOWN = lambda x: np.nextafter(F32(x), F32(-np.inf))         # noqa: E731
EDGES = (
    # PLC: P, r, word 3
    (cs.W_META, 239, cs.BAD_STATE), (cs.W_META, 240, cs.OK), (cs.W_META, 720, cs.OK), (cs.W_META, 721, cs.BAD_STATE), (cs.W_META, 1, cs.BAD_STATE),
    (cs.W_META, 0, cs.BAD_STATE),                                # r is 2 in this record: a run without a lag
    (cs.W_META, 0xFFFFFFFF, cs.BAD_STATE), (cs.W_META + 1, 0x7FFFFFFF, cs.OK), (cs.W_META + 2, 0xFFFFFFFF, cs.OK), (cs.W_META + 3, 1, cs.BAD_STATE),
    # AGC: lev, gain, spare
    (cs.W_AGC, bits(0.0), cs.OK), (cs.W_AGC, bits(np.inf), cs.OK), (cs.W_AGC, bits(np.nan), cs.BAD_STATE), (cs.W_AGC, bits(-1e-30), cs.BAD_STATE),
    (cs.W_AGC + 1, 0, cs.OK), (cs.W_AGC + 1, bits(1.0 / 1024.0), cs.OK), (cs.W_AGC + 1, bits(ONE_DOWN(1.0 / 1024.0)), cs.BAD_STATE), (cs.W_AGC + 1, bits(1024.0), cs.OK),
    (cs.W_AGC + 1, bits(ONE_UP(1024.0)), cs.BAD_STATE), (cs.W_AGC + 1, bits(np.nan), cs.BAD_STATE), (cs.W_AGC + 1, bits(np.inf), cs.BAD_STATE),
    (cs.W_AGC + 1, bits(-1.0), cs.BAD_STATE), (cs.W_AGC + 1, bits(-0.0), cs.BAD_STATE), (cs.W_AGC + 3, 1, cs.BAD_STATE),
    # limiter: gain bits 0, the smallest subnormal, 1.0, the float above it, NaN; spare
    (cs.W_LIM, 0, cs.OK), (cs.W_LIM, 1, cs.OK), (cs.W_LIM, bits(1.0), cs.OK), (cs.W_LIM, bits(ONE_UP(1.0)), cs.BAD_STATE), (cs.W_LIM, bits(np.nan), cs.BAD_STATE),
    (cs.W_LIM, bits(2.0), cs.BAD_STATE), (cs.W_LIM, bits(-0.0), cs.BAD_STATE), (cs.W_LIM, bits(-0.5), cs.BAD_STATE), (cs.W_LIM + 1, 1000, cs.OK), (cs.W_LIM + 3, 1, cs.BAD_STATE),
    # MIX: level, padding
    (cs.W_MIX, 0, cs.OK), (cs.W_MIX, bits(3.4028235e38), cs.OK), (cs.W_MIX, bits(np.inf), cs.BAD_STATE), (cs.W_MIX, bits(np.nan), cs.BAD_STATE), (cs.W_MIX, bits(-1.0), cs.BAD_STATE),
    (cs.W_MIX + 1, 1, cs.BAD_STATE), (cs.W_MIX + 2, 1, cs.BAD_STATE), (cs.W_MIX + 3, 1, cs.BAD_STATE),
)


@pytest.mark.parametrize("word,value,want", EDGES, ids=lambda v: hex(v) if isinstance(v, int) and v > 4000 else str(v))
def test_each_invariant_at_its_edge(word, value, want):
    rec = good()
    assert words(rec)[4 + cs.W_META:4 + cs.W_AGC].tolist() == [480, 2, 9, 0]
    words(rec)[4 + word] = value
    assert both(rec) == want
    # the same word under a mask WITHOUT its section: not an invariant then, but a non-zero word of an absent section
    bit = next(b for b, (lo, hi) in cs.SECTION.items() if lo <= word < hi)
    rec = good(cs.ALL & ~bit)
    words(rec)[4 + word] = value
    assert both(rec) == (cs.OK if value == 0 else cs.BAD_STATE)


def test_p_zero_is_legal_only_without_a_run():
    rec = good()
    words(rec)[4 + cs.W_META:4 + cs.W_META + 2] = (0, 0)
    assert both(rec) == cs.OK
    words(rec)[4 + cs.W_META + 1] = 1
    assert both(rec) == cs.BAD_STATE


@pytest.mark.parametrize("bit", (cs.PLC, cs.AGC, cs.LIM, cs.MIX))
def test_an_absent_section_with_one_non_zero_word(bit):
    lo, hi = cs.SECTION[bit]
    for w in sorted({lo, hi - 1, (lo + hi) // 2, min(lo + 1919, hi - 1), min(lo + 1920, hi - 1), min(lo + 2639, hi - 1)}):
        for v in (1, 0x80000000):                                          # (-0.0f is not zero)
            rec = good(cs.ALL & ~bit)
            words(rec)[4 + w] = v
            assert both(rec) == cs.BAD_STATE, (bit, w, v)
    rec = good(0)
    rec[-1] = 1
    assert both(rec) == cs.BAD_STATE


def test_random_records_get_the_models_verdict():
    rng = np.random.default_rng(17)
    seen = set()
    for it in range(300):
        rec = good(int(rng.integers(0, 16)))
        b = words(rec)[4:]
        for _ in range(int(rng.integers(0, 3))):
            w = int(rng.choice([cs.W_META, cs.W_META + 1, cs.W_META + 3, cs.W_AGC, cs.W_AGC + 1, cs.W_AGC + 3, cs.W_LIM, cs.W_LIM + 3, cs.W_MIX, cs.W_MIX + 2, 5, 2000]))
            b[w] = rng.choice([0, 1, 239, 240, 720, 721, bits(1.0), bits(-1.0), bits(np.nan), bits(np.inf), bits(0.5), bits(2000.0), int(rng.integers(0, 2 ** 32))])
        seen.add(both(rec))
    assert seen == {cs.OK, cs.BAD_STATE}


def test_rules_under_sanitizers(tmp_path):
    """tests/c/call_state_sanitize.cpp = pn_call_rules.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined and run as its own executable: the check over heap buffers of exactly the bytes handed in — every
    length around 16 and around 10640 — and over hostile records."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "call_state_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "call_state_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
