"""Per-stream state records without a GPU: the documented layout and the host-side validator pn_stream_state_check
(include/percepnet_hip.h, "per-stream state records").  A record that arrives from another process or machine is
checked with it before pn_ctx_import_streams_host; here it is fed well-formed, truncated, mis-sized, foreign and
garbage bytes."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from percepnet_amd import api, build, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, floats) of the body in record order: the live ring entries, oldest first, then the in-place state
BODY = [("HIST", 11 * 480), ("SPEC", 5 * 400 * 2), ("EY", 5 * 36), ("CONV1", 4 * 128), ("CONV2", 2 * 512),
        ("GRU", 4 * 512), ("GRU_RB", 128), ("SYNTH", 480), ("TAIL", 4)]


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return api.load_library()


@pytest.fixture(scope="module")
def models(lib):
    a, b = api.Model(weights.default_blob(1234)), api.Model(weights.default_blob(4321))
    yield a, b
    a.close(); b.close()


def header_constants():
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    return {k: int(v, 0) for k, v in re.findall(r"#define (PN_SS_\w+|PN_STREAM_STATE_\w+) (0x[0-9a-f]+|\d+)u?\b", hdr)}


def digest(lib, model):
    out = ctypes.create_string_buffer(32)          # (fits the argtypes tests/test_abi.py gives this symbol, and none)
    lib.pn_model_digest(ctypes.c_void_p(model.h), out)
    return out.raw


def record(lib, model, nn_mode=api.NN_MFMA, magic=0x53534E50, version=1, size=api.STREAM_STATE_BYTES, seed=0):
    body = np.random.default_rng(seed).standard_normal((api.STREAM_STATE_BYTES - 64) // 4).astype(np.float32).tobytes()
    return struct.pack("<IIIi", magic, version, size, nn_mode) + digest(lib, model) + bytes(16) + body


def check(lib, rec, model):
    buf = ctypes.create_string_buffer(bytes(rec), max(len(rec), 1))
    return lib.pn_stream_state_check(buf, len(rec), ctypes.c_void_p(model.h))


def test_record_size_equals_the_documented_layout(lib):
    c = header_constants()
    assert lib.pn_stream_state_bytes() == api.STREAM_STATE_BYTES == 64 + 4 * sum(n for _, n in BODY) == 54688
    assert c["PN_STREAM_STATE_HEADER_BYTES"] == 64 and c["PN_STREAM_STATE_VERSION"] == 1
    assert struct.pack("<I", c["PN_STREAM_STATE_MAGIC"]) == b"PNSS"
    off = 0
    for name, n in BODY:
        assert c["PN_SS_" + name] == off, name
        assert off % 4 == 0, name                      # every section float4-aligned
        off += n
    assert c["PN_SS_BODY_WORDS"] == off


def test_check_accepts_a_well_formed_record_of_any_source_mode(lib, models):
    a, _ = models
    for mode in (api.NN_MFMA, api.NN_STRICT, api.NN_MFMA_F16, api.NN_MFMA_X3, 77):
        assert check(lib, record(lib, a, nn_mode=mode), a) == api.SS_OK, lib.pn_last_error()
    assert api.stream_state_check(record(lib, a), a) == api.SS_OK


def test_check_refuses_bad_headers_sizes_and_foreign_models(lib, models):
    a, b = models
    good = record(lib, a)
    assert check(lib, record(lib, a, magic=0x53534E51), a) == api.SS_BAD_MAGIC
    assert check(lib, record(lib, a, version=2), a) == api.SS_BAD_VERSION
    assert check(lib, record(lib, a, size=api.STREAM_STATE_BYTES - 16), a) == api.SS_BAD_SIZE     # header names another size
    assert check(lib, good[:-1], a) == api.SS_BAD_SIZE                                            # truncated
    assert check(lib, good[:64], a) == api.SS_BAD_SIZE                                            # header only
    assert check(lib, good + bytes(16), a) == api.SS_BAD_SIZE                                     # too long
    assert check(lib, good, b) == api.SS_BAD_MODEL and "another model" in lib.pn_last_error().decode()
    assert check(lib, record(lib, b), b) == api.SS_OK
    flipped = bytearray(good); flipped[16 + 31] ^= 1                                              # one digest bit
    assert check(lib, flipped, a) == api.SS_BAD_MODEL
    assert lib.pn_stream_state_check(None, api.STREAM_STATE_BYTES, ctypes.c_void_p(a.h)) == api.SS_BAD_ARG
    assert lib.pn_stream_state_check(ctypes.create_string_buffer(good, len(good)), len(good), None) == api.SS_BAD_ARG


def test_check_survives_garbage(lib, models):
    a, _ = models
    rng = np.random.default_rng(7)
    for n in list(range(0, 80)) + [api.STREAM_STATE_BYTES - 1, api.STREAM_STATE_BYTES, api.STREAM_STATE_BYTES + 1]:
        junk = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert check(lib, junk, a) < 0, n
    # garbage that starts like a record still needs the right version, size and digest
    junk = struct.pack("<I", 0x53534E50) + rng.integers(0, 256, api.STREAM_STATE_BYTES - 4, dtype=np.uint8).tobytes()
    assert check(lib, junk, a) in (api.SS_BAD_VERSION, api.SS_BAD_SIZE, api.SS_BAD_MODEL)
