"""The host-only surface behind the converter's pipelined path, device-side records and kernel timing, no GPU
(include/percepnet_hip.h "batched rate converter"): the fixed record stride, the new symbols exported and declared, the verdicts of
pn_rate_state_check unchanged on the table of hostile headers the GPU test feeds the device import (tests/rate_records_cases.py),
and the list rule and the shared header verdict under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/c/rate_records_sanitize.cpp)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import rate_records_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pn_rate_submit_host_f32", "pn_rate_submit_host_i16", "pn_rate_submit_host_f32_active", "pn_rate_submit_host_i16_active",
               "pn_rate_host_pipeline_prepare", "pn_rate_state_max_bytes", "pn_rate_record_stride", "pn_rate_export_streams",
               "pn_rate_import_streams", "pn_rate_set_profiling", "pn_rate_kernel_time", "pn_rate_reset_profile")


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def test_max_record_bytes(lib):
    assert api.rate_state_max_bytes() == 912 == max(api.rate_state_bytes(r) for r in api.RATES)
    assert cases.STATE_BYTES == {r: api.rate_state_bytes(r) for r in api.RATES}
    header = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    assert re.search(r"#define\s+PN_RATE_STATE_MAX_BYTES\s+912\b", header)


def test_new_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout if shutil.which("nm") else None
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/percepnet_hip.h"
        if exported is not None:
            assert re.search(r"\bT %s$" % name, exported, re.M), f"{name} is not in the dynamic symbol table"
    for name in ("host_pipeline_prepare", "frames_delivered"):
        assert callable(getattr(api.Context, name))
    for name in ("submit_host_i16", "submit_host_f32", "host_pipeline_prepare", "record_stride", "export_streams_dev", "import_streams_dev",
                 "set_profiling", "kernel_times", "reset_profile"):
        assert callable(getattr(api.RateConverter, name)) and callable(getattr(api.MixedRateConverter, name))
    # what the header no longer disclaims
    section = header[header.index("batched rate converter"):header.index("mixed rates: 8, 16, 24 and 48 kHz")]
    assert "NOT provided: other rates." in section


@pytest.mark.parametrize("rate", api.RATES)
def test_state_check_verdicts_are_unchanged(lib, rate):
    assert (api.SS_OK, api.SS_BAD_MAGIC, api.SS_BAD_VERSION, api.SS_BAD_SIZE, api.SS_BAD_RATE) == \
        (cases.SS_OK, cases.SS_BAD_MAGIC, cases.SS_BAD_VERSION, cases.SS_BAD_SIZE, cases.SS_BAD_RATE)
    seen = set()
    for name, hdr, verdict in cases.hostile_headers(rate):
        rec = np.full(api.rate_state_bytes(rate), 0x5A, np.uint8)
        rec[:16] = np.frombuffer(hdr, np.uint8)
        assert api.rate_state_check(rec, rate) == verdict, (rate, name)
        if verdict != api.SS_OK:
            assert lib.pn_last_error(), (rate, name)
        seen.add(verdict)
    assert seen == {cases.SS_OK, cases.SS_BAD_MAGIC, cases.SS_BAD_VERSION, cases.SS_BAD_SIZE, cases.SS_BAD_RATE}
    # the messages of the three verdicts a converter words itself
    good = cases.hostile_headers(rate)[0][1]
    short = np.zeros(api.rate_state_bytes(rate) - 4, np.uint8)
    short[:16] = np.frombuffer(good, np.uint8)
    assert api.rate_state_check(short, rate) == api.SS_BAD_SIZE and b"rate-state record of" in lib.pn_last_error()
    assert api.rate_state_check(np.zeros(8, np.uint8), rate) == api.SS_BAD_SIZE
    other = dict((n, h) for n, h, _ in cases.hostile_headers(rate))["other_rate"]
    rec = np.zeros(api.rate_state_bytes(rate), np.uint8)
    rec[:16] = np.frombuffer(other, np.uint8)
    assert api.rate_state_check(rec, rate) == api.SS_BAD_RATE and b"this converter runs at %d" % rate in lib.pn_last_error()
    rec[:16] = np.frombuffer(dict((n, h) for n, h, _ in cases.hostile_headers(rate))["magic"], np.uint8)
    assert api.rate_state_check(rec, rate) == api.SS_BAD_MAGIC and b"not a rate-state record" in lib.pn_last_error()


def test_rules_under_sanitizers(tmp_path):
    """tests/c/rate_records_sanitize.cpp = pn_rate_mixed.h and pn_rate_design.h (+ pn_model.cpp for the error string) built WITHOUT HIP
    by plain g++ with -fsanitize=address,undefined: the list rule of a device record call and the header verdict the device import
    shares with pn_rate_state_check, over exactly-sized copies."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "rate_records_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "rate_records_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
