"""The conference table's host-only surface, no GPU (include/percepnet_hip.h "conferences"; the rules live in the HIP-free
percepnet_amd/csrc/pn_conf.h): the constants, pn_rate_confs_check naming the first bad index, the CLI's refusals that need no
device, the numpy model's own arithmetic (tests/conf_model.py), and the table rules under the address and undefined-behaviour
sanitizers in a stand-alone program (tests/c/conf_sanitize.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from percepnet_amd import api, build
from tests import conf_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return api.load_library()


def test_constants():
    assert (api.CONF_NONE, api.CONF_MAX_MEMBERS) == (cm.NONE, cm.MAX_MEMBERS) == (-1, 32)
    hdr = open(os.path.join(ROOT, "include", "percepnet_hip.h")).read()
    assert "#define PN_CONF_NONE (-1)" in hdr and "#define PN_CONF_MAX_MEMBERS 32" in hdr


def test_confs_check_names_the_first_bad_index(lib):
    good = np.array([-1, 0, 5, 5, -1, 3], np.int32)
    assert lib.pn_rate_confs_check(good.ctypes.data, 6, 6) == 0
    assert lib.pn_rate_confs_check(good.ctypes.data, 0, 6) == 0 and lib.pn_rate_confs_check(None, 0, 6) == 0
    assert lib.pn_rate_confs_check(None, 3, 6) == -1 and lib.pn_rate_confs_check(good.ctypes.data, -1, 6) == -1
    assert lib.pn_rate_confs_check(good.ctypes.data, 6, 5) == -1 and b"at index 2:" in lib.pn_last_error(), "5 is no conference of 5 streams"
    for at in range(6):
        for bad in (6, -2, 8000):
            t = good.copy()
            t[at] = bad
            if at < 5:
                t[5] = 77                                          # a later bad one is not the one named
            assert lib.pn_rate_confs_check(t.ctypes.data, 6, 6) == -1
            err = lib.pn_last_error()
            assert b"at index %d:" % at in err and str(bad).encode() in err, err
    api.rate_confs_check(good, 6)
    with pytest.raises(api.PercepNetError, match="at index 1:"):
        api.rate_confs_check([0, 4, 9], 4)


def test_the_model_adds_in_ascending_order_and_skips_the_listener():
    # 1e30, 1, -1e30 in slots 0, 2, 3 of one conference: the order decides the answer
    y = np.zeros((5, 480), F32)
    y[0], y[2], y[3], y[4] = F32(1e30), F32(1.0), F32(-1e30), F32(7.0)
    confs = [1, cm.NONE, 1, 1, 4]
    o = cm.mix(y, confs)
    assert (o[0] == F32(1.0) + F32(-1e30)).all() and (o[2] == 0).all() and (o[3] == F32(1e30)).all()      # (1e30 + 1) - 1e30... without the listener
    assert cm.same(o[1], y[1]) and (o[4] == 0).all() and not np.signbit(o[4]).any(), "no conference: the row itself; alone: +0.0"
    # an unlisted member contributes nothing and keeps its sentinel
    o = cm.mix(y, confs, ids=[3, 0], out=np.full_like(y, 9))
    assert (o[0] == F32(-1e30)).all() and (o[3] == F32(1e30)).all() and (o[[1, 2, 4]] == 9).all()
    # -0.0 alone in a sum becomes +0.0 (acc starts at +0.0); inf - inf and NaN are NaN
    y[:] = 0
    y[2], y[3] = F32(-0.0), F32(np.inf)
    y[0, 1] = F32(-np.inf)
    y[0, 2] = F32(np.nan)
    o = cm.mix(y, confs)
    assert not np.signbit(o[3, 0]) and np.isnan(o[2, 1]) and np.isnan(o[2, 2]) and o[2, 0] == np.inf
    assert cm.same(o, o.copy()) and not cm.same(o, np.zeros_like(o)) and not cm.same(np.array([-0.0], F32), np.array([0.0], F32))


def test_cli_refuses_conference_with_slots_and_bad_lists(tmp_path):
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    for i in range(2):
        (tmp_path / f"in{i}.pcm").write_bytes(bytes(1920))
    files = ["in0.pcm", "out0.pcm", "in1.pcm", "out1.pcm"]
    for opts, word in ((["--conference", "0,0", "--slots", "1"], "--slots"), (["--conference", "0"], "entries"), (["--conference", "0,2"], "at index 1"),
                       (["--conference", "0,x"], "expected"), (["--conference", "-,-,0"], "entries")):
        run = subprocess.run([exe] + opts + files, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and "conference" in run.stderr and word in run.stderr, (opts, run.stderr)
        assert not (tmp_path / "out0.pcm").exists(), opts


def test_table_rules_under_sanitizers(tmp_path):
    """tests/c/conf_sanitize.cpp = pn_conf.h (+ pn_model.cpp for the error string) built WITHOUT HIP by plain g++ with
    -fsanitize=address,undefined: tables of 0 and 1 streams, a conference of exactly 32 and one of 33, ascending order for
    interleaved members, a stream moved between two full conferences."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "conf_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DPN_NO_HIP", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c", "conf_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
