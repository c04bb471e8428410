"""The kernel-family plan without a GPU (percepnet_amd/csrc/pn_plan.h through pn_debug_plan): the default regime map that the GPU
tests pin (tests/families.py REGIMES), the row-range shares, and every family override as INTEGRATION.md and tools/README.md
document it."""
import ctypes

import pytest

from percepnet_amd import api, build
from tests import families

MODES = {"mfma": api.NN_MFMA, "x3": api.NN_MFMA_X3, "f16": api.NN_MFMA_F16, "strict": api.NN_STRICT}
NN_NAME = {"mfma": "mfma_f32", "x3": "mfma_x3", "f16": "mfma_f16", "strict": "strict"}


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return ctypes.CDLL(api.LIB_PATH)


@pytest.fixture
def plan(lib, monkeypatch):
    """plan(B, mode, **env) -> pn_debug_plan's fields with exactly the overrides `env` set."""
    def run(B, mode, **env):
        for k in families.FAMILY_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        return families.debug_plan(lib, B, MODES[mode])
    return run


def fam(p):
    return (p["dense"], p["gru"], p["gru_rb"], p["narrow"])


def test_the_regime_map(plan):
    for (mode, B), reg in families.REGIMES.items():
        p = plan(B, mode)
        assert p["nn"] == NN_NAME[mode] and p["frontend"] == "split", (mode, B, p)
        assert fam(p) == (reg["dense"], reg["gru"], reg["gru_rb"], reg["narrow"]), (mode, B, p)
        assert int(p["nn_chains"]) == reg["chains"], (mode, B, p)
        assert int(p["tile"]) == families.rows_per_block(reg), (mode, B, p)
        assert int(p["share"]) == (reg["share"] or 0), (mode, B, p)


def test_the_shares_are_the_tests_shares(plan):
    for B in (16385, 20000, 24575, 24876, 32767, 49152, 65535, 65836, 100003, 131072):
        for rg in (1, 2):
            for k in (1, 2, 3, 4):
                p = plan(B, "mfma", PERCEPNET_NN_DIRECT_RG=rg, PN_NN_CHAINS=k)
                n, tile = int(p["nn_chains"]), int(p["tile"])
                assert n == k and tile == (256 if p["gru"] == "direct_rows64" else 128), (B, rg, k, p)
                assert int(p["share"]) == (families.chain_share(B, n, tile) if n > 1 else 0), (B, rg, k, p)


def test_small_batch_overrides(plan):
    assert fam(plan(1024, "mfma", PERCEPNET_SMALL_ROWS=0)) == ("batch", "batch", "batch", "n16")    # the GRU default follows: min(0, 1536)
    assert fam(plan(1000, "mfma", PERCEPNET_SMALL_ROWS=1000)) == ("small", "small", "small", "n16")
    assert fam(plan(1024, "mfma", PERCEPNET_SMALL_ROWS=1000)) == ("batch", "batch", "batch", "n16")
    assert fam(plan(8192, "mfma", PERCEPNET_SMALL_ROWS=8192)) == ("small", "batch", "small", "n16")   # GRU crossover stays at 1536
    assert fam(plan(2048, "mfma", PERCEPNET_SMALL_GRU_ROWS=4096)) == ("small", "small", "small", "n16")
    assert fam(plan(1024, "mfma", PERCEPNET_SMALL_GRU_ROWS=0)) == ("small", "batch", "small", "n16")
    assert fam(plan(1024, "x3", PERCEPNET_SMALL_ROWS=0))[0] == "x3_rows32"     # the shadow-operand layers have no small family


def test_direct_overrides(plan):
    assert plan(8192, "mfma", PERCEPNET_NN_DIRECT=1)["gru"] == "direct_rows32"
    assert plan(65536, "mfma", PERCEPNET_NN_DIRECT=0)["gru"] == "batch"
    assert plan(65536, "mfma", PERCEPNET_NN_DIRECT=0)["nn_chains"] == "1"      # an exact fit for the batch family: one chain
    assert plan(1024, "mfma", PERCEPNET_NN_DIRECT=1)["gru"] == "small"         # never together with the small families
    assert plan(2048, "mfma", PERCEPNET_NN_DIRECT=1)["gru"] == "batch"         # (small dense layers)
    assert plan(8192, "mfma", PERCEPNET_NN_DIRECT=1, PERCEPNET_SMALL_ROWS=0)["gru"] == "direct_rows32"
    assert plan(65536, "x3", PERCEPNET_NN_DIRECT=1)["gru"] == "x3_rows64"      # fp32 MFMA only
    assert plan(65536, "strict", PERCEPNET_NN_DIRECT=1)["gru"] == "batch"
    p = plan(65536, "mfma", PERCEPNET_NN_DIRECT_RG=1)
    assert (p["gru"], p["gru_rb"], p["tile"]) == ("direct_rows32", "direct_rows32", "128")
    p = plan(24576, "mfma", PERCEPNET_NN_DIRECT_RG=2)
    assert (p["gru"], p["gru_rb"], p["tile"]) == ("direct_rows64", "direct_rows64", "256")
    assert plan(24576, "mfma", PERCEPNET_NN_DIRECT_RG=3)["gru"] == "direct_rows32"   # not a direct-family value: the default
    assert plan(65536, "mfma", PERCEPNET_X3_RG=1)["gru"] == "direct_rows64"          # the shadow-operand override does not apply


@pytest.mark.parametrize("mode", ["x3", "f16"])
def test_rows_per_wave_overrides(plan, mode):
    for B in (1024, 65536):
        assert fam(plan(B, mode, PERCEPNET_X3_RG=1))[:3] == (f"{mode}_rows32",) * 3
        assert fam(plan(B, mode, PERCEPNET_X3_RG=2))[:3] == (f"{mode}_rows64",) * 3
        assert fam(plan(B, mode, PERCEPNET_X3_RG=3))[:3] == (f"{mode}_rows64", f"{mode}_rows64_paired", f"{mode}_rows64_paired")
        assert plan(B, mode, PERCEPNET_X3_RG=4)["dense"] == f"{mode}_rows{64 if B >= 32768 else 32}"
        assert plan(B, mode, PERCEPNET_NN_DIRECT_RG=2)["dense"] == f"{mode}_rows{64 if B >= 32768 else 32}"


def test_narrow_layer_overrides(plan):
    assert plan(1024, "mfma", PERCEPNET_N16_ROWS=0)["narrow"] == "small"        # n48 needs the batch family
    assert plan(8192, "mfma", PERCEPNET_N16_ROWS=0)["narrow"] == families.N48
    assert plan(65536, "mfma", PERCEPNET_N16_ROWS=65536)["narrow"] == "n16"
    assert plan(1024, "x3", PERCEPNET_N16_ROWS=0)["narrow"] == "fc_gb:x3+fc_rb:fp32"
    assert plan(65536, "f16", PERCEPNET_N16_ROWS=65536)["narrow"] == "fc_gb:x3+fc_rb:n16"
    assert plan(24576, "mfma", PERCEPNET_N48=0)["narrow"] == "batch"
    assert plan(24576, "mfma", PERCEPNET_N48=1)["narrow"] == families.N48
    assert plan(24576, "x3", PERCEPNET_N48=1)["narrow"] == "fc_gb:x3+fc_rb:fp32"   # fp32 MFMA only
    # n48 does not need the small GRU family off: only the small dense one
    assert plan(2048, "mfma", PERCEPNET_N16_ROWS=0, PERCEPNET_SMALL_ROWS=0, PERCEPNET_SMALL_GRU_ROWS=4096)["narrow"] == families.N48


def test_chain_overrides(plan):
    for k in (1, 2, 3, 4):
        p = plan(65836, "mfma", PN_NN_CHAINS=k)
        assert p["nn_chains"] == str(k) and p["tile"] == "256", p
    assert plan(8492, "mfma", PN_NN_CHAINS=3)["nn_chains"] == "2"    # at least 4096 rows per chain
    assert plan(8192, "mfma", PN_NN_CHAINS=4)["nn_chains"] == "2"
    assert plan(65836, "mfma", PN_NN_CHAINS=0)["nn_chains"] == "1"
    assert plan(65836, "mfma", PN_NN_CHAINS=9)["nn_chains"] == "4"
    assert plan(65836, "mfma", PN_NN_CHAINS=-3)["nn_chains"] == "1"
    assert plan(1024, "mfma", PN_NN_CHAINS=4)["nn_chains"] == "1"                  # the small families run one chain
    assert plan(65536, "mfma", PN_NN_CHAINS=4, PERCEPNET_SMALL_GRU_ROWS=65536)["nn_chains"] == "1"
    for mode in ("x3", "f16", "strict"):
        p = plan(65836, mode, PN_NN_CHAINS=4)
        assert (p["nn_chains"], p["share"]) == ("1", "0"), (mode, p)


def test_front_end_overrides(plan):
    for mode in MODES:
        assert plan(1024, mode)["frontend"] == "split"
        assert plan(1024, mode, PERCEPNET_FE="split")["frontend"] == "split"
        assert plan(1024, mode, PERCEPNET_FE="mono")["frontend"] == "g4"
        assert plan(1024, mode, PERCEPNET_FE="g4")["frontend"] == "g4"
        assert plan(1024, mode, PERCEPNET_FE="g2")["frontend"] == "g2"
        assert plan(1024, mode, PERCEPNET_FE_G2=0)["frontend"] == "g4"
        assert plan(1024, mode, PERCEPNET_FE_G2=1)["frontend"] == "g2"
        assert plan(1024, mode, PERCEPNET_FE="split", PERCEPNET_FE_G2=1)["frontend"] == "split"   # PERCEPNET_FE first
        assert plan(1024, mode, PERCEPNET_FE="other", PERCEPNET_FE_G2=1)["frontend"] == "g2"      # an unknown value is not set


def test_strict(plan):
    for B in (1024, 20481, 65536):
        p = plan(B, "strict", PERCEPNET_SMALL_ROWS=65536, PERCEPNET_N16_ROWS=65536, PN_NN_CHAINS=2)
        assert p["nn"] == "strict" and fam(p) == ("batch", "batch", "batch", "batch") and p["nn_chains"] == "1", p


def test_refusals(lib):
    lib.pn_debug_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    lib.pn_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(256)
    assert lib.pn_debug_plan(0, api.NN_MFMA, buf, len(buf)) == -1
    assert lib.pn_debug_plan(1024, 7, buf, len(buf)) == -1 and b"nn_mode" in lib.pn_last_error()
    assert lib.pn_debug_plan(1024, api.NN_MFMA, buf, 40) == -1 and b"too small" in lib.pn_last_error()
    assert lib.pn_debug_plan(1024, api.NN_MFMA, None, 0) == -1
