"""The kernel-family map the tests pin (imported as `from tests import families`).

A context picks its kernel families once, at creation, from its batch size and network mode (percepnet_amd/csrc/pn_plan.h);
the environment variables below override the choice.  REGIMES is the map with none of them set."""
import ctypes

# every override pn_plan_for reads: a test that relies on the default families clears them all
FAMILY_ENV = ("PERCEPNET_SMALL_ROWS", "PERCEPNET_SMALL_GRU_ROWS", "PERCEPNET_NN_DIRECT", "PERCEPNET_NN_DIRECT_RG",
              "PERCEPNET_X3_RG", "PERCEPNET_N16_ROWS", "PERCEPNET_N48", "PN_NN_CHAINS", "PERCEPNET_FE",
              "PERCEPNET_FE_G2")
N48 = "fc_gb:n48+fc_rb:batch"


def _r(dense, gru, gru_rb, narrow, chains, share=None):
    return dict(dense=dense, gru=gru, gru_rb=gru_rb, narrow=narrow, chains=chains, share=share)


# The regime map with default settings: (mode, B) -> the families ctx_create picks.  Moving a threshold moves a row of
# this table; move the sizes with it so that each boundary keeps a size on both sides.
REGIMES = {
    ("mfma", 1536): _r("small", "small", "small", "n16", 1),
    ("mfma", 1537): _r("small", "batch", "small", "n16", 1),
    ("mfma", 4096): _r("small", "batch", "small", "n16", 1),
    ("mfma", 4097): _r("batch", "batch", "batch", "n16", 1),
    ("mfma", 16384): _r("batch", "batch", "batch", "n16", 1),
    ("mfma", 16385): _r("batch", "batch", "batch", "n16", 2, 8320),
    ("mfma", 20480): _r("batch", "batch", "batch", "n16", 2, 10240),
    ("mfma", 20481): _r("batch", "batch", "batch", N48, 2, 10368),
    ("mfma", 24575): _r("batch", "batch", "batch", N48, 2, 12288),
    ("mfma", 24576): _r("batch", "direct_rows32", "direct_rows32", N48, 2, 12288),
    ("mfma", 32767): _r("batch", "direct_rows32", "direct_rows32", N48, 2, 16384),
    ("mfma", 32768): _r("batch", "direct_rows64", "direct_rows64", N48, 1),          # an exact fit: one chain
    ("mfma", 65536): _r("batch", "direct_rows64", "direct_rows64", N48, 2, 32768),
    ("mfma", 65836): _r("batch", "direct_rows64", "direct_rows64", N48, 2, 33024),
}
for _m in ("x3", "f16"):
    for _B, _k, _rb in ((20480, "rows32", "n16"), (20481, "rows32", "fp32"), (32767, "rows32", "fp32"),
                        (32768, "rows64", "fp32"), (32897, "rows64", "fp32")):
        _f = f"{_m}_{_k}"
        REGIMES[(_m, _B)] = _r(_f, _f, _f, f"fc_gb:x3+fc_rb:{_rb}", 1)


def rows_per_block(reg):
    """Rows per block of the family's chained kernels (pn_plan_tile): 128, or 256 for the direct family at 64 rows per wave."""
    return 256 if reg["gru"] == "direct_rows64" else 128


def chain_share(B, chains, tile):
    """pn_plan_share: equal shares rounded up to whole `tile` rows; the last chain takes what is left."""
    return ((B + chains - 1) // chains + tile - 1) // tile * tile


def debug_plan(lib, n_streams, nn_mode):
    """pn_debug_plan through the library handle `lib` -> {"nn": ..., "dense": ..., ..., "frontend": ..., "nn_chains": "N",
    "tile": "T", "share": "S"}: the families a context created now would run, from the host alone."""
    lib.pn_debug_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    lib.pn_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(256)
    n = lib.pn_debug_plan(n_streams, nn_mode, buf, len(buf))
    assert n == len(buf.value), (n_streams, nn_mode, lib.pn_last_error())
    return dict(kv.split("=", 1) for kv in buf.value.decode().split())
