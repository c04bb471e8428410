"""Is a per-layer comparison against float64 sharp enough?  Proven on the CPU, with the float64 model alone (no GPU).

tests/test_gpu_layers.py holds every layer's output to a tolerance of at most LAYER_TOL_CAP.  Here a fixed list of weight
mutations — each a stand-in for a packing, fragment or epilogue slip: one element dropped, two columns or two K rows swapped, a
bias forgotten; the last K row, the last column, every gate, the recurrent bias half and every layer kind among them — must
move ITS OWN layer's output by at least 10 x LAYER_TOL_CAP at an operating point that loads every term (GRU states up to
+-0.95: free-running default-init states stay below 0.2 and never load the blend).  At g|r the same errors arrive attenuated
50-200x by the layers and the sigmoid behind them (printed beside each own-layer delta): free-running from the zero state,
three of the ten stay below the 2e-5 the rest of the suite holds g|r to, and all but one below the 1e-3 of the fp16-operand mode.

The interpolated tanh table (vec.h:53-75) jumps where the index floor(.5 + 25|x|) steps: two roundings of one pre-activation
that fall on either side of a cell boundary differ by up to J whatever their quality.  activation_jump measures it; the GPU test
uses it as the floor of its max-error tolerances.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from percepnet_amd import api, weights

LAYER_TOL_CAP = 5e-5      # the largest max tolerance any layer may get in any mode = 1/10 of the smallest mutation's own-layer delta
B, SEED = 96, 2024
N = {name: nn_ for name, kind, nin, nn_, ks, act in weights.LAYERS}


def _swap(a, i, j, axis):
    a = np.moveaxis(a, axis, 0)
    a[[i, j]] = a[[j, i]]


def _mutate(lay, layer, array, what, *idx):
    """A copy of `lay` with one array of one layer changed.  Weight arrays are [K, columns] (GRU: columns = gate * N + neuron,
    gates z, r, candidate; bias = [input | recurrent] x [z, r, candidate] x N): zero (k, column) / swap_cols (i, j) /
    swap_rows (i, j); bias: zero (index)."""
    out = {k: dict(v) for k, v in lay.items()}
    a = out[layer][array].copy()
    cols = N[layer] * (3 if "recurrent_weights" in lay[layer] else 1)
    v = a if array == "bias" else a.reshape(-1, cols)
    if what == "zero":
        assert v[idx] != 0
        v[idx] = 0
    else:
        _swap(v, idx[0], idx[1], 1 if what == "swap_cols" else 0)
    out[layer][array] = a
    return out


# (name, layer, array, operation, indices)
MUTATIONS = [
    ("gru1: swap update-gate columns 510 and 511", "gru1", "input_weights", "swap_cols", 510, 511),
    ("gru3 recurrent: zero (k 511, candidate 511)", "gru3", "recurrent_weights", "zero", 511, 2 * 512 + 511),
    ("gru1 input: zero (k 17, update 33)", "gru1", "input_weights", "zero", 17, 33),
    ("gru2: drop the recurrent candidate bias of neuron 511", "gru2", "bias", "zero", 5 * 512 + 511),
    ("gru_gb recurrent: swap K rows 31 and 32", "gru_gb", "recurrent_weights", "swap_rows", 31, 32),
    ("gru2 recurrent: swap K rows 510 and 511", "gru2", "recurrent_weights", "swap_rows", 510, 511),
    ("conv2: zero (k 1535, n 511)", "conv2", "input_weights", "zero", 1535, 511),
    ("fc_gb: zero (k 2559, n 33)", "fc_gb", "input_weights", "zero", 2559, 33),
    ("gru_rb input: zero (k 1023, candidate 127)", "gru_rb", "input_weights", "zero", 1023, 2 * 128 + 127),
    ("conv1: swap K rows 638 and 639", "conv1", "input_weights", "swap_rows", 638, 639),
]


def operating_point(rows, seed):
    """Random features, non-negative conv FIFOs (they hold ReLU outputs) and GRU states uniform in +-0.95, one set per row."""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((rows, 70)).astype(np.float32)
    st = {}
    for k, n in api.Context.RNN_STATE_SHAPES:
        st[k] = (np.abs(rng.standard_normal((rows, n))) if k.startswith("conv") else rng.uniform(-0.95, 0.95, (rows, n))).astype(np.float32)
    return feat, st


def activation_jump(tab, act):
    """Largest jump of the table activation across a cell boundary |x| = (i - 1/2) / 25, i = 1..200 (0 for ReLU / linear)."""
    import nn_f64_model as M
    if act not in (weights.ACT_SIGMOID, weights.ACT_TANH):
        return 0.0
    tab = np.asarray(tab, np.float64)[:201]
    edge = (np.arange(1, 201) - .5) / 25
    lo, hi = edge - 1e-9, edge + 1e-9                            # (the function moves by <= 2e-9 over that distance without a jump)
    assert np.array_equal(np.floor(.5 + 25 * lo) + 1, np.floor(.5 + 25 * hi))     # every boundary is straddled
    j = float(np.abs(M._tansig(hi, tab) - M._tansig(lo, tab)).max())
    return .5 * j if act == weights.ACT_SIGMOID else j


def test_table_activation_jump(oracle):
    tab = oracle.tansig_table()
    j = activation_jump(tab, weights.ACT_TANH)
    assert 5.0e-6 <= j <= 6.0e-6, j                              # 5.5e-6 from the reference's table
    assert activation_jump(tab, weights.ACT_SIGMOID) == .5 * j
    assert activation_jump(tab, weights.ACT_RELU) == 0.0
    assert 2 * j <= LAYER_TOL_CAP                                # the floor of the GPU test's tolerances fits under the cap


@pytest.fixture(scope="module")
def base(blob, oracle):
    import nn_f64_model as M
    lay = weights.unpack_blob(blob)
    tab = oracle.tansig_table()
    feat, st = operating_point(B, SEED)
    return lay, tab, feat, st, M.layer_outputs(lay, tab, st, feat)


def test_every_mutation_moves_its_own_layer_by_ten_times_the_cap(base):
    import nn_f64_model as M
    lay, tab, feat, st, ref = base
    assert len(MUTATIONS) >= 10 and {m[1] for m in MUTATIONS} >= {"conv1", "conv2", "gru1", "gru2", "gru3", "gru_gb", "gru_rb", "fc_gb"}
    own, at_gr = {}, {}
    for name, layer, array, what, *idx in MUTATIONS:
        got = M.layer_outputs(_mutate(lay, layer, array, what, *idx), tab, st, feat)
        own[name] = float(np.abs(got[layer] - ref[layer]).max())
        at_gr[name] = float(max(np.abs(got[k] - ref[k]).max() for k in ("fc_gb", "fc_rb")))
        for k in M.LAYER_NAMES[:M.LAYER_NAMES.index(layer)]:
            assert np.array_equal(got[k], ref[k]), (name, k)     # nothing upstream moves
        print(f"{name:55s} own layer {own[name]:.2e}   g|r {at_gr[name]:.2e}")
    smallest = min(own.values())
    assert smallest >= 10 * LAYER_TOL_CAP, own


def test_teacher_forcing_and_fp16_operand_emulation(base):
    """forced= replaces a layer's output as the INPUT of what follows (the returned output stays the model's own); f16_layers=
    rounds the named layers' GEMM operands only, to fp16 with subnormals kept."""
    import nn_f64_model as M
    lay, tab, feat, st, ref = base
    rng = np.random.default_rng(1)
    c2 = rng.uniform(-1, 1, ref["conv2"].shape)
    got = M.layer_outputs(lay, tab, st, feat, forced={"conv2": c2})
    for k in ("fc", "conv1", "conv2"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["gru1"], M._gru(lay["gru1"], c2, st["gru1"], 512, weights.ACT_TANH, np.asarray(tab, np.float64)[:201]))
    assert np.abs(got["gru1"] - ref["gru1"]).max() > 1e-2 and np.array_equal(got["fc_rb"] != ref["fc_rb"], np.ones_like(ref["fc_rb"], bool))
    # forcing every layer with the model's own outputs changes nothing
    same = M.layer_outputs(lay, tab, st, feat, forced=ref)
    assert all(np.array_equal(same[k], ref[k]) for k in M.LAYER_NAMES)
    # fp16 operands: only the named layers move, by about 2^-11 relative per operand; an operand exactly representable stays
    f16 = M.layer_outputs(lay, tab, st, feat, forced=ref, f16_layers={"gru2"})
    assert all(np.array_equal(f16[k], ref[k]) for k in M.LAYER_NAMES if k != "gru2")
    d = np.abs(f16["gru2"] - ref["gru2"]).max()
    assert 1e-6 < d < 2e-3, d
    assert M.F16_LAYERS == set(M.LAYER_NAMES) - {"fc", "fc_rb"}
    tiny = np.array([2.0 ** -20, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11])       # a subnormal kept; ties to even, both ways
    assert np.array_equal(M._operand(tiny, True), [2.0 ** -20, 1.0, 1 + 2.0 ** -9])
