"""Every network layer's output against float64, in every kernel family (-m gpu; test_layer_cases_* needs none).

The rest of the suite judges the gain network by its last 68 numbers, g|r, which sit behind four to six layers of small weights
and a sigmoid: a localized error in a hidden layer arrives there attenuated 50-200x, below the g|r tolerances
(tests/test_layers_host.py shows it on the CPU).  Here the ten outputs the API exposes — fc and conv1 as the newest FIFO entries,
c2out (pn_ctx_debug_copy 3), the five GRU states, g and r — are each compared with the float64 evaluation of THAT layer alone
(tools/nn_f64_model.py, teacher-forced from the context's own read-backs: every layer is judged on exactly the operands its
kernel saw), for 7 steps (every residue of the 5-, 3- and 2-slot rings) with a fresh large-magnitude state imposed at steps 0
and 4 and free-running in between, every row carrying its own features and state, with the default weights and the scale3 set
(saturated gates, |conv1| up to 4).  The fp16-operand mode is compared with the same model with its GEMM operands rounded to
fp16 (its own definition, pn_nn_x3.hip), so what is left is fp32 accumulation of exact products.  The FIFOs must come back as the
old ones shifted plus the new output, bit for bit.

Tolerances come from the reference's own rounding, per layer: a STRICT context (= the CPU reference's arithmetic, bit for bit)
on the same rows, features and states gives E_ref[layer] = {max, rms} of |STRICT - float64|, and a mode passes a layer when
    max <= 2 x max(E_ref.max, J)      and      rms <= RMS_RATIO x E_ref.rms
J = the table activation's jump at a cell boundary (test_layers_host.activation_jump): two roundings of one pre-activation that
fall on either side of a boundary differ by that much whatever their quality.  RMS_RATIO is 1.5 for the fp32 MFMA kernels and 2.5
for split precision (the ratios test_gpu_x3.py uses at g|r), and the fp32 MFMA ratio for fp16 operands against their own
reference.  The yardstick is itself held to a derived bound where one exists: every STRICT dense / conv output within
L gamma_(K+1) (|b| + sum |x_k| |w_k|) + J of float64 (L = 1 for ReLU and tanh, 1/4 for the sigmoid).  Whatever the ratios, every
effective max tolerance stays <= LAYER_TOL_CAP, a tenth of the smallest own-layer delta of the mutation list of
tests/test_layers_host.py.  Every measured figure is recorded as
parity_layers_<mode>_<case>.json by the _record helper of test_gpu_longrun.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from percepnet_amd import api, weights
from tests import families
from test_layers_host import LAYER_TOL_CAP, activation_jump

T = 7                      # steps: every residue of the conv rings (5, 3 slots) and of the GRU pairs
IMPOSE = (0, 4)            # steps that start from a fresh random state
MODES = {"strict": api.NN_STRICT, "mfma": api.NN_MFMA, "x3": api.NN_MFMA_X3, "f16": api.NN_MFMA_F16}
NN_NAME = {"strict": "strict", "mfma": "mfma_f32", "x3": "mfma_x3", "f16": "mfma_f16"}
RMS_RATIO = {"mfma": 1.5, "x3": 2.5, "f16": 1.5}
RMS_RATIO_LAYER = {}       # (mode, layer) -> a ratio measured not to fit the mode's, with the reason beside it
SAMPLED = 256              # the chained case checks its boundary rows plus this many random ones
GEOM = {name: (kind, nin * ks, nn_, act) for name, kind, nin, nn_, ks, act in weights.LAYERS}


def _x3(m, rows):
    return dict(dense=f"{m}_{rows}", gru=f"{m}_{rows}", gru_rb=f"{m}_{rows}")


_BATCH = {"PERCEPNET_SMALL_ROWS": "0"}
_DIRECT = {**_BATCH, "PERCEPNET_NN_DIRECT": "1"}        # (the plan keeps the direct family off the small-batch regime: PERCEPNET_SMALL_ROWS=0)
# (id, mode, B, overrides, describe() fields): the smallest sizes at which each family's tiling can go wrong
CASES = [
    ("strict-129", "strict", 129, {}, {}),
    ("small-300", "mfma", 300, {}, dict(dense="small", gru="small", gru_rb="small", narrow="n16")),
    ("small_dense_batch_gru-129", "mfma", 129, {"PERCEPNET_SMALL_GRU_ROWS": "0"}, dict(dense="small", gru="batch", gru_rb="small", narrow="n16")),
    ("batch-300", "mfma", 300, {**_BATCH, "PERCEPNET_N16_ROWS": "0", "PERCEPNET_N48": "0"}, dict(dense="batch", gru="batch", gru_rb="batch", narrow="batch")),
    ("batch_n48-641", "mfma", 641, {**_BATCH, "PERCEPNET_N16_ROWS": "0"}, dict(dense="batch", gru="batch", gru_rb="batch", narrow=families.N48)),
    ("direct32-300", "mfma", 300, {**_DIRECT, "PERCEPNET_NN_DIRECT_RG": "1"}, dict(dense="batch", gru="direct_rows32", gru_rb="direct_rows32", narrow="n16")),
    ("direct64-129", "mfma", 129, {**_DIRECT, "PERCEPNET_NN_DIRECT_RG": "2"}, dict(dense="batch", gru="direct_rows64", gru_rb="direct_rows64", narrow="n16")),
    ("direct64-700", "mfma", 700, {**_DIRECT, "PERCEPNET_NN_DIRECT_RG": "2"}, dict(dense="batch", gru="direct_rows64", gru_rb="direct_rows64", narrow="n16")),
    ("direct64_chains2-8492", "mfma", 8492, {**_DIRECT, "PERCEPNET_NN_DIRECT_RG": "2", "PN_NN_CHAINS": "2"},
     dict(dense="batch", gru="direct_rows64", gru_rb="direct_rows64", narrow="n16", nn_chains="2")),
]
for _m in ("x3", "f16"):
    CASES += [
        (f"{_m}_rows32-300", _m, 300, {"PERCEPNET_X3_RG": "1"}, dict(_x3(_m, "rows32"), narrow="fc_gb:x3+fc_rb:n16")),
        (f"{_m}_rows64-129", _m, 129, {"PERCEPNET_X3_RG": "2"}, dict(_x3(_m, "rows64"), narrow="fc_gb:x3+fc_rb:n16")),
        (f"{_m}_rows64-700", _m, 700, {"PERCEPNET_X3_RG": "2"}, dict(_x3(_m, "rows64"), narrow="fc_gb:x3+fc_rb:n16")),
        (f"{_m}_paired-300", _m, 300, {"PERCEPNET_X3_RG": "3"}, dict(_x3(_m, "rows64_paired"), dense=f"{_m}_rows64", narrow="fc_gb:x3+fc_rb:n16")),
        (f"{_m}_rows32_fc_rb_fp32-300", _m, 300, {"PERCEPNET_X3_RG": "1", "PERCEPNET_N16_ROWS": "0"}, dict(_x3(_m, "rows32"), narrow="fc_gb:x3+fc_rb:fp32")),
        # the same with fc and fc_rb on the fp32 batch kernels instead of the small-batch ones (describe() does not tell the two apart)
        (f"{_m}_rows32_fc_batch-300", _m, 300, {**_BATCH, "PERCEPNET_X3_RG": "1", "PERCEPNET_N16_ROWS": "0"}, dict(_x3(_m, "rows32"), narrow="fc_gb:x3+fc_rb:fp32")),
    ]
WEIGHTS = ("default", "scale3")


def _set_env(monkeypatch, env):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in families.FAMILY_ENV, k
        monkeypatch.setenv(k, v)


def _families(d, want):
    got = {k: (d[k].split(":")[0] if k == "nn_chains" else d[k]) for k in want}
    return got


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_layer_cases_land_where_intended(case, monkeypatch):
    """The plan computed on the host (pn_debug_plan) puts every case on the families it is meant to exercise."""
    name, mode, B, env, want = case
    _set_env(monkeypatch, env)
    plan = families.debug_plan(api.load_library(), B, MODES[mode])
    assert plan["nn"] == NN_NAME[mode] and _families(plan, want) == want, (name, plan)
    if "nn_chains" in want:
        assert int(plan["share"]) == families.chain_share(B, 2, 256) and B - int(plan["share"]) >= 4096, plan
    assert len({c[0] for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _layers(name, blob):
    import test_gpu_stress_weights as stress
    return weights.unpack_blob(blob) if name == "default" else stress.SETS[name]()


@pytest.fixture(scope="module")
def nets(blob, oracle):
    """{weights name: (layers, model)} and the tanh table, once per module."""
    out = {}
    for name in WEIGHTS:
        lay = _layers(name, blob)
        out[name] = (lay, api.Model(blob if name == "default" else weights.pack_blob(lay)))
    yield out, oracle.tansig_table()
    for lay, m in out.values():
        m.close()


def _inputs(B, t, seed):
    """Features of step t for every row and, on the imposing steps, a fresh state: non-negative conv FIFOs (they hold ReLU
    outputs), GRU states uniform in +-0.95."""
    rng = np.random.default_rng([seed, t])
    feat = rng.standard_normal((B, 70)).astype(np.float32)
    st = None
    if t in IMPOSE:
        st = {k: (np.abs(rng.standard_normal((B, n))) if k.startswith("conv") else rng.uniform(-0.95, 0.95, (B, n))).astype(np.float32)
              for k, n in api.Context.RNN_STATE_SHAPES}
    return feat, st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(ctx, B, rows, seed, where):
    """T steps; -> per step (state before, features, the ten outputs), each restricted to `rows`.  Checks on every row that the
    state a step starts from is the one imposed / the one the last step left, and that the FIFOs shift bit for bit."""
    steps, after = [], None
    padded = ((B + 255) // 256 * 256 + 256) * 512
    for t in range(T):
        feat, st = _inputs(B, t, seed)
        if st is not None:
            ctx.set_rnn_state(st)
        before = ctx.get_rnn_state()
        for k, v in (st if st is not None else after).items():
            assert np.array_equal(_bits(before[k]), _bits(v)), f"{where}: state {k} read back differs before step {t}"
        gr = ctx.compute_rnn(feat)
        after = ctx.get_rnn_state()
        c2 = ctx.debug_copy(3, padded)
        assert c2.size % 512 == 0 and c2.size // 512 >= B, c2.size
        c2 = c2.reshape(-1, 512)[:B]
        for k, n in (("conv1", 128), ("conv2", 512)):
            bad = np.argwhere(_bits(after[k][:, :-n]) != _bits(before[k][:, n:]))
            assert not bad.size, f"{where}: {k} FIFO is not the old one shifted at step {t}, row {bad[0][0]}, word {bad[0][1]}"
        out = {"fc": after["conv1"][:, -128:], "conv1": after["conv2"][:, -512:], "conv2": c2, "fc_gb": gr[:, :34], "fc_rb": gr[:, 34:]}
        out.update({k: after[k] for k in ("gru1", "gru2", "gru3", "gru_gb", "gru_rb")})
        for k, v in out.items():
            assert np.isfinite(v).all(), f"{where}: {k} not finite at step {t}"
        steps.append(({k: v[rows].copy() for k, v in before.items()}, feat[rows].copy(), {k: v[rows].copy() for k, v in out.items()}))
    return steps


def _errors(M, lay, tab, steps, f16_layers=()):
    """-> {layer: |GPU - float64| [T, rows, n]}, each layer teacher-forced from the GPU's own read-backs."""
    err = {k: [] for k in M.LAYER_NAMES}
    for before, feat, out in steps:
        ref = M.layer_outputs(lay, tab, before, feat, forced=out, f16_layers=f16_layers)
        for k in M.LAYER_NAMES:
            err[k].append(np.abs(out[k].astype(np.float64) - ref[k]))
    return {k: np.stack(v) for k, v in err.items()}


def _stats(e):
    return {"max": float(e.max()), "rms": float(np.sqrt(np.mean(np.square(e))))}


def _rows_of(B, env):
    if "PN_NN_CHAINS" not in env:
        return np.arange(B)
    from test_gpu_regimes import boundary_rows
    fixed = boundary_rows(B, families.chain_share(B, int(env["PN_NN_CHAINS"]), 256))
    rest = np.random.default_rng(B).permutation(np.setdiff1d(np.arange(B), fixed))[:SAMPLED]
    return np.sort(np.concatenate([fixed, rest]))


def _seed(wname, B):
    return 1000 * WEIGHTS.index(wname) + B


_yard = {}


def _yardstick(M, nets, wname, B, rows, monkeypatch):
    """E_ref of (weights, B): a STRICT context on the same rows, features and states against float64, and the derived bound on
    its dense / conv layers.  -> ({layer: {max, rms}}, {layer: largest |err| / bound})."""
    key = (wname, B)
    if key not in _yard:
        (lay, model), tab = nets[0][wname], nets[1]
        _set_env(monkeypatch, {})
        ctx = api.Context(model, B, nn_mode=api.NN_STRICT)
        try:
            assert ctx.describe()["nn"] == "strict", ctx.describe()
            steps = _run(ctx, B, rows, _seed(wname, B), f"strict yardstick B={B} {wname}")
        finally:
            ctx.close()
        err = _errors(M, lay, tab, steps)
        u, used = 2.0 ** -24, {}
        for name, (kind, K, nn_, act) in GEOM.items():
            if kind == weights.KIND_GRU:
                continue
            g = (K + 1) * u / (1 - (K + 1) * u)
            L, J = (.25 if act == weights.ACT_SIGMOID else 1.0), activation_jump(tab, act)
            W = np.abs(lay[name]["input_weights"].astype(np.float64)).reshape(K, nn_)
            b = np.abs(lay[name]["bias"].astype(np.float64))
            worst = 0.0
            for t, (before, feat, out) in enumerate(steps):
                bound = L * g * (b + np.abs(M.layer_input(name, before, feat, out)) @ W) + J
                over = np.argwhere(err[name][t] > bound)
                assert not over.size, (f"STRICT {name} ({wname}, B={B}) is further from float64 than sequential fp32 accumulation allows: step {t}, "
                                       f"row {rows[over[0][0]]}, column {over[0][1]}: {err[name][t][tuple(over[0])]:.3e} > {bound[tuple(over[0])]:.3e}")
                worst = max(worst, float((err[name][t] / np.maximum(bound, 1e-300)).max()))
            used[name] = worst
        _yard[key] = ({k: _stats(e) for k, e in err.items()}, used)
    return _yard[key]


@pytest.mark.gpu
@pytest.mark.parametrize("wname", WEIGHTS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_layer_against_float64(case, wname, nets, monkeypatch):
    import nn_f64_model as M
    from test_gpu_longrun import _record
    name, mode, B, env, want = case
    (lay, model), tab = nets[0][wname], nets[1]
    rows = _rows_of(B, env)
    where = f"{name} {wname}"
    e_ref, bound_used = _yardstick(M, nets, wname, B, rows, monkeypatch)
    J = {k: activation_jump(tab, GEOM[k][3]) for k in M.LAYER_NAMES}
    rec = {"mode": mode, "case": name, "weights": wname, "streams": B, "rows_checked": int(rows.size), "steps": T,
           "layer_tol_cap": LAYER_TOL_CAP, "strict_dense_error_over_derived_bound": bound_used, "layers": {}}
    if mode == "strict":                                   # the yardstick itself: its run and its bound are the check
        for k in M.LAYER_NAMES:
            rec["layers"][k] = {"strict_vs_float64": e_ref[k], "activation_jump": J[k]}
        _record(f"layers_{mode}_{name}_{wname}", rec)
        assert max(bound_used.values()) <= 1.0
        return
    _set_env(monkeypatch, env)
    ctx = api.Context(model, B, nn_mode=MODES[mode])
    try:
        d = ctx.describe()
        assert d["nn"] == NN_NAME[mode] and _families(d, want) == want, (where, d)
        steps = _run(ctx, B, rows, _seed(wname, B), where)
    finally:
        ctx.close()
    err = _errors(M, lay, tab, steps, M.F16_LAYERS if mode == "f16" else ())
    failed = []
    for k in M.LAYER_NAMES:
        got = _stats(err[k])
        ratio = RMS_RATIO_LAYER.get((mode, k), RMS_RATIO[mode])
        tol_max, tol_rms = 2 * max(e_ref[k]["max"], J[k]), ratio * e_ref[k]["rms"]
        t, r, c = (int(v) for v in np.unravel_index(np.argmax(err[k]), err[k].shape))
        at = f"step {t}, row {rows[r]} (offset {rows[r] % 128} in its 128-row tile), column {c} (offset {c % 32} in its 32-column tile)"
        rec["layers"][k] = {"strict_vs_float64": e_ref[k], "activation_jump": J[k], "max": got["max"], "rms": got["rms"],
                            "max_over_strict_max": got["max"] / max(e_ref[k]["max"], 1e-300), "rms_over_strict_rms": got["rms"] / max(e_ref[k]["rms"], 1e-300),
                            "rms_ratio_allowed": ratio, "tolerance_max": tol_max, "tolerance_rms": tol_rms, "worst_at": at}
        print(f"{where:40s} {k:7s} max {got['max']:.3e} (tol {tol_max:.3e})  rms {got['rms']:.3e} (tol {tol_rms:.3e}, strict {e_ref[k]['rms']:.3e})  {at}")
        if tol_max > LAYER_TOL_CAP:
            failed.append(f"{k}: the max tolerance {tol_max:.3e} exceeds LAYER_TOL_CAP {LAYER_TOL_CAP:.1e}: it would swallow the mutation list")
        if got["max"] > tol_max:
            failed.append(f"{k}: max |GPU - float64| {got['max']:.3e} > {tol_max:.3e} at {at}")
        if got["rms"] > tol_rms:
            failed.append(f"{k}: rms |GPU - float64| {got['rms']:.3e} > {ratio} x {e_ref[k]['rms']:.3e} (STRICT's own); worst at {at}")
    _record(f"layers_{mode}_{name}_{wname}", rec)
    assert not failed, f"{where}:\n  " + "\n  ".join(failed)
