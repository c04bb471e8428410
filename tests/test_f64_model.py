"""tools/nn_f64_model.py (the float64 yardstick of tests/test_gpu_x3.py and tests/test_gpu_layers.py) against the CPU oracle, no
GPU needed: free-running from the zero state on the same features, the float64 evaluation of the reference's formulas and the
oracle's fp32 one must stay within fp32 rounding of each other (a wrong weight layout, gate order or FIFO order would be off by
O(0.1))."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from percepnet_amd import api, synth, weights


def test_float64_model_tracks_the_oracle(blob, oracle):
    import nn_f64_model as M
    B, T = 6, 12
    lay = weights.unpack_blob(blob)
    pcm = synth.synth_batch(B, T)
    ro, rg, rf, rs = oracle.run_batch(pcm)
    tab = oracle.tansig_table()
    st = {k: np.zeros((B, n)) for k, n in api.Context.RNN_STATE_SHAPES}
    worst = 0.0
    for t in range(T):
        # one step of the model, then advance ITS state the way compute_rnn does (FIFOs shift, GRUs take the new values)
        out = M.layer_outputs(lay, tab, st, rf[:, t])
        g = M.step(lay, tab, st, rf[:, t])
        assert np.array_equal(g, np.concatenate([out["fc_gb"], out["fc_rb"]], axis=1))       # step() = the last two layers
        worst = max(worst, float(np.abs(g - rg[:, t]).max()))
        st = M.next_state(st, out)
    assert worst < 2e-5, worst          # fp32 rounding accumulated over 12 free-running steps; a layout error is O(0.1)
