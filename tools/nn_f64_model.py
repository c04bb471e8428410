"""float64 evaluation of ONE compute_rnn step (rnn.cpp:42-81, nnet.cpp) from a given RNN state: the yardstick for "how far
is each network mode from exact arithmetic".  Same formulas as the reference — table-interpolated tanh/sigmoid
(vec.h:53-75, evaluated in double on the float table), reset-after GRU (nnet.cpp:122-180), conv as dense over the FIFO
(nnet.cpp:182-200) — with every product and sum in double, so what remains between a mode's output and this one is that
mode's rounding (operand representation + accumulation order), not the model.

  layer_outputs(layers, table, state, feat, forced=None, f16_layers=()) -> {layer: [B, n]}, the ten outputs in pn_kNet order
      (LAYER_NAMES).  forced: {layer: [B, n]} outputs to use as the INPUTS of the downstream layers instead of the model's
      own (teacher forcing: a GPU test passes what it read back, so every layer is judged alone, on the operands its kernel
      saw; the outputs returned are always the model's own).  f16_layers: names of the layers whose GEMM operands — weights,
      input panels, the GRU's recurrent operand — are rounded to fp16 (round to nearest even, subnormals kept) before the
      float64 products, the fp16-operand mode's definition (pn_nn_x3.hip); bias, activation, tmp*r and the blend
      z*h + (1-z)*hc with the unrounded h stay as they are.  F16_LAYERS is the set that mode applies it to (pn_layer_kernel).
  step(layers, table, state, feat) -> gr [B, 68]: the last two of them
  layer_input(name, state, feat, out) -> [B, K]: the input panels of one layer, in K order
  next_state(state, out) -> the state after the step (FIFOs shift, GRUs take the new values)
      layers: percepnet_amd.weights.unpack_blob(...) ; table: the 201 float tanh table ; state: Context.get_rnn_state() ;
      feat [B, 70]
"""
import numpy as np

LAYER_NAMES = ("fc", "conv1", "conv2", "gru1", "gru2", "gru3", "gru_gb", "gru_rb", "fc_gb", "fc_rb")
F16_LAYERS = frozenset(LAYER_NAMES) - {"fc", "fc_rb"}         # pn_layer_kernel: fc and fc_rb stay fp32 in the shadow-operand modes
# input panels in K order (pn_kNet): ("state", entry) = the stored FIFO, oldest first; ("out", layer) = this step's output
INPUTS = {"fc": (("feat", None),), "conv1": (("state", "conv1"), ("out", "fc")), "conv2": (("state", "conv2"), ("out", "conv1")),
          "gru1": (("out", "conv2"),), "gru2": (("out", "gru1"),), "gru3": (("out", "gru2"),), "gru_gb": (("out", "gru3"),),
          "gru_rb": (("out", "gru3"), ("out", "conv2")),
          "fc_gb": (("out", "conv2"), ("out", "gru1"), ("out", "gru2"), ("out", "gru3"), ("out", "gru_gb")), "fc_rb": (("out", "gru_rb"),)}


def _tansig(x, tab):
    x = np.asarray(x, np.float64)
    sign = np.where(x < 0, -1.0, 1.0)
    ax = np.abs(x)
    i = np.clip(np.floor(.5 + 25 * ax), 0, 200).astype(np.int64)
    ax = ax - .04 * i
    y = tab[i]
    dy = 1 - y * y
    y = y + ax * dy * (1 - y * ax)
    return sign * y


def _act(x, act, tab):
    if act == 1:
        return .5 + .5 * _tansig(.5 * x, tab)
    if act == 2:
        return _tansig(x, tab)
    if act == 3:
        return np.maximum(x, 0)
    return x


def _operand(a, f16):
    a = np.asarray(a)
    return a.astype(np.float16).astype(np.float64) if f16 else a.astype(np.float64)


_weights = {}       # (id of a weight array, f16) -> (the array, its float64 operand form): converted once per array (change a copy, not the array)


def _weight(w, f16):
    hit = _weights.get((id(w), f16))
    if hit is None or hit[0] is not w:
        if len(_weights) >= 64:
            _weights.clear()
        hit = _weights[(id(w), f16)] = (w, _operand(w, f16))
    return hit[1]


def _dense(lay, x, nn_, act, tab, f16=False):
    W = _weight(lay["input_weights"], f16).reshape(-1, nn_)
    return _act(lay["bias"].astype(np.float64) + _operand(x, f16) @ W, act, tab)


def _gru(lay, x, h, nn_, act, tab, f16=False):
    W = _weight(lay["input_weights"], f16).reshape(-1, 3 * nn_)
    U = _weight(lay["recurrent_weights"], f16).reshape(nn_, 3 * nn_)
    b = lay["bias"].astype(np.float64)
    x, hk = _operand(x, f16), _operand(h, f16)               # hk: h as the recurrent GEMM's operand; the blend takes h itself
    z = _act(b[0:nn_] + b[3 * nn_:4 * nn_] + x @ W[:, 0:nn_] + hk @ U[:, 0:nn_], 1, tab)
    r = _act(b[nn_:2 * nn_] + b[4 * nn_:5 * nn_] + x @ W[:, nn_:2 * nn_] + hk @ U[:, nn_:2 * nn_], 1, tab)
    tmp = b[5 * nn_:6 * nn_] + hk @ U[:, 2 * nn_:3 * nn_]
    hc = _act(b[2 * nn_:3 * nn_] + tmp * r + x @ W[:, 2 * nn_:3 * nn_], act, tab)
    return z * h + (1 - z) * hc


def layer_input(name, state, feat, out):
    """The [B, K] input of layer `name`: its panels in K order, from the state, the features and the outputs `out` of this step."""
    panels = [np.asarray(feat if src == "feat" else state[ref] if src == "state" else out[ref], np.float64) for src, ref in INPUTS[name]]
    return panels[0] if len(panels) == 1 else np.concatenate(panels, axis=1)


def layer_outputs(layers, table, state, feat, forced=None, f16_layers=(), acts=None):
    from percepnet_amd import weights
    forced = forced or {}
    tab = np.asarray(table, np.float64)[:201]
    out, src = {}, {}                                          # the model's own outputs / what the downstream layers read
    for name, kind, nin, nn_, ks, act in weights.LAYERS:
        if acts and name in acts:
            act = acts[name]
        x = layer_input(name, state, feat, src)
        if kind == weights.KIND_GRU:
            out[name] = _gru(layers[name], x, np.asarray(state[name], np.float64), nn_, act, tab, name in f16_layers)
        else:
            out[name] = _dense(layers[name], x, nn_, act, tab, name in f16_layers)
        src[name] = forced[name] if name in forced else out[name]
    return out


def next_state(state, out):
    st = {k: np.asarray(out[k], np.float64) for k in ("gru1", "gru2", "gru3", "gru_gb", "gru_rb")}
    st["conv1"] = np.concatenate([np.asarray(state["conv1"], np.float64)[:, 128:], out["fc"]], axis=1)
    st["conv2"] = np.concatenate([np.asarray(state["conv2"], np.float64)[:, 512:], out["conv1"]], axis=1)
    return st


def step(layers, table, state, feat, acts=None):
    out = layer_outputs(layers, table, state, feat, acts=acts)
    return np.concatenate([out["fc_gb"], out["fc_rb"]], axis=1)
