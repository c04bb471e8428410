"""Which event clears which per-stream state of the rate converter (-m gpu): the matrix of percepnet_amd/csrc/pn_rate_layout.h, ten
buffers by eight events, pinned on the device cell by cell.  Host side pn_rate.cpp; the existing tests of each stage cover some of
its cells, this one covers all of them.

Rig: a mixed converter on a context of B = 6 streams at 8000 / 16000 / 24000 / 32000 / 48000 / 8000 Hz (the engine at the bypass),
PLC on, AGC with targets, limiter with ceilings, detection and removal on for everybody, everybody in one conference with a hold.
Sixteen whole frames of seeded noise, four of them with a DTMF tone on top and one lost, leave every buffer non-zero for every
stream; the removal state, which is back at zero once the key has left, is then driven by the stage alone over hand-made rows.

The ten buffers are read through the existing API alone: the two tails from the tails records (export_streams_dev), the three PLC
buffers, the AGC and limiter words and the level from the call-state records (export_call_state), the detector's and the removal's
words from dtmf_state() / dtmf_clamp_state().  An event is applied to a fresh rig; behind it the rows the matrix names are all
zero and every other row of every buffer holds the bits it held before.

The 48000 Hz stream (4) has no filter and therefore no tails: the library refuses to move them, so its two tails cells are read
only where an event has given the stream another rate.  For the same reason the tails import, which refuses a list with a 48000
slot (asserted below), runs over streams (1, 3); every other event that takes a list runs over (1, 4)."""
import numpy as np
import pytest

from percepnet_amd import api
from tests import call_state_model as cs
from tests import test_gpu_plc as tq

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
to_dev, to_host, dev_full, nof = tq.to_dev, tq.to_host, tq.dev_full, tq.nof
model = tq.model
default_families = tq.default_families

B = 6
RATES = (8000, 16000, 24000, 32000, 48000, 8000)
T, TONE, LOST_AT = 16, (1, 5), 10
LISTED, IMPORTED, EVERYBODY = (1, 4), (1, 3), tuple(range(B))
BUFFERS = ("tail_up", "tail_down", "level", "plc_hist", "plc_q", "plc_meta", "agc", "lim", "dtmf", "clamp")
# event -> (the buffers it clears, the streams whose rows it clears): the matrix, written out
MATRIX = {
    "reset": (("tail_up", "tail_down", "level", "plc_hist", "plc_q", "plc_meta", "agc", "lim", "dtmf", "clamp"), EVERYBODY),
    "reset_streams": (("tail_up", "tail_down", "level", "plc_hist", "plc_q", "plc_meta", "agc", "lim", "dtmf", "clamp"), LISTED),
    "rate_change": (("tail_up", "tail_down", "level", "plc_hist", "plc_q", "plc_meta", "agc", "lim", "dtmf", "clamp"), LISTED),
    "conf_change": (("level",), LISTED),
    "hold_change": (("level",), EVERYBODY),
    "import_dev": (("plc_hist", "plc_q", "plc_meta", "agc", "lim", "dtmf", "clamp"), IMPORTED),
    "import_host": (("plc_hist", "plc_q", "plc_meta", "agc", "lim", "dtmf", "clamp"), IMPORTED),
    "plc_again": (("plc_hist", "plc_q", "plc_meta"), EVERYBODY),
    "agc_again": (("agc",), EVERYBODY),
    "dtmf_switch_on": (("dtmf",), LISTED),
    "clamp_switch_on": (("clamp",), LISTED),
}

_x = []


def inputs():
    """[T, B, 480] float32: stream s has its own rate's samples in the first n_s of its row — noise, and in the frames TONE the two sines of a
    key on top (removal mutes the key where it leaves the engine, six frames on: the frames behind it carry the noise to the mix)"""
    if not _x:
        rng = np.random.default_rng(20)
        x = np.zeros((T, B, 480), F32)
        for s, rate in enumerate(RATES):
            n = nof(rate)
            t = np.arange(T * n) / float(rate)
            v = rng.standard_normal(T * n) * 0.02
            tone = 0.1 * np.sin(2 * np.pi * 770.0 * t) + 0.1 * np.sin(2 * np.pi * 1336.0 * t)        # the key 5
            v[TONE[0] * n:TONE[1] * n] += tone[TONE[0] * n:TONE[1] * n]
            x[:, s, :n] = v.reshape(T, n).astype(F32)
        x.setflags(write=False)
        _x.append(x)
    return _x[0]


class Rig:
    def __init__(self, model):
        import torch
        every = list(EVERYBODY)
        self.B = B
        self.ctx = api.Context(model, B)
        self.ctx.set_atten_limit(every, 0.0)
        self.rc = rc = api.MixedRateConverter(self.ctx, list(RATES))
        self.w = rc.frame
        rc.set_stream_confs(every, [0] * B)
        rc.set_mix_hold(0.9)
        rc.set_plc(True)
        rc.set_agc(True)
        rc.set_stream_agc_targets(every, [0.05 + 0.01 * s for s in range(B)])
        rc.set_stream_limiter(every, [0.05] * B)
        rc.set_stream_dtmf(every, True)
        rc.set_stream_dtmf_clamp(every, True)
        x = inputs()
        for t in range(T):
            if t == LOST_AT:
                rc.set_lost(every)
            tq.frame(self, "f32", x[t])
        if not rc.dtmf_clamp_state().any(axis=1).all():
            # the frames left a removal state at zero: the stage alone over hand-made detector rows "a digit, frame after frame"
            busy = np.tile(np.array([1 | 2 | ord("7") << 8, 9, 1, ord("7")], U32), (B, 1))
            for _ in range(8):
                rc.set_dtmf_report_rows(busy)
                rc.dtmf_clamp_f32_dev(dev_full((B, 480), torch.float32, 0.25).data_ptr())
        self.ctx.synchronize()

    def tails_records(self, ids):
        """-> {stream: uint32 words of its tails record} through the device form, which takes streams of different rates"""
        import torch
        stride = self.rc.record_stride()
        d_rec = dev_full((len(ids), stride), torch.uint8, 0xEE)
        self.rc.export_streams_dev(list(ids), d_rec.data_ptr())
        rec = to_host(self.ctx, d_rec).copy()
        return {s: rec[i].view(U32) for i, s in enumerate(ids)}, d_rec

    def snap(self):
        """-> {buffer: [B rows, None where the stream has none]}"""
        out = {k: [None] * B for k in BUFFERS}
        rates = self.rc.stream_rates().tolist()
        tails, _ = self.tails_records([s for s in EVERYBODY if rates[s] != 48000])
        for s, w in tails.items():
            assert int(w[3]) == rates[s] and int(w[2]) == api.rate_state_bytes(rates[s])
            body = w[4:int(w[2]) // 4]
            out["tail_up"][s], out["tail_down"][s] = body[:32].copy(), body[32:].copy()
        assert self.rc.call_state_sections() == cs.ALL
        call = self.rc.export_call_state(list(EVERYBODY)).view(U32).reshape(B, -1)[:, cs.HEADER_WORDS:]
        for name, lo, hi in (("plc_hist", cs.W_HIST, cs.W_Q), ("plc_q", cs.W_Q, cs.W_META), ("plc_meta", cs.W_META, cs.W_AGC), ("agc", cs.W_AGC, cs.W_LIM),
                             ("lim", cs.W_LIM, cs.W_MIX), ("level", cs.W_MIX, cs.BODY_WORDS)):
            out[name] = [call[s, lo:hi].copy() for s in EVERYBODY]
        out["dtmf"] = list(self.rc.dtmf_state().copy())
        out["clamp"] = list(self.rc.dtmf_clamp_state().copy())
        return out

    def close(self):
        self.rc.close()
        self.ctx.close()


def apply(rig, event):
    import torch
    rc = rig.rc
    if event == "reset":
        rc.reset()
    elif event == "reset_streams":
        rc.reset_streams(list(LISTED))
    elif event == "rate_change":
        rc.set_stream_rates(list(LISTED), [24000, 8000])
    elif event == "conf_change":
        rc.set_stream_confs(list(LISTED), [1, 1])
    elif event == "hold_change":
        rc.set_mix_hold(0.5)
    elif event == "import_dev":
        _, d_rec = rig.tails_records(IMPORTED)
        d_st = dev_full((len(IMPORTED),), torch.int32, 99)
        with pytest.raises(api.PercepNetError, match="48000"):           # a 48000 slot has no tails: the whole call is refused
            rc.import_streams_dev(list(LISTED), d_rec.data_ptr(), d_st.data_ptr())
        rc.import_streams_dev(list(IMPORTED), d_rec.data_ptr(), d_st.data_ptr())
        assert to_host(rig.ctx, d_st).tolist() == [api.SS_OK] * len(IMPORTED)
    elif event == "import_host":
        with pytest.raises(api.PercepNetError, match="48000"):
            rc.import_streams([LISTED[1]], np.zeros(16, np.uint8))
        for s in IMPORTED:                                                   # (the host form moves one rate per call)
            rc.import_streams([s], rc.export_streams([s]))
    elif event == "plc_again":
        rc.set_plc(False)
        rc.set_plc(True)
    elif event == "agc_again":
        rc.set_agc(False)
        rc.set_agc(True)
    elif event == "dtmf_switch_on":
        rc.set_stream_dtmf(list(LISTED), False)                              # (off keeps the state)
        rc.set_stream_dtmf(list(LISTED), True)
    elif event == "clamp_switch_on":
        rc.set_stream_dtmf_clamp(list(LISTED), False)
        rc.set_stream_dtmf_clamp(list(LISTED), True)
    else:
        raise AssertionError(event)


@pytest.mark.parametrize("event", list(MATRIX))
def test_an_event_clears_the_rows_the_matrix_names_and_no_other(model, event):
    rig = Rig(model)
    before = rig.snap()
    no_tails = [(name, s) for name in ("tail_up", "tail_down") for s in EVERYBODY if RATES[s] == 48000]
    assert all(before[name][s] is None for name, s in no_tails)
    empty = [(name, s) for name in BUFFERS for s in EVERYBODY if (name, s) not in no_tails and not before[name][s].any()]
    assert not empty, f"precondition: every buffer holds state for every stream, but not {empty}"
    apply(rig, event)
    after = rig.snap()
    buffers, streams = MATRIX[event]
    for name in BUFFERS:
        for s in EVERYBODY:
            got, was = after[name][s], before[name][s]
            if got is None:
                assert was is None
            elif name in buffers and s in streams:
                assert not got.any(), f"{event}: {name} of stream {s} is cleared"
            else:
                assert was is not None and got.tobytes() == was.tobytes(), f"{event}: {name} of stream {s} keeps its bits"
    rig.close()
