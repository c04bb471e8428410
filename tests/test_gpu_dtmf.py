"""In-band DTMF detection on the rate converter (-m gpu): include/percepnet_hip.h "DTMF detection"; kernel
percepnet_amd/csrc/pn_rate_dtmf.hip, host side pn_rate.cpp (pn_rate_set_stream_dtmf / pn_rate_dtmf_f32 and the hook in rate_frame), the
rule pn_dtmf_rules.h, bindings api.RateConverter.set_stream_dtmf / dtmf_f32_dev / read_dtmf_report / dtmf_state.

The oracle is the numpy float32 model tests/dtmf_model.py: alone for the kernel, and for whole frames applied to the 48 kHz rows that
pn_rate_up_* (and the PLC model, where a frame is lost) give on a SECOND context and converter that never enables detection, whose
output and g|r the detecting converter's must equal byte for byte.  Every comparison is equality of bits; no tolerance.

Shapes: contexts of 3 and 19 streams, neither a multiple of the kernel's four rows a block; 2049 streams for the kernel alone, the
smallest count at which a block makes a second pass (the grid covers api.DTMF_ROWS_PER_PASS = 2048 rows at once), and no multiple of four."""
import numpy as np
import pytest

from percepnet_amd import api
from tests import dtmf_model as dm
from tests import g711_model
from tests import plc_model as pm
from tests import test_gpu_plc as tq
from tests import test_gpu_rate_pipe as tp
from tests.test_agc_host import hostile_rows, voice

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
BS = (3, 19)
T = 12
KT = 40
D = dm.DEFAULTS
Twin, frame, assert_frame, same, to_dev, to_host = tq.Twin, tq.frame, tq.assert_frame, tq.same, tq.to_dev, tq.to_host
model = tq.model
default_families = tq.default_families


@pytest.fixture(scope="module", autouse=True)
def tables():
    """the model computes with the library's tables wherever numpy's cos or sin rounds an entry the other way (tests/test_dtmf_host.py bounds that)"""
    ct, st, rot = api.dtmf_tables()
    dm.use_tables(ct, st, rot)


class Det:
    """The model over B streams: switches, states, the report rows as the kernel leaves them"""

    def __init__(self, B, on=None, params=None):
        self.B, self.params = B, D.copy() if params is None else np.asarray(params, F32)
        self.on = np.ones(B, bool) if on is None else np.asarray(on, bool).copy()
        self.state, self.report = dm.fresh(B), np.zeros((B, 4), U32)

    def set(self, ids, on):
        for s, v in zip(ids, np.broadcast_to(on, (len(ids),))):
            if v and not self.on[s]:
                self.state[s] = 0
            self.on[s] = bool(v)

    def reset(self, ids=None):
        self.state[slice(None) if ids is None else list(ids)] = 0

    def frame(self, rows, ids=None, concealed=()):
        adv = np.ones(self.B, bool) if ids is None else np.isin(np.arange(self.B), list(ids))
        lost = np.isin(np.arange(self.B), list(concealed))
        st, rep = dm.frame(self.params, self.state, np.where(adv[:, None], rows, F32(0.0)), on=self.on, concealed=lost)
        self.state[adv], self.report[adv] = st[adv], rep[adv]

    def begun(self, s):
        return chr(int(self.report[s, 0] >> 8) & 0xff) if int(self.report[s, 0]) & dm.BEGIN else ""


def on_of(B):
    return [s % 5 != 3 for s in range(B)]


def det_twin(model, B, case="mixed", on=None, plc=False):
    tw = Twin(model, B, case, plc=plc)
    tw.rc.set_dtmf_report(True)
    tw.rc.set_stream_dtmf(list(range(B)), on_of(B) if on is None else on)
    return tw


def assert_same_as_model(tw, m, what):
    rep, st = tw.rc.read_dtmf_report(), tw.rc.dtmf_state()
    assert rep.tobytes() == m.report.tobytes(), f"{what}: report\n{rep.view(U32).reshape(-1, 4)}\n{m.report}"
    assert st.tobytes() == m.state.tobytes(), f"{what}: state, streams {sorted(set(np.argwhere(st != m.state)[:, 0].tolist()))}"


def launches(tw, name="rate_dtmf"):
    return tw.rc.kernel_times((name,))[name][1]


# ---------------------------------------------------------------------------------------------------------------- 1
_kernel_rows = {}


def kernel_rows(B):
    """[KT, B, 480]: per stream a keypad sequence of its own (digits, start offset, level, some in noise), a voice on every fourth,
    with one hostile row per frame from frame 3 on, walking over the streams"""
    if B not in _kernel_rows:
        rng = np.random.default_rng(4733 + B)
        rows = np.empty((KT, B, 480), F32)
        for s in range(B):
            if s % 4 == 2:
                rows[:, s] = voice(0.05 * (1 + s % 3), KT, f0=100.0 + 9.0 * s)
                continue
            digits = "".join(dm.DIGITS[(5 * s + 3 * i) % 16] for i in range(5))
            v = dm.keypad(digits, lead=(37 * s) % 480, amp=(0.3, 0.1, 0.02, 0.008)[s % 4], tail=19200)[:KT]
            if s % 3 == 1:
                v = v + (rng.standard_normal(v.shape) * 0.005).astype(F32)
            rows[:, s] = v
        h = list(hostile_rows().values())
        for t in range(3, KT):
            rows[t, (5 * t) % B] = h[t % len(h)]
        rows.setflags(write=False)
        _kernel_rows[B] = rows
    return _kernel_rows[B]


@pytest.mark.parametrize("B", BS)
def test_the_kernel_alone_against_the_model(model, B):
    tw, m = det_twin(model, B), Det(B, on_of(B))
    x = kernel_rows(B)
    rng = np.random.default_rng(77)
    seen, begun = 0, 0
    for t in range(KT):
        ids = None
        if t % 4 == 2:                                                   # an id list in scrambled order; the others keep state and report rows
            ids = [int(v) for v in rng.permutation(B)[:max(1, B - 1 - t % 3)]]
        if t == 25:                                                      # a parameter change between two frames
            p = D.copy()
            p[[dm.MIN_RMS, dm.PURITY, dm.ON_FRAMES, dm.OFF_FRAMES]] = (0.001, 0.4, 2, 1)
            tw.rc.set_dtmf_params(p)
            m.params = p
            assert same(tw.rc.dtmf_params(), p)
        rows = np.array(x[t])
        d = to_dev(rows)
        tw.rc.dtmf_f32_dev(d.data_ptr(), ids=ids)
        assert to_host(tw.ctx, d).tobytes() == rows.tobytes(), f"frame {t}: the kernel only reads the rows"
        m.frame(rows, ids=ids)
        assert_same_as_model(tw, m, f"frame {t}")
        seen |= int(np.bitwise_or.reduce(m.report[:, 0] & U32(0xff)))
        begun += int(np.count_nonzero(m.report[:, 0] & dm.BEGIN))
    assert seen == dm.ON | dm.HIT | dm.BEGIN | dm.END, "every flag but HELD_LOST, which needs the concealer"
    assert begun >= B and (m.state[~m.on] == 0).all() and (m.report[~m.on] == 0).all()
    assert tw.rc.stream_dtmf().tolist() == [int(v) for v in on_of(B)] and launches(tw) == KT
    tw.close()


def test_a_block_that_makes_a_second_pass(model):
    """2049 streams: block 0 runs rows 0..3 and, in a second pass with its twiddles still in registers, row 2048; no engine frame"""
    B = api.DTMF_ROWS_PER_PASS + 1
    assert B % 4 != 0
    ctx = api.Context(model, B)
    rc = api.MixedRateConverter(ctx, [48000] * B)
    rc.set_dtmf_report(True)
    on = np.arange(B) % 7 != 5
    rc.set_stream_dtmf(list(range(B)), on)
    m = Det(B, on)
    base = dm.keypad("1D", lead=100, tail=960)[:6]
    amp = (0.2 + 0.75 * ((7 * np.arange(B)) % 64) / 64.0).astype(F32)       # tones of 0.02 .. 0.094
    for t in range(6):
        rows = (base[t][None, :] * amp[:, None]).astype(F32)
        rows[(3 * t) % B] = np.nan
        d = to_dev(rows)
        ids = None if t != 4 else [int(v) for v in np.random.default_rng(3).permutation(B)[:B - 2]]
        rc.dtmf_f32_dev(d.data_ptr(), ids=ids)
        m.frame(rows, ids=ids)
        rep, st = rc.read_dtmf_report(), rc.dtmf_state()
        bad = sorted(set(np.argwhere(st != m.state)[:, 0].tolist()) | set(np.argwhere(rep.view(U32).reshape(B, 4) != m.report)[:, 0].tolist()))
        assert not bad, f"frame {t}: streams {bad[:10]}"
    assert np.count_nonzero(m.state[:, 20]) > B // 2 and int(m.state[B - 1, 20]) == 1, "the digit was found, in the second pass too"
    rc.close()
    ctx.close()


def test_refusals_change_nothing(model):
    B = 3
    tw = Twin(model, B, 8000)
    d = to_dev(np.zeros((B, 480), F32))
    assert same(tw.rc.dtmf_params(), D) and tw.rc.stream_dtmf().tolist() == [0] * B
    with pytest.raises(api.PercepNetError, match="pn_rate_set_dtmf_report"):
        tw.rc.read_dtmf_report()
    tw.rc.set_stream_dtmf([2, 0], [1, 0])
    x = dm.keypad("5", lead=10)[:4]
    for t in range(4):
        d_x = to_dev(np.repeat(x[t][None], B, 0))                      # (kept until the context's stream has been waited for)
        tw.rc.dtmf_f32_dev(d_x.data_ptr())
        tw.ctx.synchronize()
    st, n = tw.rc.dtmf_state(), launches(tw)
    assert st[2].any() and not st[:2].any() and n == 4
    for ids, on, word in (([B], [1], "out of range"), ([-1], [1], "out of range"), ([1, 1], [1, 1], "twice")):
        with pytest.raises(api.PercepNetError, match=word):
            tw.rc.set_stream_dtmf(ids, on)
    with pytest.raises(api.PercepNetError, match="twice"):
        tw.rc.dtmf_f32_dev(d.data_ptr(), ids=[2, 2])
    with pytest.raises(api.PercepNetError, match="aligned"):
        tw.rc.dtmf_f32_dev(d.data_ptr() + 4)
    for i, v in ((dm.PURITY, 0.0), (dm.ON_FRAMES, 2.5), (dm.REL, np.nan)):
        p = D.copy()
        p[i] = v
        with pytest.raises(api.PercepNetError, match=f"index {i} "):
            tw.rc.set_dtmf_params(p)
    with pytest.raises(api.PercepNetError, match="rate_up, rate_down, rate_mix, rate_plc, rate_agc, rate_lim, rate_dtmf"):
        tw.rc.kernel_times(("rate_xyz",))
    tw.rc.set_stream_dtmf([], [])
    assert same(tw.rc.dtmf_params(), D) and tw.rc.stream_dtmf().tolist() == [0, 0, 1]
    assert tw.rc.dtmf_state().tobytes() == st.tobytes() and launches(tw) == n
    tw.close()


# ---------------------------------------------------------------------------------------------------------------- 2
_tone_inputs = {}


def tone_inputs(kind, tw, frames, seed=0):
    """[frames, B, w] rows in a sample format at each stream's OWN rate (the first n samples of a mixed converter's row): a keypad
    sequence per stream over a little noise; stream s starts 7 s + 3 samples into the first frame"""
    key = (kind, tuple(tw.rates), tw.w, frames, seed)
    if key not in _tone_inputs:
        rng = np.random.default_rng(100 + seed)
        x = np.zeros((frames, tw.B, tw.w), np.float64)
        for s, rate in enumerate(tw.rates):
            n = tq.nof(rate)
            k = np.arange(frames * n)
            v = rng.standard_normal(k.size) * 0.002
            per = 8 * n                                                  # 40 ms on, 40 ms off
            for i in range(frames // 8 + 1):
                j = (3 * s + 5 * i + seed) % 16
                a = k[(k >= 7 * s + 3 + i * per) & (k < 7 * s + 3 + i * per + 4 * n)]
                v[a] += (0.25, 0.05, 0.02)[s % 3] * (np.sin(2 * np.pi * dm.FREQS[j // 4] * a / rate) + np.sin(2 * np.pi * dm.FREQS[4 + j % 4] * a / rate))
            x[:, s, :n] = v.reshape(frames, n)
        if kind == "f32":
            a = x.astype(F32)
        else:
            a = np.rint(x * 32767.0).astype(np.int16)
            if kind == "g711":
                a = np.stack([g711_model.encode_rows([s % 2 for s in range(tw.B)], a[t]) for t in range(frames)])
        a.setflags(write=False)
        _tone_inputs[key] = a
    return _tone_inputs[key]


@pytest.mark.parametrize("B,case,kind,lists", ((3, 8000, "f32", False), (3, "mixed", "g711", True), (19, "mixed", "i16", True), (19, "mixed", "f32", False),
                                               (19, "mixed", "g711", False), (19, 32000, "i16", True)), ids=str)
def test_whole_frame_against_a_twin_that_never_detects(model, B, case, kind, lists):
    a, b = det_twin(model, B, case), Twin(model, B, case)
    m, plc = Det(B, on_of(B)), pm.Plc(B)
    frames = 16
    x = tone_inputs(kind, a, frames)
    rng = np.random.default_rng(5)
    digits = [""] * B
    for t in range(frames):
        ids = sorted(int(v) for v in rng.permutation(B)[:B - 1]) if lists and t in (5, 9, 10) else None      # the _active entry points
        got = frame(a, kind, x[t], ids)
        want = tq.composed(b, plc, kind, x[t], (), ids)                  # (nothing is lost: the PLC model hands the up-converted rows on)
        assert_frame(a, got, want, ids, f"{case} {kind} frame {t}:")
        m.frame(want[2], ids=ids)
        assert_same_as_model(a, m, f"{case} {kind} frame {t}")
        for s in range(B):
            digits[s] += m.begun(s) if ids is None or s in ids else ""
    assert sum(len(d) >= 1 for d in digits) >= (B * 3) // 5, f"digits were found on most enabled streams: {digits}"
    assert launches(a) == frames and launches(b) == 0
    for name in ("rate_up", "rate_down"):
        assert launches(a, name) == launches(b, name)
    a.close()
    b.close()


def test_pipelined_path_with_a_setting_call_between_two_submits(model):
    B = 19
    sync = det_twin(model, B)
    x = tone_inputs("i16", sync, T, seed=2)
    rng = np.random.default_rng(56)
    ids_at = [None if t % 3 else sorted(int(v) for v in rng.permutation(B)[:B - 2]) for t in range(T)]
    p2 = D.copy()
    p2[[dm.ON_FRAMES, dm.OFF_FRAMES]] = (1, 1)

    def settings(tw, t):
        if t == 5:
            tw.rc.set_stream_dtmf([1, 3, 4], [0, 1, 1])                  # 3 was off: it starts fresh; 4 was on: it keeps its state
        if t == 7:
            tw.rc.set_dtmf_params(p2)
        if t == 9:
            tw.rc.set_stream_dtmf([1], [1])

    plain = Twin(model, B, "mixed")
    want, reports = [], []
    for t in range(T):
        settings(sync, t)
        want.append(frame(sync, "i16", x[t], ids_at[t]))
        reports.append(sync.rc.read_dtmf_report().tobytes())
        assert_frame(sync, want[-1], frame(plain, "i16", x[t], ids_at[t]), ids_at[t], f"frame {t}: detection leaves the audio alone:")
    final = sync.rc.dtmf_state().tobytes()
    assert len(set(reports)) > 3
    sync.close()
    plain.close()
    p = det_twin(model, B)
    rot = tp.Rot(p.ctx, 480, "i16", b=B)

    def submit(t, h_in, h_out, h_gr, h_rep):
        settings(p, t)                                                   # no wait before or after
        p.rc.submit_host_i16(h_in, h_out, h_gr, ids=ids_at[t])

    got = rot.run(np.array(x), submit)
    for t in range(T):
        for s in range(B) if ids_at[t] is None else ids_at[t]:
            n = tq.nof(p.rates[s])
            assert same(got[t][0][s, :n], want[t][0][s, :n]) and same(got[t][1][s], want[t][1][s]), f"frame {t} stream {s}"
    assert p.rc.read_dtmf_report().tobytes() == reports[-1] and p.rc.dtmf_state().tobytes() == final
    assert p.ctx.frames_delivered() == T and launches(p) == T
    p.close()
    rot.free()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_loss_in_the_middle_of_a_digit(model):
    B = 3
    a, b = det_twin(model, B, 16000, on=[1, 1, 1], plc=True), Twin(model, B, 16000)
    m, plc = Det(B), pm.Plc(B)
    frames = 18
    n = a.w
    k = np.arange(frames * n)
    v = np.zeros((B, k.size))
    for s, digit in enumerate("7#2"):                                    # 100 ms of a digit from frame 4 on, in a little noise
        j = dm.DIGITS.index(digit)
        w = (k >= 4 * n + 20 + 11 * s) & (k < 14 * n + 20 + 11 * s)
        v[s, w] = 0.1 * (np.sin(2 * np.pi * dm.FREQS[j // 4] * k[w] / 16000.0) + np.sin(2 * np.pi * dm.FREQS[4 + j % 4] * k[w] / 16000.0))
    v += np.random.default_rng(9).standard_normal(v.shape) * 0.002
    x = np.rint(v.reshape(B, frames, n).transpose(1, 0, 2) * 32767.0).astype(np.int16)
    losses = {10: [1], 11: [1], 9: [0, 2]}                              # behind the digit's BEGIN, in front of its END
    begun = [""] * B
    for t in range(frames):
        lost = losses.get(t, [])
        rows = tq.poison(x[t], lost, "i16")
        before = m.state.copy()
        tq.mark(a.rc, lost)
        got = frame(a, "i16", rows)
        want = tq.composed(b, plc, "i16", rows, lost)
        assert_frame(a, got, want, None, f"frame {t}:")
        m.frame(want[2], concealed=lost)
        assert_same_as_model(a, m, f"frame {t}")
        for s in range(B):
            held = bool(int(m.report[s, 0]) & dm.HELD_LOST)
            assert held == (s in lost), (t, s)
            if held:
                assert (m.state[s] == before[s]).all() and int(m.report[s, 0] >> 8) & 0xff == int(before[s, 18]) & 0xff == ord("7#2"[s])
            begun[s] += m.begun(s)
    assert begun == ["7", "#", "2"], "each digit is reported once, the loss inside it notwithstanding"
    assert [int(c) for c in m.state[:, 20]] == [1, 1, 1]
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("B", BS)
def test_nothing_new_while_nobody_is_enabled(model, B):
    never, plain, off = Twin(model, B, "mixed"), Twin(model, B, "mixed"), Twin(model, B, "mixed")
    off.rc.set_stream_dtmf(list(range(B)), 1)                            # enabled, then everybody off again
    off.rc.set_stream_dtmf(list(range(B)), 0)
    n = 0
    for kind in ("f32", "i16", "g711"):
        x = tone_inputs(kind, never, 4, seed=3)
        for t in range(4):
            want = frame(plain, kind, x[t])
            for tw, what in ((never, "never enabled"), (off, "everybody off again")):
                assert_frame(tw, frame(tw, kind, x[t]), want, None, f"{what}: {kind} frame {t}:")
            n += 1
    for tw in (never, off):
        assert tw.rc.kernel_times(("rate_dtmf",))["rate_dtmf"] == (0.0, 0), "nobody enabled, no launch"
        for name in ("rate_up", "rate_down", "rate_mix", "rate_plc", "rate_agc", "rate_lim"):
            assert launches(tw, name) == launches(plain, name)
    assert launches(never, "rate_up") == n and not never.rc.dtmf_state().any()
    for tw in (never, plain, off):
        tw.close()


def test_enabling_and_the_resets_zero_the_state(model):
    B = 19
    tw, m = det_twin(model, B, "mixed", on=[1] * B), Det(B)
    x = np.stack([dm.keypad("".join(dm.DIGITS[(s + i) % 16] for i in range(4)), lead=20 * s, tail=19200)[:30] for s in range(B)], axis=1)
    t = 0

    def tick(ids=None):
        nonlocal t
        d_x = to_dev(np.array(x[t]))
        tw.rc.dtmf_f32_dev(d_x.data_ptr(), ids=ids)
        m.frame(x[t], ids=ids)
        assert_same_as_model(tw, m, f"tick {t}")                          # (its reads wait for the context's stream: d_x lives until here)
        t += 1

    for _ in range(5):
        tick()
    assert (m.state[:, 20] == 1).all(), "every stream has begun a digit"
    tw.rc.set_stream_dtmf([2, 5, 6], [0, 0, 1])                          # off keeps the state; on for a stream that is on keeps it too
    m.set([2, 5, 6], [0, 0, 1])
    tick()
    assert m.state[2, 20] == 1 and m.state[6, 20] == 1
    tw.rc.set_stream_dtmf([2, 6], [1, 1])                                # on for a stream that was off: a fresh state
    m.set([2, 6], [1, 1])
    assert not tw.rc.dtmf_state()[2].any() and tw.rc.dtmf_state()[6].any()
    tick()
    tw.rc.reset_streams([1, 4])
    m.reset([1, 4])
    tick()
    tick(ids=[0, 1, 2])                                                  # a stream that does not advance keeps its state
    tw.rc.set_stream_rates([3, 7], [16000, 48000])
    m.reset([3, 7])
    tick()
    eight = [s for s in range(B) if tw.rates[s] == 8000][:3]
    tw.rc.import_streams(eight[1:], tw.rc.export_streams([eight[0]] * 2))
    m.reset(eight[1:])
    tick()
    assert m.state[eight[0], 0:17].any()
    tw.rc.reset()
    m.reset()
    assert not tw.rc.dtmf_state().any()
    tick()
    assert tw.rc.stream_dtmf().tolist() == [int(v) for v in m.on], "the switches are settings: they survive"
    tw.close()


def test_parameters_reach_the_kernel(model):
    """on_frames = 1 reports the digit with its first hit, on_frames = 2 one frame and the default of 3 two frames later (run counts
    the hits in a row from 1)"""
    B = 3
    x = dm.keypad("9", lead=100)[:8]
    first = []
    for on_frames in (1, 2, 3):
        tw = det_twin(model, B, 8000, on=[1] * B)
        p = D.copy()
        p[dm.ON_FRAMES] = on_frames
        tw.rc.set_dtmf_params(p)
        m = Det(B, params=p)
        at = None
        for t in range(8):
            rows = np.repeat(x[t][None], B, 0)
            d_x = to_dev(rows)                                          # (alive until assert_same_as_model has waited for the stream)
            tw.rc.dtmf_f32_dev(d_x.data_ptr())
            m.frame(rows)
            assert_same_as_model(tw, m, f"on_frames {on_frames} frame {t}")
            if at is None and int(tw.rc.read_dtmf_report()[1]["word0"]) & dm.BEGIN:
                at = t
        first.append(at)
        tw.close()
    assert first[0] is not None and first == [first[0], first[0] + 1, first[0] + 2]


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_dtmf_prints_each_digit_and_leaves_the_audio_alone(model, blob, tmp_path):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(api.__file__), "lib", "percepnet_run")
    (tmp_path / "m.pnw").write_bytes(blob)
    frames = 20
    for opts, rate in ((["--rate", "8000"], 8000), ([], 48000)):
        n = tq.nof(rate)
        tw = det_twin(model, 3, rate if rate != 48000 else "mixed", on=[1, 1, 1])
        if rate == 48000:
            tw.rc.set_stream_rates([0, 1, 2], [48000] * 3)
            tw.rates, tw.w = [48000] * 3, 480
        x = tone_inputs("i16", tw, frames, seed=4)
        args = []
        for i in range(3):
            np.ascontiguousarray(x[:, i, :n]).tofile(tmp_path / f"in{i}.pcm")
            args += [f"in{i}.pcm", f"out{i}.pcm"]
        run = subprocess.run([exe, "--model", "m.pnw"] + opts + ["--dtmf"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr
        plain = subprocess.run([exe, "--model", "m.pnw"] + opts + [a.replace("out", "plain") for a in args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0, plain.stderr
        want = []
        for t in range(frames):
            frame(tw, "i16", x[t])
            rep = tw.rc.read_dtmf_report()
            want += [f"dtmf: pair {s} frame {t} digit {chr(int(rep[s]['word0']) >> 8 & 0xff)}" for s in range(3) if int(rep[s]["word0"]) & dm.BEGIN]
        tw.close()
        got = [ln for ln in run.stdout.splitlines() if ln.startswith("dtmf:")]
        assert len(want) >= 6 and sorted(got) == sorted(want), (rate, got, want)
        for i in range(3):
            assert (tmp_path / f"out{i}.pcm").read_bytes() == (tmp_path / f"plain{i}.pcm").read_bytes(), f"{rate} Hz pair {i}: the audio is what it is without --dtmf"
