"""Moving live streams between contexts: per-stream state export and import (-m gpu).

A record (include/percepnet_hip.h, "per-stream state records") holds the whole state of one stream in age order, free of
the ring phases of its context; an import scatters it at the target's phase and re-derives the target's operand shadows
for the imported rows only.  Every comparison is bit for bit: PCM, g|r, features and silence flags.  Contexts are run to
frame counts that differ modulo 12, 6, 5, 3 and 2, so every ring of the target is at another phase than the source's."""
import ctypes

import numpy as np
import pytest

from percepnet_amd import api, synth, weights
from tests import families

pytestmark = pytest.mark.gpu
MODES = {"strict": api.NN_STRICT, "mfma": api.NN_MFMA, "x3": api.NN_MFMA_X3, "f16": api.NN_MFMA_F16}


@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


def fr(pcm, t):
    return np.ascontiguousarray(pcm[:, t * 480:(t + 1) * 480])


def step(ctx, frame):
    """One frame on the host path -> (out, gr, feat, sil)."""
    out, gr = ctx.process_i16(frame)
    feat, sil = ctx.read_features()
    return out, gr, feat, sil


def assert_rows_equal(a, b, rows_a, rows_b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = x[rows_a], y[rows_b]
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (what, ("pcm", "gr", "feat", "silence")[k])


def without_mode(rec):
    """A record with the header's source-mode field (bytes 12..15) blanked."""
    r = np.array(rec, copy=True)
    r[..., 12:16] = 0
    return r


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
def test_a_moved_stream_continues_exactly(model, oracle, mode):
    """A (300 streams) runs 23 frames, B (300) 30; A's rows 127, 128, 299 move to B's rows 5, 200, 256; both run 30 more
    frames with the moved streams fed the same frames.  B's imported rows = A's source rows; B's other rows = a twin of B
    that imported nothing; in STRICT mode each moved stream's whole output (A's 23 frames, then B's) = the CPU oracle."""
    B, TA, TB, K = 300, 23, 30, 30
    src, dst = [127, 128, 299], [5, 200, 256]
    m = MODES[mode]
    pcm_a = synth.synth_batch(B, TA + K)
    pcm_b = synth.synth_batch(B, TB + K, first_stream=400)
    A, Bc, twin = (api.Context(model, B, nn_mode=m) for _ in range(3))
    early = [step(A, fr(pcm_a, t)) for t in range(TA)]
    for t in range(TB):
        o1, o2 = step(Bc, fr(pcm_b, t)), step(twin, fr(pcm_b, t))
        assert_rows_equal(o1, o2, slice(None), slice(None), ("warm-up", t))
    rec = A.export_streams(src)
    assert rec.shape == (3, api.STREAM_STATE_BYTES) and rec.dtype == np.uint8
    Bc.import_streams(dst, rec)
    others = np.setdiff1d(np.arange(B), dst)
    late = []
    for k in range(K):
        fa = fr(pcm_a, TA + k)
        fb = fr(pcm_b, TB + k)
        fb[dst] = fa[src]
        oa, ob, ot = step(A, fa), step(Bc, fb), step(twin, fb)
        assert_rows_equal(ob, oa, dst, src, ("moved", k))
        assert_rows_equal(ob, ot, others, others, ("untouched", k))
        late.append(ob)
    for c in (A, Bc, twin):
        c.close()
    if m == api.NN_STRICT:
        for s, d in zip(src, dst):
            ro, rg = oracle.run_pcm(pcm_a[s, :(TA + K) * 480])
            out = np.concatenate([o[0][s] for o in early[1:]] + [o[0][d] for o in late])
            gr = np.stack([o[1][s] for o in early] + [o[1][d] for o in late])
            assert np.array_equal(out, ro) and np.array_equal(gr.view(np.uint32), rg.view(np.uint32)), (s, d)


# ---------------------------------------------------------------------------------------------------------------- 2
P = 256
GRU_FAMILY = {1024: "small", 8192: "batch", 24876: "direct_rows32", 65536: "direct_rows64"}
# rows at 128-row tile, 256-row block and chain boundaries (tests/test_gpu_regimes.py: chain shares 12544 at 24 876 and
# 32 768 at 65 536 streams)
EDGE_ROWS = {1024: [0, 127, 128, 1023], 8192: [1, 255, 256, 8191], 24876: [127, 12543, 12544, 24875],
             65536: [255, 32767, 32768, 65535]}


class Rows:
    """Distinct inputs on every row: row r carries pool stream (r + off) % P rotated inside each frame by
    (37 * (r // P) + off) % 480 (37 is prime to 480: no two rows of one pool stream share a rotation below 480 * P rows)."""

    def __init__(self, pool, B, off):
        r = np.arange(B)
        self.pool, self.idx, self.rot = pool, (r + off) % P, (37 * (r // P) + off) % 480
        self.ar = np.arange(480)

    def frame(self, t):
        x = self.pool[self.idx, t * 480:(t + 1) * 480]
        return np.ascontiguousarray(np.take_along_axis(x, (self.ar[None, :] + self.rot[:, None]) % 480, axis=1))


@pytest.mark.parametrize("b1,b2", [(1024, 24876), (24876, 1024), (8192, 65536)], ids=["1024-24876", "24876-1024", "8192-65536"])
def test_moves_across_fp32_kernel_families_are_bit_exact(model, default_families, b1, b2):
    """The batch size picks the fp32 kernel family (small / batch / direct-operand GRUs with two row-range chains), and the
    families are bit-identical: a stream moved between them continues bit for bit, here onto rows at tile and chain edges."""
    T1, T2, K = 4, 11, 13                          # 7 apart: another phase of every ring
    pool = synth.synth_batch(P, T2 + K, first_stream=2000)
    c1, c2 = api.Context(model, b1, nn_mode=api.NN_MFMA), api.Context(model, b2, nn_mode=api.NN_MFMA)
    for c, b in ((c1, b1), (c2, b2)):
        assert c.describe()["gru"] == GRU_FAMILY[b], (b, c.describe())
    r1, r2 = Rows(pool, b1, 3), Rows(pool, b2, 101)
    src = EDGE_ROWS[b1][::-1]
    dst = EDGE_ROWS[b2]
    for t in range(T1):
        c1.process_i16(r1.frame(t), want_gr=False)
    for t in range(T2):
        c2.process_i16(r2.frame(t), want_gr=False)
    c2.import_streams(dst, c1.export_streams(src))
    for k in range(K):
        f1, f2 = r1.frame(T1 + k), r2.frame(T2 + k)
        f2[dst] = f1[src]
        assert_rows_equal(step(c2, f2), step(c1, f1), dst, src, (b1, b2, k))
    c1.close(); c2.close()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
def test_round_trip_through_every_other_mode_is_byte_exact(model, mode):
    """Export -> import into a context of each other mode (other phase) -> export again, before any frame: the records are
    byte-equal apart from the header's source-mode field.  What an fp16-operand context exports, an fp32 or STRICT one
    can import, and the shadows are not part of the record."""
    B = 64
    pcm = synth.synth_batch(B, 9, first_stream=50)
    a = api.Context(model, B, nn_mode=MODES[mode])
    for t in range(9):
        a.process_i16(fr(pcm, t), want_gr=False)
    rec = a.export_streams([0, 17, 63])
    assert (rec[:, 12:16].view(np.int32).ravel() == MODES[mode]).all()
    for other, m in MODES.items():
        if other == mode:
            continue
        b = api.Context(model, 40, nn_mode=m)
        for t in range(5):
            b.process_i16(fr(pcm[:40], t), want_gr=False)
        b.import_streams([3, 39, 20], rec)
        back = b.export_streams([3, 39, 20])
        assert (back[:, 12:16].view(np.int32).ravel() == m).all()
        assert np.array_equal(without_mode(back), without_mode(rec)), other
        b.close()
    a.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_a_stream_that_skipped_ticks_moves_exactly(model):
    """A stream that skipped ticks through the active set sits one ring slot behind the global phase per skipped tick
    (pn_active.hip shifts its rings); its record is still in age order and continues bit for bit elsewhere."""
    import torch
    from test_gpu_longrun import shared_stream
    B, T, K = 64, 20, 14
    skips = {10: {3, 4, 11}, 63: {0, 19}}
    pcm = synth.synth_batch(B, T + K, first_stream=70)
    dev = torch.device("cuda:0")
    ts = shared_stream(dev)
    with torch.cuda.stream(ts):
        a = api.Context(model, B, nn_mode=api.NN_MFMA, stream=ts.cuda_stream)
        d_out = torch.zeros((B, 480), dtype=torch.int16, device=dev)
        for t in range(T):
            act = [s for s in range(B) if not (s in skips and t in skips[s])]
            d_in = torch.from_numpy(fr(pcm, t)).to(dev)
            a.process_i16_active_dev(d_in.data_ptr(), d_out.data_ptr(), None, act)
        ts.synchronize()
    b = api.Context(model, 48, nn_mode=api.NN_MFMA)
    for t in range(13):
        b.process_i16(fr(pcm[:48], t), want_gr=False)
    src, dst = [10, 63, 2], [47, 0, 30]
    b.import_streams(dst, a.export_streams(src))
    for k in range(K):
        fa = fr(pcm, T + k)
        fb = fr(pcm[:48], 13 + k)
        fb[dst] = fa[src]
        assert_rows_equal(step(b, fb), step(a, fa), dst, src, k)
    a.close(); b.close()


@pytest.mark.parametrize("mode", ["mfma", "x3"])
def test_a_context_whose_network_ran_alone_exports_and_imports_exactly(model, mode):
    """After pn_ctx_compute_rnn_host the network rings (tn) run ahead of the DSP rings (t), on both sides of the move."""
    B, K = 32, 14
    m = MODES[mode]
    pcm = synth.synth_batch(B, 27 + K, first_stream=90)
    feat = np.random.default_rng(5).standard_normal((B, 70)).astype(np.float32)
    a, b = api.Context(model, B, nn_mode=m), api.Context(model, B, nn_mode=m)
    for t in range(10):
        a.process_i16(fr(pcm, t), want_gr=False)
    for _ in range(3):
        a.compute_rnn(feat)                        # tn = t + 3
    for t in range(10, 15):
        a.process_i16(fr(pcm, t), want_gr=False)
    for t in range(7):
        b.process_i16(fr(pcm, 20 + t), want_gr=False)
    b.compute_rnn(feat)                            # tn = t + 1
    src, dst = [0, 31, 5], [9, 8, 31]
    b.import_streams(dst, a.export_streams(src))
    for k in range(K):
        fa, fb = fr(pcm, 15 + k), fr(pcm, 27 + k)
        fb[dst] = fa[src]
        assert_rows_equal(step(b, fb), step(a, fa), dst, src, k)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def _pinned_frames(L, pcm, T, B):
    n = B * 480
    bufs = [(L.pn_host_alloc(n * 2), L.pn_host_alloc(n * 2)) for _ in range(T)]
    for t in range(T):
        f = fr(pcm, t)
        ctypes.memmove(bufs[t][0], f.ctypes.data, n * 2)
    return bufs


def _pinned_out(buf, B):
    return np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_int16)), shape=(B, 480)).copy()


def test_ordering_on_the_pipelined_host_path(model):
    """A device-form export queued between two pn_submit_host_i16 calls captures exactly the state between those frames;
    a host-form import during a pipelined run takes effect at the next frame."""
    import torch
    B, T, T0 = 32, 12, 6
    ids = [1, 30, 7]
    pcm = synth.synth_batch(B, T, first_stream=120)
    other = synth.synth_batch(B, 9, first_stream=300)
    donor = api.Context(model, B, nn_mode=api.NN_MFMA)
    for t in range(9):
        donor.process_i16(fr(other, t), want_gr=False)
    incoming = donor.export_streams([4, 5, 6])
    donor.close()
    # synchronous twin: export, then import, between frames T0 - 1 and T0
    twin = api.Context(model, B, nn_mode=api.NN_MFMA)
    want = []
    for t in range(T):
        if t == T0:
            want_rec = twin.export_streams(ids)
            twin.import_streams(ids, incoming)
        want.append(twin.process_i16(fr(pcm, t), want_gr=False)[0])
    twin.close()
    ctx = api.Context(model, B, nn_mode=api.NN_MFMA)
    L = ctx.L
    bufs = _pinned_frames(L, pcm, T, B)
    d_rec = torch.zeros((len(ids), api.STREAM_STATE_BYTES), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for t in range(T):
        if t == T0:
            ctx.export_streams_dev(ids, d_rec.data_ptr())      # queued behind frame T0 - 1, in front of frame T0
            ctx.import_streams(ids, incoming)                  # host form: drains the pipeline, lands before frame T0
        ctx.submit_host_i16(bufs[t][0], bufs[t][1])
    ctx.host_wait()
    ctx.synchronize()
    assert np.array_equal(d_rec.cpu().numpy(), want_rec)
    for t in range(T):
        assert np.array_equal(_pinned_out(bufs[t][1], B), want[t]), t
    for a, b in bufs:
        L.pn_host_free(a); L.pn_host_free(b)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_refusals(model, blob):
    """Out-of-range ids, duplicate import ids, bad magic / version / size and another model's records are refused.  The
    host form refuses all or nothing (the context then continues bit-equal to a twin); the device form names the refused
    records in d_status and imports the others."""
    import torch
    B = 24
    pcm = synth.synth_batch(B, 16, first_stream=140)
    ctx, twin, src = (api.Context(model, B, nn_mode=api.NN_MFMA_X3) for _ in range(3))
    for t in range(5):
        for c in (ctx, twin):
            c.process_i16(fr(pcm, t), want_gr=False)
    for t in range(8):
        src.process_i16(fr(pcm, 8 + t), want_gr=False)
    good = src.export_streams([0, 1, 2, 3])
    other_model = api.Model(weights.default_blob(4321))
    foreign_ctx = api.Context(other_model, 4, nn_mode=api.NN_MFMA_X3)
    foreign = foreign_ctx.export_streams([0, 1, 2, 3])
    foreign_ctx.close(); other_model.close()
    bad_magic, bad_version, bad_size = good.copy(), good.copy(), good.copy()
    bad_magic[2, 0] ^= 1
    bad_version[1, 4] = 2
    bad_size[3, 8:12] = np.frombuffer(np.uint32(api.STREAM_STATE_BYTES + 16).tobytes(), np.uint8)
    with pytest.raises(api.PercepNetError):
        ctx.export_streams([0, B])
    for ids, rec in (([0, 1, 2, B], good), ([0, 1, 2, -1], good), ([0, 1, 1, 3], good), ([0, 1, 2, 3], bad_magic),
                     ([0, 1, 2, 3], bad_version), ([0, 1, 2, 3], bad_size), ([0, 1, 2, 3], foreign),
                     ([0, 1, 2], good)):
        with pytest.raises(api.PercepNetError):
            ctx.import_streams(ids, rec)
    for t in range(5, 8):                          # all or nothing: nothing was imported
        assert_rows_equal(step(ctx, fr(pcm, t)), step(twin, fr(pcm, t)), slice(None), slice(None), t)
    # device form: records 1 (bad version), 2 (bad magic) and 3 (another model) refused, 0 imported
    mixed = np.stack([good[0], bad_version[1], bad_magic[2], foreign[3]])
    dev = torch.device("cuda:0")
    d_rec = torch.from_numpy(mixed).to(dev)
    d_status = torch.full((4,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(api.PercepNetError):        # duplicate ids: refused before anything is launched
        ctx.import_streams_dev([4, 4, 5, 6], d_rec.data_ptr(), d_status.data_ptr())
    ctx.synchronize()
    assert (d_status.cpu().numpy() == 99).all()
    ids = [10, 11, 12, 13]
    ctx.import_streams_dev(ids, d_rec.data_ptr(), d_status.data_ptr())
    ctx.synchronize()
    assert d_status.cpu().numpy().tolist() == [api.SS_OK, api.SS_BAD_VERSION, api.SS_BAD_MAGIC, api.SS_BAD_MODEL]
    assert np.array_equal(ctx.export_streams([10]), good[:1])
    assert np.array_equal(ctx.export_streams(ids[1:]), twin.export_streams(ids[1:]))
    rest = np.setdiff1d(np.arange(B), [10])
    for t in range(8, 16):
        assert_rows_equal(step(ctx, fr(pcm, t)), step(twin, fr(pcm, t)), rest, rest, t)
    for c in (ctx, twin, src):
        c.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_move_between_devices(model):
    L = api.load_library()
    if L.pn_device_count() < 2:
        pytest.skip("one device")
    B, K = 16, 12
    pcm = synth.synth_batch(B, 30, first_stream=160)
    a, b = api.Context(model, B, device=0, nn_mode=api.NN_MFMA), api.Context(model, B, device=1, nn_mode=api.NN_MFMA)
    for t in range(9):
        a.process_i16(fr(pcm, t), want_gr=False)
    for t in range(4):
        b.process_i16(fr(pcm, 10 + t), want_gr=False)
    src, dst = [0, 15], [15, 3]
    b.import_streams(dst, a.export_streams(src))
    for k in range(K):
        fa, fb = fr(pcm, 9 + k), fr(pcm, 14 + k)
        fb[dst] = fa[src]
        assert_rows_equal(step(b, fb), step(a, fa), dst, src, k)
    a.close(); b.close()
