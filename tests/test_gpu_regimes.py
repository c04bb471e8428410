"""Row independence at every default kernel-family boundary, checked on EVERY row with distinct inputs (-m gpu).

The batch size picks the network kernels, once, when the context is created (percepnet_amd/csrc/pn_plan.h: pn_plan_for,
the only reader of the family overrides), and every non-STRICT mode promises that a stream's PCM, g|r, features and
silence flag depend, bit for bit, only on that stream's own input.  The large-batch tests elsewhere fill their batches
with copies of 16 or 64 streams, so a kernel that hands row r the result of row r +- 16 k (a lane or fragment
permutation, a wrong 128-row chunk of a 256-row block, a chain's r0 off by a block) still passes them.  Here no two rows carry the same input: row r carries pool stream r % 256 rotated inside each frame by an
amount that never repeats for rows sharing a pool stream, and 256 slots — the tile, chain and last-block boundaries
among them — carry the pool streams unrotated for the oracle anchor.

  * test_every_row_of_a_regime_*: describe() against the regime map REGIMES (tests/families.py) and against pn_debug_plan
    (the plan computed without a GPU, as tests/test_plan_host.py checks it); 14 frames (every ring and both GRU halves
    wrap); every row bit-identical to a 1024-stream context of the same nn_mode fed the same rows chunk by chunk (the
    family that test_gpu_longrun checks against the oracle for every stream); the unrotated slots against the oracle.
  * test_lifecycle_at_chained_and_direct_sizes: per-stream reset and the active set (pn_state.hip, pn_active.hip) on
    rows at the tile, chain and last-block boundaries of contexts with two chains / direct GRUs / 64 rows per wave.

test_regime_layouts (no GPU) checks the input layout and the chain shares the GPU tests rely on.
"""
import numpy as np
import pytest

from percepnet_amd import api, synth
from tests import families
from tests.families import REGIMES, chain_share, rows_per_block

P = 256                 # distinct pool streams
T_ROWS = 14             # frames of the every-row check: the 12-slot history ring and the 6-slot look-ahead ring wrap
T_LIFE, T_RESET = 30, 13
REF_ROWS = 1024         # the reference context
PCM_TOL_LSB = 1
GR_TOL = 2e-5
MODES = {"mfma": api.NN_MFMA, "x3": api.NN_MFMA_X3, "f16": api.NN_MFMA_F16}
NN_NAME = {"mfma": "mfma_f32", "x3": "mfma_x3", "f16": "mfma_f16"}


def boundary_rows(B, share=None):
    """Rows where a kernel can go wrong: first rows, 32-row wave groups, 128-row tiles, 256-row blocks, the chain boundary
    (share = first row of the second chain), the first row of the last 256-row block and the last rows."""
    rows = [0, 1, 31, 32, 127, 128, 255, 256, (B - 1) // 256 * 256, B - 129, B - 128, B - 2, B - 1]
    if share is not None:
        rows += [share - 1, share, share + 1]
    return np.unique(np.array([r for r in rows if 0 <= r < B], dtype=np.int64))


def row_layout(B, share=None, seed=0):
    """Batch slot -> (pool stream, in-frame rotation).  P slots — every boundary row plus random ones (fixed seed) — carry
    the P pool streams unrotated; every other row r carries pool stream r % P rotated by 1 + ((r // P) * 37 + 11) % 479,
    which never repeats for rows of one pool stream below 479 * P rows: no two rows see the same input."""
    fixed = boundary_rows(B, share)
    rng = np.random.default_rng(seed + B)
    rest = rng.permutation(np.setdiff1d(np.arange(B), fixed))[:P - fixed.size]
    slots = np.sort(np.concatenate([fixed, rest]))
    r = np.arange(B)
    idx = r % P
    rot = 1 + ((r // P) * 37 + 11) % 479
    idx[slots] = np.arange(P)
    rot[slots] = 0
    return slots, idx, rot


def test_regime_layouts():
    for (mode, B), reg in REGIMES.items():
        tile = rows_per_block(reg)
        share = chain_share(B, reg["chains"], tile) if reg["chains"] > 1 else None
        if reg["share"] is not None:
            assert share == reg["share"], (mode, B, share)
        if share is not None:
            assert share % tile == 0 and share < B <= 2 * share, (mode, B, share)
        slots, idx, rot = row_layout(B, share)
        assert slots.size == P and np.unique(slots).size == P and 0 <= slots[0] and slots[-1] < B, (mode, B)
        assert np.array_equal(np.sort(idx[slots]), np.arange(P)) and not rot[slots].any()
        assert idx.min() >= 0 and idx.max() < P and rot.min() >= 0 and rot.max() < 480
        assert np.unique(idx.astype(np.int64) * 480 + rot).size == B, (mode, B)      # every row a distinct input
        want = [0, 1, 31, 32, 127, 128, 255, 256, (B - 1) // 256 * 256, B - 129, B - 128, B - 2, B - 1]
        if share is not None:
            want += [share - 1, share, share + 1]
        assert np.isin(want, slots).all(), (mode, B, np.setdiff1d(want, slots))
    # the launcher's shares at the sizes the lifecycle test uses
    assert chain_share(24876, 2, 128) == 12544 and chain_share(65836, 2, 256) == 33024


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def model(blob):
    m = api.Model(blob)
    yield m
    m.close()


@pytest.fixture(scope="module")
def pool(oracle):
    """P synth streams of T_LIFE frames and the oracle's results for their first T_ROWS frames (once per module)."""
    pcm = synth.synth_batch_parallel(P, T_LIFE, workers=16)
    assert {synth.stream_kind(s) for s in range(P)} == {"voiced", "loud", "bursts", "twotone"}
    ref = oracle.run_batch(np.ascontiguousarray(pcm[:, :T_ROWS * 480]), group=8, threads=16)
    assert (ref[3] == 0).sum() > 0                   # the loud streams' frames are not silent: the pitch filter ran
    return pcm, ref


@pytest.fixture
def default_families(monkeypatch):
    for k in families.FAMILY_ENV:
        monkeypatch.delenv(k, raising=False)


class Rows:
    """The distinct-input batch on the device: frame(t, rows) -> int16 [len(rows), 480]."""

    def __init__(self, pool_pcm, idx, rot, dev):
        import torch
        self.pool = torch.from_numpy(pool_pcm).to(dev)
        self.idx = torch.from_numpy(idx).to(dev)
        self.rot = torch.from_numpy(rot).to(dev)
        self.ar = torch.arange(480, device=dev)

    def frame(self, t, rows):
        import torch
        x = self.pool[:, t * 480:(t + 1) * 480][self.idx[rows]]
        return torch.gather(x, 1, (self.ar[None, :] + self.rot[rows][:, None]) % 480).contiguous()


def _check_describe(ctx, mode, B, reg):
    d = ctx.describe()
    got = dict(dense=d["dense"], gru=d["gru"], gru_rb=d["gru_rb"], narrow=d["narrow"], chains=int(d["nn_chains"].split(":")[0]))
    want = {k: reg[k] for k in got}
    assert d["nn"] == NN_NAME[mode] and d["frontend"] == "split", d
    assert got == want, f"{mode} at B={B} now lands in {got}, the regime map says {want}: move the sizes with the threshold"
    plan = families.debug_plan(api.load_library(), B, MODES[mode])        # the host-only plan is what the context runs
    assert {k: d[k] for k in ("nn", "dense", "gru", "gru_rb", "narrow", "frontend")} == {k: plan[k] for k in ("nn", "dense", "gru", "gru_rb", "narrow", "frontend")}, (d, plan)
    assert d["nn_chains"].split(":")[0] == plan["nn_chains"], (d, plan)


def _where(B, r, share):
    return f"row {r} (offset {r % 128} in its 128-row tile, chain {r // share if share else 0})"


def _run_all_rows(ctx, rows, B, T, dev):
    """T frames of the whole batch; per-frame outputs kept on the device: out [T,B,480] i16, gr [T,B,68], feat [T,B,70], sil [T,B]."""
    import torch
    out = torch.empty((T, B, 480), dtype=torch.int16, device=dev)
    gr = torch.empty((T, B, 68), dtype=torch.float32, device=dev)
    feat = torch.empty((T, B, 70), dtype=torch.float32, device=dev)
    sil = torch.empty((T, B), dtype=torch.int32, device=dev)
    everyone = torch.arange(B, device=dev)
    for t in range(T):
        fr = rows.frame(t, everyone)
        ctx.process_i16_dev(fr.data_ptr(), out[t].data_ptr(), gr[t].data_ptr())
        ctx.read_features_dev(feat[t].data_ptr(), sil[t].data_ptr())
    return out, gr, feat, sil


@pytest.mark.gpu
@pytest.mark.parametrize("mode,B", list(REGIMES), ids=[f"{m}-{b}" for m, b in REGIMES])
def test_every_row_of_a_regime_is_bit_identical_to_the_reference_family(model, oracle, pool, default_families, mode, B):
    import torch
    from test_gpu_longrun import shared_stream
    from test_gpu_parity import F16_PCM_TOL_LSB, F16_GR_TOL
    reg = REGIMES[(mode, B)]
    share = reg["share"] if reg["chains"] > 1 else None
    tile = rows_per_block(reg)
    if share is None and reg["chains"] > 1:
        share = chain_share(B, reg["chains"], tile)
    slots, idx, rot = row_layout(B, share)
    T = T_ROWS
    dev = torch.device("cuda:0")
    ts = shared_stream(dev)
    with torch.cuda.stream(ts):
        rows = Rows(pool[0], idx, rot, dev)
        ctx = api.Context(model, B, nn_mode=MODES[mode], stream=ts.cuda_stream)
        try:
            _check_describe(ctx, mode, B, reg)
            out, gr, feat, sil = _run_all_rows(ctx, rows, B, T, dev)
        finally:
            ctx.close()
        # every row against the 1024-stream context of the same mode, fed the same rows chunk by chunk
        ref = api.Context(model, REF_ROWS, nn_mode=MODES[mode], stream=ts.cuda_stream)
        o = torch.empty((REF_ROWS, 480), dtype=torch.int16, device=dev)
        g = torch.empty((REF_ROWS, 68), dtype=torch.float32, device=dev)
        f = torch.empty((REF_ROWS, 70), dtype=torch.float32, device=dev)
        s = torch.empty((REF_ROWS,), dtype=torch.int32, device=dev)
        bad = torch.zeros((T, B), dtype=torch.int8, device=dev)     # bit 0 PCM, 1 g|r, 2 features, 3 silence
        for c0 in range(0, B, REF_ROWS):
            n = min(REF_ROWS, B - c0)
            chunk = torch.arange(c0, c0 + REF_ROWS, device=dev)
            chunk[n:] = 0                                            # padding rows: any input, ignored
            ref.reset()
            for t in range(T):
                ref.process_i16_dev(rows.frame(t, chunk).data_ptr(), o.data_ptr(), g.data_ptr())
                ref.read_features_dev(f.data_ptr(), s.data_ptr())
                bad[t, c0:c0 + n] = ((o[:n] != out[t, c0:c0 + n]).any(1).to(torch.int8)
                                     | ((g[:n].view(torch.int32) != gr[t, c0:c0 + n].view(torch.int32)).any(1).to(torch.int8) << 1)
                                     | ((f[:n].view(torch.int32) != feat[t, c0:c0 + n].view(torch.int32)).any(1).to(torch.int8) << 2)
                                     | ((s[:n] != sil[t, c0:c0 + n]).to(torch.int8) << 3))
        ref.close()
        torch.cuda.synchronize()
        nz = torch.nonzero(bad)
        if nz.numel():
            t, r = (int(v) for v in nz[0])
            what = [w for b, w in enumerate(("PCM", "g|r", "features", "silence")) if int(bad[t, r]) >> b & 1]
            rows_bad = int(bad.any(0).sum())
            pytest.fail(f"{mode} B={B}: {rows_bad} rows differ from the {REF_ROWS}-stream reference; first at frame {t}, "
                        f"{_where(B, r, share)}: {', '.join(what)} (row carries pool stream {idx[r]} rotated by {rot[r]})")
        d_slots = torch.from_numpy(slots).to(dev)
        got_o = out[:, d_slots].cpu().numpy()                       # [T, P, 480]
        got_g = gr[:, d_slots].cpu().numpy()
        got_f = feat[:, d_slots].cpu().numpy()
        got_s = sil[:, d_slots].cpu().numpy()
        del out, gr, feat, sil
    # the unrotated slots against the CPU oracle
    ro, rg, rf, rs = pool[1]
    got_o = got_o[1:].transpose(1, 0, 2).reshape(P, (T - 1) * 480)     # first output frame dropped (main.cpp:37)
    got_g, got_f, got_s = got_g.transpose(1, 0, 2), got_f.transpose(1, 0, 2), got_s.T
    pcm_tol, gr_tol = (F16_PCM_TOL_LSB, F16_GR_TOL) if mode == "f16" else (PCM_TOL_LSB, GR_TOL)
    fb = got_f.view(np.uint32) != rf.view(np.uint32)
    assert not fb.any(), f"features differ from the oracle at slot {slots[np.argwhere(fb)[0][0]]}"
    assert np.array_equal(got_s, rs)
    d = np.abs(got_o.astype(np.int32) - ro.astype(np.int32))
    assert d.max() <= pcm_tol, (int(d.max()), int(slots[np.argwhere(d == d.max())[0][0]]))
    dg = np.abs(got_g - rg)
    assert dg.max() <= gr_tol, (float(dg.max()), int(slots[np.argwhere(dg == dg.max())[0][0]]))


# Skip schedules of the lifecycle test: together they cover every residue of the ring phases (12, 6, 5, 3, 2), the first
# and the last tick, the reset tick and runs of consecutive skips.
SKIP_TICKS = [{0}, {1, 2}, {3, 4, 5}, {6, 18}, {7, 8, 9, 10, 11}, {13, 14}, {20, 25, T_LIFE - 1}, {12, 27}]
LIFECYCLE = [("mfma", 24876, 2, 128), ("mfma", 65836, 2, 256), ("x3", 32897, 1, 256), ("f16", 32897, 1, 256)]


def lifecycle_rows(B, chains, tile):
    """-> (share or None, rows reset at T_RESET, rows that skip ticks) at the tile, chain and last-block boundaries."""
    share = chain_share(B, chains, tile) if chains > 1 else None
    last = (B - 1) // 256 * 256
    reset = [128, last, B - 1] + ([share - 1] if share else [])
    skip = [0, 127, 255, 256, B - 129, B - 2] + ([share, share + 1] if share else [])
    reset = sorted(set(reset))
    skip = sorted(set(skip) - set(reset))
    return share, reset, skip


def test_lifecycle_schedules():
    ticks = set().union(*SKIP_TICKS)
    assert max(ticks) < T_LIFE and 0 in ticks and T_RESET in ticks
    for m in (12, 6, 5, 3, 2):
        assert {x % m for x in ticks} == set(range(m)), m
    assert T_RESET % 12 and T_RESET % 6 and T_RESET % 5 and T_RESET % 3 and T_RESET % 2      # every ring phase nonzero
    for mode, B, chains, tile in LIFECYCLE:
        share, reset, skip = lifecycle_rows(B, chains, tile)
        assert 0 <= min(reset + skip) and max(reset + skip) < B and not set(reset) & set(skip)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,B,chains,tile", LIFECYCLE, ids=[f"{m}-{b}" for m, b, _, _ in LIFECYCLE])
def test_lifecycle_at_chained_and_direct_sizes(model, oracle, pool, default_families, mode, B, chains, tile):
    """reset_streams at tick 13 (history slot 1 of 12, look-ahead 1 of 6, conv 3 of 5 / 1 of 3, odd GRU half) on rows at the
    tile, chain and last-block boundaries; other boundary rows skip ticks through the active set.  Untouched rows equal an
    unperturbed run bit for bit; a reset row equals a fresh 1024-stream context fed its new stream; a skipping row's
    active ticks equal a 1024-stream context fed only those frames, and its output rows keep their values on the ticks it
    skips; the special rows stay within the oracle bounds."""
    import torch
    from test_gpu_longrun import shared_stream
    from test_gpu_parity import F16_PCM_TOL_LSB, F16_GR_TOL
    T, T0 = T_LIFE, T_RESET
    share, reset, skip = lifecycle_rows(B, chains, tile)
    sched = {s: SKIP_TICKS[k % len(SKIP_TICKS)] for k, s in enumerate(skip)}
    special = reset + skip
    slots, idx, rot = row_layout(B, share, seed=1)
    fresh = synth.synth_batch(len(reset), T - T0, first_stream=1000)   # the reset rows' new streams
    dev = torch.device("cuda:0")
    ts = shared_stream(dev)
    with torch.cuda.stream(ts):
        rows = Rows(pool[0], idx, rot, dev)
        everyone = torch.arange(B, device=dev)
        # unperturbed run
        ctx = api.Context(model, B, nn_mode=MODES[mode], stream=ts.cuda_stream)
        try:
            d = ctx.describe()
            assert int(d["nn_chains"].split(":")[0]) == chains, d
            if mode == "mfma":
                assert d["gru"] == ("direct_rows64" if tile == 256 else "direct_rows32"), d
            else:
                assert d["gru"].endswith("rows64"), d
            ref_o = torch.empty((T, B, 480), dtype=torch.int16, device=dev)
            ref_g = torch.empty((T, B, 68), dtype=torch.float32, device=dev)
            for t in range(T):
                ctx.process_i16_dev(rows.frame(t, everyone).data_ptr(), ref_o[t].data_ptr(), ref_g[t].data_ptr())
        finally:
            ctx.close()
        # the same run with resets and skipped ticks
        d_fresh = torch.from_numpy(fresh).to(dev)
        d_reset = torch.tensor(reset, device=dev)
        d_special = torch.tensor(special, device=dev)
        d_out = torch.full((B, 480), 12345, dtype=torch.int16, device=dev)
        d_gr = torch.full((B, 68), -7.0, dtype=torch.float32, device=dev)
        sp_o = torch.empty((T + 1, len(special), 480), dtype=torch.int16, device=dev)
        sp_g = torch.empty((T + 1, len(special), 68), dtype=torch.float32, device=dev)
        sp_o[0] = d_out[d_special]; sp_g[0] = d_gr[d_special]
        bad = torch.zeros((T, B), dtype=torch.bool, device=dev)
        ctx = api.Context(model, B, nn_mode=MODES[mode], stream=ts.cuda_stream)
        try:
            for t in range(T):
                if t == T0:
                    ctx.reset_streams(reset)
                fr = rows.frame(t, everyone)
                if t >= T0:
                    fr[d_reset] = d_fresh[:, (t - T0) * 480:(t - T0 + 1) * 480]
                off = [s for s in skip if t in sched[s]]
                for s in off:
                    fr[s] = 31000                                   # a skipped row's input must not matter
                active = np.setdiff1d(np.arange(B), off)
                ctx.process_i16_active_dev(fr.data_ptr(), d_out.data_ptr(), d_gr.data_ptr(), active[::-1] if t % 2 else active)
                touched = torch.zeros(B, dtype=torch.bool, device=dev)
                touched[torch.tensor(skip, device=dev)] = True
                if t >= T0:
                    touched[d_reset] = True
                bad[t] = ((d_out != ref_o[t]).any(1) | (d_gr.view(torch.int32) != ref_g[t].view(torch.int32)).any(1)) & ~touched
                sp_o[t + 1] = d_out[d_special]; sp_g[t + 1] = d_gr[d_special]
        finally:
            ctx.close()
        torch.cuda.synchronize()
        nz = torch.nonzero(bad)
        if nz.numel():
            t, r = (int(v) for v in nz[0])
            pytest.fail(f"{mode} B={B}: {int(bad.any(0).sum())} untouched rows differ from the unperturbed run; first at frame "
                        f"{t}, {_where(B, r, share)}")
        del ref_o, ref_g, bad
        # expected: the reset rows' new streams from frame 0 and the skipping rows fed only their frames, back to back
        packed = torch.zeros((REF_ROWS, T * 480), dtype=torch.int16, device=dev)
        packed[:len(reset), :(T - T0) * 480] = d_fresh
        n_on = {}
        for k, s in enumerate(skip):
            on = [t for t in range(T) if t not in sched[s]]
            n_on[s] = len(on)
            for j, t in enumerate(on):
                packed[len(reset) + k, j * 480:(j + 1) * 480] = rows.frame(t, everyone[s:s + 1])[0]
        small = api.Context(model, REF_ROWS, nn_mode=MODES[mode], stream=ts.cuda_stream)
        o = torch.empty((T, REF_ROWS, 480), dtype=torch.int16, device=dev)
        g = torch.empty((T, REF_ROWS, 68), dtype=torch.float32, device=dev)
        try:
            for t in range(T):
                small.process_i16_dev(packed[:, t * 480:(t + 1) * 480].contiguous().data_ptr(), o[t].data_ptr(), g[t].data_ptr())
        finally:
            small.close()
        torch.cuda.synchronize()
        ns = len(special)
        exp_o, exp_g = o[:, :ns].cpu().numpy(), g[:, :ns].cpu().numpy()
        got_o, got_g = sp_o.cpu().numpy(), sp_g.cpu().numpy()          # [T + 1, ns, ...]: index t + 1 = after tick t
        packed = packed[:ns].cpu().numpy()
    for k, s in enumerate(reset):
        for t in range(T0, T):
            assert np.array_equal(got_o[t + 1, k], exp_o[t - T0, k]), f"reset {_where(B, s, share)}, frame {t}: PCM"
            assert np.array_equal(got_g[t + 1, k].view(np.uint32), exp_g[t - T0, k].view(np.uint32)), f"reset {_where(B, s, share)}, frame {t}: g|r"
    for k, s in enumerate(skip):
        kk, j = len(reset) + k, 0
        for t in range(T):
            if t in sched[s]:
                assert np.array_equal(got_o[t + 1, kk], got_o[t, kk]), f"skipping {_where(B, s, share)}, tick {t}: output row changed"
                assert np.array_equal(got_g[t + 1, kk].view(np.uint32), got_g[t, kk].view(np.uint32)), f"skipping {_where(B, s, share)}, tick {t}: g|r row changed"
            else:
                assert np.array_equal(got_o[t + 1, kk], exp_o[j, kk]), f"skipping {_where(B, s, share)}, tick {t} (its frame {j}): PCM"
                assert np.array_equal(got_g[t + 1, kk].view(np.uint32), exp_g[j, kk].view(np.uint32)), f"skipping {_where(B, s, share)}, tick {t}: g|r"
                j += 1
    # the special rows' streams against the CPU oracle
    pcm_tol, gr_tol = (F16_PCM_TOL_LSB, F16_GR_TOL) if mode == "f16" else (PCM_TOL_LSB, GR_TOL)
    for k, s in enumerate(special):
        n = T - T0 if k < len(reset) else n_on[s]
        ro, rg = oracle.run_pcm(packed[k, :n * 480])
        got = np.concatenate([exp_o[j, k] for j in range(1, n)])
        d = np.abs(got.astype(np.int32) - ro.astype(np.int32)).max()
        assert d <= pcm_tol, (s, int(d))
        assert np.abs(exp_g[:n, k] - rg).max() <= gr_tol, s
