#!/usr/bin/env python
"""Throughput bench of the batched PercepNet hot path (BASELINE.json metric).

One "step" = one pass of the hot path over one batch: every one of the B streams of this GPU
advances by one 10 ms frame (480 samples in -> 480 samples out), i.e. B stream-frames.
Inputs (int16 PCM, the CLI's format) are resident in HBM before the timed region starts.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--streams B] [--dump-outputs DIR] [--full]

A plain run measures the headline alone: setup, W warm-up steps, K timed steps, the outputs of the last step when
--dump-outputs is given, and the result line (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).
Everything else — CPU baseline, parity against the CPU oracle, per-kernel events and rooflines, the other
configurations, the sustained and paced real-time legs, the detail file — runs with --full.

N > 1: `python bench.py --gpus N` launches its own N ranks through torch.distributed.run (one rank per GPU); when
the driver launches the ranks itself (WORLD_SIZE/RANK in the environment) the script joins that world instead.
RCCL is used only for the start/stop barrier, the max-over-ranks time and the report gather — streams are
independent, weak scaling.  `--force-dist` makes an N = 1 run go through the same RCCL calls (world of one).

Workload choice (config.workload): BASELINE.json's metric is a CAPACITY ("real-time 48 kHz
streams per GPU", target >= 50 k), which only configs[2] (65 536 concurrent streams per GPU, the
largest single-GPU configuration) can exhibit; configs[1] (1024 streams) is available through
`--streams 1024` and is covered by the parity tests.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
# the paced 10 ms-clock harness and the capacity search over batch sizes live in tools/realtime_capacity.py (measurement, not product)
from realtime_capacity import ClockSampler, gpu_clock_mhz, paced_realtime, percentiles, realtime_capacity  # noqa: E402

FRAME = 480
FLOP_PER_STREAM_FRAME = 15896576          # 2 x 7 948 288 MAC, network only
GRU512_FLOP_PER_STREAM_FRAME = 2 * 1572864  # one 512->512 GRU layer
PEAK_FP32_MFMA_TFLOPS = 157.3             # MI355X_MICROARCH.md chip-level parameters
PEAK_HBM_TBS = 8.0


def _cpu_worker(args):
    """Time the CPU baseline on one core for ~budget seconds: percepNet_run semantics
    (main.cpp:30-39) on in-memory PCM, 100-frame (1 s of audio) chunks.  pin: logical CPU to bind to, or None."""
    kind, budget, seed, pin = args
    if pin is not None:
        try:
            os.sched_setaffinity(0, {pin})
        except OSError:
            pass
    from percepnet_amd import synth, weights
    from oracle import oracle as orc
    blob = weights.default_blob(1234)
    if kind == "reference":
        eng = orc.Reference(blob)
    elif kind == "reference_avx2":
        eng = orc.Reference(blob, so=orc.REF_AVX2_SO)
    else:
        eng = orc.Oracle(blob)
    pcm = synth.synth_stream(seed, 100)
    eng.run_pcm(pcm[:480 * 5], want_gr=False)     # touch code + weights once
    n = 0
    t0 = time.perf_counter()
    while True:
        eng.run_pcm(pcm, want_gr=False)
        n += 100
        dt = time.perf_counter() - t0
        if dt >= budget:
            return n, dt


def physical_cores():
    """One logical CPU per physical core of this process's affinity mask (first SMT sibling)."""
    try:
        allowed = sorted(os.sched_getaffinity(0))
    except AttributeError:
        return list(range(os.cpu_count() or 1))
    seen, picks = set(), []
    for c in allowed:
        try:
            sib = open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip()
        except OSError:
            sib = str(c)
        if sib not in seen:
            seen.add(sib)
            picks.append(c)
    return picks


def cpu_baseline(budget=6.0, full=False):
    """Reference CPU path (oracle/_ref = the untouched reference sources built with the README
    flags; falls back to the C restatement, kind "port", if that .so did not travel) timed on
    this host, SURVEY §8(d): (1) one process alone; (2) one process per PHYSICAL core, each pinned to its core —
    the headline `value`; (3) footnote: the -mavx2 -mfma -U__AVX__ build on one core; full=True adds (4) the unpinned
    one-process-per-logical-CPU pool (the "as shipped" fan-out of utils/run.sh) for context.  ~12 s of wall by default."""
    import multiprocessing as mp
    from oracle import oracle as orc
    from percepnet_amd import weights
    orc.build()
    weights.default_blob(1234)                     # create the on-disk cache before forking
    kind = "reference" if os.path.exists(orc.REF_SO) else "port"
    try:
        logical = len(os.sched_getaffinity(0))
    except AttributeError:
        logical = os.cpu_count() or 1
    phys = physical_cores()
    n1, t1 = _cpu_worker((kind, min(budget, 2.0), 0, None))
    avx = None
    if kind == "reference" and os.path.exists(orc.REF_AVX2_SO):
        na, ta = _cpu_worker(("reference_avx2", 1.5, 0, None))
        avx = na / ta
    ctx = mp.get_context("fork")
    t0 = time.perf_counter()
    with ctx.Pool(len(phys)) as pool:
        res = pool.map(_cpu_worker, [(kind, budget, s, c) for s, c in enumerate(phys)], chunksize=1)
    fps_phys = sum(n / dt for n, dt in res)
    frames_phys = sum(n for n, _ in res)
    unpinned = None
    if full:
        with ctx.Pool(logical) as pool:
            res2 = pool.map(_cpu_worker, [(kind, budget * 0.6, s, None) for s in range(logical)], chunksize=1)
        fps_all = sum(n / dt for n, dt in res2)
        unpinned = {"cores": logical, "frames_per_s": round(fps_all, 1), "streams": round(fps_all / 100.0, 3)}
    wall = time.perf_counter() - t0
    print(f"[bench] cpu baseline: kind={kind} one-core {n1 / t1:.1f} fps, {len(phys)} pinned physical cores "
          f"{fps_phys:.1f} fps" + (f", {logical} unpinned logical CPUs {unpinned['frames_per_s']:.1f} fps" if unpinned else "")
          + f", pools wall {wall:.1f} s", file=sys.stderr, flush=True)
    return {
        "value": round(fps_phys / 100.0, 3), "unit": "real-time 48 kHz streams (one pinned process per physical host core)",
        "frames_per_s": round(fps_phys, 1), "frames_per_s_one_core": round(n1 / t1, 1),
        "cores": len(phys), "kind": kind,
        "sample": f"{len(phys)} processes, one synthetic stream each, pinned one per physical core, ~{budget:.0f} s wall, "
                  f"{frames_phys} stream-frames in total, 100-frame chunks; plus one process alone for the one-core figure",
        "unpinned_all_logical_cpus": unpinned,
        "best_effort_avx2_fma_one_core_fps": None if avx is None else round(avx, 1),
        "note": "all-core figures are DRAM-bound: every process re-streams its own 32 MB of weights per frame",
    }


def kernel_sources():
    """Every file a kernel is compiled from: all .hip / .h / .inc under csrc/ (any depth) + the launch sequence."""
    csrc = os.path.join(ROOT, "percepnet_amd", "csrc")
    out = []
    for d, _, fs in sorted(os.walk(csrc)):
        out += [os.path.join(d, f) for f in sorted(fs) if f.endswith((".hip", ".h", ".inc")) or f == "pn_context.cpp"]
    return out


def kernels_snapshot():
    """Identity of the kernels a profile was taken with: sha256 over every kernel source (first 12 hex digits).
    tools/summarize_prof.py stamps it into profiles/*_pmc_per_launch.csv; a CSV from other kernels is refused."""
    import hashlib
    h = hashlib.sha256()
    for f in kernel_sources():
        h.update(os.path.relpath(f, ROOT).encode() + b"\0" + open(f, "rb").read())
    return h.hexdigest()[:12]


def pmc_traffic_bytes(streams, kernel_prefix="pn_gru_mfma", tag=""):
    """HBM-side bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of
    this same command (profiles/*_pmc_per_launch.csv; FETCH_SIZE and WRITE_SIZE are collected in
    separate --pmc runs, both in KB).  Per MI355X_MICROARCH.md the gfx950 FETCH_SIZE counts 64 B
    per 128-B request for 16 B/lane streaming loads, so it is doubled; WRITE_SIZE is used as is
    (it equals the algorithmic store bytes exactly).  Only a CSV stamped with the CURRENT kernels' snapshot id is
    accepted (a profile of other kernels says nothing about this run): -> (bytes | None, source note)."""
    import csv, glob
    snap = kernels_snapshot()
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_per_launch{tag}.csv")))
    fresh = [f for f in files if open(f).readline().strip() == f"# kernels_snapshot={snap}"]
    if not fresh:
        return None, f"no PMC profile of kernels snapshot {snap} under profiles/ (tools/gpu_profile.sh + tools/summarize_prof.py)"
    fetch = write = None
    rows = [l for l in open(fresh[-1]) if not l.startswith("#")]
    recs = [r for r in csv.DictReader(rows) if r["kernel"].startswith(kernel_prefix)]
    grids = sorted({int(r["kernel"].rsplit("grid=", 1)[1]) for r in recs if "grid=" in r["kernel"]})
    grid = f"grid={grids[-1]}" if grids else "grid=?"        # the 512->512 layers are the largest grid of the family
    for r in recs:
        if r["kernel"].endswith(grid):
            if r["counter"] == "FETCH_SIZE":
                fetch = float(r["avg"]) * 1024 * 2
            elif r["counter"] == "WRITE_SIZE":
                write = float(r["avg"]) * 1024
    if fetch is None or write is None:
        return None, f"{os.path.basename(fresh[-1])} has no FETCH/WRITE rows for {grid}"
    return fetch + write, os.path.basename(fresh[-1])


def measure_parity(ctx, frames, pool_pcm, out, torch):
    """BASELINE metric part (iii), MEASURED on this run's own batch, outside the timed region: the context is reset,
    the same W+K frames are run again and the first P batch slots (the pool's P distinct, unrotated streams) are
    captured every frame and compared with the CPU oracle on the same PCM.  Also checks that the replay ends on the
    same output as the timed run (the kernels are deterministic)."""
    from oracle.oracle import Oracle
    from percepnet_amd import weights
    P, T = pool_pcm.shape[0], len(frames)
    B = ctx.n_streams
    last_timed = out.clone()
    dev = out.device
    g = torch.empty((B, 68), dtype=torch.float32, device=dev)
    acc_o = torch.empty((T, P, 480), dtype=torch.int16, device=dev)
    acc_g = torch.empty((T, P, 68), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.reset()
    for t in range(T):
        ctx.process_i16_dev(frames[t].data_ptr(), out.data_ptr(), g.data_ptr())
        acc_o[t].copy_(out[:P]); acc_g[t].copy_(g[:P])
    torch.cuda.synchronize()
    replay_identical = bool(torch.equal(out, last_timed))
    ro, rg, _, _ = Oracle(weights.default_blob(1234)).run_batch(pool_pcm, want_feat=False)
    got = acc_o[1:].permute(1, 0, 2).reshape(P, (T - 1) * 480).cpu().numpy().astype("int32")
    d = abs(got - ro.astype("int32"))
    dg = abs(acc_g.permute(1, 0, 2).cpu().numpy() - rg)
    return {"max_abs_delta_vs_cpu_ref_lsb": int(d.max()), "pcm_samples_differing": int((d != 0).sum()),
            "pcm_samples_checked": int(d.size), "max_abs_delta_gr": float(dg.max()),
            "sample": f"the {P} distinct pool streams (batch slots 0..{P - 1}) x all {T} frames of this run vs the CPU oracle "
                      f"(oracle/percepnet_oracle.c, bit-exact to the compiled reference)",
            "replay_of_timed_run_bit_identical": replay_identical,
            "long_horizon": "tests/test_gpu_longrun.py: 1024 streams x 1000 frames and 256 sampled of 65536 x 1000 frames"}


def gru_roofline(kt, B, fp16, desc, n_gpus=1, fps=None, traffic_tag=""):
    """The roofline object of the dominant kernel (the 512->512 GRU step, 4 layers per frame) from HIP-event kernel
    times `kt` of a context described by `desc` (Context.describe()).
    Row-range chains (round 6; desc["nn_chains"] = "2:n"): a layer step over the batch is N launches of the kernel, one per chain
    on its own stream, each over 1/N of the rows, and the N launches of a layer overlap in time — each is bracketed by HIP events on
    the stream it is launched on and `avg_launch_ms` is the mean over ALL of them.  One launch alone does not have the chip; the chip
    does `concurrent_launches` of them in that time.  So `achieved` = concurrent_launches x flop_per_launch / avg_launch_ms (the
    chip's rate while this kernel runs), with the per-launch figures beside it; `whole_pipeline_tflops` — from the wall clock of
    the timed region alone — is the independent check that the chip-level rate is not double counted."""
    ms, n = kt.get("gru512", (0.0, 0))
    if not n:
        return None
    avg_s = ms / n * 1e-3
    chains = max(1, int(str(desc.get("nn_chains", "1")).split(":")[0]))
    rows = B / chains                                     # rows per launch (the chains are equal to within one 128-row tile)
    flops = rows * GRU512_FLOP_PER_STREAM_FRAME
    x3 = desc.get("nn") == "mfma_x3"
    # the fp16-operand mode runs the hi-plane-only instantiation of the split-precision kernels (pn_nn_x3.hip)
    direct = str(desc.get("gru", "")).startswith("direct")     # round 6: A fragments straight from fragment-order fp32 shadows (pn_nn_d.hip)
    kname = "pn_gru_x3_kernel" if (x3 or fp16) else ("pn_gru_small_kernel" if desc.get("gru") == "small" else
                                                      ("pn_gru_d_kernel" if direct else "pn_gru_mfma_p_kernel"))
    traffic, traffic_src = pmc_traffic_bytes(B, kname[:11], traffic_tag)
    ach = chains * flops / avg_s / 1e12
    # dense fp16 / fp32 MFMA peaks (MI355X_MICROARCH.md).  Split precision: `achieved` stays the ALGORITHMIC rate (2 M N K per
    # launch); every product costs three fp16 MFMAs, so the bound is a third of the dense fp16 peak
    peak = round(2500.0 / 3, 1) if x3 else (2500.0 if fp16 else PEAK_FP32_MFMA_TFLOPS)
    # x, h_old, h_new once each (+ the fp32 state read for the blend in the shadow-operand modes) + the weights; the direct-operand
    # kernel reads x and h_old as shadows, h_old again as rows for the blend, and writes h_new as rows AND as shadow: 5 arrays
    alg_launch = int((5 if direct else 3) * rows * 512 * (2 if fp16 else 4) + (rows * 512 * 4 if (fp16 or x3) else 0) + 2 * 512 * 1536 * (2 if fp16 else 4))
    r = {"kernel": kname + ("<rows/32, planes=1>" if fp16 else ("<rows/32, planes=2>" if x3 else "")) +
                   f" (512->512 reset-after GRU step, 4 layers per frame x {chains} launch(es) per layer)",
         "bound": "mfma", "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
         "frac": round(ach / peak, 4), "traffic": None if traffic is None else traffic * chains,
         "traffic_source": traffic_src, "kernels_snapshot": kernels_snapshot(),
         "algorithmic_bytes_per_launch": alg_launch * chains,
         **({"operands": "A fragments from fragment-order fp32 shadows, 64 rows per wave (pn_nn_d.hip), bit-identical to the batch-GEMM family"} if direct else {}),
         "flop_per_launch": int(flops), "avg_launch_ms": round(avg_s * 1e3, 4), "concurrent_launches": chains,
         "rows_per_launch": int(rows)}
    if chains > 1:
        r["achieved_one_launch"] = round(flops / avg_s / 1e12, 2)
        r["note"] = (f"{chains} launches of this kernel (one per row-range chain, each on its own stream, {int(rows)} rows) overlap; achieved / traffic / "
                     "algorithmic_bytes_per_launch are the CONCURRENT launches together over the average launch duration")
    if x3:
        r["peak_note"] = ("dense fp16 MFMA peak 2500 TFLOP/s / 3 (three fp16 MFMA products per fp32 product); executed MFMA rate = "
                          f"{round(3 * ach, 1)} TFLOP/s; the fp32 MFMA peak this replaces is {PEAK_FP32_MFMA_TFLOPS} TFLOP/s")
    if fps is not None:
        # report BOTH bounds of the whole pipeline and say which one binds
        hbm_bytes = 62608 + 31850256 / B
        r["whole_pipeline_tflops"] = round(fps / n_gpus * FLOP_PER_STREAM_FRAME / 1e12, 2)
        r["whole_pipeline_frac_of_mfma_peak"] = round(fps / n_gpus * FLOP_PER_STREAM_FRAME / 1e12 / peak, 4)
        r["algorithmic_hbm_gbs"] = round(fps / n_gpus * hbm_bytes / 1e9, 1)
        r["whole_pipeline_frac_of_hbm_peak"] = round(fps / n_gpus * hbm_bytes / 1e12 / PEAK_HBM_TBS, 4)
        intensity = FLOP_PER_STREAM_FRAME / hbm_bytes
        ridge = peak * 1e12 / (PEAK_HBM_TBS * 1e12)
        r["both_bounds"] = {"mfma": {"peak_tflops": peak, "frac_dominant_kernel": r["frac"], "frac_whole_pipeline": r["whole_pipeline_frac_of_mfma_peak"]},
                            "hbm": {"peak_gbs": PEAK_HBM_TBS * 1e3, "frac_whole_pipeline": r["whole_pipeline_frac_of_hbm_peak"]},
                            "arithmetic_intensity_flop_per_byte": round(intensity, 1), "ridge_flop_per_byte": round(ridge, 1),
                            "binding": "hbm" if intensity < ridge else "mfma",
                            "note": "at these operand rates the whole pipeline sits " + ("BELOW the ridge: HBM binds" if intensity < ridge else "above the ridge: the matrix pipe binds")}
    return r


# Per-kernel algorithmic bytes of the DSP kernels per stream-frame (what each kernel must move given the phase split; the
# history window is read by three kernels, so their sum exceeds SURVEY 8(d)'s whole-pipeline minimum of 32.9 KB):
#   fe_spec_in   int16 PCM in 960 + previous frame of the history 1920 (the look-ahead window) | history slot 1920 +
#                look-ahead spectrum 3200 + band energies 144 written
#   fe_pitch     pitch_buf view of the history 1728 x 4 = 6912 | period, gain, two features 16
#   fe_spec_out  comb-tap window of the history for the longest period 5568 x 4 = 22272 + X 3200 + 2 x 144 band energies |
#                comb-filtered spectrum 3200 + feature row 512 + silence flag 4
#   backend      X 3200 + P 3200 + g|r 272 + synthesis memory 1920 + silence 4 | synthesis memory 1920 + int16 PCM 960
DSP_KERNELS = {
    "fe_spec_in": ("pn_fe_spec_in_kernel", 960 + 1920 + 1920 + 3200 + 144),
    "fe_pitch": ("pn_fe_pitch_kernel", 6912 + 16),
    "fe_spec_out": ("pn_fe_spec_out_kernel", 22272 + 3200 + 288 + 3200 + 512 + 4),
    "backend": ("pn_backend_kernel", 3200 + 3200 + 272 + 1920 + 4 + 1920 + 960),
}


def pmc_kernel_counters(kernel_prefix, tag=""):
    """{counter: average per launch} of one kernel from the committed, snapshot-matched PMC summary (the largest grid of
    that kernel name), or (None, why)."""
    import csv, glob
    snap = kernels_snapshot()
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_per_launch{tag}.csv")))
    fresh = [f for f in files if open(f).readline().strip() == f"# kernels_snapshot={snap}"]
    if not fresh:
        return None, f"no PMC profile of kernels snapshot {snap} under profiles/"
    rows = [l for l in open(fresh[-1]) if not l.startswith("#")]
    recs = [r for r in csv.DictReader(rows) if r["kernel"].startswith(kernel_prefix) and "grid=" in r["kernel"]]
    if not recs:
        return None, f"{os.path.basename(fresh[-1])} has no rows for {kernel_prefix}"
    g = max(int(r["kernel"].rsplit("grid=", 1)[1]) for r in recs)
    return {r["counter"]: float(r["avg"]) for r in recs if r["kernel"].endswith(f"grid={g}")}, os.path.basename(fresh[-1])


SPEC_OUT_FIXED = 3200 + 288 + 3200 + 512 + 4          # X + two band-energy rows read | comb-filtered spectrum + feature row + silence flag written


def dsp_roofline(kt, B, tag="", periods=None, silent=None):
    """HBM roofline of the DSP kernels, ONE OBJECT PER KERNEL: `achieved` = algorithmic bytes of that kernel / its HIP-event
    time; `traffic` = HBM-side bytes per launch from the rocprofv3 counters of the same kernels (FETCH_SIZE x 2 — the gfx950
    counter tallies the 128-byte requests of 16-byte-per-lane streaming loads at 64 B, MI355X_MICROARCH.md; calibrated for this
    kernel family's own access patterns, the comb filter's UNALIGNED dwordx4 windows included, by
    tools/probes/fetch_unaligned_probe.hip: profiles/r05_fetch_size_calibration.log — + WRITE_SIZE as is), `traffic_gbs` the same
    over the event time, `traffic_over_algorithmic` what the phase split and re-reads cost.
    periods (int array, one per stream): the pitch periods the run's own last frame filtered at (pn_ctx_debug_copy 13).  The comb
    filter of a stream reads the window [2400 - 3T, 3360 + 3T) = 960 + 6T samples (reference denoise.cpp:416-422), so
    fe_spec_out's algorithmic bytes are sum_s (960 + 6 T_s) * 4 + the fixed rows — they FOLLOW FROM THE RUN; the figure for the
    longest period (T = 768) is kept as `algorithmic_bytes_worst_case`.  `frontend` / `dsp_total` lump the kernels."""
    out, tot_ms, tot_alg, tot_tr = {}, 0.0, 0, 0
    for fam, (kname, per_stream) in DSP_KERNELS.items():
        ms, n = kt.get(fam, (0.0, 0))
        if not n:
            continue
        ms /= n
        alg = B * per_stream
        extra = {}
        if fam == "fe_spec_out":
            extra["algorithmic_bytes_worst_case"] = alg
            if periods is not None and len(periods) == B:
                import numpy as np
                T = np.asarray(periods, dtype=np.int64)
                alg = int(((960 + 6 * T) * 4).sum()) + B * SPEC_OUT_FIXED
                extra["pitch_period_mean"] = round(float(T.mean()), 1)
                extra["comb_window_bytes_mean"] = round(float(((960 + 6 * T) * 4).mean()), 1)
                extra["algorithmic_bytes_source"] = "sum over this run's streams of (960 + 6 T) * 4 (T = the period the last frame filtered at) + fixed rows"
            else:
                extra["algorithmic_bytes_source"] = "worst case (T = 768): the run's periods were not read"
        if fam == "backend" and silent is not None:
            # round 6: a stream whose frame is silent skips pitch_filter (reference denoise.cpp:536-538) and the kernel no longer
            # fetches its comb-filtered spectrum P (3200 B): the algorithmic bytes follow from the run's own silence flags (the
            # synthetic suite keeps 5 % loud streams; by the reference's 1/960^2 silence test every other stream is "silent")
            extra["algorithmic_bytes_all_streams_non_silent"] = alg
            extra["silent_streams"] = int(silent)
            alg -= int(silent) * 3200
            extra["algorithmic_bytes_source"] = "P (3200 B) counted for the non-silent streams of this run's last frame only"
        o = {"kernel": kname, "bound": "hbm", "ms": round(ms, 4), "algorithmic_bytes": alg,
             "achieved": round(alg / (ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_TBS * 1e3, "unit": "GB/s",
             "frac": round(alg / (ms * 1e-3) / 1e12 / PEAK_HBM_TBS, 4)}
        o.update(extra)
        ctr, src = pmc_kernel_counters(kname, tag)
        if ctr and "FETCH_SIZE" in ctr and "WRITE_SIZE" in ctr:
            tr = ctr["FETCH_SIZE"] * 1024 * 2 + ctr["WRITE_SIZE"] * 1024
            o.update({"traffic": tr, "traffic_gbs": round(tr / (ms * 1e-3) / 1e9, 1), "traffic_frac_of_peak": round(tr / (ms * 1e-3) / 1e12 / PEAK_HBM_TBS, 4),
                      "traffic_over_algorithmic": round(tr / alg, 3), "traffic_source": src})
            if "SQ_LDS_BANK_CONFLICT" in ctr and ctr.get("SQ_LDS_IDX_ACTIVE"):
                o["lds_bank_conflict_share"] = round(ctr["SQ_LDS_BANK_CONFLICT"] / ctr["SQ_LDS_IDX_ACTIVE"], 4)
            tot_tr += tr
        else:
            o.update({"traffic": None, "traffic_source": src})
        out[fam] = o
        tot_ms += ms; tot_alg += alg
    if out:
        out["dsp_total"] = {"ms": round(tot_ms, 4), "algorithmic_bytes": tot_alg, "achieved": round(tot_alg / (tot_ms * 1e-3) / 1e9, 1),
                            "frac": round(tot_alg / (tot_ms * 1e-3) / 1e12 / PEAK_HBM_TBS, 4), "unit": "GB/s",
                            "traffic": tot_tr or None, "traffic_over_algorithmic": round(tot_tr / tot_alg, 3) if tot_tr else None,
                            "whole_pipeline_minimum_bytes": B * (62608 - 29696),
                            "traffic_over_whole_pipeline_minimum": round(tot_tr / (B * (62608 - 29696)), 3) if tot_tr else None,
                            "note": "per-kernel algorithmic bytes count the history window once per kernel that needs it (fe_spec_out: the "
                                    "window of each stream's own period); whole_pipeline_minimum_bytes is SURVEY 8(d)'s 62 608 - 29 696 B per stream-frame"}
    # the single-launch front ends (PERCEPNET_FE=mono|g2) have no per-phase kernels
    fe = kt.get("frontend", (0.0, 0))
    if fe[1]:
        ms = fe[0] / fe[1]; by = B * (27 * 1024 + 9 * 1024)
        out["frontend"] = {"bound": "hbm", "ms": round(ms, 4), "achieved": round(by / (ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_TBS * 1e3,
                           "unit": "GB/s", "frac": round(by / (ms * 1e-3) / 1e12 / PEAK_HBM_TBS, 4), "algorithmic_bytes": by}
    return out


def read_periods(ctx, B):
    """The pitch period every stream's comb filter used in the context's last frame (int32 per stream)."""
    import numpy as np
    try:
        return np.frombuffer(ctx.debug_copy(13, B).tobytes(), dtype=np.int32).copy()
    except Exception:                         # noqa: BLE001 — the roofline then falls back to the worst case and says so
        return None


def read_silent(ctx, B):
    """How many streams the context's last frame flagged silent (they skip pitch_filter and the back end's read of P)."""
    try:
        return int((ctx.read_features()[1] != 0).sum())
    except Exception:                         # noqa: BLE001 — the back end's algorithmic bytes then count P for every stream
        return None


def distinct_streams_leg(api, torch, ctx, dev, B, K, W, seed=2026, prime=12):
    """65 536 DISTINCT streams (round-4 verdict item 4): the headline tiles 64 pool streams over the batch, so the
    data-dependent paths of the pitch kernel see 64 behaviours.  Here every stream is synthesised on the device from its own
    parameters — a harmonic tone with its own fundamental (60-500 Hz, gliding), harmonic count, level (5 % near full scale, so
    the non-silent branch runs) and noise floor — and the same K steps are timed with per-kernel events."""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    W = W + prime                                            # stream priming (one history ring) + warm-up, as in the headline
    T = K + W
    f0 = 60.0 + 440.0 * torch.rand(B, 1, device=dev, generator=g)
    glide = 1.0 + 0.2 * (torch.rand(B, 1, device=dev, generator=g) - 0.5)
    nh = torch.randint(1, 9, (B, 1), device=dev, generator=g).float()
    loud = torch.rand(B, 1, device=dev, generator=g) < 0.05
    amp = torch.where(loud, 20000.0 + 10000.0 * torch.rand(B, 1, device=dev, generator=g), 300.0 + 5000.0 * torch.rand(B, 1, device=dev, generator=g))
    noise = 20.0 + 400.0 * torch.rand(B, 1, device=dev, generator=g)
    ph0 = 6.2831853 * torch.rand(B, 1, device=dev, generator=g)
    frames = []
    for t in range(T):
        nidx = (t * FRAME + torch.arange(FRAME, device=dev, dtype=torch.float32))[None, :]
        f = f0 * (1.0 + (glide - 1.0) * nidx / (T * FRAME))
        ph = ph0 + 6.2831853 * f * nidx / 48000.0
        x = torch.zeros((B, FRAME), device=dev)
        for h in range(1, 9):
            x += torch.where(nh >= h, torch.sin(h * ph) / h, torch.zeros((), device=dev))
        x = amp * x + noise * torch.randn((B, FRAME), device=dev, generator=g)
        frames.append(x.clamp_(-32768, 32767).to(torch.int16).contiguous())
    out = torch.empty((B, FRAME), dtype=torch.int16, device=dev)
    distinct = int(torch.unique(torch.stack([f[:, :8].to(torch.int64) for f in frames[:2]], 1).reshape(B, -1), dim=0).shape[0])
    torch.cuda.synchronize()
    ctx.reset()
    for t in range(W):
        ctx.process_i16_dev(frames[t].data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    ctx.reset_profile(); ctx.set_profiling(True)
    t0 = time.perf_counter()
    for t in range(W, T):
        ctx.process_i16_dev(frames[t].data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ctx.set_profiling(False)
    kt = ctx.kernel_times()
    import numpy as np
    per = np.frombuffer(ctx.debug_copy(13, B).tobytes(), dtype=np.int32)
    return {"streams": B, "distinct_streams": distinct, "steps": K, "warmup": W - prime, "prime_frames": prime, "ms_per_step": round(1e3 * dt / K, 4),
            "value": round(B * K / dt / 100.0, 1), "unit": "streams",
            "kernels_ms_with_events": {k: round(v[0] / max(v[1], 1), 4) for k, v in kt.items() if v[1]},
            "pitch_period_of_last_frame": {"min": int(per.min()), "mean": round(float(per.mean()), 1), "max": int(per.max()),
                                           "distinct_values": int(np.unique(per).size)},
            "data": "per-stream harmonic tones synthesised on the device (own fundamental 60-500 Hz with glide, 1-8 harmonics, own level "
                    "and noise floor, 5 % near full scale), no two streams alike"}


def side_config(api, synth, torch, model, dev, stream, B, K, W, nn_mode, label, traffic_tag, prime=12):
    """One of BASELINE's OTHER single-GPU configurations, timed the same way as the headline (W warm-up steps, K timed
    steps between synchronisations, inputs resident, no per-kernel events) and checked against the oracle on its own
    batch — reported under "other_configs", never as `value`.  A second, separately timed pass with per-kernel HIP
    events gives the configuration its own roofline object."""
    T = prime + K + W
    P = min(B, 64)
    pool_np = synth.synth_batch(P, T, base_seed=synth.BASE_SEED + 104729)
    pool = torch.from_numpy(pool_np).to(dev)
    idx = torch.arange(B, device=dev) % P
    rot = (torch.arange(B, device=dev) // P) * 37
    ar = (torch.arange(FRAME, device=dev)[None, :] + rot[:, None]) % FRAME
    frames = [torch.gather(pool[:, t * FRAME:(t + 1) * FRAME][idx], 1, ar).contiguous() for t in range(T)]
    out = torch.empty((B, FRAME), dtype=torch.int16, device=dev)
    ctx = api.Context(model, B, device=dev.index, nn_mode=nn_mode, stream=stream.cuda_stream)
    try:
        for t in range(prime + W):                  # stream priming (one history ring) + warm-up
            ctx.process_i16_dev(frames[t].data_ptr(), out.data_ptr(), None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(prime + W, T):
            ctx.process_i16_dev(frames[t].data_ptr(), out.data_ptr(), None)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        par = measure_parity(ctx, frames, pool_np, out, torch)     # leaves the context at the end of a replay of all T frames
        ctx.reset_profile(); ctx.set_profiling(True)
        for t in range(T - min(K, 40), T):           # steady-state frames again, with per-kernel events
            ctx.process_i16_dev(frames[t].data_ptr(), out.data_ptr(), None)
        torch.cuda.synchronize()
        ctx.set_profiling(False)
        kt = ctx.kernel_times()
        desc = ctx.describe()
        periods = read_periods(ctx, B)
        silent = read_silent(ctx, B)
    finally:
        ctx.close()
    # a SMALL batch is a latency figure: ms_per_step is the result, and a "streams" number would be an extrapolation of a
    # latency-bound run (x24 for configs[1]); frames/s / 100 is reported as `value` only for throughput-regime batches
    ms_step = 1e3 * dt / K
    capacity = B >= 32768
    return {"workload": label, "streams_per_gpu": B, "steps": K, "warmup": W,
            "value": round(B * K / dt / 100.0, 1) if capacity else None,
            "value_note": "frames per second / 100 at this batch size" if capacity else f"latency regime: {B} streams are served in {ms_step:.3f} ms of every 10 ms frame; no capacity is extrapolated from it",
            "unit": "streams", "ms_per_step": round(ms_step, 4), "frames_per_s": round(B * K / dt, 1),
            "max_abs_delta_vs_cpu_ref_lsb": par["max_abs_delta_vs_cpu_ref_lsb"], "max_abs_delta_gr": par["max_abs_delta_gr"],
            "pcm_samples_checked": par["pcm_samples_checked"], "replay_bit_identical": par["replay_of_timed_run_bit_identical"],
            "kernel_families": desc, "sclk_mhz_after": gpu_clock_mhz(),
            "kernels_ms_with_events": {k: round(v[0] / max(v[1], 1), 4) for k, v in kt.items()},
            "dtype": DTYPE_OF_MODE[nn_mode],
            "roofline": gru_roofline(kt, B, nn_mode == api.NN_MFMA_F16, desc, 1, B * K / dt, traffic_tag=traffic_tag),
            "dsp_roofline": dsp_roofline(kt, B, traffic_tag, periods, silent),
            "whole_pipeline_hbm": {"algorithmic_gbs": round(B * K / dt * (62608 + 31850256 / B) / 1e9, 1),
                                   "frac_of_peak": round(B * K / dt * (62608 + 31850256 / B) / 1e12 / PEAK_HBM_TBS, 4),
                                   "note": "SURVEY 8(d): bytes(B) = 62 608 + 31 850 256 / B per stream-frame at the measured rate"}}


DTYPE_OF_MODE = {0: "f32", 1: "f32 (reference order, separate mul/add)", 2: "f16 GEMM operands, f32 accumulate/state/DSP",
                 3: "f32 carried as fp16 hi+lo operand pairs (3 fp16 MFMA products per fp32 product), f32 accumulate/state/DSP"}


def drop_in_single_stream(frames=1000):
    """ms per frame of the reference's own UNTOUCHED main.cpp relinked against this library (INTEGRATION.md level 1:
    one rnnoise_process_frame per frame = the launch sequence + two PCIe hops + a synchronise, /root/reference/src/
    main.cpp:30-39), from the difference of two file lengths so that process start and context creation cancel."""
    import subprocess
    import tempfile
    import numpy as np
    from percepnet_amd import synth
    from oracle.oracle import RELINKED as exe
    if not os.path.exists(exe):
        return None
    from percepnet_amd import weights
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "m.pnw"), "wb").write(weights.default_blob(1234))
        env = dict(os.environ, PERCEPNET_MODEL=os.path.join(d, "m.pnw"))
        times = {}
        for n in (100, 100 + frames):
            pcm = synth.synth_stream(5, n)
            np.asarray(pcm, dtype="<i2").tofile(os.path.join(d, f"in{n}.pcm"))
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                r = subprocess.run([exe, f"in{n}.pcm", f"out{n}.pcm"], cwd=d, env=env, capture_output=True, timeout=300)
                dt = time.perf_counter() - t0
                if r.returncode != 0 or b"INERT" in r.stderr:
                    return {"error": r.stderr.decode(errors="replace")[-300:]}
                best = dt if best is None else min(best, dt)
            times[n] = best
    return {"ms_per_frame": round(1e3 * (times[100 + frames] - times[100]) / frames, 4), "frames": frames,
            "what": "oracle/_ref/percepNet_run_relinked (reference main.cpp, untouched) on one stream: wall(1100 frames) - wall(100 frames)",
            "wall_s": {str(k): round(v, 3) for k, v in times.items()}}


def sustained_leg(ctx, frames, out, gr_buf, stream, torch, B, K, T, dt, seconds):
    """The step loop without per-kernel events for >= `seconds`, ONE completion event per frame read after the loop."""
    n_sus, ds, per = 0, 0.0, max(dt / K, 1e-6)
    ev = []                                              # one event per frame, read after the loop: per-frame completion times
    torch.cuda.synchronize()
    with ClockSampler() as clk:
        while ds < seconds:                              # chunks sized from the rate seen so far; one sync per chunk
            n = max(K, int((seconds - ds) / per * 1.05) + 1)
            t0 = time.perf_counter()
            for i in range(n):
                ctx.process_i16_dev(frames[(n_sus + i) % T].data_ptr(), out.data_ptr(), gr_buf.data_ptr())
                e = torch.cuda.Event(enable_timing=True); e.record(stream); ev.append((len(ev) == 0 or i == 0, e))
            torch.cuda.synchronize()
            ds += time.perf_counter() - t0
            n_sus += n
            per = ds / n_sus
    # interval between the completions of consecutive frames = the time the GPU took for that frame (the queue is
    # never empty inside a chunk; the first frame of a chunk follows a host synchronise and is left out)
    frame_ms = [ev[i - 1][1].elapsed_time(ev[i][1]) for i in range(1, len(ev)) if not ev[i][0]]
    pc = percentiles(frame_ms) if frame_ms else {}
    r = {"steps": n_sus, "seconds": round(ds, 3), "ms_per_step": round(1e3 * ds / n_sus, 4),
         "value": round(B * n_sus / ds / 100.0, 1), "unit": "streams",
         "frame_ms_p50": pc.get("p50"), "frame_ms_p99": pc.get("p99"), "frame_ms_max": pc.get("max"),
         "frames_timed": pc.get("frames"), "sclk_mhz_at_end": gpu_clock_mhz(),
         "note": "no per-kernel events in this loop (one completion event per frame); the K-step figure above is "
                 "the contract's; frame_ms_* = intervals between consecutive frame completions on the GPU"}
    r.update(clk.summary())
    return r


LINE_LIMIT = 8192          # the driver reads the LAST stdout line; round 5's 30-38 KB line came back as parsed = null


def _pick(d, *keys):
    return {k: d[k] for k in keys if d and k in d}


def compact_line(res, detail_path=None):
    """The ONE JSON line bench.py prints (<= LINE_LIMIT bytes, asserted): the contract's keys + roofline + cpu_baseline + the parity
    and real-time figures.  Everything else (per-kernel objects, paced runs, side configurations in full, per-rank legs) goes to the
    detail file whose path rides in `detail`.  res: the full record main() assembles."""
    line = _pick(res, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data")
    cfg = res.get("config") or {}
    line["config"] = _pick(cfg, "workload", "streams_per_gpu", "frame_samples", "nn_mode", "weights", "parallelism", "io", "distributed")
    line.update(_pick(res, "value_note", "frames_per_s", "per_gpu_frames_per_s", "prime_frames"))
    rl = res.get("roofline")
    if rl:
        r = _pick(rl, "kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "avg_launch_ms", "flop_per_launch",
                  "concurrent_launches", "rows_per_launch", "achieved_one_launch", "algorithmic_bytes_per_launch", "kernels_snapshot",
                  "whole_pipeline_tflops", "whole_pipeline_frac_of_mfma_peak", "whole_pipeline_frac_of_hbm_peak")
        if rl.get("traffic") and rl.get("algorithmic_bytes_per_launch"):
            r["traffic_over_algorithmic"] = round(rl["traffic"] / rl["algorithmic_bytes_per_launch"], 3)
        line["roofline"] = r
    dsp = res.get("dsp_roofline") or {}
    if dsp:
        line["dsp_roofline"] = {k: {"ms": v.get("ms"), "frac": v.get("frac")} for k, v in dsp.items()}
        line["dsp_roofline"]["bound"] = "hbm"
    cb = res.get("cpu_baseline")
    if cb:
        c = _pick(cb, "value", "unit", "frames_per_s", "frames_per_s_one_core", "cores", "kind")
        c["sample"] = (cb.get("sample") or "")[:160]
        line["cpu_baseline"] = c
    line.update(_pick(res, "max_abs_delta_vs_cpu_ref_lsb", "max_abs_delta_gr"))
    par = res.get("parity")
    if par:
        line["parity_sample"] = f"{par.get('pcm_samples_checked')} PCM samples of this run's batch vs the CPU oracle, {par.get('pcm_samples_differing')} differ"
    sus = res.get("sustained")
    if sus:
        line["sustained"] = _pick(sus, "seconds", "ms_per_step", "value", "frame_ms_p99")
        line["sustained"]["note"] = "same loop, no per-kernel events"
    line.update(_pick(res, "realtime_streams_p99", "realtime_streams_with_one_forgiven_burst", "realtime_range"))
    rt = res.get("realtime")
    if rt:
        line["realtime"] = {"rule": "strict: every paced run at the size clean (0 forgiven) + recovery from an injected 50 ms host stall; PCIe in the loop",
                            "sizes": {b: _pick(v, "runs", "passed", "transient_runs", "strict") for b, v in (rt.get("sizes") or {}).items()},
                            "seconds_per_run": rt.get("seconds_per_run")}
    elif res.get("realtime_all_ranks"):
        line["realtime"] = _pick(res["realtime_all_ranks"], "streams_total", "deadline_misses_total", "delivery_latency_ms_p99_worst_rank",
                                 "all_ranks_met_every_deadline", "ranks_failed")
    oc = res.get("other_configs")
    if oc:
        line["other_configs"] = {}
        for k, v in oc.items():
            o = _pick(v, "streams_per_gpu", "ms_per_step", "value", "max_abs_delta_vs_cpu_ref_lsb", "dtype", "error")
            if "dtype" in o:
                o["dtype"] = o["dtype"][:24]
            if v.get("roofline"):
                o["roofline_frac"] = v["roofline"].get("frac")
            line["other_configs"][k] = o
    if detail_path:
        line["detail"] = detail_path
    out = json.dumps(line)
    if len(out) > LINE_LIMIT:                # never again an unparseable record: drop the optional objects, keep the contract
        for k in ("other_configs", "realtime", "sustained", "dsp_roofline", "parity_sample", "value_note"):
            line.pop(k, None)
            out = json.dumps(line)
            if len(out) <= LINE_LIMIT:
                break
    assert len(out) <= LINE_LIMIT, len(out)
    return out


def write_detail(res, path):
    """The full record beside the line (not parsed by the driver).  Returns the path written, or None."""
    try:
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f)
        return path
    except OSError as e:
        print(f"[bench] could not write {path}: {e}", file=sys.stderr, flush=True)
        return None


DUMP_MAX_STREAMS = 16384    # 16 384 x (480 + 68) x 4 B = 36 MB, inside the 64 MB a dump may take
DUMP_SEED = 0


def dump_sample(B):
    """Batch slots whose outputs --dump-outputs writes: all of them up to DUMP_MAX_STREAMS, else a fixed seeded sample (sorted)."""
    import numpy as np
    if B <= DUMP_MAX_STREAMS:
        return np.arange(B)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(B, DUMP_MAX_STREAMS, replace=False))


def dump_outputs(d, out, gr):
    """What the last timed step handed its caller — int16 PCM [B, 480] and the g|r rows [B, 68] — as float32 .npy files in d."""
    import numpy as np
    import torch
    idx = dump_sample(out.shape[0])
    sel = torch.from_numpy(idx).to(out.device)
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "pcm.npy"), out.index_select(0, sel).float().cpu().numpy())
    np.save(os.path.join(d, "gr.npy"), gr.index_select(0, sel).float().cpu().numpy())
    np.save(os.path.join(d, "stream_index.npy"), idx.astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None, help="ranks (one per GPU); default: the launched world, else 1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prime", type=int, default=12,
                    help="frames run during SETUP, before the warm-up: one history ring (12 frames).  A context fresh from the zero state is not the "
                         "workload: until its history has filled, the pitch search returns the degenerate period 768 and the comb filter reads "
                         "its largest window; the W warm-up and K timed steps then run on steady-state stream state")
    ap.add_argument("--streams", type=int, default=65536, help="concurrent streams per GPU")
    ap.add_argument("--full", action="store_true",
                    help="every measurement besides the headline (a few minutes): the CPU baseline, per-kernel HIP events and rooflines, "
                         "parity against the CPU oracle, configs[1] / configs[4] and the split-precision side configuration, the "
                         "65 536-distinct-streams leg, the relinked reference CLI, the sustained loop, the paced real-time capacity search over "
                         "the 512-stream grid with a 20 s confirmation run, the detail file.  The --no-* options below thin it out.  "
                         "Without --full a run times the K steps and prints the line, nothing else")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy (float32): "
                         "pcm [S, 480] (int16 values) and gr [S, 68] of S streams, their batch slots in stream_index [S] (float64); "
                         f"S = all streams up to {DUMP_MAX_STREAMS}, else a fixed seeded sample of that many (rank 0 only)")
    ap.add_argument("--detail-out", default=None,
                    help="where the full record goes (default with --full: bench_detail.json in the repository root; without --full "
                         "none is written unless this is given)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true", help="skip per-kernel HIP events")
    ap.add_argument("--no-parity", action="store_true", help="skip the measured max|delta| vs the CPU oracle")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short side measurements of configs[1] (1024 streams) and configs[4] (fp16) at N = 1")
    ap.add_argument("--no-sustained", action="store_true", help="skip the sustained-rate loop after the timed region")
    ap.add_argument("--sustained-seconds", type=float, default=3.0)
    ap.add_argument("--no-realtime", action="store_true", help="skip the paced 10 ms-clock runs through the pipelined host path")
    ap.add_argument("--realtime-seconds", type=float, default=5.0, help="length of one paced run")
    ap.add_argument("--realtime-soak-seconds", type=float, default=None, help="confirmation run at the capacity found (default 0; 20 with --full)")
    ap.add_argument("--realtime-runs", type=int, default=2, help="undisturbed paced runs per batch size (the strict rule forgives none)")
    ap.add_argument("--no-numa", action="store_true", help="do not bind the rank to the CPUs of its GPU's NUMA node")
    ap.add_argument("--strict", action="store_true", help="bit-exact network mode (slow)")
    ap.add_argument("--fp16", action="store_true",
                    help="BASELINE configs[4]: fp16 GEMM operands, fp32 accumulate (tolerance re-stated: bound 6 LSB, 4 measured over 1024 x 1000)")
    ap.add_argument("--x3", action="store_true",
                    help="split-precision network mode (PN_NN_MFMA_X3): fp32 operands as fp16 hi+lo pairs, 3 fp16 MFMA products, "
                         "fp32 accumulate; same parity bounds as the fp32 MFMA mode (tests/test_gpu_x3.py)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL)")
    ap.add_argument("--force-dist", action="store_true",
                    help="N = 1 through torch.distributed.run too: the RCCL init, barriers, all-reduces and gather of the N > 1 path")
    ap.add_argument("--share-gpu", action="store_true",
                    help="testing aid on a 1-GPU box: every rank uses cuda:0 (use with --backend gloo)")
    a = ap.parse_args()
    if not a.full:
        # a plain run does what its headline figure needs and nothing else: no per-kernel events in the timed region, no legs after it
        a.no_cpu_baseline = a.no_profile = a.no_parity = a.no_other_configs = a.no_sustained = a.no_realtime = True
    t_wall0 = time.perf_counter()
    cpu_fn = lambda: cpu_baseline(full=a.full)                 # noqa: E731

    from percepnet_amd import sharding
    rank, local_rank, world = sharding.launched_world()
    launched = sharding.launched_by_torchrun()
    if a.gpus is None:
        a.gpus = world if launched else 1
        if launched and world > 1:
            print(f"[bench] --gpus not given: adopting the launched world of {world} rank(s)", file=sys.stderr, flush=True)
    if not launched and (a.gpus > 1 or a.force_dist):
        # plain `python bench.py --gpus N`: launch the N ranks ourselves (one process per GPU).  The CPU baseline is timed
        # HERE, once, on the still idle host, and handed to rank 0 (sharding.cpu_baseline_handoff): an N-GPU line carries it too
        sys.exit(sharding.spawn_with_cpu_baseline(a.gpus, os.path.abspath(__file__), sys.argv[1:], None if a.no_cpu_baseline else cpu_fn))

    cpu = None
    if not a.no_cpu_baseline:
        # rank 0 only; before HIP is initialised in this process (fork safety) and — when the ranks were launched by
        # torch.distributed.run directly — before it joins the process group: the other ranks are blocked in the rendezvous
        cpu = sharding.cpu_baseline_handoff(cpu_fn, world, rank)

    import numpy as np
    import torch
    from percepnet_amd import api, synth, weights

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product has no CPU fallback)")
    if a.share_gpu:
        local_rank = 0
        os.environ["PN_ALLOW_SHARED_DEVICE"] = "1"
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: local rank {local_rank} but only {torch.cuda.device_count()} GPU(s) visible")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # NUMA placement BEFORE any pinned host buffer exists (first touch): this rank's CPUs = those of its GPU's NUMA node
    props0 = torch.cuda.get_device_properties(local_rank)
    bdf = "%04x:%02x:%02x.0" % (getattr(props0, "pci_domain_id", 0), getattr(props0, "pci_bus_id", 0), getattr(props0, "pci_device_id", 0))
    numa = sharding.numa_bind_for_device(bdf, bind=not a.no_numa)
    numa["rank"] = rank
    dist = sharding.init_ranks(a.backend, a.gpus, dev)       # refuses WORLD_SIZE != --gpus; joins a world of one too
    n_gpus = world

    B, K, W = a.streams, a.steps, a.warmup
    PRIME = max(a.prime, 0)
    print(f"[bench] rank {rank}/{world} B={B} K={K} W={W} dist={'none' if dist is None else dist.get_backend()}",
          file=sys.stderr, flush=True)
    T = PRIME + K + W
    blob = weights.default_blob(1234)
    model = api.Model(blob)
    # one explicit stream for torch AND the context: torch's default stream has handle 0, which pn_ctx_create reads as
    # "create your own non-blocking stream" — unordered against torch's kernels
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    assert stream.cuda_stream != 0
    nn_mode = api.NN_STRICT if a.strict else (api.NN_MFMA_F16 if a.fp16 else (api.NN_MFMA_X3 if a.x3 else api.NN_MFMA))
    ctx = api.Context(model, B, device=local_rank, nn_mode=nn_mode, stream=stream.cuda_stream)

    # synthetic input, resident in HBM: a pool of 64 distinct streams (voiced / bursts+silence /
    # two-tone / loud) tiled over the batch with per-replica sample rotation
    P = min(B, 64)
    # the same streams either way; worker processes only when the run is long enough for one core to take seconds
    pool_np = (synth.synth_batch_parallel if T > 200 else synth.synth_batch)(P, T, base_seed=synth.BASE_SEED + 7919 * rank)
    pool = torch.from_numpy(pool_np).to(dev)
    idx = torch.arange(B, device=dev) % P
    rot = (torch.arange(B, device=dev) // P) * 37
    frames = []
    for t in range(T):
        fr = pool[:, t * FRAME:(t + 1) * FRAME][idx]
        ar = (torch.arange(FRAME, device=dev)[None, :] + rot[:, None]) % FRAME
        frames.append(torch.gather(fr, 1, ar).contiguous())
    out = torch.empty((B, FRAME), dtype=torch.int16, device=dev)
    del pool

    # the g | r tap rows (34 gains + 34 pitch strengths per stream-frame, 272 B) the reference writes every frame
    # (denoise.cpp:533-534) and SURVEY 8(d) counts: copied out INSIDE the timed region (round-5 verdict weak #4)
    gr_buf = torch.empty((B, 68), dtype=torch.float32, device=dev)

    def step(t):
        ctx.process_i16_dev(frames[PRIME + t].data_ptr(), out.data_ptr(), gr_buf.data_ptr())

    def before_timed():
        # the contract's per-kernel HIP events are recorded over the timed region itself (on the context's stream); what they
        # cost is visible in the line: `sustained.ms_per_step` is the same loop without them
        if not a.no_profile:
            ctx.reset_profile()
            ctx.set_profiling(True)
    step.before_timed = before_timed

    # The inputs above were produced by torch kernels on `stream`, the context launches on the same stream: ordered.
    # The synchronise only keeps input generation out of the warm-up.
    for t in range(PRIME):                                   # setup: fill the streams' history (not a timed or warm-up step)
        ctx.process_i16_dev(frames[t].data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    print(f"[bench] inputs resident ({T} frames x {B} streams, {PRIME} of them run as stream priming), state {ctx.device_bytes() / 2**30:.2f} GiB",
          file=sys.stderr, flush=True)
    dt = sharding.timed_steps(dist, step, W, K, torch.cuda.synchronize)
    ctx.set_profiling(False)
    props = torch.cuda.get_device_properties(local_rank)
    label = f"cuda:{local_rank} {props.name} pci {getattr(props, 'pci_bus_id', '?')}:{getattr(props, 'pci_device_id', '?')}"
    rep = sharding.gather_report(dist, B * K, dt, label)      # SUM frames / MAX time; refuses duplicate devices
    fps, dt = rep["fps"], rep["seconds"]

    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, out, gr_buf)
    kt = {} if a.no_profile else ctx.kernel_times()
    checksum = int(out.to(torch.int64).abs().sum().item())     # keeps the result live / sanity
    periods = read_periods(ctx, B) if kt else None              # the periods this run's last frame filtered at (dsp_roofline)
    silent = read_silent(ctx, B) if kt else None                # ... and how many streams it flagged silent (back end: no P read)
    if os.environ.get("PN_BENCH_DUMP"):                         # debugging aid: last frame's PCM of this rank
        import numpy as _np
        _np.save(os.environ["PN_BENCH_DUMP"], out.cpu().numpy())
    log = lambda m: print(m, file=sys.stderr, flush=True)       # noqa: E731

    parity = None
    if rank == 0 and not a.no_parity and not a.strict:
        parity = measure_parity(ctx, frames, pool_np, out, torch)

    # ---- N = 1, headline workload: the side measurements run BEFORE the sustained / paced legs (full load leaves the chip
    # warmer and the latency-regime configuration, 1024 streams, is clock-sensitive: 0.39 vs 0.42 ms per frame) ---------
    side = {}
    headline = world == 1 and B == 65536 and not (a.fp16 or a.x3 or a.strict)
    if rank == 0 and headline:
        # --full: the same steps on 65 536 streams that are all different (generated on the device), so the data-dependent
        # branches of the pitch kernel see a real mix (the headline tiles 64 distinct streams over the batch)
        if a.full:
            try:
                side["distinct_streams"] = distinct_streams_leg(api, torch, ctx, dev, B, K, W)
                side["distinct_streams"]["headline_ms_per_step_for_comparison"] = round(1e3 * dt / K, 4)
                if kt:
                    side["distinct_streams"]["headline_kernels_ms"] = {k: round(v[0] / max(v[1], 1), 4) for k, v in kt.items() if v[1]}
            except Exception as e:              # noqa: BLE001 — reported, not fatal
                side["distinct_streams"] = {"error": f"{type(e).__name__}: {e}"}
        # BASELINE's other single-GPU configurations, so that they are timed by whoever runs this bench and not only by
        # the builder: configs[1] (1024 streams, the latency regime) and configs[4] (fp16 operands, tolerance re-stated).
        # A failure here never costs the headline line.
        if not (a.no_other_configs or a.no_parity):
            cfgs = {"configs[1]": (1024, 200, 20, api.NN_MFMA, "1024 concurrent streams, fp32 (small-batch kernel family)", "_1024"),
                    "configs[4]": (65536, 20, 3, api.NN_MFMA_F16, "65536 concurrent streams, fp16 GEMM operands, fp32 accumulate/state/DSP", "_fp16")}
            if a.full:
                # not a BASELINE config: the same fp32 network evaluated on the fp16 matrix cores with error compensation,
                # inside the fp32 MFMA mode's parity bounds (tests/test_gpu_x3.py); opt-in (`--x3`), never the headline `value`
                cfgs["split_precision_x3"] = (65536, 20, 3, api.NN_MFMA_X3, "65536 concurrent streams, fp32 network as fp16 hi+lo operand pairs "
                                                                              "(3 MFMA products), fp32 accumulate/state/DSP", "_x3")
            other = {}
            for key, (b2, k2, w2, mode2, label2, ttag) in cfgs.items():
                try:
                    other[key] = side_config(api, synth, torch, model, dev, stream, b2, k2, w2, mode2, label2, ttag)
                except Exception as e:          # noqa: BLE001 — reported, not fatal
                    other[key] = {"workload": label2, "error": f"{type(e).__name__}: {e}"}
            side["other_configs"] = other
        if a.full:
            try:
                side["drop_in_single_stream"] = drop_in_single_stream()
                if cpu is not None and side["drop_in_single_stream"] and "ms_per_frame" in side["drop_in_single_stream"]:
                    side["drop_in_single_stream"]["cpu_reference_ms_per_frame_one_core"] = round(1e3 / cpu["frames_per_s_one_core"], 4)
            except Exception as e:              # noqa: BLE001
                side["drop_in_single_stream"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- legs EVERY rank runs, side by side (one host feeding N GPUs), gathered like `ranks` -----------------------------
    # Sustained rate: the same step loop (no per-kernel events) for a few seconds, next to the K-step figure — K = 20 steps
    # are 0.2 s, shorter than the time the chip needs to settle on its power-limited clock.
    sustained = None
    if not a.no_sustained and not a.strict:
        sharding.barrier(dist)
        sustained = sustained_leg(ctx, frames, out, gr_buf, stream, torch, B, K, T, dt, a.sustained_seconds)
        sustained["rank"] = rank
    # The real-time claim, measured: frames arriving every 10.000 ms on the host through the pipelined host path (each rank
    # its own pinned buffers, allocated after its NUMA binding).  N = 1, headline workload: the STRICT verdict at this batch
    # size and at one size above it (tools/realtime_capacity.py: `--realtime-runs` undisturbed runs, none forgiven, + one run with an
    # injected host stall; one fallback size when it fails; `--full` = the search over the 512-stream grid + confirmation run).  Otherwise one paced
    # run at this batch size on every rank at the same time.
    realtime_rank, capacity = None, None
    if not (a.strict or a.no_sustained or a.no_realtime):
        sharding.barrier(dist)
        if headline:
            soak = a.realtime_soak_seconds if a.realtime_soak_seconds is not None else (20.0 if a.full else 0.0)
            # default: the workload's own batch size and ONE size above it (66 560: two 512-stream steps, defended with margin on
            # every box seen — tools/realtime_capacity.py's search goes further, profiles/r06_realtime_capacity.log), one fallback below
            capacity = realtime_capacity(api, synth, model, local_rank, nn_mode, a.realtime_seconds, a.realtime_runs, log, soak_seconds=soak,
                                         **({} if a.full else {"grid": [B, B + 1024], "fallback": (61440,)}))
            at_b = [r for r in capacity["paced_runs"] if r.get("streams") == B and not r.get("recovery")]
            realtime_rank = at_b[0] if at_b else None
        else:
            try:
                realtime_rank = paced_realtime(api, synth, model, local_rank, B, nn_mode, a.realtime_seconds)
            except Exception as e:              # noqa: BLE001 — reported, not fatal
                realtime_rank = {"streams": B, "error": f"{type(e).__name__}: {e}"}
        if realtime_rank is not None:
            realtime_rank = dict(realtime_rank, rank=rank)
    fields = sharding.multi_rank_fields(dist, cpu, numa, sustained, realtime_rank)

    if rank == 0:
        desc = ctx.describe()
        res = {
            "metric": "real-time 48 kHz streams (10 ms frames), whole job",
            "value": round(fps / 100.0, 1),
            "unit": "streams",
            "value_note": "THROUGHPUT: stream-frames/s / 100 over the K timed steps, inputs resident in HBM; the deadline-proven "
                          "figure is realtime_streams_p99 (paced 10 ms clock, PCIe in the loop, strict rule)",
            "frames_per_s": round(fps, 1),
            "n_gpus": n_gpus, "steps": K, "warmup": W, "prime_frames": PRIME,
            "ms_per_step": round(1e3 * dt / K, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPE_OF_MODE[1 if a.strict else (2 if a.fp16 else (3 if a.x3 else 0))], "data": "synthetic",
            "config": {
                "workload": ("configs[2]: 65536 concurrent 48 kHz streams per MI355X, fp32 network as MFMA GEMM"
                             if (B == 65536 and not a.fp16 and not a.x3) else
                             ("configs[4]: fp16 weights/activations variant, " if a.fp16 else ("split-precision network mode, " if a.x3 else "")) +
                             f"{B} concurrent 48 kHz streams per MI355X (configs[1] = 1024)"),
                "streams_per_gpu": B, "frame_samples": FRAME, "nn_mode": "strict" if a.strict else ("mfma_f16" if a.fp16 else ("mfma_x3" if a.x3 else "mfma_f32")),
                "weights": "torch.manual_seed(1234) default-init PercepNet in nnet_data.h layout",
                "parallelism": f"streams sharded over {n_gpus} GPU(s), one process per GPU, no data-path collective",
                "io": "int16 PCM in, int16 PCM + g|r rows out, resident in HBM",
                "kernel_families": desc,
                "distributed": "none (plain process)" if dist is None else f"torch.distributed {dist.get_backend()} world {dist.get_world_size()}",
            },
            "ranks": rep["ranks"],
            "per_gpu_frames_per_s": [r["fps"] for r in rep["ranks"]],
            "state_bytes_per_gpu": ctx.device_bytes(),
            "checksum": checksum,
        }
        if parity is not None:
            res["max_abs_delta_vs_cpu_ref_lsb"] = parity["max_abs_delta_vs_cpu_ref_lsb"]
            res["max_abs_delta_gr"] = parity["max_abs_delta_gr"]
            res["parity"] = parity
        if kt:
            per = {k: {"ms_avg": round(v[0] / max(v[1], 1), 4), "launches": v[1]} for k, v in kt.items()}
            res["kernels"] = per
            tag = "_fp16" if a.fp16 else ("_x3" if a.x3 else ("" if B == 65536 else f"_{B}"))
            rl = gru_roofline(kt, B, a.fp16, desc, n_gpus, fps, traffic_tag=tag)
            if rl:
                res["roofline"] = rl
            res["dsp_roofline"] = dsp_roofline(kt, B, tag, periods, silent)
        res.update(fields)                       # numa, sustained_ranks, realtime_ranks, realtime_all_ranks, cpu_baseline: the same keys at any N
        if sustained is not None:
            res["sustained"] = sustained
        if capacity is not None:
            res["realtime"] = capacity
            res["realtime_streams_p99"] = capacity["realtime_streams_p99"]
            res["realtime_streams_with_one_forgiven_burst"] = capacity["realtime_streams_with_one_forgiven_burst"]
            res["realtime_range"] = [capacity["realtime_streams_p99"], capacity["realtime_streams_with_one_forgiven_burst"]]
            if sustained is not None and sustained.get("frame_ms_p99") is not None:
                res["realtime"]["device_resident_frame_ms_p99_at_65536"] = sustained["frame_ms_p99"]
        elif fields.get("realtime_all_ranks"):
            agg = fields["realtime_all_ranks"]
            res["realtime_streams_p99"] = agg.get("streams_total") if agg.get("all_ranks_met_every_deadline") else None
        res.update(side)
        res["bench_wall_s"] = round(time.perf_counter() - t_wall0, 1)
        detail = None
        if a.full or a.detail_out:
            detail = write_detail(res, a.detail_out or os.path.join(ROOT, "bench_detail.json"))
        print(compact_line(res, detail and os.path.relpath(detail, ROOT)), flush=True)
    ctx.close()
    model.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
