"""bench.py's own launch paths on a real GPU (-m gpu): the single-rank line carries measured parity numbers, and
`--gpus 2` with WORLD_SIZE unset launches two ranks itself (both on cuda:0 here: --share-gpu, gloo) and reports
what really ran."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


LINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
             "data", "config")


def _bench(*args):
    """Runs bench.py --full; checks the ONE printed line (the driver's record: compact, complete, agreeing with the full record) and returns
    the full record from the detail file the line points at."""
    import tempfile
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    with tempfile.TemporaryDirectory() as d:
        detail = os.path.join(d, "detail.json")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--detail-out", detail, *args], capture_output=True, text=True,
                             timeout=900, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and out.stdout.rstrip().endswith(lines[0]), out.stdout[-2000:]
        assert len(lines[0]) < 8192, len(lines[0])
        line = json.loads(lines[0])
        full = json.load(open(detail))
    for k in LINE_KEYS:
        assert k in line and line[k] == (full[k] if k != "config" else {c: full[k][c] for c in line[k]}), k
    if "roofline" in full:
        assert line["roofline"]["frac"] == full["roofline"]["frac"] and line["roofline"]["bound"] in ("mfma", "hbm")
        assert set(line["roofline"]) >= {"achieved", "peak", "unit", "traffic"}
    if "cpu_baseline" in full:
        assert line["cpu_baseline"]["value"] == full["cpu_baseline"]["value"] and line["cpu_baseline"]["kind"] == full["cpu_baseline"]["kind"]
    return full


def test_single_rank_line_has_measured_parity_and_roofline():
    r = _bench("--streams", "2048", "--steps", "8", "--warmup", "2", "--no-cpu-baseline", "--sustained-seconds", "0.3", "--realtime-seconds", "0.6")
    assert r["n_gpus"] == 1 and len(r["ranks"]) == 1
    # fe_spec_out's algorithmic bytes follow from the run's own pitch periods (the worst case is kept beside them)
    so = r["dsp_roofline"]["fe_spec_out"]
    assert 60 <= so["pitch_period_mean"] <= 768 and so["algorithmic_bytes"] <= so["algorithmic_bytes_worst_case"]
    assert abs(so["algorithmic_bytes"] - 2048 * (so["comb_window_bytes_mean"] + 3200 + 288 + 3200 + 512 + 4)) < 2048
    # the per-rank legs and the NUMA record exist at N = 1 too (the same keys at any N)
    assert len(r["numa"]) == 1 and "numa_node" in r["numa"][0] and r["numa"][0]["pci"].count(":") == 2
    assert len(r["sustained_ranks"]) == 1 and len(r["realtime_ranks"]) == 1
    rt = r["realtime_ranks"][0]
    assert rt["streams"] == 2048 and rt["frames"] == 60 and rt["deadline_misses"] == 0 and rt["met_contract"] is True
    assert 0 < rt["delivery_latency_ms"]["p50"] <= rt["delivery_latency_ms"]["p99"] <= 20.0
    assert r["realtime_all_ranks"]["all_ranks_met_every_deadline"] is True and r["realtime_streams_p99"] == 2048
    assert "value_note" in r
    assert r["config"]["distributed"].startswith("none")
    assert "g|r rows out" in r["config"]["io"]                     # the tap rows are copied out inside the timed region
    assert r["sustained"]["steps"] >= 8 and r["sustained"]["seconds"] >= 0.3 and r["sustained"]["value"] > 0
    assert r["config"]["kernel_families"]["gru"] == "batch" and r["config"]["kernel_families"]["dense"] == "small"   # 2048 streams
    for k in ("fe_spec_in", "fe_pitch", "fe_spec_out", "backend"):       # one roofline object per DSP kernel
        assert r["dsp_roofline"][k]["bound"] == "hbm" and 0 < r["dsp_roofline"][k]["frac"] < 1, k
        assert "traffic" in r["dsp_roofline"][k] and r["dsp_roofline"][k]["kernel"].startswith("pn_")
    assert 0 < r["dsp_roofline"]["dsp_total"]["frac"] < 1
    assert r["sustained"]["frame_ms_p99"] >= r["sustained"]["frame_ms_p50"] > 0 and r["sustained"]["frames_timed"] >= 4
    assert isinstance(r["max_abs_delta_vs_cpu_ref_lsb"], int) and r["max_abs_delta_vs_cpu_ref_lsb"] <= 1
    assert r["max_abs_delta_gr"] <= 2e-5
    assert r["parity"]["replay_of_timed_run_bit_identical"] is True
    assert r["prime_frames"] == 12 and r["parity"]["pcm_samples_checked"] == 64 * (12 + 9) * 480
    assert r["roofline"]["bound"] == "mfma" and 0 < r["roofline"]["frac"] < 1
    assert abs(r["value"] * 100 - r["frames_per_s"]) < 10


def test_plain_run_times_the_steps_and_dumps_the_last_outputs(tmp_path):
    """Without --full: the line carries the headline (no legs after the timed steps, no detail file), --steps sets the timed
    steps, and --dump-outputs writes the last timed step's PCM and g|r rows — the same bits from run to run, and the same
    as the oracle gives for the pool streams in their unrotated slots."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    lines = []
    for i in range(2):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--streams", "128", "--steps", "7", "--warmup", "2",
                              "--dump-outputs", str(tmp_path / f"d{i}")], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        lines.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1]))
    r = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == 7 and r["warmup"] == 2 and r["ms_per_step"] > 0 and r["higher_is_better"] is True
    assert abs(r["value"] * 100 - 128 * 7 / (r["ms_per_step"] * 7e-3)) < 1e-2 * r["value"] * 100
    assert not {"cpu_baseline", "roofline", "dsp_roofline", "sustained", "realtime", "other_configs", "detail"} & set(r)
    d0, d1 = tmp_path / "d0", tmp_path / "d1"
    assert sorted(os.listdir(d0)) == ["gr.npy", "pcm.npy", "stream_index.npy"]
    for name in ("pcm", "gr", "stream_index"):
        a, b = np.load(d0 / f"{name}.npy"), np.load(d1 / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    pcm, gr = np.load(d0 / "pcm.npy"), np.load(d0 / "gr.npy")
    assert pcm.shape == (128, 480) and gr.shape == (128, 68) and np.array_equal(np.load(d0 / "stream_index.npy"), np.arange(128))
    assert np.array_equal(pcm, np.round(pcm)) and np.abs(pcm).max() <= 32768 and np.abs(pcm).max() > 0
    # slots 0..63 carry the 64 pool streams unrotated: the last timed step is frame 12 + 2 + 7 - 1 = 20, its PCM output frame 19
    from oracle.oracle import Oracle
    from percepnet_amd import synth, weights
    ro, rg, _, _ = Oracle(weights.default_blob(1234)).run_batch(synth.synth_batch(64, 21), want_feat=False)
    assert np.abs(pcm[:64] - ro[:, 19 * 480:20 * 480]).max() <= 1
    assert np.abs(gr[:64] - rg[:, 20]).max() <= 2e-5


def test_paced_real_time_run_through_the_pipelined_host_path():
    """tools/realtime_capacity.py paced_realtime: frames arrive on the host every 10 ms and go through pn_submit_host_i16 (copy-in / compute /
    copy-out on three streams, each copy stream probed to have a hardware queue of its own).  A small batch must meet every deadline, the
    submit call must return in well under a period, and the serial host call (copy + frame + copy) is reported for scale.
    The process owns other streams when it runs (torch's, a second context's), as bench.py's does."""
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import realtime_capacity as bench
    from percepnet_amd import api, synth, weights
    model = api.Model(weights.default_blob(1234))
    side = [torch.cuda.Stream() for _ in range(4)]          # noqa: F841 — streams that compete for HIP's hardware queues
    other = api.Context(model, 256)
    r = bench.paced_realtime(api, synth, model, 0, 4096, api.NN_MFMA, seconds=0.6)
    # the disturbed run: a 40 ms host stall at frame 10 — four frames arrive late at the pipeline; a batch this far below the
    # capacity is back on its clock within a few frames and misses nothing after that
    d = bench.paced_realtime(api, synth, model, 0, 4096, api.NN_MFMA, seconds=0.8, stall=(10, 40.0))
    other.close()
    rec = d["recovery"]
    assert rec["recovered"] is True and d["met_contract"] is True, rec
    assert 1 <= rec["frames_to_recover_submit_clock"] <= 12, rec           # the submit clock: four frames arrived late, back within a few
    assert rec["frames_to_recover_submit_clock"] <= rec["frames_to_recover"] <= 50, rec      # ... the last disturbed frame (deliveries included)
    assert rec["clean_frames_after_recovery"] >= 20 and 0 < rec["delivery_p99_ms_after_recovery"] <= 20.0, rec
    assert d["deadline_misses"] >= 1                        # the stall itself is a missed deadline: it is visible, not hidden
    # the copy streams: default priority and probed ("n"), or the priority fallback ("h" / "l"); back to back the pipeline runs well
    # inside a period at this size
    assert len(r["copy_streams"]) == 2 and set(r["copy_streams"]) <= set("nhl")
    assert 0 < r["host_pipeline_back_to_back_ms"] < 5.0
    assert r["frames"] == 60 and r["streams"] == 4096
    assert r["deadline_misses"] == 0 and r["submit_call_ms"]["p99"] < 5.0 and r["finished_behind_schedule_ms"] < 10.0
    assert 0 < r["serial_host_call_ms"] < 10.0
    # arrival-to-delivery latency per frame (polled between arrivals), not only back-pressure of the submit call
    assert r["delivery_latency_ms"]["frames"] == 60 and 0 < r["delivery_latency_ms"]["p50"] <= r["delivery_latency_ms"]["max"] < 20.0
    assert r["frames_delivered_late"] == 0 and r["met_contract"] is True


def test_split_precision_and_fp16_lines():
    """`--x3` and `--fp16`: the line names the mode, the dtype string says what is computed, the parity numbers are the
    run's own and inside the mode's bound, and the roofline is priced against the fp16 matrix peak (a third of it for the
    three-product mode)."""
    r = _bench("--x3", "--streams", "2048", "--steps", "6", "--warmup", "2", "--no-cpu-baseline", "--no-sustained")
    assert r["config"]["nn_mode"] == "mfma_x3" and "hi+lo" in r["dtype"]
    assert r["config"]["kernel_families"]["gru"] == "x3_rows32"
    assert r["max_abs_delta_vs_cpu_ref_lsb"] <= 1 and r["max_abs_delta_gr"] <= 2e-5
    assert abs(r["roofline"]["peak"] - 2500.0 / 3) < 0.1 and r["roofline"]["kernel"].startswith("pn_gru_x3_kernel")
    r = _bench("--fp16", "--streams", "2048", "--steps", "6", "--warmup", "2", "--no-cpu-baseline", "--no-sustained")
    assert r["config"]["nn_mode"] == "mfma_f16" and r["dtype"].startswith("f16")
    assert r["config"]["kernel_families"]["gru"] == "f16_rows32"
    assert r["max_abs_delta_vs_cpu_ref_lsb"] <= 6 and r["max_abs_delta_gr"] <= 1e-3
    assert r["roofline"]["peak"] == 2500.0


def test_two_ranks_self_launched():
    r = _bench("--gpus", "2", "--share-gpu", "--backend", "gloo", "--streams", "1024", "--steps", "5", "--warmup", "2",
               "--sustained-seconds", "0.3", "--realtime-seconds", "0.6")
    assert r["n_gpus"] == 2 and [x["rank"] for x in r["ranks"]] == [0, 1]
    assert all(x["stream_frames"] == 1024 * 5 for x in r["ranks"])
    assert abs(r["frames_per_s"] - 2 * 1024 * 5 / (r["ms_per_step"] * 5e-3)) < 1e-3 * r["frames_per_s"]
    _complete_multi_rank_record(r, 2, 1024)


def _complete_multi_rank_record(r, n, streams):
    """Round-4 verdict item 3: an N > 1 line is a COMPLETE record — the CPU baseline (timed once by the launcher parent), one
    sustained and one paced real-time object per rank with their aggregate, and each rank's NUMA placement."""
    assert r["cpu_baseline"]["kind"] in ("reference", "port") and r["cpu_baseline"]["value"] > 0 and r["cpu_baseline"]["cores"] >= 1
    assert [x["rank"] for x in r["numa"]] == list(range(n)) and all("numa_node" in x and "bound" in x for x in r["numa"])
    assert [x["rank"] for x in r["sustained_ranks"]] == list(range(n)) and all(x["ms_per_step"] > 0 for x in r["sustained_ranks"])
    assert [x["rank"] for x in r["realtime_ranks"]] == list(range(n))
    for x in r["realtime_ranks"]:
        assert x["streams"] == streams and x["frames"] == 60 and "deadline_misses" in x and x["delivery_latency_ms"]["frames"] == 60
    agg = r["realtime_all_ranks"]
    assert agg["streams_total"] == n * streams and len(agg["deadline_misses_per_rank"]) == n
    assert agg["deadline_misses_total"] == sum(x["deadline_misses"] for x in r["realtime_ranks"])


def test_world_of_one_through_rccl_carries_the_same_keys():
    """The same record through RCCL ("nccl") on the hardware this box has: `--force-dist` = one rank launched by
    torch.distributed.run, the CPU baseline handed over by the launcher parent, the per-rank legs gathered with
    all_gather_object over RCCL."""
    r = _bench("--force-dist", "--streams", "1024", "--steps", "5", "--warmup", "2", "--sustained-seconds", "0.3", "--realtime-seconds", "0.6", "--no-parity")
    assert r["config"]["distributed"] == "torch.distributed nccl world 1"
    _complete_multi_rank_record(r, 1, 1024)


def test_world_of_one_runs_the_rccl_path():
    """The N > 1 code path on the hardware this box has: `--force-dist` launches ONE rank through torch.distributed.run,
    which joins an RCCL ("nccl") process group bound to its device and goes through both barriers, both CUDA-tensor
    all-reduces and the object gather of sharding.py — the calls `bench.py --gpus 8` makes, first executed here and not
    inside the 8-GPU run.  Same work as the plain process: same checksum, rate within noise."""
    common = ("--streams", "2048", "--steps", "8", "--warmup", "2", "--no-cpu-baseline", "--no-sustained", "--no-parity")
    d = _bench("--force-dist", *common)
    assert d["n_gpus"] == 1 and len(d["ranks"]) == 1 and d["ranks"][0]["rank"] == 0
    assert d["config"]["distributed"] == "torch.distributed nccl world 1"
    p = _bench(*common)
    assert p["config"]["distributed"].startswith("none")
    assert d["checksum"] == p["checksum"]
    assert 0.6 < d["value"] / p["value"] < 1.6, (d["value"], p["value"])


def test_launched_world_is_adopted_without_the_flag():
    """torch.distributed.run --nproc-per-node=1 bench.py (no --gpus): the launched world is adopted, not refused."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                          "--master-port", "29631", os.path.join(ROOT, "bench.py"), "--streams", "1024", "--steps", "4", "--warmup", "1",
                          "--no-cpu-baseline", "--no-sustained", "--no-parity"], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["n_gpus"] == 1 and r["config"]["distributed"] == "torch.distributed nccl world 1"

