"""Back-to-back frame times of the rate converter's pipelined host path next to its synchronous one, and the times of its two
kernels inside a frame (DESIGN.md 4.8 "Pipelined host path": the numbers there come from this script).

    python tools/rate_pipe_times.py [streams] [frames] [warmup] [result.json]        defaults 65536 60 10, no file

Every part runs in a child process of its own under a time limit of its own (PART_LIMIT_S), one after the other; the first part
that fails or runs out of time ends the run, and nothing more is started on the device.  Parts:
  single 8000   every stream at 8 kHz, int16: pn_rate_submit_host_i16 against pn_rate_process_host_i16 on the same pair
  mixed         8000 / 16000 / 24000 / 48000 by slot, int16 rows of 480: the same two entry points on one mixed pair
  context 48000 pn_submit_host_i16 of a plain context at the same batch size, for scale
Method: pinned buffers in three rotating sets; one time stamp when each call returns; a frame's time is the interval between two
consecutive returns (in steady state a pipelined submit returns when the frame two before it has been delivered, a synchronous
call when its own frame has).  Medians over `frames` intervals after `warmup`, with min and max.  The converter parts then run
`frames` more pipelined frames with pn_rate_set_profiling on (the context's own profiling stays off): rate_up / rate_down are the
totals of the HIP events around the two launches inside those frames divided by the launches — a mean, the converter's timing
keeps totals only."""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = ("single 8000", "mixed", "context 48000")
PART_LIMIT_S = 240


def stats(ms, warm):
    ms = np.asarray(ms[warm:])
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(ms.min()), "max_ms": float(ms.max()), "max_over_median": float(ms.max() / med)}


def part(name, B, N, WARM):
    from percepnet_amd import api, weights
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    L = ctx.L
    if name == "single 8000":
        rc = api.RateConverter(ctx, 8000)
    elif name == "mixed":
        rc = api.MixedRateConverter(ctx, np.array(api.MIXED_RATES, np.int32)[np.arange(B) % 4])
    else:
        rc = None
    row = rc.frame if rc else 480
    rng = np.random.default_rng(5)
    sets = []
    for k in range(3):
        p_in, p_out, p_gr = L.pn_host_alloc(B * row * 2), L.pn_host_alloc(B * row * 2), L.pn_host_alloc(B * 68 * 4)
        assert p_in and p_out and p_gr
        a = np.ctypeslib.as_array((ctypes.c_int16 * (B * row)).from_address(p_in))
        a[:] = np.rint(rng.standard_normal(B * row) * 8192).clip(-32768, 32767).astype(np.int16)      # about -12 dBFS
        sets.append((p_in, p_out, p_gr))

    def run(call, wait):
        stamps = [time.perf_counter()]
        for t in range(WARM + N):
            call(*sets[t % 3])
            stamps.append(time.perf_counter())
        wait()
        return stats(np.diff(stamps) * 1e3, WARM)

    res = {}
    if rc:
        rc.host_pipeline_prepare()
        res["pipelined"] = run(lambda i, o, g: rc.submit_host_i16(i, o, g), ctx.host_wait)
        res["synchronous"] = run(lambda i, o, g: rc._chk(L.pn_rate_process_host_i16(rc.h, i, o, g)), ctx.synchronize)
        res["pipelined_over_synchronous"] = res["pipelined"]["median_ms"] / res["synchronous"]["median_ms"]
        rc.set_profiling(True)
        for t in range(N):
            rc.submit_host_i16(*sets[t % 3])
        ctx.host_wait()
        for k, (ms, n) in rc.kernel_times().items():
            res[k] = {"mean_ms": ms / n, "launches": n}
        rc.close()
    else:
        ctx.host_pipeline_prepare()
        res["pipelined"] = run(lambda i, o, g: ctx.submit_host_i16(i, o, g), ctx.host_wait)
    res["pipe_streams"] = ctx.pipe_streams()
    ctx.close()
    for s in sets:
        for p in s:
            L.pn_host_free(p)
    model.close()
    return res


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--part":
        print("RESULT " + json.dumps(part(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))), flush=True)
        return 0
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    out = sys.argv[4] if len(sys.argv) > 4 else None
    result = {"streams": B, "frames": N, "warmup": WARM}
    rc = 0
    for name in PARTS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", name, str(B), str(N), str(WARM)],
                               capture_output=True, text=True, timeout=PART_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {PART_LIMIT_S} s; nothing more is started", flush=True)
            rc = 124
            break
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode or not line:
            print(f"{name}: exit status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}", flush=True)
            rc = r.returncode or 1
            break
        res = result[name] = json.loads(line[0][7:])
        print(f"{name}, {B} streams (copy streams: {res['pipe_streams']})")
        for k in ("pipelined", "synchronous"):
            if k in res:
                v = res[k]
                print(f"  {k:12s} median {v['median_ms']:.3f} ms per frame   min {v['min_ms']:.3f}   max {v['max_ms']:.3f}   max/median {v['max_over_median']:.3f}")
        if "pipelined_over_synchronous" in res:
            print(f"  pipelined / synchronous = {res['pipelined_over_synchronous']:.3f}")
        for k in ("rate_up", "rate_down"):
            if k in res:
                print(f"  {k:12s} mean {res[k]['mean_ms']:.4f} ms over {res[k]['launches']} launches inside pipelined frames")
        sys.stdout.flush()
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
