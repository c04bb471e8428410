"""Times of the comfort-noise stage (DESIGN.md 4.8 "comfort noise": the numbers there come from this script).

    python tools/rate_cng_times.py [streams] [launches] [rounds] [result.json]        defaults 65536 20 3, no file

A mixed converter with 8000 / 16000 / 24000 / 48000 by slot, int16 rows, SIDs of order 12 (the longest lattice).
  copy      a device-to-device copy of the silent streams' low-rate rows, timed with events through torch: what moving the rows costs
  frame     wall time of `launches` whole frames (pn_rate_process_i16) behind one synchronise, per frame: with comfort noise never
            enabled, enabled and nobody marked, and with 10 % and 40 % of the streams marked silent in front of every frame
  rate_cng  the converter's own profiling (pn_rate_set_profiling: HIP events around each launch; the MEAN of the launches) of the kernel
  rate_up   ... and of the up-conversion launches of the same frames: one a frame with nobody marked, two otherwise
The cases take turns round by round; one warm-up round is thrown away; the median of the rounds with the smallest and largest.
With a library that has no comfort noise (PERCEPNET_LIB pointing at an older build) only the first frame case is measured: that is how
a parent's frame is taken in the same process setup."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from percepnet_amd import api, weights  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
OUT = sys.argv[4] if len(sys.argv) > 4 else None
DEV = "cuda:0"
FRACTIONS = (0.0, 0.10, 0.40)


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def main():
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    rates = np.array(api.MIXED_RATES, np.int32)[np.arange(B) % 4]
    rc = api.MixedRateConverter(ctx, rates)
    has = hasattr(ctx.L, "pn_rate_set_cng")
    g = torch.Generator(device=DEV).manual_seed(1)
    xi = (torch.randn((B, 480), device=DEV, generator=g) * 8192).clamp(-32768, 32767).to(torch.int16)
    yi = torch.empty_like(xi)
    torch.cuda.synchronize()
    rng = np.random.default_rng(2)
    marks = {f: np.sort(rng.choice(B, int(round(f * B)), replace=False)).astype(np.int32) for f in FRACTIONS if f}

    def frames(silent=None):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            if silent is not None:
                rc.set_silent(silent)
            rc.process_i16_dev(xi.data_ptr(), yi.data_ptr())
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / N

    cases = {"frame, CNG never on": []}
    for rnd in range(ROUNDS + 1):                       # before the first enable: what the parent launches
        ms = frames()
        if rnd > 0:
            cases["frame, CNG never on"].append(ms)
    result = {"streams": B, "launches_per_round": N, "rounds": ROUNDS, "library_has_cng": has}
    if has:
        rc.set_cng(True)
        sid = api.cng_sid(40, [7, 220, 90, 150, 110, 140, 120, 135, 125, 130, 127, 128])
        for at in range(0, B, 16384):
            ids = np.arange(at, min(at + 16384, B), dtype=np.int32)
            rc.set_stream_sid(ids, np.tile(sid, (ids.size, 1)))
        for f in FRACTIONS:
            name = f"{100 * f:g} % silent"
            for k in ("frame, CNG on, ", "rate_cng, ", "rate_up per launch, ", "copy of the rows, "):
                cases[k + name] = []
        for rnd in range(ROUNDS + 1):
            for f in FRACTIONS:
                name = f"{100 * f:g} % silent"
                ms = frames(marks.get(f))
                rc.set_profiling(True)
                rc.reset_profile()
                frames(marks.get(f))
                t = rc.kernel_times(("rate_cng", "rate_up"))
                rc.set_profiling(False)
                assert t["rate_cng"][1] == (N if f else 0) and t["rate_up"][1] == (2 * N if f else N)
                copy = 0.0
                if f:                                     # the rows the kernel writes, as a plain copy (4 bytes a sample, the streams' own lengths)
                    words = int(sum(api.rate_mixed_frame_samples(int(r)) for r in rates[marks[f]]))
                    src = torch.empty(words, device=DEV, dtype=torch.float32)
                    dst = torch.empty_like(src)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(N):
                        dst.copy_(src)
                    b.record()
                    torch.cuda.synchronize()
                    copy = a.elapsed_time(b) / N
                if rnd > 0:
                    cases["frame, CNG on, " + name].append(ms)
                    cases["rate_cng, " + name].append(t["rate_cng"][0] / max(t["rate_cng"][1], 1))
                    cases["rate_up per launch, " + name].append(t["rate_up"][0] / t["rate_up"][1])
                    cases["copy of the rows, " + name].append(copy)
    print(f"{B} streams, mean of {N} launches, median (min-max) of {ROUNDS} rounds, ms")
    for name, v in cases.items():
        result[name] = stat(v)
        print(f"  {name:40s} {result[name]['median_ms']:.4f} ({result[name]['min_ms']:.4f}-{result[name]['max_ms']:.4f})")
    rc.close()
    ctx.close()
    model.close()
    if OUT:
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
