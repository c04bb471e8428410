"""Times of the output limiter (DESIGN.md 4.8 "output limiter": the numbers there come from this script).

    python tools/rate_lim_times.py [streams] [launches] [rounds] [result.json]        defaults 65536 20 3, no file

Two converters, int16 rows: a single-rate one at 16000 and a mixed one with 8000 / 16000 / 24000 / 48000 by slot.
  copy      a device-to-device copy of [streams][480] float rows, timed with events through torch in the same run: the yardstick —
            the kernel with every row scaled moves exactly these bytes, each row read once and written once; a row that needs no gain
            is only read, half of them
  rate_lim  the converter's own profiling (pn_rate_set_profiling: HIP events around each launch on the context's stream; a figure is
            the MEAN of `launches` launches) of pn_rate_lim_f32 on its own with EVERY stream limited: nothing over the ceiling (rows
            read, none written), 10 % of the rows attacking (every tenth slot's ceiling under its row's peak), every row attacking,
            and every row holding (the level control's ramp).  The rows are copied afresh and, for the attacks, the converter's state
            is reset in front of every launch, outside the events: a second launch over the same rows would hold, not attack
  frame     wall time of `launches` whole frames (pn_rate_process_i16) behind one synchronise, per frame: with no ceiling ever set —
            and the launches the converter's own profiling counts for them ("rate_lim" must stay at zero) — with ceilings set and
            every one 0 again, with every stream limited and nothing over the ceiling, and with every row scaled
The cases take turns round by round; one warm-up round is thrown away; the median of the rounds with the smallest and largest.
With a library that has no limiter (PERCEPNET_LIB pointing at an older build) only the copy and the frames are measured: that is how
the parent's frame in DESIGN 4.8 is taken, in the same process setup — twice, for the spread between runs of the parent itself."""
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
LOW = np.float32(1.0 / 1024.0)                              # under every row's peak
# name -> (ceiling by slot, reset the state in front of every launch)
KERNEL_CASES = {"nothing over the ceiling": (lambda ids: np.full(ids.size, 1.0, np.float32), False),
                "10 % attacking": (lambda ids: np.where(ids % 10 == 0, LOW, np.float32(1.0)).astype(np.float32), True),
                "every row attacking": (lambda ids: np.full(ids.size, LOW, np.float32), True),
                "every row holding": (lambda ids: np.full(ids.size, LOW, np.float32), False)}


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def main():
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    has = hasattr(ctx.L, "pn_rate_set_stream_limiter")
    g = torch.Generator(device=DEV).manual_seed(1)
    t = torch.arange(480, device=DEV)[None, :]
    f0 = 90.0 + 160.0 * torch.rand((B, 1), device=DEV, generator=g)
    level = 10.0 ** (-2.5 + 2.0 * torch.rand((B, 1), device=DEV, generator=g))          # 0.003 .. 0.3: peaks between 1 / 1024 and 1
    y48 = (sum(torch.cos(2 * np.pi * k * f0 * t / 48000.0 + k) / k for k in range(1, 5)) * level).contiguous()
    peaks = y48.abs().amax(dim=1)
    assert float(peaks.min()) > float(LOW) and float(peaks.max()) < 1.0
    w48 = torch.empty_like(y48)
    xi = (torch.randn((B, 480), device=DEV, generator=g) * 8192).clamp(-32768, 32767).to(torch.int16)
    yi = torch.empty_like(xi)
    torch.cuda.synchronize()
    copy_ms = []
    for rnd in range(ROUNDS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(N):
            w48.copy_(y48)
        b.record()
        torch.cuda.synchronize()
        if rnd > 0:
            copy_ms.append(a.elapsed_time(b) / N)
    bound_ms = float(np.median(copy_ms))
    moved = 2 * 1920 * B
    result = {"streams": B, "launches_per_round": N, "rounds": ROUNDS, "library_has_limiter": has,
              "copy": dict(stat(copy_ms), bytes=moved, gb_per_s=moved / bound_ms / 1e6)}
    print(f"{B} streams, mean of {N} launches, median (min-max) of {ROUNDS} rounds, ms")
    print(f"  device-to-device copy of the rows: {bound_ms:.4f} ms = {moved / bound_ms / 1e6:.0f} GB/s for {moved} bytes")
    all_ids = np.arange(B, dtype=np.int32)
    families = ("rate_up", "rate_down", "rate_mix") + (("rate_lim",) if has else ())
    for label, make in (("16000", lambda: api.RateConverter(ctx, 16000)),
                        ("mixed", lambda: api.MixedRateConverter(ctx, np.array(api.MIXED_RATES, np.int32)[np.arange(B) % 4]))):
        rc = make()

        def frames():
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(N):
                rc.process_i16_dev(xi.data_ptr(), yi.data_ptr())
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / N

        def counted():
            rc.set_profiling(True)
            rc.reset_profile()
            frames()
            n = {k: n for k, (ms, n) in rc.kernel_times(families).items()}
            rc.set_profiling(False)
            return n

        cases = {"frame, no ceiling ever set": []}
        launched = {}
        for rnd in range(ROUNDS + 1):                       # before the first ceiling: what the parent launches
            ms = frames()
            if rnd > 0:
                cases["frame, no ceiling ever set"].append(ms)
        launched["no ceiling ever set"] = counted()
        if has:
            frame_cases = {"frame, every ceiling 0 again": np.zeros(B, np.float32), "frame, all limited, nothing over": np.full(B, 1.0, np.float32),
                           "frame, all limited, every row scaled": np.full(B, LOW, np.float32)}
            for name in frame_cases:
                cases[name] = []
            for name in KERNEL_CASES:
                cases[f"rate_lim {name}"] = []
            for rnd in range(ROUNDS + 1):
                for name, ceil in frame_cases.items():
                    rc.set_stream_limiter(all_ids, ceil)
                    rc.reset()
                    ms = frames()
                    if rnd > 0:
                        cases[name].append(ms)
                for name, (ceil, fresh) in KERNEL_CASES.items():
                    rc.set_stream_limiter(all_ids, ceil(all_ids))
                    rc.reset()
                    if not fresh:                           # one launch outside the timing: the state the case is about
                        w48.copy_(y48)
                        rc.lim_f32_dev(w48.data_ptr())
                    rc.set_profiling(True)
                    rc.reset_profile()
                    for _ in range(N):
                        w48.copy_(y48)
                        if fresh:
                            rc.reset()
                        torch.cuda.synchronize()
                        ctx.synchronize()
                        rc.lim_f32_dev(w48.data_ptr())
                    ms, n = rc.kernel_times(("rate_lim",))["rate_lim"]
                    assert n == N
                    rc.set_profiling(False)
                    if rnd > 0:
                        cases[f"rate_lim {name}"].append(ms / n)
            rc.set_stream_limiter(all_ids, np.zeros(B, np.float32))
            launched["every ceiling 0 again"] = counted()
            rc.set_stream_limiter(all_ids, np.full(B, 1.0, np.float32))
            launched["all limited"] = counted()
        res_rc = {}
        print(f" converter {label}:")
        for name, v in cases.items():
            res = stat(v)
            line = f"  {name:40s} {res['median_ms']:.4f} ({res['min_ms']:.4f}-{res['max_ms']:.4f})"
            if name.startswith("rate_lim"):
                res["times_the_copy"] = res["median_ms"] / bound_ms
                line += f"   {res['times_the_copy']:.2f} x the copy"
            res_rc[name] = res
            print(line)
        res_rc["launches_in_%d_frames" % N] = launched
        print(f"  launches in {N} frames: {launched}")
        result[label] = res_rc
        rc.close()
    ctx.close()
    model.close()
    if OUT:
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
