"""Times of the packet-loss concealer (DESIGN.md 4.8 "packet-loss concealment": the numbers there come from this script).

    python tools/rate_plc_times.py [streams] [launches] [rounds] [result.json]        defaults 65536 20 3, no file

A mixed converter with 8000 / 16000 / 24000 / 48000 by slot, int16 rows.
  copy      a device-to-device copy of [streams][480] float rows, timed with events through torch: the bandwidth the bound is taken at
  frame     wall time of `launches` whole frames (pn_rate_process_i16) behind one synchronise, per frame, with PLC never enabled —
            and the launches the converter's own profiling counts for them ("rate_plc" must stay at zero) — then with PLC on and
            nothing lost
  rate_plc  the converter's own profiling (pn_rate_set_profiling: HIP events around each launch on the context's stream; a figure is
            the MEAN of `launches` launches) of pn_rate_plc_f32 on its own with 0 %, 1 % and 10 % of the streams marked lost in
            front of every launch.  The marked streams are drawn anew for every launch, so nearly all of them are FIRST lost
            frames — the lag search and the period — and the streams lost the launch before cross-fade; the marks travel as one id list
            per launch, whose staging is outside the events
  bound     3840 bytes per received stream (its row read once, written once into the history) at the copy's bandwidth
The cases take turns round by round; one warm-up round is thrown away; the median of the rounds with the smallest and largest.
With a library that has no concealer (PERCEPNET_LIB pointing at an older build) only the copy and the frame are measured: that is
how the parent's frame in DESIGN 4.8 was taken, in the same process setup."""
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
FRACTIONS = (0.0, 0.01, 0.10)


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def main():
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    rc = api.MixedRateConverter(ctx, np.array(api.MIXED_RATES, np.int32)[np.arange(B) % 4])
    has = hasattr(ctx.L, "pn_rate_set_plc")
    g = torch.Generator(device=DEV).manual_seed(1)
    # voiced rows: a few harmonics of a pitch per stream in noise, so that the search has something to find
    t = torch.arange(480, device=DEV)[None, :]
    f0 = 90.0 + 160.0 * torch.rand((B, 1), device=DEV, generator=g)
    x48 = sum(torch.cos(2 * np.pi * k * f0 * t / 48000.0 + k) / k for k in range(1, 5)) * 0.15 + torch.randn((B, 480), device=DEV, generator=g) * 0.02
    w48 = torch.empty_like(x48)
    xi = (torch.randn((B, 480), device=DEV, generator=g) * 8192).clamp(-32768, 32767).to(torch.int16)
    yi = torch.empty_like(xi)
    torch.cuda.synchronize()
    copy_ms = []
    for rnd in range(ROUNDS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(N):
            w48.copy_(x48)
        b.record()
        torch.cuda.synchronize()
        if rnd > 0:
            copy_ms.append(a.elapsed_time(b) / N)
    bound_ms = float(np.median(copy_ms))
    moved = 2 * 1920 * B
    result = {"streams": B, "launches_per_round": N, "rounds": ROUNDS, "library_has_plc": has,
              "copy": dict(stat(copy_ms), bytes=moved, gb_per_s=moved / bound_ms / 1e6)}
    print(f"{B} streams, mean of {N} launches, median (min-max) of {ROUNDS} rounds, ms")
    print(f"  device-to-device copy of the rows: {bound_ms:.4f} ms = {moved / bound_ms / 1e6:.0f} GB/s for {moved} bytes")

    def frames():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            rc.process_i16_dev(xi.data_ptr(), yi.data_ptr())
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / N

    rng = np.random.default_rng(2)
    cases = {"frame, PLC never on": []}
    launched = {}
    for rnd in range(ROUNDS + 1):                       # before the first enable: what the parent launches
        ms = frames()
        if rnd > 0:
            cases["frame, PLC never on"].append(ms)
    if hasattr(ctx.L, "pn_rate_set_profiling"):
        names = ("rate_up", "rate_down", "rate_mix") + (("rate_plc",) if has else ())
        rc.set_profiling(True)
        rc.reset_profile()
        frames()
        launched["PLC never on"] = {k: n for k, (ms, n) in rc.kernel_times(names).items()}
        rc.set_profiling(False)
    if has:
        rc.set_plc(True)
        cases["frame, PLC on, none lost"] = []
        for f in FRACTIONS:
            cases[f"rate_plc {100 * f:g} % lost"] = []
        for rnd in range(ROUNDS + 1):
            ms = frames()
            if rnd > 0:
                cases["frame, PLC on, none lost"].append(ms)
            for f in FRACTIONS:
                k = int(round(f * B))
                rc.set_profiling(True)
                rc.reset_profile()
                for _ in range(N):
                    w48.copy_(x48)
                    torch.cuda.synchronize()
                    if k:
                        rc.set_lost(np.sort(rng.choice(B, k, replace=False)).astype(np.int32))
                    rc.plc_f32_dev(w48.data_ptr())
                ms, n = rc.kernel_times(("rate_plc",))["rate_plc"]
                assert n == N
                rc.set_profiling(False)
                if rnd > 0:
                    cases[f"rate_plc {100 * f:g} % lost"].append(ms / n)
        rc.set_profiling(True)
        rc.reset_profile()
        frames()
        launched["PLC on"] = {k: n for k, (ms, n) in rc.kernel_times(("rate_up", "rate_down", "rate_mix", "rate_plc")).items()}
        rc.set_profiling(False)
    for name, v in cases.items():
        res = stat(v)
        line = f"  {name:28s} {res['median_ms']:.4f} ({res['min_ms']:.4f}-{res['max_ms']:.4f})"
        if name.startswith("rate_plc"):
            res["fraction_of_bound"] = bound_ms / res["median_ms"]
            line += f"   bound / rate_plc {res['fraction_of_bound']:.2f}"
        result[name] = res
        print(line)
    result["launches_in_%d_frames" % N] = launched
    print(f"  launches in {N} frames: {launched}")
    rc.close()
    ctx.close()
    model.close()
    if OUT:
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
