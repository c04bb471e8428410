"""Times of the DTMF detector (DESIGN.md 4.8 "DTMF detection": the numbers there come from this script).

    python tools/rate_dtmf_times.py [streams] [launches] [rounds] [result.json]        defaults 65536 20 3, no file

Two converters, int16 rows: a single-rate one at 16000 and a mixed one with 8000 / 16000 / 24000 / 48000 by slot.
  copy       a device-to-device copy of [streams][480] float rows, timed with events through torch in the same run: the yardstick.
             It reads and writes every row; the detector reads every row once and writes 112 bytes a row
  rate_dtmf  the converter's own profiling (pn_rate_set_profiling: HIP events around each launch on the context's stream; a figure is
             the MEAN of `launches` launches) of pn_rate_dtmf_f32 on its own, with every stream enabled and with 10 % enabled (every
             tenth slot).  The rows are a dual tone per stream in a little noise; the detector does not write them, so they stay
  rate_agc   pn_rate_agc_f32 with every stream levelled, in the same run and the same way (its rows copied afresh in front of every
             launch, outside the events): the kernel this one is built after, which also writes the row
  frame      wall time of `launches` whole frames (pn_rate_process_i16) behind one synchronise, per frame: with detection never
             enabled — and the launches the converter's own profiling counts for them ("rate_dtmf" must stay at zero) — then with
             every stream enabled
The cases take turns round by round; one warm-up round is thrown away; the median of the rounds with the smallest and largest.
With a library that has no detector (PERCEPNET_LIB pointing at an older build) only the copy and the frames are measured: that is
how the parent's frame in DESIGN 4.8 is taken, in the same process setup."""
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
SHARES = {"all enabled": 1, "10 % enabled": 10}          # every k-th slot is enabled
FREQS = (697, 770, 852, 941, 1209, 1336, 1477, 1633)


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def main():
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    has = hasattr(ctx.L, "pn_rate_set_stream_dtmf")
    g = torch.Generator(device=DEV).manual_seed(1)
    t = torch.arange(480, device=DEV)[None, :]
    digit = torch.arange(B, device=DEV)[:, None] % 16
    fr = torch.tensor(FREQS[:4], device=DEV, dtype=torch.float32)[digit // 4]
    fc = torch.tensor(FREQS[4:], device=DEV, dtype=torch.float32)[digit % 4]
    x48 = (0.1 * (torch.sin(2 * np.pi * fr * t / 48000.0) + torch.sin(2 * np.pi * fc * t / 48000.0)) + 0.005 * torch.randn((B, 480), device=DEV, generator=g)).contiguous()
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
    result = {"streams": B, "launches_per_round": N, "rounds": ROUNDS, "library_has_dtmf": has,
              "copy": dict(stat(copy_ms), bytes=moved, gb_per_s=moved / bound_ms / 1e6)}
    print(f"{B} streams, mean of {N} launches, median (min-max) of {ROUNDS} rounds, ms")
    print(f"  device-to-device copy of the rows: {bound_ms:.4f} ms = {moved / bound_ms / 1e6:.0f} GB/s for {moved} bytes")
    all_ids = np.arange(B, dtype=np.int32)
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

        def counted(names):
            rc.set_profiling(True)
            rc.reset_profile()
            frames()
            n = {k: n for k, (ms, n) in rc.kernel_times(names).items()}
            rc.set_profiling(False)
            return n

        def kernel(name, launch, refresh):
            rc.set_profiling(True)
            rc.reset_profile()
            for _ in range(N):
                if refresh:
                    w48.copy_(x48)
                    torch.cuda.synchronize()
                launch()
            ms, n = rc.kernel_times((name,))[name]
            assert n == N
            rc.set_profiling(False)
            return ms / n

        cases = {"frame, DTMF never on": []}
        launched = {}
        for rnd in range(ROUNDS + 1):                       # before the first enabling: what the parent launches
            ms = frames()
            if rnd > 0:
                cases["frame, DTMF never on"].append(ms)
        launched["DTMF never on"] = counted(("rate_up", "rate_down", "rate_mix") + (("rate_dtmf",) if has else ()))
        if has:
            rc.set_agc(True)
            rc.set_stream_agc_targets(all_ids, np.full(B, 0.1, np.float32))
            cases["frame, DTMF on, all enabled"] = []
            for share in SHARES:
                cases[f"rate_dtmf {share}"] = []
            cases["rate_agc all levelled"] = []
            for rnd in range(ROUNDS + 1):
                rc.set_stream_agc_targets(all_ids, np.zeros(B, np.float32))      # (the frames: no level control in them)
                rc.set_stream_dtmf(all_ids, np.ones(B, np.uint8))
                ms = frames()
                if rnd > 0:
                    cases["frame, DTMF on, all enabled"].append(ms)
                for share, k in SHARES.items():
                    rc.set_stream_dtmf(all_ids, (all_ids % k == 0).astype(np.uint8))
                    ms = kernel("rate_dtmf", lambda: rc.dtmf_f32_dev(x48.data_ptr()), False)
                    if rnd > 0:
                        cases[f"rate_dtmf {share}"].append(ms)
                rc.set_stream_agc_targets(all_ids, np.full(B, 0.1, np.float32))
                ms = kernel("rate_agc", lambda: rc.agc_f32_dev(w48.data_ptr()), True)
                if rnd > 0:
                    cases["rate_agc all levelled"].append(ms)
            rc.set_stream_agc_targets(all_ids, np.zeros(B, np.float32))
            rc.set_stream_dtmf(all_ids, np.ones(B, np.uint8))
            launched["DTMF on"] = counted(("rate_up", "rate_down", "rate_mix", "rate_agc", "rate_dtmf"))
        res_rc = {}
        print(f" converter {label}:")
        for name, v in cases.items():
            res = stat(v)
            line = f"  {name:30s} {res['median_ms']:.4f} ({res['min_ms']:.4f}-{res['max_ms']:.4f})"
            if name.startswith("rate_"):
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
