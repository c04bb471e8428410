"""Times of the mixed rate converter's kernels next to the single-rate ones, and of one mixed context next to one context per
rate (DESIGN.md 4.8 "Mixed rates": the numbers there come from this script).

    python tools/rate_mixed_times.py [streams] [launches] [warmup] [result.json]        defaults 65536 50 5, no file

Method of DESIGN 4.8: HIP events around SINGLE launches on the context's stream, median of `launches` after `warmup`; the spread
of a kernel is the largest of its launches over its median.  Parts:
  uniform      every stream at 8 kHz / at 24 kHz: the mixed kernels against the single-rate kernels of the same process, the two
               taking turns launch by launch
  interleaved  rates 8000 / 16000 / 24000 / 48000 by slot (every block diverges four ways), and the same population sorted by rate
  contexts     3/4 of `streams` split evenly over 8, 16 and 24 kHz: ONE mixed converter on one context against THREE single-rate
               pairs of a third each that submit one frame each per tick; wall clock per tick (submit all, synchronise all),
               device rows, float
Prints a table; with a fourth argument the figures also go to that file as JSON."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from percepnet_amd import api, weights  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 5
OUT = sys.argv[4] if len(sys.argv) > 4 else None
DEV = "cuda:0"


def stats(ms):
    ms = np.asarray(ms[WARM:])
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(ms.min()), "max_ms": float(ms.max()), "max_over_median": float(ms.max() / med)}


_busy = None


def time_launches(stream, calls):
    """ms between two events around each of `calls` on `stream`, the calls taking turns launch by launch, so that whatever else
    the machine does meets all of them alike -> one stats() per call.  A 512 MB fill is queued in front of every launch, so that
    both events and the launch are in the queue before the GPU reaches them: the interval holds the kernel and not the host's
    launch path."""
    global _busy
    if _busy is None:
        _busy = torch.empty(128 << 20, dtype=torch.float32, device=DEV)
    out = [[] for _ in calls]
    for _ in range(WARM + N):
        for k, call in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                _busy.zero_()
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return [stats(o) for o in out]


def kernel_times(named, stream):
    """named: {title: (converter, samples per low-rate row)} -> {title: {kernel: stats}}, the converters taking turns"""
    g = torch.Generator(device=DEV).manual_seed(1)
    x48 = torch.rand((B, 480), device=DEV, generator=g) * 2 - 1
    y48 = torch.empty_like(x48)
    buf = {}
    for row in {row for _, row in named.values()}:
        xf = torch.rand((B, row), device=DEV, generator=g) * 2 - 1
        xi = torch.randint(-32768, 32768, (B, row), device=DEV, generator=g, dtype=torch.int32).to(torch.int16)
        buf[row] = (xf, xi, torch.empty_like(xf), torch.empty_like(xi))
    torch.cuda.synchronize()
    res = {t: {} for t in named}
    kernels = {"up f32": lambda rc, b: rc.up_f32_dev(b[0].data_ptr(), y48.data_ptr()),
               "up i16": lambda rc, b: rc.up_i16_dev(b[1].data_ptr(), y48.data_ptr()),
               "down f32": lambda rc, b: rc.down_f32_dev(x48.data_ptr(), b[2].data_ptr()),
               "down i16": lambda rc, b: rc.down_i16_dev(x48.data_ptr(), b[3].data_ptr())}
    for name, launch in kernels.items():
        calls = [(lambda rc=rc, row=row: launch(rc, buf[row])) for rc, row in named.values()]
        for t, st in zip(named, time_launches(stream, calls)):
            res[t][name] = st
    torch.cuda.synchronize()
    return res


def show(title, res):
    print(title)
    for k, v in res.items():
        print(f"  {k:9s} median {v['median_ms']:.4f} ms   min {v['min_ms']:.4f}   max {v['max_ms']:.4f}   max/median {v['max_over_median']:.3f}")
    sys.stdout.flush()


def main():
    model = api.Model(weights.default_blob(1234))
    result = {"streams": B, "launches": N, "warmup": WARM}
    stream = torch.cuda.Stream(device=DEV)
    ctx = api.Context(model, B, stream=stream.cuda_stream)
    # ---- uniform rates: mixed against single-rate, same process, launch by launch in turns
    ids = np.arange(B, dtype=np.int32)
    inter = np.array(api.MIXED_RATES, np.int32)[ids % 4]
    for rate in (8000, 24000):
        single = api.RateConverter(ctx, rate)
        named = {f"single-rate {rate} Hz": (single, single.frame),
                 f"mixed, all streams at {rate} Hz": (api.MixedRateConverter(ctx, np.full(B, rate, np.int32)), 480)}
        if rate == 24000:                     # ---- the four rates by slot (every block diverges four ways), and sorted by rate
            named["mixed, 8000 / 16000 / 24000 / 48000 interleaved"] = (api.MixedRateConverter(ctx, inter), 480)
            named["mixed, 8000 / 16000 / 24000 / 48000 sorted"] = (api.MixedRateConverter(ctx, np.sort(inter)), 480)
        for title, r in kernel_times(named, stream).items():
            show(f"{title}, {B} streams", r)
            result[title] = r
        for rc, _ in named.values():
            rc.close()
    ctx.close()
    # ---- one mixed context against one context per rate
    per = (B * 3 // 4) // 3
    rates3 = (8000, 16000, 24000)
    g = torch.Generator(device=DEV).manual_seed(2)

    def ticks(submit, sync):
        out = []
        for _ in range(WARM + N):
            sync()
            t0 = time.perf_counter()
            submit()
            sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return stats(out)

    one = api.Context(model, 3 * per)
    rc = api.MixedRateConverter(one, np.repeat(np.array(rates3, np.int32), per))
    x = torch.rand((3 * per, 480), device=DEV, generator=g) * 2 - 1
    y, gr = torch.empty_like(x), torch.empty((3 * per, 68), device=DEV)
    torch.cuda.synchronize()
    r1 = ticks(lambda: rc.process_f32_dev(x.data_ptr(), y.data_ptr(), gr.data_ptr()), one.synchronize)
    rc.close(); one.close()
    pairs = []
    for rate in rates3:
        c = api.Context(model, per)
        k = api.RateConverter(c, rate)
        xi = torch.rand((per, k.frame), device=DEV, generator=g) * 2 - 1
        pairs.append((c, k, xi, torch.empty_like(xi), torch.empty((per, 68), device=DEV)))
    torch.cuda.synchronize()

    def submit3():
        for c, k, xi, yi, gi in pairs:
            k.process_f32_dev(xi.data_ptr(), yi.data_ptr(), gi.data_ptr())

    def sync3():
        for c, *_ in pairs:
            c.synchronize()
    r3 = ticks(submit3, sync3)
    for c, k, *_ in pairs:
        k.close(); c.close()
    res = {"one mixed context": r1, "three single-rate pairs": r3}
    show(f"ms per tick of {3 * per} streams split evenly over 8, 16 and 24 kHz (device rows, f32, wall clock)", res)
    print(f"  ratio one / three = {r1['median_ms'] / r3['median_ms']:.3f}")
    result["contexts"] = {"streams": 3 * per, "one_mixed": r1, "three_pairs": r3, "ratio": r1["median_ms"] / r3["median_ms"]}
    if OUT:
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)
    model.close()


if __name__ == "__main__":
    main()
