"""Times of the DTX send side (DESIGN.md 4.8 "DTX send side": the numbers there come from this script).

    python tools/rate_dtx_times.py [streams] [launches] [rounds] [result.json]        defaults 65536 20 3, no file

  rate_dtx  the converter's own profiling (pn_rate_set_profiling: HIP events around each launch; the MEAN of the launches) of the kernel on
            its own (pn_rate_dtx_i16 / pn_rate_dtx_f32): an 8000 Hz converter with int16 rows, every stream switched on and 10 % of them; a
            converter of all 48000 Hz with float rows, every stream.  "pause": quiet rows, no frame is active and the kernel forms all 13
            lags; "talk": loud rows behind a quiet one, every frame is active and the kernel forms r[0] alone
  copy      a device-to-device copy of the rows the kernel reads, timed with events through torch: what moving the rows costs
  frame     wall time of `launches` whole frames (pn_rate_process_i16 at 8000 Hz) behind one synchronise, per frame: with the stage never
            enabled, and with every stream switched on
The cases take turns round by round; one warm-up round is thrown away; the median of the rounds with the smallest and largest.
With a library that has no DTX send side (PERCEPNET_LIB pointing at an older build) only the first frame case is measured: that is how
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


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def copy_ms(t):
    dst = torch.empty_like(t)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(N):
        dst.copy_(t)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / N


def switch(rc, ids, on):
    for at in range(0, len(ids), 16384):
        rc.set_stream_dtx(ids[at:at + 16384], on)


def kernel_ms(ctx, rc, rows, fmt, talk=False):
    """the mean of N launches of the stage on its own behind one quiet row that sets the floor: over quiet rows (a pause: no frame is
    active, the kernel forms all 13 lags) or, talk, over loud ones (every frame is active: the kernel forms r[0] alone)"""
    quiet, loud = rows
    rc.dtx_dev(quiet.data_ptr(), fmt)
    rc.set_profiling(True)
    rc.reset_profile()
    for i in range(N):
        rc.dtx_dev((loud if talk else quiet).data_ptr(), fmt)
    t = rc.kernel_times(("rate_dtx",))["rate_dtx"]
    rc.set_profiling(False)
    assert t[1] == N
    return t[0] / N


def main():
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    has = hasattr(ctx.L, "pn_rate_set_stream_dtx")
    g = torch.Generator(device=DEV).manual_seed(1)
    every = np.arange(B, dtype=np.int32)
    tenth = np.sort(np.random.default_rng(2).choice(B, B // 10, replace=False)).astype(np.int32)
    result = {"streams": B, "launches_per_round": N, "rounds": ROUNDS, "library_has_dtx": has}
    cases = {}

    # ---- 8000 Hz, int16: whole frames, then the kernel alone
    rc = api.RateConverter(ctx, 8000)
    xi = (torch.randn((B, 80), device=DEV, generator=g) * 2048).clamp(-32768, 32767).to(torch.int16)
    yi = torch.empty_like(xi)
    torch.cuda.synchronize()

    def frames():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            rc.process_i16_dev(xi.data_ptr(), yi.data_ptr())
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / N

    cases["frame, 8000 Hz int16, DTX never on"] = []
    for rnd in range(ROUNDS + 1):                       # before the first enabling: what the parent launches
        ms = frames()
        if rnd > 0:
            cases["frame, 8000 Hz int16, DTX never on"].append(ms)
    if has:
        quiet = (torch.randn((B, 80), device=DEV, generator=g) * 33).to(torch.int16)      # -60 dBov
        rows8 = (quiet, xi)
        names = ("frame, 8000 Hz int16, every stream on", "rate_dtx, 8000 Hz int16, every stream on, pause", "rate_dtx, 8000 Hz int16, every stream on, talk",
                 "rate_dtx, 8000 Hz int16, 10 % on, pause", "copy of the rows, 8000 Hz int16, every stream", "copy of the rows, 8000 Hz int16, 10 %")
        for k in names:
            cases[k] = []
        tenth_rows = quiet[: B // 10].contiguous()
        for rnd in range(ROUNDS + 1):
            switch(rc, every, 1)
            v = [frames(), kernel_ms(ctx, rc, rows8, "i16")]
            switch(rc, every, 0)
            switch(rc, every, 1)
            v.append(kernel_ms(ctx, rc, rows8, "i16", talk=True))
            switch(rc, every, 0)
            switch(rc, tenth, 1)
            v.append(kernel_ms(ctx, rc, rows8, "i16"))
            switch(rc, every, 0)
            v += [copy_ms(quiet), copy_ms(tenth_rows)]
            if rnd > 0:
                for k, ms in zip(names, v):
                    cases[k].append(ms)
    rc.close()

    # ---- 48000 Hz, float: the kernel alone
    if has:
        rc = api.MixedRateConverter(ctx, np.full(B, 48000, np.int32))
        quiet = torch.randn((B, 480), device=DEV, generator=g) * 1e-3
        loud = torch.randn((B, 480), device=DEV, generator=g) * 0.1
        torch.cuda.synchronize()
        names = ("rate_dtx, 48000 Hz float, every stream on, pause", "rate_dtx, 48000 Hz float, every stream on, talk", "copy of the rows, 48000 Hz float, every stream")
        for k in names:
            cases[k] = []
        for rnd in range(ROUNDS + 1):
            switch(rc, every, 1)
            v = [kernel_ms(ctx, rc, (quiet, loud), "f32")]
            switch(rc, every, 0)
            switch(rc, every, 1)
            v += [kernel_ms(ctx, rc, (quiet, loud), "f32", talk=True), copy_ms(quiet)]
            switch(rc, every, 0)
            if rnd > 0:
                for k, ms in zip(names, v):
                    cases[k].append(ms)
        rc.close()
    print(f"{B} streams, mean of {N} launches, median (min-max) of {ROUNDS} rounds, ms")
    for name, v in cases.items():
        result[name] = stat(v)
        print(f"  {name:52s} {result[name]['median_ms']:.4f} ({result[name]['min_ms']:.4f}-{result[name]['max_ms']:.4f})")
    ctx.close()
    model.close()
    if OUT:
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
