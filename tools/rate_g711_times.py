"""Times of the rate converter's kernels on G.711 rows next to int16 rows (DESIGN.md 4.8 "G.711 rows": the numbers there come
from this script).

    python tools/rate_g711_times.py [streams] [launches] [rounds] [result.json]        defaults 65536 50 5, no file

Method: the converter's own profiling (pn_rate_set_profiling: HIP events around each launch of the two kernels on the context's
stream; the converter keeps totals, so a figure is the MEAN of `launches` launches).  The two formats take turns round by round,
so that whatever else the machine does meets both alike; one warm-up round of each is thrown away; per format and kernel the
median of the rounds' means, with the smallest and largest round.  Converters: single-rate 8 kHz and 24 kHz (the sizes of the
table in DESIGN 4.8) and a mixed one with 8000 / 16000 / 24000 / 48000 by slot, laws alternating by stream.
Prints a table; with a fourth argument the figures also go to that file as JSON."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from percepnet_amd import api, weights  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
OUT = sys.argv[4] if len(sys.argv) > 4 else None
DEV = "cuda:0"


def measure(ctx, rc, row):
    g = torch.Generator(device=DEV).manual_seed(1)
    x48 = torch.rand((B, 480), device=DEV, generator=g) * 2 - 1
    y48 = torch.empty_like(x48)
    xi = torch.randint(-32768, 32768, (B, row), device=DEV, generator=g, dtype=torch.int32).to(torch.int16)
    xb = torch.randint(0, 256, (B, row), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    yi, yb = torch.empty_like(xi), torch.empty_like(xb)
    torch.cuda.synchronize()
    rc.set_stream_laws(np.arange(B, dtype=np.int32), np.arange(B, dtype=np.int32) % 2)
    launch = {"i16": lambda: (rc.up_i16_dev(xi.data_ptr(), y48.data_ptr()), rc.down_i16_dev(x48.data_ptr(), yi.data_ptr())),
              "g711": lambda: (rc.up_g711_dev(xb.data_ptr(), y48.data_ptr()), rc.down_g711_dev(x48.data_ptr(), yb.data_ptr()))}
    rc.set_profiling(True)
    means = {f: {"rate_up": [], "rate_down": []} for f in launch}
    for rnd in range(ROUNDS + 1):
        for fmt, call in launch.items():
            rc.reset_profile()
            for _ in range(N):
                call()
            for name, (ms, n) in rc.kernel_times().items():
                assert n == N
                if rnd > 0:
                    means[fmt][name].append(ms / n)
    rc.set_profiling(False)
    ctx.synchronize()
    return {f: {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in d.items()}
            for f, d in means.items()}


def main():
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    result = {"streams": B, "launches_per_round": N, "rounds": ROUNDS}
    inter = np.array(api.MIXED_RATES, np.int32)[np.arange(B) % 4]
    for title, make, row in (("single-rate 8000 Hz", lambda: api.RateConverter(ctx, 8000), 80),
                             ("single-rate 24000 Hz", lambda: api.RateConverter(ctx, 24000), 240),
                             ("mixed, 8000 / 16000 / 24000 / 48000 interleaved", lambda: api.MixedRateConverter(ctx, inter), 480)):
        rc = make()
        res = measure(ctx, rc, row)
        rc.close()
        result[title] = res
        print(f"{title}, {B} streams, mean of {N} launches, median (min-max) of {ROUNDS} rounds, ms")
        for k in ("rate_up", "rate_down"):
            a, b = res["i16"][k], res["g711"][k]
            print(f"  {k:9s} int16 {a['median_ms']:.4f} ({a['min_ms']:.4f}-{a['max_ms']:.4f})   G.711 {b['median_ms']:.4f} "
                  f"({b['min_ms']:.4f}-{b['max_ms']:.4f})   G.711 / int16 {b['median_ms'] / a['median_ms']:.3f}")
        sys.stdout.flush()
    ctx.close()
    model.close()
    if OUT:
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
