"""Times of the rate converter's kernels with 32000 Hz among the rates (DESIGN.md 4.8 "32 kHz": the numbers there come from this
script), by the method of tools/rate_mixed_times.py: HIP events around SINGLE launches on the context's stream, int16 rows,
the kernels of one part taking turns launch by launch, median of `launches` after `warmup`.

    python tools/rate32_times.py run [--tree DIR] [streams] [launches] [warmup] [result.json]      defaults 65536 50 5, no file
    python tools/rate32_times.py compare parent.json this.json

run      --tree DIR imports percepnet_amd from DIR instead of this checkout, so that the SAME script times a build of the parent
         commit in the same session on the same machine (a tree that refuses 32000 runs the old-rate parts only).  Parts:
           single   rate_up / rate_down of single-rate converters at 16000, 24000 and 32000
           mixed    the mixed kernels over the population 8000 / 16000 / 24000 / 48000 by slot (every block diverges four ways):
                    what the 32000 branch and its LDS cost the streams that do not use it
           mixed32  the same with 32000 as a fifth rate by slot
compare  the check of DESIGN 4.8 on the `mixed` part: a kernel fails if its median in this.json exceeds the parent's maximum by
         more than the parent's own max - min; also prints the 32000 / 24000 and 32000 / 16000 ratios of the `single` part."""
import json
import os
import sys

import numpy as np


def stats(ms, warm):
    ms = np.asarray(ms[warm:])
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def run(argv):
    tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if argv[:1] == ["--tree"]:
        tree, argv = os.path.abspath(argv[1]), argv[2:]
    sys.path.insert(0, tree)
    import torch
    from percepnet_amd import api, weights
    B = int(argv[0]) if len(argv) > 0 else 65536
    N = int(argv[1]) if len(argv) > 1 else 50
    warm = int(argv[2]) if len(argv) > 2 else 5
    out_path = argv[3] if len(argv) > 3 else None
    dev = "cuda:0"
    assert os.path.abspath(api.__file__).startswith(tree + os.sep), "percepnet_amd must come from --tree"
    busy = torch.empty(128 << 20, dtype=torch.float32, device=dev)

    def time_launches(stream, calls):
        """a 512 MB fill is queued in front of every launch, so that both events and the launch are in the queue before the GPU
        reaches them: the interval holds the kernel and not the host's launch path"""
        res = [[] for _ in calls]
        for _ in range(warm + N):
            for k, call in enumerate(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    busy.zero_()
                a.record(stream)
                call()
                b.record(stream)
                b.synchronize()
                res[k].append(a.elapsed_time(b))
        return [stats(r, warm) for r in res]

    model = api.Model(weights.default_blob(1234))
    stream = torch.cuda.Stream(device=dev)
    ctx = api.Context(model, B, stream=stream.cuda_stream)
    has32 = api.rate_frame_samples(32000) == 320
    g = torch.Generator(device=dev).manual_seed(1)
    x48 = torch.rand((B, 480), device=dev, generator=g) * 2 - 1
    y48 = torch.empty_like(x48)
    xi = torch.randint(-32768, 32768, (B, 480), device=dev, generator=g, dtype=torch.int32).to(torch.int16)
    zi = torch.empty_like(xi)
    torch.cuda.synchronize()
    result = {"streams": B, "launches": N, "warmup": warm, "has_32000": has32}
    slot = np.arange(B)

    def part(title, named):
        """named: {name: converter}; rows of [B][480] int16 serve every converter (a single-rate one reads its first B * n)"""
        res = {}
        for kernel, launch in (("rate_up", lambda rc: rc.up_i16_dev(xi.data_ptr(), y48.data_ptr())),
                               ("rate_down", lambda rc: rc.down_i16_dev(x48.data_ptr(), zi.data_ptr()))):
            for name, st in zip(named, time_launches(stream, [(lambda rc=rc: launch(rc)) for rc in named.values()])):
                res[f"{kernel} {name}"] = st
        torch.cuda.synchronize()
        for rc in named.values():
            rc.close()
        print(title)
        for k, v in res.items():
            print(f"  {k:40s} median {v['median_ms']:.4f} ms   min {v['min_ms']:.4f}   max {v['max_ms']:.4f}")
        sys.stdout.flush()
        result[title] = res

    part("single", {str(r): api.RateConverter(ctx, r) for r in (16000, 24000) + ((32000,) if has32 else ())})
    part("mixed", {"8000/16000/24000/48000": api.MixedRateConverter(ctx, np.array((8000, 16000, 24000, 48000), np.int32)[slot % 4])})
    if has32:
        part("mixed32", {"8000/16000/24000/32000/48000": api.MixedRateConverter(ctx, np.array((8000, 16000, 24000, 32000, 48000), np.int32)[slot % 5])})
    ctx.close()
    model.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)


def compare(argv):
    parent, this = (json.load(open(p)) for p in argv[:2])
    ok = True
    for k, p in parent["mixed"].items():
        t = this["mixed"][k]
        bound = p["max_ms"] + (p["max_ms"] - p["min_ms"])
        verdict = "ok" if t["median_ms"] <= bound else "FAIL"
        ok &= verdict == "ok"
        print(f"mixed {k}: parent median {p['median_ms']:.4f} (min {p['min_ms']:.4f}, max {p['max_ms']:.4f}), this median {t['median_ms']:.4f} "
              f"(min {t['min_ms']:.4f}, max {t['max_ms']:.4f}); bound {bound:.4f}: {verdict}")
    s = this["single"]
    for kernel in ("rate_up", "rate_down"):
        m = {r: s[f"{kernel} {r}"]["median_ms"] for r in (16000, 24000, 32000)}
        print(f"single {kernel}: 16000 {m[16000]:.4f} ms, 24000 {m[24000]:.4f} ms, 32000 {m[32000]:.4f} ms; 32000 / 24000 = {m[32000] / m[24000]:.3f}, "
              f"32000 / 16000 = {m[32000] / m[16000]:.3f}")
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run(sys.argv[2:])
    elif sys.argv[1:2] == ["compare"] and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2:]))
    else:
        sys.exit(__doc__)
