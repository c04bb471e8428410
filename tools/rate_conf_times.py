"""Times of the conference mix (DESIGN.md 4.8 "conferences": the numbers there come from this script).

    python tools/rate_conf_times.py [streams] [launches] [rounds] [result.json]        defaults 65536 20 3, no file

A mixed converter with 8000 / 16000 / 24000 / 48000 by slot, int16 rows, and four tables: every stream without a conference, and
every stream in a conference of 2, of 4 and of 32 (neighbouring slots, so the members of one conference run at all four rates).
With a library that has loudest-N selection five more, which run the selecting kernel: conferences of 4, 8 and 32 that mix their
N = 3 loudest talkers, conferences of 32 with send gains only (0.5 everywhere, N = 0) and with the mix report only.
Per table:
  kernels   the converter's own profiling (pn_rate_set_profiling: HIP events around each launch on the context's stream; a figure is
            the MEAN of `launches` launches) of pn_rate_mix_f32 and pn_rate_down_i16 on their own — with no conference the mix is
            the plain copy a frame never launches
  bound     the bytes the mix must move, 1920 B read + 1920 B written per stream, at the bandwidth a device-to-device copy of the
            same rows reaches here (measured with the same events, through torch), and the fraction of it the mix reaches
  frame     wall time of `launches` whole frames (pn_rate_process_i16) behind one synchronise, per frame
The tables take turns round by round; one warm-up round is thrown away; the median of the rounds with the smallest and largest.
With a library that has no conferences (PERCEPNET_LIB pointing at an older build) only the no-conference frame time is measured,
and with one that has no selection only the first four tables: that is how the parent's figures in DESIGN 4.8 were taken, in the
same process setup."""
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
NONE = -1


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def main():
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    rc = api.MixedRateConverter(ctx, np.array(api.MIXED_RATES, np.int32)[np.arange(B) % 4])
    has = hasattr(ctx.L, "pn_rate_set_stream_confs")
    has_sel = hasattr(ctx.L, "pn_rate_set_conf_speakers")
    conf_of = lambda k: (np.arange(B, dtype=np.int32) // k) * k                  # the conference's number: its lowest slot
    tables = {"none": np.full(B, NONE, np.int32)}
    setting = {}                                                                 # table -> (N of every conference, gain of every stream, report)
    if has:
        for k in (2, 4, 32):
            tables[f"of {k}"] = conf_of(k)
    if has_sel:
        for k in (4, 8, 32):
            tables[f"of {k} N=3"] = conf_of(k)
            setting[f"of {k} N=3"] = (3, 1.0, False)
        tables["of 32 gains"], setting["of 32 gains"] = conf_of(32), (0, 0.5, False)
        tables["of 32 report"], setting["of 32 report"] = conf_of(32), (0, 1.0, True)
    g = torch.Generator(device=DEV).manual_seed(1)
    y48 = torch.rand((B, 480), device=DEV, generator=g) * 2 - 1
    o48 = torch.empty_like(y48)
    xi = (torch.randn((B, 480), device=DEV, generator=g) * 8192).clamp(-32768, 32767).to(torch.int16)
    yi = torch.empty_like(xi)
    torch.cuda.synchronize()
    # the copy bandwidth: the same rows, device to device
    copy_ms = []
    for rnd in range(ROUNDS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(N):
            o48.copy_(y48)
        b.record()
        torch.cuda.synchronize()
        if rnd > 0:
            copy_ms.append(a.elapsed_time(b) / N)
    bound_ms = float(np.median(copy_ms))
    moved = 2 * 1920 * B
    result = {"streams": B, "launches_per_round": N, "rounds": ROUNDS, "library_has_conferences": has, "library_has_selection": has_sel,
              "copy": dict(stat(copy_ms), bytes=moved, gb_per_s=moved / bound_ms / 1e6)}
    print(f"{B} streams, mean of {N} launches, median (min-max) of {ROUNDS} rounds, ms")
    print(f"  device-to-device copy of the rows: {bound_ms:.4f} ms = {moved / bound_ms / 1e6:.0f} GB/s for {moved} bytes")
    all_ids = np.arange(B, dtype=np.int32)
    means = {name: {"rate_mix": [], "rate_down": [], "frame": []} for name in tables}
    for rnd in range(ROUNDS + 1):
        for name, table in tables.items():
            if has:
                rc.set_stream_confs(all_ids, table)
                if has_sel:
                    n_max, gain, report = setting.get(name, (0, 1.0, False))
                    rc.set_conf_speakers(all_ids, np.full(B, n_max, np.int32))
                    rc.set_stream_mix_gains(all_ids, np.full(B, gain, np.float32))
                    rc.set_mix_report(report)
                rc.set_profiling(True)
                rc.reset_profile()
                for _ in range(N):
                    rc.mix_f32_dev(y48.data_ptr(), o48.data_ptr())
                    rc.down_i16_dev(o48.data_ptr(), yi.data_ptr())
                for k, (ms, n) in rc.kernel_times(("rate_mix", "rate_down")).items():
                    assert n == N
                    if rnd > 0:
                        means[name][k].append(ms / n)
                rc.set_profiling(False)
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(N):
                rc.process_i16_dev(xi.data_ptr(), yi.data_ptr())
            ctx.synchronize()
            if rnd > 0:
                means[name]["frame"].append((time.perf_counter() - t0) * 1e3 / N)
    for name in tables:
        res = {k: stat(v) for k, v in means[name].items() if v}
        line = f"  {name:12s} frame {res['frame']['median_ms']:.3f} ({res['frame']['min_ms']:.3f}-{res['frame']['max_ms']:.3f})"
        if has:
            res["fraction_of_bound"] = bound_ms / res["rate_mix"]["median_ms"]
            line += (f"   rate_mix {res['rate_mix']['median_ms']:.4f} ({res['rate_mix']['min_ms']:.4f}-{res['rate_mix']['max_ms']:.4f})"
                     f"   rate_down {res['rate_down']['median_ms']:.4f}   bound / rate_mix {res['fraction_of_bound']:.2f}")
        result[name] = res
        print(line)
    rc.close()
    ctx.close()
    model.close()
    if OUT:
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
