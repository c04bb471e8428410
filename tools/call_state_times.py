"""Times of the call-state records (DESIGN.md 4.8 "call-state records": the numbers there come from this script).

    python tools/call_state_times.py [streams] [calls] [rounds] [result.json]        defaults 65536 10 3, no file

One mixed converter with 8000 / 16000 / 24000 / 48000 by slot that holds all four states (PLC on, AGC on, a ceiling and a mix hold set).
  copy      a device-to-device copy of [streams][10640] bytes, timed with events through torch in the same run: the yardstick — an
            export reads every stream's state once and writes its record once, an import the other way round: exactly these bytes
  export    pn_rate_export_call_state of EVERY stream: wall time of `calls` calls behind one synchronise, per call.  The call stages
            its id list through the context's id ring (a host-to-device copy of 4 bytes a stream), which is inside the figure
  import    pn_rate_import_call_state of every stream from those records, the same way; every status is checked to be PN_SS_OK once
  frame     wall time of `calls` whole frames (pn_rate_process_i16) of a converter that never enables a feature and never calls a
            record function, behind one synchronise, per frame.  These rounds run FIRST, before the converter with the states
            exists, so that the process is then what a process of the parent is
Copy, export and import take turns round by round; one warm-up round is thrown away; the median of the rounds with the smallest and
largest.  The ratio of export and import to the copy is reported, not judged.
With a library that has no call-state records (PERCEPNET_LIB pointing at an older build) only the copy and the frame are measured:
that is how the parent's frame in DESIGN 4.8 is taken, in the same process setup — twice, for the spread between runs of the parent
itself."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from percepnet_amd import api, weights  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
OUT = sys.argv[4] if len(sys.argv) > 4 else None
DEV = "cuda:0"
REC = 10640


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def main():
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    has = hasattr(ctx.L, "pn_rate_export_call_state")
    g = torch.Generator(device=DEV).manual_seed(1)
    xi = (torch.randn((B, 480), device=DEV, generator=g) * 8192).clamp(-32768, 32767).to(torch.int16)
    yi = torch.empty_like(xi)
    rec = torch.zeros((B, REC), dtype=torch.uint8, device=DEV)
    rec2 = torch.empty_like(rec)
    status = torch.full((B,), 99, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    all_ids = np.arange(B, dtype=np.int32)
    rates = np.array(api.MIXED_RATES, np.int32)[np.arange(B) % 4]
    plain = api.MixedRateConverter(ctx, rates)
    cases = {"frame, no feature ever used": [], "copy": []}
    rc = None

    def wall(call):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            call()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / N

    for rnd in range(ROUNDS + 1):
        ms = wall(lambda: plain.process_i16_dev(xi.data_ptr(), yi.data_ptr()))
        if rnd > 0:
            cases["frame, no feature ever used"].append(ms)
    if has:
        rc = api.MixedRateConverter(ctx, rates)
        rc.set_plc(True)
        rc.set_agc(True)
        rc.set_stream_agc_targets(all_ids, np.full(B, 0.1, np.float32))
        rc.set_stream_limiter(all_ids, np.full(B, 0.5, np.float32))
        rc.set_mix_hold(0.9)
        assert rc.call_state_sections() == 15
        for _ in range(5):                                  # some state to move: histories, levels, gains
            rc.process_i16_dev(xi.data_ptr(), yi.data_ptr())
        cases["export"], cases["import"] = [], []

    for rnd in range(ROUNDS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(N):
            rec2.copy_(rec)
        b.record()
        torch.cuda.synchronize()
        ms = {"copy": a.elapsed_time(b) / N}
        if has:
            ms["export"] = wall(lambda: rc.export_call_state_dev(all_ids, rec.data_ptr()))
            ms["import"] = wall(lambda: rc.import_call_state_dev(all_ids, rec.data_ptr(), status.data_ptr()))
            if rnd == 0:
                ctx.synchronize()
                assert int(status.abs().max().cpu()) == 0, "every record is accepted"
        if rnd > 0:
            for k, v in ms.items():
                cases[k].append(v)
    bound_ms = float(np.median(cases["copy"]))
    moved = 2 * REC * B
    result = {"streams": B, "calls_per_round": N, "rounds": ROUNDS, "library_has_call_state": has, "bytes_moved": moved}
    print(f"{B} streams, mean of {N} calls, median (min-max) of {ROUNDS} rounds, ms")
    for name, v in cases.items():
        res = stat(v)
        line = f"  {name:32s} {res['median_ms']:.4f} ({res['min_ms']:.4f}-{res['max_ms']:.4f})"
        if name in ("copy", "export", "import"):
            res["gb_per_s"] = moved / res["median_ms"] / 1e6
            line += f"   {res['gb_per_s']:.0f} GB/s"
        if name in ("export", "import"):
            res["times_the_copy"] = res["median_ms"] / bound_ms
            line += f"   {res['times_the_copy']:.2f} x the copy"
        result[name] = res
        print(line)
    if rc is not None:
        rc.close()
    plain.close()
    ctx.close()
    model.close()
    if OUT:
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
