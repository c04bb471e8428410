"""Times of DTMF removal, and what the engine leaks past the muted rows (DESIGN.md 4.8 "DTMF removal": the numbers there come from
this script).

    python tools/rate_dtmf_clamp_times.py [streams] [launches] [rounds] [result.json] [--parent-lib PATH] [--processes K]
                                                                                       defaults 65536 20 3, no file, no parent, 3

  copy        a device-to-device copy of [streams][480] float rows, timed with events through torch in the same run: the yardstick
  rate_clamp  the converter's own profiling (pn_rate_set_profiling: HIP events around each launch on the context's stream; a figure is
              the MEAN of `launches` launches) of pn_rate_dtmf_clamp_f32 on its own on a mixed converter, removal on for every stream,
              in three steady states made with hand-set detector report rows: nobody in a digit (every row at unity gain: 32 bytes
              read and 32 written a stream, no audio), every tenth stream in a digit, everybody in a digit (every row zeroed).  Seven
              launches in front of each case bring the marks to the row that leaves
  frame       wall time of `launches` whole frames (pn_rate_process_i16, mixed converter of 8000 / 16000 / 24000 / 48000 by slot) behind
              one synchronise, per frame, with removal NEVER on — in K fresh processes of this library and, with --parent-lib, K of the
              parent's (PERCEPNET_LIB), taking turns: the spread between the processes of one library is the yardstick for the
              difference between the two — then, in this process, with detection and removal on for everybody
  leak        the default seeded weights, NO attenuation limit, 16 streams: a digit of 100 ms over speech-like noise.  The energy at the
              digit's two frequencies (a Goertzel sum per row) in the output rows around the digit that are NOT muted, with removal
              on, with removal off, and for the same input without the digit — for the guard rows (pre, post) = (1, 0), (2, 0), (2, 2)
The cases take turns round by round; one warm-up round is thrown away; the median of the rounds with the smallest and largest."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_ap = argparse.ArgumentParser()
_ap.add_argument("streams", nargs="?", type=int, default=65536)
_ap.add_argument("launches", nargs="?", type=int, default=20)
_ap.add_argument("rounds", nargs="?", type=int, default=3)
_ap.add_argument("out", nargs="?", default=None)
_ap.add_argument("--parent-lib", default=None)
_ap.add_argument("--processes", type=int, default=3)
_ap.add_argument("--child", default=None)                 # "frame": this process measures the frame and prints one JSON line
_a = _ap.parse_args()
B, N, ROUNDS, OUT, PARENT, PROCS, CHILD = _a.streams, _a.launches, _a.rounds, _a.out, _a.parent_lib, _a.processes, _a.child
DEV = "cuda:0"
FREQS = (697, 770, 852, 941, 1209, 1336, 1477, 1633)
DIGITS = "123A456B789C*0#D"


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def frame_times(api, ctx, rc, xi, yi):
    out = []
    for rnd in range(ROUNDS + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            rc.process_i16_dev(xi.data_ptr(), yi.data_ptr())
        ctx.synchronize()
        if rnd > 0:
            out.append((time.perf_counter() - t0) * 1e3 / N)
    return out


def child_frame():
    """one process: a mixed converter, removal never touched -> {"frame": stat, "launches": {...}, "has_clamp": bool}"""
    import torch
    from percepnet_amd import api, weights
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    rc = api.MixedRateConverter(ctx, np.array(api.MIXED_RATES, np.int32)[np.arange(B) % 4])
    has = hasattr(ctx.L, "pn_rate_set_stream_dtmf_clamp")
    g = torch.Generator(device=DEV).manual_seed(1)
    xi = (torch.randn((B, 480), device=DEV, generator=g) * 8192).clamp(-32768, 32767).to(torch.int16)
    yi = torch.empty_like(xi)
    ms = frame_times(api, ctx, rc, xi, yi)
    rc.set_profiling(True)
    rc.reset_profile()
    for _ in range(N):
        rc.process_i16_dev(xi.data_ptr(), yi.data_ptr())
    names = ("rate_up", "rate_down", "rate_mix", "rate_plc", "rate_agc", "rate_lim", "rate_dtmf") + (("rate_clamp",) if has else ())
    launched = {k: n for k, (_, n) in rc.kernel_times(names).items()}
    rc.close(); ctx.close(); model.close()
    print("RESULT " + json.dumps({"frame": stat(ms), "launches": launched, "has_clamp": has}), flush=True)


def goertzel(rows, f):
    """rows [..., 480] float64 -> the squared magnitude of the row's component at f Hz, over 480 (a full-scale sine gives 120)"""
    j = np.arange(480)
    c, s = np.cos(2 * np.pi * f * j / 48000.0), np.sin(2 * np.pi * f * j / 48000.0)
    return ((rows * c).sum(-1) ** 2 + (rows * s).sum(-1) ** 2) / 480.0


def leak(api, model):
    """-> per guard setting: the energy at the digit's two frequencies in the unmuted output rows around the digit"""
    S, frames, at, n = 16, 40, 10 * 480 + 137, 4800
    rng = np.random.default_rng(7)
    t = np.arange(frames * 480) / 48000.0
    base, tone = np.empty((S, frames * 480)), np.zeros((S, frames * 480))
    for s in range(S):                                         # speech-like: six harmonics of 100..250 Hz under a slow envelope, in noise
        f0 = 100.0 + 10.0 * s
        v = sum(np.cos(2 * np.pi * k * f0 * t + k * k) / k for k in range(1, 7)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t + s))
        base[s] = 0.05 * v + rng.standard_normal(t.size) * 0.01
        fr, fc = FREQS[(s % 16) // 4], FREQS[4 + s % 4]
        k = np.arange(n)
        tone[s, at:at + n] = 0.1 * (np.sin(2 * np.pi * fr * k / 48000.0) + np.sin(2 * np.pi * fc * k / 48000.0))
    res = {}

    def run(x, clamp):
        ctx = api.Context(model, S)
        rc = api.MixedRateConverter(ctx, [48000] * S)
        rc.set_stream_dtmf(np.arange(S), 1)
        if clamp is not None:
            rc.set_dtmf_clamp_params([clamp[0], clamp[1], 10, 80])
            rc.set_stream_dtmf_clamp(np.arange(S), 1)
            rc.set_dtmf_clamp_report(True)
        rows = x.astype(np.float32).reshape(S, frames, 480)
        out, muted = np.empty((frames, S, 480), np.float32), np.zeros((frames, S), bool)
        for f in range(frames):
            o, _ = rc.process_f32(np.ascontiguousarray(rows[:, f]), want_gr=False)
            out[f] = o
            if clamp is not None:
                muted[f] = (rc.read_dtmf_clamp_report()["flags"] & api.DTMF_CLAMP_MUTED) != 0
        rc.close(); ctx.close()
        return out.astype(np.float64), muted

    def tone_energy(out, rows_mask):
        e = np.zeros(out.shape[:2])
        for s in range(S):
            e[:, s] = goertzel(out[:, s], FREQS[(s % 16) // 4]) + goertzel(out[:, s], FREQS[4 + s % 4])
        return float((e * rows_mask).sum() / max(rows_mask.sum(), 1))

    with_tone, without = base + tone, base
    off, _ = run(with_tone, None)
    clean, _ = run(without, None)
    first, last = at // 480 + 6, (at + n - 1) // 480 + 6                # the output rows that hold the digit at the engine's delay of 6
    digit_rows = np.zeros((frames, S), bool)
    digit_rows[first:last + 1] = True
    res["tone rows, removal off: energy at the two frequencies per row"] = tone_energy(off, digit_rows)
    res["the same rows without the digit in the input"] = tone_energy(clean, digit_rows)
    for guard in ((1, 0), (2, 0), (2, 2)):                              # (pre = 2 is the longest guard in time at on_frames = 3)
        on, muted = run(with_tone, guard)
        around = np.zeros((frames, S), bool)
        around[first - 6:last + 9] = True
        around &= ~muted
        res[f"pre {guard[0]} post {guard[1]}"] = {
            "muted rows per stream": float(muted.sum() / S),
            "unmuted rows within 6 in front and 8 behind, per stream": float(around.sum() / S),
            "energy there, removal on": tone_energy(on, around), "removal off": tone_energy(off, around), "no digit in the input": tone_energy(clean, around)}
    return res


def main():
    import torch
    here = os.path.abspath(__file__)
    result = {"streams": B, "launches_per_round": N, "rounds": ROUNDS}
    # ---- frames with removal never on, in fresh processes taking turns
    procs = {"this": []}
    if PARENT:
        procs["parent"] = []
    for k in range(PROCS):
        for name in procs:
            env = dict(os.environ)
            if name == "parent":
                env["PERCEPNET_LIB"] = os.path.abspath(PARENT)
            else:
                env.pop("PERCEPNET_LIB", None)
            r = subprocess.run([sys.executable, here, str(B), str(N), str(ROUNDS), "--child", "frame"], env=env, capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode or not line:
                raise SystemExit(f"child process ({name}) failed: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            procs[name].append(json.loads(line[0][7:]))
            print(f"  frame, removal never on, {name} library, process {k}: {procs[name][-1]['frame']['median_ms']:.4f} ms   launches {procs[name][-1]['launches']}", flush=True)
    for name, v in procs.items():
        med = [p["frame"]["median_ms"] for p in v]
        result[f"frame never on, {name}"] = {"processes": v, "medians_ms": med, "spread_ms": [min(med), max(med)], "spread_rel": (max(med) - min(med)) / min(med)}
        print(f" {name}: process medians {min(med):.4f} .. {max(med):.4f} ms, spread {100 * (max(med) - min(med)) / min(med):.2f} %")
    from percepnet_amd import api, weights
    model = api.Model(weights.default_blob(1234))
    ctx = api.Context(model, B)
    g = torch.Generator(device=DEV).manual_seed(1)
    x48 = (0.05 * torch.randn((B, 480), device=DEV, generator=g)).contiguous()
    w48 = torch.empty_like(x48)
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
    result["copy"] = dict(stat(copy_ms), bytes=moved, gb_per_s=moved / bound_ms / 1e6)
    print(f"{B} streams, mean of {N} launches, median (min-max) of {ROUNDS} rounds, ms")
    print(f"  device-to-device copy of the rows: {bound_ms:.4f} ms = {moved / bound_ms / 1e6:.0f} GB/s for {moved} bytes")
    rc = api.MixedRateConverter(ctx, np.array(api.MIXED_RATES, np.int32)[np.arange(B) % 4])
    all_ids = np.arange(B, dtype=np.int32)
    rc.set_stream_dtmf_clamp(all_ids, 1)
    idle = np.tile(np.array([api.DTMF_ON, 0, 0, 0], np.uint32), (B, 1))
    busy = np.tile(np.array([api.DTMF_ON | api.DTMF_HIT | ord("5") << 8, 9, 1, ord("5")], np.uint32), (B, 1))
    states = {"nobody in a digit": idle, "10 % in a digit": np.where((all_ids % 10 == 0)[:, None], busy, idle), "everybody in a digit": busy}
    cases = {f"rate_clamp {k}": [] for k in states}
    for rnd in range(ROUNDS + 1):
        for k, rows in states.items():
            rc.set_dtmf_report_rows(rows)
            rc.reset_streams(all_ids)
            for _ in range(7):                                             # the marks reach the row that leaves
                rc.dtmf_clamp_f32_dev(w48.data_ptr())
            rc.set_profiling(True)
            rc.reset_profile()
            for _ in range(N):
                rc.dtmf_clamp_f32_dev(w48.data_ptr())
            ms, n = rc.kernel_times(("rate_clamp",))["rate_clamp"]
            assert n == N
            rc.set_profiling(False)
            if rnd > 0:
                cases[f"rate_clamp {k}"].append(ms / n)
    st = rc.dtmf_clamp_state()                                             # (the report is off in the timed launches: the state says what they did)
    assert np.all(st[:, 1] == 1) and np.all(st[:, 2] == N + 2), "the last case muted every row of every timed launch"
    # ---- whole frames with detection and removal on for everybody, in this process
    xi = (torch.randn((B, 480), device=DEV, generator=g) * 8192).clamp(-32768, 32767).to(torch.int16)
    yi = torch.empty_like(xi)
    rc.set_dtmf_clamp_report(False)
    rc.set_stream_dtmf_clamp(all_ids, 0)
    cases["frame, removal never on for anybody now (this process)"] = frame_times(api, ctx, rc, xi, yi)
    rc.set_stream_dtmf(all_ids, 1)
    cases["frame, detection on, all enabled"] = frame_times(api, ctx, rc, xi, yi)
    rc.set_stream_dtmf_clamp(all_ids, 1)
    cases["frame, detection and removal on, all enabled"] = frame_times(api, ctx, rc, xi, yi)
    for name, v in cases.items():
        res = stat(v)
        line = f"  {name:55s} {res['median_ms']:.4f} ({res['min_ms']:.4f}-{res['max_ms']:.4f})"
        if name.startswith("rate_"):
            res["times_the_copy"] = res["median_ms"] / bound_ms
            line += f"   {res['times_the_copy']:.2f} x the copy"
        result[name] = res
        print(line)
    rc.close()
    ctx.close()
    result["leak"] = leak(api, model)
    print(json.dumps(result["leak"], indent=1))
    model.close()
    if OUT:
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    if CHILD == "frame":
        child_frame()
    else:
        main()
