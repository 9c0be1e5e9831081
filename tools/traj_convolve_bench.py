"""Trajectory convolution of the on-device simulator for moving sources (profiles/README.md, "Room simulation"): the torch path of
convolve_traj_aligned (convolve='fft': the weighted source through rocFFT once per trajectory point, accumulated, then a gather) beside the HIP kernel of
csrc/conv_traj.hip (convolve='native': nbss_rir_delay + nbss_fir_convolve_traj with its status read-back), in the same run on the same device.

  points   B = 32, S = 2, M = 6, N = 32 000, L in {3 200, 5 600}, hop H in {1 000, 3 333} samples per trajectory point (0.4 and 0.12 m/s at 5 cm and
           8 kHz), trapezium window with ramp 20, P = ceil((N + H - 1) / H) responses per source, no rir_target.
           --warmup untimed calls, then --reps calls each between a pair of HIP events (median, min, max in ms) and the peak of
           torch.cuda.max_memory_allocated over the calls above what the inputs hold (MB), for 'fft', 'native', the kernel alone
           (ops.fir_convolve_traj, check=False: no read-back) and, for scale, the static nbss_fir_convolve at the same N and L (one response per
           source: half the useful work wherever two responses overlap, and no weights).  rel-L2 distance of the two results.
           FLOP/s of the kernel alone: 2 N L MACs per output row (the useful work of a static convolution; the cross-fade adds ramp / H), over its time.

The driver starts every point as a child process of its own under a time limit (--limit seconds) and stops at the first one that fails, so a fault
in one point starts nothing more on the device.  One JSON line per point, then a markdown table.
usage: python tools/traj_convolve_bench.py [--reps 10] [--warmup 2] [--limit 180] [--json out.json]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
S, M, N, RAMP = 2, 6, 32000, 20


def timed(torch, fn, warmup, reps):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    peak = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
    return out, {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "peak_mb": peak}


def point(a):
    import torch
    from data_loaders.gpu_simulation import convolve_traj_aligned, traj_rirs_needed
    from nbss_amd import ops
    from nbss_amd._lib import hip
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    P = traj_rirs_needed(N, a.H)
    wav = torch.randn(a.B, S, N, generator=g, device=dev)
    t = torch.arange(a.L, device=dev) / 8000.0
    rir = torch.randn(a.B, S, P, M, a.L, generator=g, device=dev) * torch.exp(-6.9 * t / 0.4) * 0.3
    rir[..., 40] = 1.0  # the direct path
    hop = torch.full((a.B, S), a.H, dtype=torch.int32, device=dev)
    static = rir[:, :, 0].contiguous()
    lib = hip()
    delay = ops.rir_delay(lib, static, 0)  # what convolve_traj_aligned takes: the kernel alone then gives the same bits
    torch.cuda.synchronize()
    row = {"point": "traj", "B": a.B, "S": S, "M": M, "N": N, "L": a.L, "H": a.H, "P": P, "ramp": RAMP}
    sides = {"fft": lambda: convolve_traj_aligned(wav, rir, hop, ramp=RAMP)[0],
             "native": lambda: convolve_traj_aligned(wav, rir, hop, ramp=RAMP, convolve="native")[0],
             "kernel": lambda: ops.fir_convolve_traj(lib, wav, rir, hop, delay, ramp=RAMP, check=False),
             "static": lambda: ops.fir_convolve(lib, wav, static, delay, check=False)}
    outs = {}
    for side, fn in sides.items():
        out, stats = timed(torch, fn, a.warmup, a.reps)
        outs[side] = out.clone()
        del out
        row.update({f"{side}_{k}": v for k, v in stats.items()})
    row["kernel_useful_tflops"] = round(2.0 * a.B * S * M * N * a.L / (row["kernel_median_ms"] * 1e-3) / 1e12, 2)
    row["fft_over_native"] = round(row["fft_median_ms"] / row["native_median_ms"], 3)
    row["kernel_over_static"] = round(row["kernel_median_ms"] / row["static_median_ms"], 3)
    row["rel_l2_native_vs_fft"] = float((outs["native"] - outs["fft"]).double().norm() / outs["fft"].double().norm())
    row["kernel_equals_native"] = bool(torch.equal(outs["kernel"], outs["native"]))
    print(json.dumps(row), flush=True)


def driver(a):
    rows = []
    for L in (3200, 5600):
        for H in (1000, 3333):
            p = ["--point", "traj", "--B", "32", "--L", str(L), "--H", str(H)]
            cmd = [sys.executable, str(Path(__file__).resolve()), *p, "--reps", str(a.reps), "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"stopped: {' '.join(p)} ran into its limit of {a.limit} s", flush=True)
                return 1
            if r.returncode != 0:
                print(f"stopped: {' '.join(p)} exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                return 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    print("\n| B | L | H | P | fft ms (min - max) / peak MB | native ms (min - max) / peak MB | kernel alone ms / peak MB | static nbss_fir_convolve ms | fft / native | "
          "kernel useful TFLOP/s | rel-L2 native vs fft |\n|---|---|---|---|---|---|---|---|---|---|---|")
    for w in rows:
        cell = lambda s: f"{w[s + '_median_ms']} ({w[s + '_min_ms']} - {w[s + '_max_ms']}) / {w[s + '_peak_mb']}"  # noqa: E731
        print(f"| {w['B']} | {w['L']} | {w['H']} | {w['P']} | {cell('fft')} | {cell('native')} | {w['kernel_median_ms']} / {w['kernel_peak_mb']} | {w['static_median_ms']} | "
              f"{w['fft_over_native']} | {w['kernel_useful_tflops']} | {w['rel_l2_native_vs_fft']:.1e} |")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps({"S": S, "M": M, "N": N, "ramp": RAMP, "reps": a.reps, "warmup": a.warmup, "rows": rows}, indent=1))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", default=None, choices=["traj"])
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=3200)
    ap.add_argument("--H", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=180)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.point == "traj":
        point(a)
    else:
        sys.exit(driver(a))


if __name__ == "__main__":
    main()
