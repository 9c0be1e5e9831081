"""Diffuse-noise stage of the on-device simulator (profiles/README.md, "Room simulation"): the shipped torch chain (diffuse='fft': gen_diffuse_noise,
unfold + rfft + einsum + irfft + fold) beside the fused HIP kernel of csrc/diffuse.hip (diffuse='native': nbss_diffuse_noise), in the same run on the
same device.

  noise points  gen_diffuse_noise / gen_diffuse_noise_native at B = 32, M = 6, N in {32 000, 64 000}, the mixing matrices of the six-microphone circular
                array: --warmup untimed calls, then --reps calls each between a pair of HIP events (median, min, max in ms), the peak of
                torch.cuda.max_memory_allocated over the calls above what the inputs hold (MB), and the rel-L2 distance of the two results.
                FLOP/s of the native kernel: two nfft x nfft real transforms per frame and channel (4 nfft^2 FLOP), over its time, which includes
                the tables and the row means.
  dm points     utterances/s of tools/sim_throughput.py (batch 32, 4 s, 6 channels, 2 speakers, rir ism, convolve native) with diffuse fft and native.

The driver starts every point as a child process of its own under a time limit (--limit seconds) and stops at the first one that fails, so a fault
in one point starts nothing more on the device.  One JSON line per point, then markdown tables.
usage: python tools/diffuse_noise_bench.py [--reps 20] [--warmup 3] [--batches 10] [--limit 120] [--json out.json]"""
import argparse
import json
import math
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
B, M, NFFT = 32, 6, 256


def noise_point(a):
    import torch
    from data_loaders.gpu_simulation import diffuse_mixing_matrices, gen_diffuse_noise, gen_diffuse_noise_native
    dev = torch.device("cuda:0")
    ang = torch.arange(M) * (2 * math.pi / M)
    pos = torch.stack([0.1 * torch.cos(ang), 0.1 * torch.sin(ang), torch.zeros(M)], 1)
    Cs = diffuse_mixing_matrices(pos, 8000)[1].to(torch.complex64).to(dev)
    white = torch.randn(B, M, a.N, generator=torch.Generator(device=dev).manual_seed(0), device=dev)
    torch.cuda.synchronize()
    row = {"point": "noise", "B": B, "M": M, "N": a.N}
    outs = {}
    for side, fn in (("fft", gen_diffuse_noise), ("native", gen_diffuse_noise_native)):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _ in range(a.warmup):
            fn(white, a.N, Cs)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(white, a.N, Cs)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        outs[side] = out.clone()
        del out
        row.update({f"{side}_median_ms": round(statistics.median(ms), 3), f"{side}_min_ms": round(min(ms), 3), f"{side}_max_ms": round(max(ms), 3),
                    f"{side}_peak_mb": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20)})
    frames = -(-a.N // (NFFT // 4)) + 1
    row["native_useful_tflops"] = round(4.0 * NFFT * NFFT * B * M * frames / (row["native_median_ms"] * 1e-3) / 1e12, 2)
    row["fft_over_native"] = round(row["fft_median_ms"] / row["native_median_ms"], 3)
    row["rel_l2_native_vs_fft"] = float((outs["native"] - outs["fft"]).double().norm() / outs["fft"].double().norm())
    print(json.dumps(row), flush=True)


def driver(a):
    me = [sys.executable, str(Path(__file__).resolve())]
    points = [me + ["--point", "noise", "--N", str(n), "--reps", str(a.reps), "--warmup", str(a.warmup)] for n in (32000, 64000)]
    points += [[sys.executable, str(ROOT / "tools" / "sim_throughput.py"), str(B), str(a.batches), "ism", "native", d] for d in ("fft", "native")]
    rows = []
    for cmd in points:
        what = " ".join(cmd[1:])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"stopped: {what} ran into its limit of {a.limit} s", flush=True)
            return 1
        if r.returncode != 0:
            print(f"stopped: {what} exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    print("\n| B | M | N | torch ms (min - max) / peak MB | native ms (min - max) / peak MB | torch / native | native useful TFLOP/s | rel-L2 native vs torch |\n"
          "|---|---|---|---|---|---|---|---|")
    for w in (w for w in rows if w.get("point") == "noise"):
        cell = lambda s: f"{w[s + '_median_ms']} ({w[s + '_min_ms']} - {w[s + '_max_ms']}) / {w[s + '_peak_mb']}"  # noqa: E731
        print(f"| {w['B']} | {w['M']} | {w['N']} | {cell('fft')} | {cell('native')} | {w['fft_over_native']} | {w['native_useful_tflops']} | "
              f"{w['rel_l2_native_vs_fft']:.2e} |")
    print("\n| rir | convolve | diffuse | utt/s |\n|---|---|---|---|")
    for w in (w for w in rows if "utt_per_s" in w):
        print(f"| {w['rir']} | {w['convolve']} | {w['diffuse']} | {w['utt_per_s']:.1f} |")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps({"B": B, "M": M, "reps": a.reps, "warmup": a.warmup, "rows": rows}, indent=1))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", default=None, choices=["noise"])
    ap.add_argument("--N", type=int, default=32000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.point == "noise":
        noise_point(a)
    else:
        sys.exit(driver(a))


if __name__ == "__main__":
    main()
