"""Whole-utterance inference of the narrow-band attention networks on the device: the native long-sequence path (NBSS_NB_LONG=1: the key-blocked attention
kernels of csrc/attn_kb.hip / csrc/attn_relpos_kb.hip behind nbss_nb_attention_long_fwd / nbss_nb_attention_relpos_long_fwd) against the torch.nn modules
the same call runs without the switch (beyond 256 frames: what a validate / test / predict got before), in ONE process on the same device.

Networks: config-4 NBC2 (8 layers, 96 / 192, 2 heads), NBC2-large (12 layers, 192 / 384, 2 heads), NBC (4 layers, 192 / 8 heads / 384).  Input 1 x 129 x T
for T in --lengths, fp32 and bf16, under no_grad in eval mode.  Per point: --warmup untimed calls, then --reps calls each timed with a pair of HIP events
(median, min, max in ms), and the peak of torch.cuda.max_memory_allocated over the calls (MB).  bf16 on the torch.nn side is the module converted with
.bfloat16() (the native side reads the fp32 parameters and streams bf16 activations).  A point one side cannot run (NBC beyond the 1001 frames of its sinusoid
table, an allocation that fails) is reported with its reason instead of a time.
Then each long kernel alone at 129 sequences x 251 frames beside its whole-head sibling (for information: the whole-head kernels stay the <= 256 path).
One JSON line per point, then markdown tables.
usage: python tools/nb_long_bench.py [--lengths 500,1000,2000] [--reps 5] [--warmup 1] [--dtypes fp32,bf16] [--nets nbc2,nbc2_large,nbc] [--json out.json]"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import warnings
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from models.arch.NBC import NBC  # noqa: E402
from models.arch.NBC2 import NBC2  # noqa: E402
from nbss_amd import ops  # noqa: E402
from nbss_amd._lib import NBSS_BF16, NBSS_F32, NbssError, hip  # noqa: E402

NETS = {
    "nbc2": (lambda: NBC2(dim_input=12, dim_output=4, n_layers=8, dim_hidden=96, dim_ffn=192, num_freqs=129), 12),
    "nbc2_large": (lambda: NBC2(dim_input=12, dim_output=4, n_layers=12, dim_hidden=192, dim_ffn=384, num_freqs=129), 12),
    "nbc": (lambda: NBC(dim_input=16, dim_output=4, n_layers=4, encoder_kernel_size=4, n_heads=8, hidden_size=192, ffn_size=384), 16),
}


def timed(fn, warmup, reps):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2),
            "peak_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20)}


def networks(a, dev):
    rows = []
    for name in a.nets.split(","):
        make, din = NETS[name]
        torch.manual_seed(0)
        net32 = make().to(dev).eval()
        assert net32._native() is not None, "the native path does not take this module"
        net16 = copy.deepcopy(net32).bfloat16()  # torch.nn side of the bf16 points
        for dname in a.dtypes.split(","):
            td = torch.float32 if dname == "fp32" else torch.bfloat16
            for T in map(int, a.lengths.split(",")):
                x = torch.randn(1, 129, T, din, device=dev).to(td)
                row = {"net": name, "dtype": dname, "T": T}
                for side in ("native", "torch_nn"):
                    net = net32 if (side == "native" or td == torch.float32) else net16
                    os.environ["NBSS_NB_LONG"] = "1" if side == "native" else "0"

                    # (native: the runner itself — a refusal is reported, not replaced by the torch.nn modules)
                    fwd = net._native().forward if side == "native" else net

                    def infer():
                        with torch.no_grad():
                            return fwd(x)

                    try:
                        row.update({f"{side}_{k}": v for k, v in timed(infer, a.warmup, a.reps).items()})
                    except (NbssError, RuntimeError, IndexError) as e:
                        row[f"{side}_error"] = f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"
                    torch.cuda.empty_cache()
                if "native_median_ms" in row and "torch_nn_median_ms" in row:
                    row["ratio"] = round(row["torch_nn_median_ms"] / row["native_median_ms"], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
        del net32, net16
        torch.cuda.empty_cache()
    os.environ.pop("NBSS_NB_LONG", None)
    return rows


def kernels(a, dev):
    """each long kernel alone at 129 x 251 beside its whole-head sibling: microseconds per launch (HIP events around --kreps launches)"""
    lib, rows, nseq, T = hip(), [], 129, 251
    for dname in a.dtypes.split(","):
        td, dt = (torch.float32, NBSS_F32) if dname == "fp32" else (torch.bfloat16, NBSS_BF16)
        for kind, dh, heads in (("plain", 24, 4), ("plain", 48, 2), ("plain", 96, 2), ("relpos", 24, 8), ("relpos", 48, 4)):
            H = dh * heads
            qkv = torch.randn(nseq, T, 3 * H, device=dev).to(td)
            pos = torch.randn(2 * T - 1, H, device=dev).to(td)
            u, v = torch.randn(heads, dh, device=dev) * 0.5, torch.randn(heads, dh, device=dev) * 0.5
            o = torch.empty(nseq, T, H, device=dev, dtype=td)
            st = ops._stream(lib, qkv)
            row = {"kernel": kind, "dtype": dname, "dh": dh, "heads": heads, "nseq": nseq, "T": T}
            for which, entry in (("long", f"nbss_nb_attention_{'relpos_' if kind == 'relpos' else ''}long_fwd"),
                                 ("whole", f"nbss_nb_attention_{'relpos_' if kind == 'relpos' else ''}fwd")):
                if kind == "plain":
                    call = lambda: lib.call(entry, dt, nseq, T, H, heads, ops._ptr(lib, qkv), ops._ptr(lib, o), st)  # noqa: E731
                else:
                    call = lambda: lib.call(entry, dt, nseq, T, H, heads, ops._ptr(lib, qkv), ops._ptr(lib, pos), ops._ptr(lib, u), ops._ptr(lib, v),  # noqa: E731
                                            1.0 / math.sqrt(H), ops._ptr(lib, o), st)
                try:
                    for _ in range(3):
                        call()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.kreps):
                        call()
                    e1.record()
                    e1.synchronize()
                    row[f"{which}_us"] = round(1e3 * e0.elapsed_time(e1) / a.kreps, 1)
                except NbssError as e:
                    row[f"{which}_error"] = str(e)[:120]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="500,1000,2000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kreps", type=int, default=50)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--nets", default="nbc2,nbc2_large,nbc")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    krows = kernels(a, dev)
    rows = networks(a, dev)
    cell = lambda w, s: (f"{w[s + '_median_ms']} ({w[s + '_min_ms']} - {w[s + '_max_ms']}) / {w[s + '_peak_mb']}" if s + "_median_ms" in w  # noqa: E731
                         else w.get(s + "_error", "-"))
    print("\n| net | dtype | T | native ms (min - max) / peak MB | torch.nn ms (min - max) / peak MB | torch.nn / native |\n|---|---|---|---|---|---|")
    for w in rows:
        print(f"| {w['net']} | {w['dtype']} | {w['T']} | {cell(w, 'native')} | {cell(w, 'torch_nn')} | {w.get('ratio', '-')} |")
    print("\n| kernel | dtype | dh x heads | long us | whole-head us |\n|---|---|---|---|---|")
    for w in krows:
        print(f"| {w['kernel']} | {w['dtype']} | {w['dh']} x {w['heads']} | {w.get('long_us', w.get('long_error'))} | {w.get('whole_us', w.get('whole_error'))} |")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "F": 129, "reps": a.reps, "warmup": a.warmup, "rows": rows,
                                            "kernels": krows}, indent=1))


if __name__ == "__main__":
    warnings.simplefilter("ignore")  # (the module reports its torch.nn path once per reason)
    main()
