"""NBC2-large (configs/NBC2.yaml's "large" comments: 12 layers, dim_hidden 192, dim_ffn 384, 2 heads -> attention head width 96) on the device:
the native paths (nbss_amd/nbc2.py: the key-blocked attention of csrc/attn_kb.hip + the geometry-generic building blocks) against the torch.nn modules
(NBSS_NBC2_NATIVE=0: what the module ran before head width 96 was native), in ONE process on the same device.

For B in --batches, F = 129, T = 251, fp32 and bf16: inference (no_grad forward) and one training step (forward + backward of sum(y * r), every parameter
gradient, no optimizer).  Per point: --warmup untimed calls, then --reps calls each timed with a pair of HIP events; reported: median, min, max (ms) and
ratio = torch.nn median / native median.  bf16 on the torch.nn side is the module converted with .bfloat16() (the native side reads the fp32
parameters and streams bf16 activations).  One JSON line per point, then a markdown table.
usage: python tools/nbc2_large_bench.py [--batches 1,2,4] [--reps 7] [--warmup 2] [--dtypes fp32,bf16] [--json out.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import warnings
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from models.arch.NBC2 import NBC2  # noqa: E402


def timed(fn, warmup, reps):
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
    return {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net32 = NBC2(dim_input=12, dim_output=4, n_layers=a.layers, dim_hidden=192, dim_ffn=384, num_freqs=129).to(dev)
    assert net32._native() is not None, "the native path does not take this module"
    net16 = copy.deepcopy(net32).bfloat16()  # torch.nn side of the bf16 points
    rows = []
    for dname in a.dtypes.split(","):
        td = torch.float32 if dname == "fp32" else torch.bfloat16
        for B in map(int, a.batches.split(",")):
            x = torch.randn(B, 129, 251, 12, device=dev).to(td)
            r = torch.randn(B, 129, 251, 4, device=dev).to(td)
            for mode in ("infer", "train"):
                res = {}
                for side in ("native", "torch_nn"):
                    os.environ["NBSS_NBC2_NATIVE"] = "1" if side == "native" else "0"
                    net = net32 if (side == "native" or td == torch.float32) else net16
                    net.train(mode == "train")

                    def infer():
                        with torch.no_grad():
                            return net(x)

                    def train():
                        net.zero_grad(set_to_none=True)
                        (net(x) * r).sum().backward()

                    res[side] = timed(infer if mode == "infer" else train, a.warmup, a.reps)
                    torch.cuda.empty_cache()
                row = {"dtype": dname, "B": B, "mode": mode, **{f"{s}_{k}": v for s, d in res.items() for k, v in d.items()},
                       "ratio": round(res["torch_nn"]["median_ms"] / res["native"]["median_ms"], 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.environ.pop("NBSS_NBC2_NATIVE", None)
    print("\n| dtype | B | mode | native ms (min - max) | torch.nn ms (min - max) | torch.nn / native |\n|---|---|---|---|---|---|")
    for w in rows:
        print(f"| {w['dtype']} | {w['B']} | {w['mode']} | {w['native_median_ms']} ({w['native_min_ms']} - {w['native_max_ms']}) | "
              f"{w['torch_nn_median_ms']} ({w['torch_nn_min_ms']} - {w['torch_nn_max_ms']}) | {w['ratio']}{'' if w['ratio'] >= 1.05 else '  (below 1.05)'} |")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "layers": a.layers, "F": 129, "T": 251, "reps": a.reps, "warmup": a.warmup,
                                            "rows": rows}, indent=1))


if __name__ == "__main__":
    warnings.simplefilter("ignore")  # (the module reports its torch.nn path once per reason)
    main()
