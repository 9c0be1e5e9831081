"""STOI / eSTOI timing (profiles/README.md, "The metric pass of `test`"): one nbss_stoi call on the device beside the fp64 host closed form of the same
definition (models/utils/metrics.py: native_stoi on host tensors), batch 32 x 2 speakers, 4 s, at 8 and 16 kHz, both flags.  Three alternating
rounds: in every round the device is timed first (HIP events over `reps` calls after a warm-up call), then the host (wall clock, `host_items` of the
64 pairs, scaled to the batch).  pystoi is not installed: it is not run and nothing here compares against it.
    python tools/stoi_bench.py [reps] [host_items]          one JSON line per case"""
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from models.utils.metrics import native_stoi  # noqa: E402
from nbss_amd import ops  # noqa: E402
from nbss_amd._lib import hip  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    host_items = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    dev, B, S, rounds = torch.device("cuda:0"), 32, 2, 3
    lib = hip()
    for fs in (8000, 16000):
        g = torch.Generator().manual_seed(fs)
        N = 4 * fs
        target = torch.randn(B, S, N, generator=g)
        target = 0.1 * torch.nn.functional.avg_pool1d(target, 5, 1, 2)  # low-pass noise
        preds = target + 0.03 * torch.randn(B, S, N, generator=g)
        pd, td = preds.to(dev), target.to(dev)
        for ext in (False, True):
            got = ops.stoi(lib, pd, td, fs, ext)  # warm-up
            torch.cuda.synchronize()
            dev_ms, host_ms = [], []
            for _ in range(rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    ops.stoi(lib, pd, td, fs, ext)
                e1.record()
                torch.cuda.synchronize()
                dev_ms.append(e0.elapsed_time(e1) / reps)
                t0 = time.perf_counter()
                want = native_stoi(preds.reshape(-1, N)[:host_items], target.reshape(-1, N)[:host_items], fs, ext)
                host_ms.append((time.perf_counter() - t0) * 1e3 * B * S / host_items)
            err = float((got.reshape(-1)[:host_items].cpu() - want).abs().max())
            print(json.dumps({"fs": fs, "extended": ext, "pairs": B * S, "samples": N, "device_ms_per_call": sorted(dev_ms)[1],
                              "device_ms_rounds": [round(v, 4) for v in dev_ms], "host_ms_per_batch": sorted(host_ms)[1],
                              "host_ms_rounds": [round(v, 1) for v in host_ms], "max_abs_diff_device_host": err}), flush=True)


if __name__ == "__main__":
    main()
