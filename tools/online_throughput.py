"""f2 (BASELINE config 5): frames/s of the OnlineSpatialNet streaming step — the native HIP step
(nbss_amd/online.py, HIP graph per chunk) next to the torch.nn step under the same graph capture (OnlineStreamer) and the eager
torch.nn step.  configs/onlineSpatialNet.yaml geometry (8 layers, 129 frequencies, 6 channels -> 2 speakers, ret(2)):
    python tools/online_throughput.py [chunk] [seconds] [attention, e.g. "mhsa(251)" or "mamba(16,4)"] [rounds]
The three streamers are built (and captured) once and then timed ALTERNATELY over `rounds` (default 3) passes over the same signal; one JSON line per
round, then a summary line with each streamer's slowest and fastest round and `native_faster`: the native step's SLOWEST round against the graph-captured
torch step's FASTEST.  A 'mamba(..)' attention sets NBSS_ONLINE_MAMBA=1 (the variant's own switch) and NBSS_ONLINE_NATIVE_MAMBA_STEP=1 (its native step)."""
import json
import os
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from models.arch.OnlineSpatialNet import OnlineSpatialNet, OnlineStreamer  # noqa: E402
from nbss_amd.online import NativeOnlineStreamer  # noqa: E402


def main():
    chunk = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    secs = float(sys.argv[2]) if len(sys.argv) > 2 else 32.0
    attention = sys.argv[3] if len(sys.argv) > 3 else "ret(2)"
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    if attention.startswith("mamba"):
        os.environ["NBSS_ONLINE_MAMBA"] = "1"
        os.environ["NBSS_ONLINE_NATIVE_MAMBA_STEP"] = "1"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = OnlineSpatialNet(dim_input=12, dim_output=4, num_layers=8, dim_squeeze=8, num_freqs=129, encoder_kernel_size=5, dim_hidden=96, dim_ffn=192,
                           num_heads=4, dropout=(0, 0, 0), kernel_size=(5, 3), conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], full_share=0,
                           attention=attention, decay=[4, 5, 9, 10], rope=False).eval().to(dev)
    T = int(secs * 8000) // 128 // chunk * chunk
    x = torch.randn(1, 129, T, 12, device=dev)
    what = {"what": f"OnlineSpatialNet {attention} streaming step, batch 1, 129 frequencies, 8 layers", "chunk_frames": chunk, "frames": T,
            "audio_seconds": T * 128 / 8000}
    streamers = {"native_hip_graph": NativeOnlineStreamer(net, 1, chunk, device=dev, use_graph=True),
                 "torch_nn_graph": OnlineStreamer(net, 1, chunk, device=dev, use_graph=True),
                 "torch_nn_eager": OnlineStreamer(net, 1, chunk, device=dev, use_graph=False)}
    for s in streamers.values():
        s.step(x[:, :, :chunk])  # capture / warm-up
    fps = {name: [] for name in streamers}
    for r in range(rounds):
        out, ref = {**what, "round": r}, None
        for name, s in streamers.items():
            s.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ys = [s.step(x[:, :, c:c + chunk]) for c in range(0, T, chunk)]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            y = torch.cat(ys, 2)
            if ref is None:
                ref = y
            fps[name].append(T / dt)
            out[name] = {"frames_per_s": T / dt, "ms_per_chunk": dt / (T // chunk) * 1e3, "real_time_factor": (T * 128 / 8000) / dt,
                         "rel_l2_vs_native": float((y - ref).norm() / ref.norm())}
        print(json.dumps(out), flush=True)
    summary = {**what, "rounds": rounds, **{name: {"slowest_frames_per_s": min(v), "fastest_frames_per_s": max(v)} for name, v in fps.items()}}
    summary["native_slowest_over_graph_fastest"] = min(fps["native_hip_graph"]) / max(fps["torch_nn_graph"])
    summary["native_faster"] = summary["native_slowest_over_graph_fastest"] > 1.0
    print(json.dumps(summary), flush=True)


main()
