"""Utterances/s of SimulatedRoomDataModule.batches with image-source rooms, with and without the per-room switch to the diffuse tail
(rir_att_diff; profiles/README.md, "Room simulation"): `ism` (static speakers, convolve='fft', the module's default) and `moving` (speakers at
0.12 - 0.4 m/s, convolve='native', as configs/datasets/simulated_room_moving.yaml), each with rir_att_diff None (every image down to 60 dB: the
code path of before the switch) and 15.  Batch 32, 4-s, 6-channel, 2-speaker items at 8 kHz; per row `rounds` rounds, the rows alternating, each
round a fresh iterator: 2 warm-up batches, then `batches` batches under a host clock that ends in a synchronise.
    python tools/sim_tail_throughput.py [batch] [batches] [rounds] [rows]        rows: comma-separated of ism,ism15,moving,moving15 (default: all)
one JSON line per row: utterances/s median, min - max over the rounds"""
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from data_loaders.gpu_simulation import SimulatedRoomDataModule  # noqa: E402

ROWS = {"ism": dict(convolve="fft"), "ism15": dict(convolve="fft", rir_att_diff=15.0),
        "moving": dict(convolve="native", moving=(0.12, 0.4)), "moving15": dict(convolve="native", moving=(0.12, 0.4), rir_att_diff=15.0)}


def one_round(B, nb, kw):
    dm = SimulatedRoomDataModule(batch_size=[B, B], num_samples=[B * (nb + 2), B, B], audio_time_len=[4.0, 4.0, 4.0], device="cuda:0", rir="ism", **kw)
    it = dm.batches(0)
    for _ in range(2):  # warm-up: rocFFT plans, allocator, code objects
        x, ys, _ = next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for x, ys, _ in it:
        n += x.shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), n, bool(torch.isfinite(x).all() and torch.isfinite(ys).all())


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    rows = sys.argv[4].split(",") if len(sys.argv) > 4 else list(ROWS)
    if not torch.cuda.is_available():
        raise SystemExit("sim_tail_throughput.py measures on the device: no HIP device found")
    rates = {r: [] for r in rows}
    info = {}
    for i in range(rounds):
        for r in rows:
            rate, n, finite = one_round(B, nb, ROWS[r])
            rates[r].append(rate)
            info[r] = (n, finite)
            print(json.dumps({"round": i, "row": r, "utt_per_s": rate}), file=sys.stderr, flush=True)
    for r in rows:
        s = sorted(rates[r])
        kw = ROWS[r]
        print(json.dumps({"what": "SimulatedRoomDataModule.batches, stage 0", "row": r, "rir": "ism", "moving": "moving" in kw, "convolve": kw["convolve"],
                          "rir_att_diff": kw.get("rir_att_diff"), "batch": B, "utterances_per_round": info[r][0], "rounds": rounds,
                          "utt_per_s_median": s[len(s) // 2], "utt_per_s_min": s[0], "utt_per_s_max": s[-1], "finite": info[r][1]}), flush=True)


main()
