"""Offline room-impulse-response sets in the layout the reference's dataset modules read, computed by this project's image-source simulator
(nbss_amd/rir.py: simulate_rir — HIP kernels on the device, the fp64 host path with --device cpu).

    python tools/generate_rirs.py --rir_dir dataset/rirs --rir_nums [40000,5000,3000] --spk_num 2 --noise_num 1 --fs 8000 --mic_num 6 \
        --arr_geometry circular --arr_radius 0.05 --RT60_lim [0.1,1.0] --room_size_lims [[3,8],[3,8],[3,4]] --attn_diff 15 --seed 2023 --device cuda:0

writes <rir_dir>/{train,validation,test}/<index>.npz with the keys
    fs, RT60, room_sz, pos_src [S,3], pos_rcv [M,3], pos_noise [noise_num,3], rir [S,M,L], rir_dp [S,M,L], rir_noise [noise_num,M,L] (absent sources:
    empty arrays), arr_geometry, selected_channels, beta          L = int((RT60 + 0.1) fs)
Static sources only.  Rooms are drawn and simulated in batches (--batch rooms per simulate_rir call, at the length of the batch's longest
response, each file cut to its own L).  --attn_diff D switches every room to the diffuse tail after D dB of its own decay; the switch sample
differs from room to room, and the batch goes through simulate_rir's per-room t_diff (nbss_rir_ism_rooms, nbss_rir_tail_rooms) in one call.
Without it the images are summed down to 60 dB.  Numerical parity with gpuRIR is not pinned (nbss_amd/rir.py)."""
import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from nbss_amd.rir import ARRAY_GEOMETRIES, array_geometry, att2t, beta_sabine, rotate_z, simulate_rir, t2n  # noqa: E402

SPLITS = ("train", "validation", "test")
OUT_OF_SCOPE = {"chime3": "the CHiME-3 tablet array", "libricss": "the LibriCSS array", "audiowu": "the Audio-WU array"}


def parse_args(argv=None):
    lst = lambda s: json.loads(s)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rir_dir", default="dataset/rirs")
    ap.add_argument("--rir_nums", type=lst, default=[8, 2, 2], help="[train, validation, test]")
    ap.add_argument("--spk_num", type=int, default=2)
    ap.add_argument("--noise_num", type=int, default=1)
    ap.add_argument("--fs", type=int, default=8000)
    ap.add_argument("--mic_num", type=int, default=6)
    ap.add_argument("--arr_geometry", default="circular")
    ap.add_argument("--arr_radius", type=float, default=0.05)
    ap.add_argument("--RT60_lim", type=lst, default=[0.1, 1.0])
    ap.add_argument("--room_size_lims", type=lst, default=[[3, 8], [3, 8], [3, 4]])
    ap.add_argument("--mic_zlim", type=lst, default=[1.0, 1.5])
    ap.add_argument("--spk_zlim", type=lst, default=[1.0, 1.8])
    ap.add_argument("--attn_diff", type=float, default=None, help="dB of decay after which the diffuse tail takes over (default: full ISM to 60 dB)")
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--trajectory", default=None, help="moving sources are out of scope")
    ap.add_argument("--directivity", default=None, help="microphone directivity patterns are out of scope")
    args = ap.parse_args(argv)
    if args.arr_geometry in OUT_OF_SCOPE:
        ap.error(f"--arr_geometry {args.arr_geometry}: {OUT_OF_SCOPE[args.arr_geometry]} is out of scope (supported: {', '.join(ARRAY_GEOMETRIES)})")
    if args.arr_geometry not in ARRAY_GEOMETRIES:
        ap.error(f"--arr_geometry {args.arr_geometry}: unknown (supported: {', '.join(ARRAY_GEOMETRIES)})")
    if args.trajectory is not None:
        ap.error("--trajectory: moving sources are out of scope, this tool writes static sources only")
    if args.directivity not in (None, "omni"):
        ap.error("--directivity: only omnidirectional microphones are supported")
    if len(args.rir_nums) != 3:
        ap.error("--rir_nums takes [train, validation, test]")
    return args


def draw_rooms(B, args, gen, geometry):
    """B rooms on the CPU (fp64): the draws of one batch depend on (seed, split, first index) alone"""
    u = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
    lims = torch.tensor(args.room_size_lims, dtype=torch.float64)
    room = lims[:, 0] + (lims[:, 1] - lims[:, 0]) * u(B, 3)
    floor = 0.161 * room.prod(-1) / (2.0 * (room[:, 0] * room[:, 1] + room[:, 0] * room[:, 2] + room[:, 1] * room[:, 2]))
    lo, hi = args.RT60_lim
    rt = lo + (hi - lo) * u(B)
    for _ in range(16):  # redrawn while Sabine's formula cannot reach it in that room
        rt = torch.where(rt < floor, lo + (hi - lo) * u(B), rt)
    rt = torch.maximum(rt, floor)
    xy = lambda margin, n: margin + (room[:, None, :2] - 2.0 * margin) * u(B, n, 2)
    z = lambda lim, n: lim[0] + (lim[1] - lim[0]) * u(B, n, 1)
    centre = torch.cat([xy(0.5, 1), z(args.mic_zlim, 1)], -1)
    pos_rcv = centre + rotate_z(geometry.expand(B, -1, 3), 2.0 * math.pi * u(B))
    pos_src = torch.cat([xy(0.3, args.spk_num), z(args.spk_zlim, args.spk_num)], -1)
    pos_noise = torch.cat([xy(0.3, args.noise_num), z(args.spk_zlim, args.noise_num)], -1)
    return room, rt, beta_sabine(room, rt)[0], pos_src, pos_noise, pos_rcv


def generate(args) -> int:
    dev = torch.device(args.device)
    geometry = array_geometry(args.arr_geometry, args.mic_num, args.arr_radius)
    S, written = args.spk_num, 0
    for split, count in zip(SPLITS, args.rir_nums):
        out = Path(args.rir_dir) / split
        out.mkdir(parents=True, exist_ok=True)
        for i0 in range(0, count, args.batch):
            B = min(args.batch, count - i0)
            gen = torch.Generator().manual_seed(args.seed * 1000003 + SPLITS.index(split) * 100000007 + i0)
            room, rt, beta, pos_src, pos_noise, pos_rcv = draw_rooms(B, args, gen, geometry)
            L = ((rt + 0.1) * args.fs).long().tolist()  # int((RT60 + 0.1) fs)
            to = lambda t: t.to(dev)
            pos_all = torch.cat([pos_src, pos_noise], 1)
            dp = simulate_rir(to(room), to(torch.zeros_like(beta)), to(pos_all), to(pos_rcv), (1, 1, 1), max(L), args.fs)
            if args.attn_diff is None:
                nb = t2n(att2t(60.0, rt), room)
                rir = simulate_rir(to(room), to(beta), to(pos_all), to(pos_rcv), nb, max(L), args.fs)
                rirs = [rir[b, :, :, :L[b]] for b in range(B)]
            else:
                t_diff = att2t(args.attn_diff, rt)  # [B]: every room switches after the same decay, at its own time
                rir = simulate_rir(to(room), to(beta), to(pos_all), to(pos_rcv), t2n(t_diff, room), max(L), args.fs, t_diff=t_diff, rt60=rt, seed=args.seed + i0)
                rirs = [rir[b, :, :, :L[b]] for b in range(B)]
            for b in range(B):
                r = rirs[b].float().cpu().numpy()
                d = dp[b, :, :, :L[b]].float().cpu().numpy()
                np.savez(out / f"{i0 + b}.npz", fs=args.fs, RT60=float(rt[b]), room_sz=room[b].numpy(), pos_src=pos_src[b].numpy(), pos_rcv=pos_rcv[b].numpy(),
                         pos_noise=pos_noise[b].numpy(), rir=r[:S], rir_dp=d[:S], rir_noise=r[S:], arr_geometry=args.arr_geometry,
                         selected_channels=np.arange(args.mic_num), beta=beta[b].numpy())
                written += 1
    return written


if __name__ == "__main__":
    a = parse_args()
    print(f"wrote {generate(a)} RIR files under {a.rir_dir}")
