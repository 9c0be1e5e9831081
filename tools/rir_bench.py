"""Room simulation rates (profiles/README.md, "Room simulation"): RIRs/s and ms per batch of 32 rooms with 2 sources and 6 microphones each, at 8 and
16 kHz, RT60 0.2 / 0.6 / 1.0 s — the full image-source sum down to 60 dB, and the 15-dB switch to the diffuse tail — through nbss_amd.rir.simulate_rir
on the device (HIP events over `reps` calls after a warm-up) beside the fp64 host path of the same function on this box's CPU (one room of the
batch, wall clock, scaled to the batch; skipped above `host_max_images` images per room).
    python tools/rir_bench.py [rooms] [reps] [host_max_images]          one JSON line per case; a "RIR" is one (source, receiver) response
    python tools/rir_bench.py rooms [rooms] [reps] [rounds]             the per-room switch (nbss_rir_ism_rooms, nbss_rir_tail_rooms) at 8 kHz:
        "equal k_d": RT60 0.6 s in every room, the scalar entry points and the _rooms entry points on the same inputs, alternating, `rounds` rounds
        of `reps` calls each (HIP events per round; ms per call: median, min - max over the rounds) and whether the two results are the same bits.
        Both run the same kernels (rir.hip has one image-source and one tail kernel, k_d per room; a scalar k_d is broadcast on the host), so
        the pair now times one kernel through two entry points: it stays as the guard of the broadcast path, in bits and in time;
        "k_d per room": RT60 drawn in 0.2 - 0.6 s, t_diff[b] = att2t(15, RT60[b]), beside the full sum down to 60 dB of the same rooms"""
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from nbss_amd.rir import array_geometry, att2t, beta_sabine, simulate_rir, t2n  # noqa: E402


def scene(B, rt60, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    lims = torch.tensor([[3.0, 8.0], [3.0, 8.0], [3.0, 4.0]], dtype=torch.float64)
    room = lims[:, 0] + (lims[:, 1] - lims[:, 0]) * u(B, 3)
    centre = torch.cat([0.5 + (room[:, None, :2] - 1.0) * u(B, 1, 2), 1.0 + 0.5 * u(B, 1, 1)], -1)
    rcv = centre + array_geometry("circular", 6, 0.05)
    src = torch.cat([0.3 + (room[:, None, :2] - 0.6) * u(B, 2, 2), 1.0 + 0.8 * u(B, 2, 1)], -1)
    rt = torch.full((B,), rt60, dtype=torch.float64)
    return room, beta_sabine(room, rt)[0], src, rcv, rt


def timed(fn, reps, rounds):
    """ms per call of fn, one figure per round of `reps` calls between two HIP events"""
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1]}


def rooms_main():
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    dev, fs = torch.device("cuda:0"), 8000
    # all k_d equal: what the generalisation costs
    room, beta, src, rcv, rt = scene(B, 0.6)
    T = att2t(15.0, 0.6)
    nb, n = t2n(torch.full((B,), T, dtype=torch.float64), room), int(0.7 * fs)
    args = [t.to(dev) for t in (room, beta, src, rcv)]
    scalar = lambda: simulate_rir(*args, nb, n, fs, t_diff=T, rt60=rt, seed=1)
    per_room = lambda: simulate_rir(*args, nb, n, fs, t_diff=[T] * B, rt60=rt, seed=1)
    same = bool(torch.equal(scalar().view(torch.int32), per_room().view(torch.int32)))  # also the warm-up of both
    torch.cuda.synchronize()
    ms = {"scalar": [], "rooms": []}
    for _ in range(rounds):  # alternating: both see the same box
        ms["scalar"] += timed(scalar, reps, 1)
        ms["rooms"] += timed(per_room, reps, 1)
    for k in ("scalar", "rooms"):
        print(json.dumps({"case": "equal k_d", "entry": k, "fs": fs, "rt60": 0.6, "rooms": B, "n_samples": n, "k_d": int(round(T * fs)), "reps": reps,
                          "rounds": rounds, **stats(ms[k]), "same_bits_as_scalar": same}), flush=True)
    # k_d per room
    g = torch.Generator().manual_seed(1)
    rt = 0.2 + 0.4 * torch.rand(B, generator=g, dtype=torch.float64)
    beta = beta_sabine(room, rt)[0]
    args[1] = beta.to(dev)
    Tb = att2t(15.0, rt)
    nb15, nb60, n = t2n(Tb, room), t2n(att2t(60.0, rt), room), int((float(rt.max()) + 0.1) * fs)
    per_room = lambda: simulate_rir(*args, nb15, n, fs, t_diff=Tb, rt60=rt, seed=1)
    full = lambda: simulate_rir(*args, nb60, n, fs)
    finite = bool(torch.isfinite(per_room()).all())
    full()
    torch.cuda.synchronize()
    print(json.dumps({"case": "k_d per room", "entry": "rooms", "fs": fs, "rt60": [float(rt.min()), float(rt.max())], "rooms": B, "n_samples": n,
                      "images_per_room": float(nb15.prod(-1).double().mean()), "reps": reps, "rounds": rounds, **stats(timed(per_room, reps, rounds)),
                      "finite": finite}), flush=True)
    print(json.dumps({"case": "k_d per room", "entry": "full ISM to 60 dB", "fs": fs, "rooms": B, "n_samples": n,
                      "images_per_room": float(nb60.prod(-1).double().mean()), "reps": 1, "rounds": 3, **stats(timed(full, 1, 3))}), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "rooms":
        return rooms_main()
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    host_max = float(sys.argv[3]) if len(sys.argv) > 3 else 1e6
    dev = torch.device("cuda:0")
    for fs in (8000, 16000):
        for rt60 in (0.2, 0.6, 1.0):
            for att in (60.0, 15.0):
                room, beta, src, rcv, rt = scene(B, rt60)
                T = att2t(att, rt60)
                nb = t2n(torch.full((B,), T, dtype=torch.float64), room)
                n = int((rt60 + 0.1) * fs)
                kw = dict(t_diff=T, rt60=rt, seed=1) if att < 60 else {}
                args = [t.to(dev) for t in (room, beta, src, rcv)]
                simulate_rir(*args, nb, n, fs, **kw)  # warm-up
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    h = simulate_rir(*args, nb, n, fs, **kw)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / reps
                images = float(nb.prod(-1).double().mean())
                row = {"fs": fs, "rt60": rt60, "mode": "full ISM to 60 dB" if att == 60 else "diffuse tail after 15 dB", "rooms": B, "n_samples": n,
                       "images_per_room": images, "device_ms_per_batch": ms, "device_rirs_per_s": B * 12 / ms * 1e3, "finite": bool(torch.isfinite(h).all())}
                if images <= host_max:
                    kwh = dict(t_diff=T, rt60=rt[:1], seed=1) if att < 60 else {}
                    t0 = time.perf_counter()
                    simulate_rir(room[:1], beta[:1], src[:1], rcv[:1], nb[:1], n, fs, **kwh)
                    dt = time.perf_counter() - t0
                    row.update(host_ms_per_batch=dt * B * 1e3, host_rirs_per_s=12 / dt)
                print(json.dumps(row), flush=True)


main()
