"""Room impulse responses by the image-source method, for simulating rooms where the training runs.

The reference draws its rooms with gpuRIR (generate_rirs.py: generate_rir_gpu), a CUDA-only package, or with rir_generator on the CPU; neither
exists for ROCm.  `simulate_rir` computes the published method itself — Allen & Berkley's image sources of a shoebox room, each image a
Hann-windowed sinc at its fractional delay as the gpuRIR paper describes, optionally a diffuse tail after `t_diff` — by the definition written
down in include/nbss_hip.h (nbss_rir_ism, nbss_rir_tail).  gpuRIR cannot be installed here, so numerical parity with it is NOT pinned: the
definition is the specification, and the tail is this project's own (in the spirit of gpuRIR's, not a port of it).

Device tensors go to the HIP kernels (nbss_amd/csrc/rir.hip; fp32 result), host tensors to an fp64 torch closed form of the same definition
(fp64 result) — the convention of models/utils/metrics.py.  Also here: the closed-form helpers around it (beta_sabine, att2t, t2n), the array
geometries and the rotation about z.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

C_SOUND = 343.0
TW = 8e-3
MIN_DIST = 1e-3
ARRAY_GEOMETRIES = ("circular", "circular+cm", "linear")


# ---------------------------------------------------------------- helpers (closed forms)
def beta_sabine(room_sz, rt60, abs_weights=1.0) -> Tuple[Tensor, Tensor]:
    """Wall reflection coefficients (x0, x1, y0, y1, z0, z1) that give `rt60` by Sabine's formula RT60 = 0.161 V / sum_i alpha_i S_i, with the
    absorption of wall i proportional to abs_weights[i]: w = abs_weights / max(abs_weights), x = clip(0.161 V / (rt60 sum_i w_i S_i), 0, 1),
    alpha_i = x w_i, beta_i = sqrt(1 - alpha_i).  room_sz [..., 3], rt60 [...] -> (beta [..., 6], achieved RT60 - rt60 [...]): the error is zero
    unless the clip was hit (an RT60 below 0.161 V / sum_i w_i S_i is out of reach)."""
    room = torch.as_tensor(room_sz, dtype=torch.float64)
    rt = torch.as_tensor(rt60, dtype=torch.float64, device=room.device)
    w = torch.as_tensor(abs_weights, dtype=torch.float64, device=room.device).expand(6)
    w = w / w.max()
    Lx, Ly, Lz = room[..., 0], room[..., 1], room[..., 2]
    area = torch.stack([Ly * Lz, Ly * Lz, Lx * Lz, Lx * Lz, Lx * Ly, Lx * Ly], -1)
    V = Lx * Ly * Lz
    x = (0.161 * V / (rt * (w * area).sum(-1))).clamp(0.0, 1.0)
    alpha = x[..., None] * w
    achieved = 0.161 * V / (alpha * area).sum(-1)
    return torch.sqrt(1.0 - alpha), achieved - rt


def att2t(att_db, rt60):
    """time after which a room of reverberation time rt60 has decayed by att_db decibels"""
    return att_db / 60.0 * rt60


def t2n(T, room_sz, c: float = C_SOUND) -> Tensor:
    """image counts per axis that cover every reflection arriving before T: ceil(2 T c / room_sz); T [...], room_sz [..., 3] -> int64 [..., 3]"""
    room = torch.as_tensor(room_sz, dtype=torch.float64)
    T = torch.as_tensor(T, dtype=torch.float64, device=room.device)
    return torch.ceil(2.0 * T[..., None] * c / room).long()


def array_geometry(name: str, mic_num: int, radius: float = 0.1, spacing: Optional[float] = None) -> Tensor:
    """microphone positions [mic_num, 3] (fp64) relative to the array centre, in the z = 0 plane:
      circular     mic_num points on a circle of `radius`, the first on +x, counter-clockwise
      circular+cm  the centre first, then mic_num - 1 points on the circle
      linear       mic_num points on the x axis, equally spaced (`spacing`, default 2 radius / (mic_num - 1)) and centred"""
    if name not in ARRAY_GEOMETRIES:
        raise ValueError(f"array geometry {name!r} is not supported (supported: {', '.join(ARRAY_GEOMETRIES)})")
    if name == "linear":
        if spacing is None:
            spacing = 2.0 * radius / max(mic_num - 1, 1)
        x = (torch.arange(mic_num, dtype=torch.float64) - (mic_num - 1) / 2.0) * spacing
        return torch.stack([x, torch.zeros_like(x), torch.zeros_like(x)], 1)
    ring = mic_num - 1 if name == "circular+cm" else mic_num
    if ring < 1:
        raise ValueError(f"{name} needs at least {mic_num - ring + 1} microphones")
    ang = torch.arange(ring, dtype=torch.float64) * (2.0 * math.pi / ring)
    pos = torch.stack([radius * torch.cos(ang), radius * torch.sin(ang), torch.zeros_like(ang)], 1)
    return torch.cat([torch.zeros(1, 3, dtype=torch.float64), pos]) if name == "circular+cm" else pos


def rotate_z(pos: Tensor, angle) -> Tensor:
    """pos [..., M, 3] rotated counter-clockwise about the z axis by angle [...] (radians) -> [..., M, 3]"""
    angle = torch.as_tensor(angle, dtype=pos.dtype, device=pos.device)
    ca, sa = torch.cos(angle)[..., None], torch.sin(angle)[..., None]
    x, y, z = pos[..., 0], pos[..., 1], pos[..., 2]
    return torch.stack(torch.broadcast_tensors(ca * x - sa * y, sa * x + ca * y, z), -1)


# ---------------------------------------------------------------- the diffuse tail's counter hash (integer arithmetic, as the kernel's)
_M64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _mix64_np(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def tail_gauss(seed: int, b: int, s: int, m: int, k: np.ndarray) -> np.ndarray:
    """xi(seed, b, s, m, k) of nbss_rir_tail for an array of sample indices k: fp64 unit Gaussians"""
    key = _mix64((_mix64((_mix64((int(seed) + b) & _M64) + s) & _M64) + m) & _M64)
    with np.errstate(over="ignore"):
        h1 = _mix64_np(np.uint64(key) + np.asarray(k).astype(np.uint64))
    h2 = _mix64_np(h1)
    u1 = ((h1 >> np.uint64(41)).astype(np.float64) + 1.0) / 8388608.0
    u2 = (h2 >> np.uint64(40)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


# ---------------------------------------------------------------- host path (fp64)
def _axis_terms(L: Tensor, b0: Tensor, b1: Tensor, s: Tensor, N: int) -> Tuple[Tensor, Tensor]:
    """image coordinates [S, N] and wall factors [N] along one axis"""
    n = torch.arange(N, dtype=torch.int64) - N // 2
    odd = (n % 2) == 1  # python modulo: also for negative n
    nf = n.double()
    coord = torch.where(odd[None, :], (nf[None, :] + 1.0) * L - s[:, None], nf[None, :] * L + s[:, None])
    a = n.abs()
    r0 = torch.where(n >= 0, a // 2, (a + 1) // 2).double()
    r1 = torch.where(n >= 0, (a + 1) // 2, a // 2).double()
    return coord, torch.pow(b0, r0) * torch.pow(b1, r1)  # torch.pow(0., 0.) = 1


def _host_ism_room(room: Tensor, beta: Tensor, src: Tensor, rcv: Tensor, nb: Sequence[int], n_samples: int, fs: float, c: float, tw: float,
                   x_max: float, budget: int = 1 << 22) -> Tensor:
    S, M = src.shape[0], rcv.shape[0]
    Tk = tw * fs
    half = 0.5 * Tk
    J = int(math.ceil(Tk)) + 1
    cx, fx = _axis_terms(room[0], beta[0], beta[1], src[:, 0], nb[0])
    cy, fy = _axis_terms(room[1], beta[2], beta[3], src[:, 1], nb[1])
    cz, fz = _axis_terms(room[2], beta[4], beta[5], src[:, 2], nb[2])
    dy2 = (cy[:, None, :] - rcv[None, :, 1, None]) ** 2  # [S,M,Ny]
    dz2 = (cz[:, None, :] - rcv[None, :, 2, None]) ** 2
    h = torch.zeros(S * M * n_samples, dtype=torch.float64)
    base = (torch.arange(S * M) * n_samples).reshape(S, M, 1, 1, 1)
    j = torch.arange(J, dtype=torch.float64)
    step = max(1, budget // max(1, S * M * nb[1] * nb[2] * J))
    for i0 in range(0, nb[0], step):
        dx2 = (cx[:, None, i0:i0 + step] - rcv[None, :, 0, None]) ** 2  # [S,M,cx]
        d = torch.sqrt(dx2[:, :, :, None, None] + dy2[:, :, None, :, None] + dz2[:, :, None, None, :]).clamp(min=MIN_DIST)
        A = (fx[i0:i0 + step, None, None] * fy[None, :, None] * fz[None, None, :]) / (4.0 * math.pi * d)
        x = fs * d / c
        keep = (A != 0) & (x < x_max) & (x - half < n_samples)
        A, x, row = A[keep], x[keep], base.expand_as(keep)[keep]
        k = (torch.floor(x - half) + 1.0)[:, None] + j[None, :]  # the first sample with k - x > -half, and the J after it
        u = k - x[:, None]
        w = torch.where(u.abs() < half, 0.5 * (1.0 + torch.cos(2.0 * math.pi * u / Tk)) * torch.sinc(u), torch.zeros_like(u))
        ok = (k >= 0) & (k < n_samples)
        h.index_add_(0, (row[:, None] + k.long())[ok], (A[:, None] * w)[ok])
    return h.reshape(S, M, n_samples)


def _host_rir(room_sz, beta, pos_src, pos_rcv, nb, n_samples, fs, c, tw, t_diff, rt60, seed) -> Tensor:
    from .ops import rir_tail_starts
    B = room_sz.shape[0]
    K = int(round(tw * fs))
    k_ds = [0] * B if t_diff is None else rir_tail_starts(t_diff, fs, B, n_samples, tw, what="simulate_rir")  # one number, or one switch per room
    out = []
    for b in range(B):
        k_d = k_ds[b]
        x_max = k_d + K / 2 if t_diff is not None else math.inf
        h = _host_ism_room(room_sz[b], beta[b], pos_src[b], pos_rcv[b], [int(v) for v in nb[b]], n_samples, fs, c, tw, x_max)
        if t_diff is not None:
            g = h[..., k_d - K:k_d].pow(2).mean(-1).sqrt()
            kk = np.arange(k_d, n_samples)
            decay = torch.pow(torch.tensor(10.0, dtype=torch.float64), -3.0 * torch.from_numpy(kk - k_d).double() / (fs * float(rt60[b])))
            for s in range(h.shape[0]):
                for m in range(h.shape[1]):
                    h[s, m, k_d:] = g[s, m] * decay * torch.from_numpy(tail_gauss(seed, b, s, m, kk))
        out.append(h)
    return torch.stack(out)


# ---------------------------------------------------------------- the public function
def simulate_rir(room_sz: Tensor, beta: Tensor, pos_src: Tensor, pos_rcv: Tensor, nb_img, n_samples: int, fs: float, c: float = C_SOUND, tw: float = TW,
                 t_diff=None, rt60=None, seed: int = 0) -> Tensor:
    """Room impulse responses of one shoebox room or of a batch of rooms.

    room_sz [3] or [B,3] metres; beta [6] / [B,6] reflection coefficients (x0, x1, y0, y1, z0, z1); pos_src [S,3] / [B,S,3]; pos_rcv [M,3] / [B,M,3];
    nb_img (Nx, Ny, Nz) image counts per axis, shared or [B,3] per room (host integers); n_samples output length; fs sampling rate; c speed of
    sound; tw length of the windowed sinc in seconds.  t_diff (seconds, needs rt60: a number or [B]) sums only the images arriving before it
    and continues with the diffuse tail g 10^(-3 (k - k_d) / (fs rt60)) xi(seed, b, s, m, k).  t_diff is one number for the batch or one
    positive value per room (a sequence or a [B] tensor: nbss_rir_ism_rooms, nbss_rir_tail_rooms); None is no tail for any room.  A tail that
    would start outside round(tw fs) <= k_d < n_samples raises ValueError, which names the room for a per-room t_diff.
    Returns [S,M,n_samples] resp. [B,S,M,n_samples]: fp32 from the HIP kernels for tensors on the device, fp64 from the host closed form otherwise.
    The direct-path response is the same call with nb_img = (1, 1, 1) and beta = 0."""
    single = room_sz.dim() == 1
    if single:
        room_sz, beta, pos_src, pos_rcv = room_sz[None], beta[None], pos_src[None], pos_rcv[None]
    B = room_sz.shape[0]
    if room_sz.is_cuda:
        from . import ops
        from ._lib import hip
        h = ops.rir_ism(hip(), room_sz, beta, pos_src, pos_rcv, nb_img, n_samples, fs, c, tw, t_diff, rt60, seed)
    else:
        if room_sz.shape != (B, 3) or beta.shape != (B, 6) or pos_src.shape[::2] != (B, 3) or pos_rcv.shape[::2] != (B, 3):
            raise ValueError("simulate_rir: room_sz [B,3], beta [B,6], pos_src [B,S,3], pos_rcv [B,M,3] expected")
        nb = torch.as_tensor(nb_img).long().reshape(-1, 3)
        nb = nb.expand(B, 3) if nb.shape[0] == 1 else nb
        if nb.shape[0] != B or int(nb.min()) < 1:
            raise ValueError(f"simulate_rir: nb_img must be positive (Nx, Ny, Nz) or [B,3], got {tuple(nb.shape)}")
        if t_diff is not None:
            if rt60 is None:
                raise ValueError("simulate_rir: the diffuse tail (t_diff) needs rt60")
            rt60 = torch.as_tensor(rt60, dtype=torch.float64).reshape(-1)
            rt60 = rt60.expand(B) if rt60.numel() == 1 else rt60
        h = _host_rir(room_sz.double(), beta.double(), pos_src.double(), pos_rcv.double(), nb.tolist(), int(n_samples), float(fs), float(c), float(tw),
                      t_diff, rt60, seed)
    return h[0] if single else h
