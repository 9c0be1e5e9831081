"""The image-source kernels (nbss_amd/csrc/rir.hip: nbss_rir_ism, nbss_rir_tail) against an fp64 restatement of the definition in
include/nbss_hip.h, on the emulator and, under -m gpu, on the device.

The restatement `ref_rir` is a plain triple loop over the images; it returns h_ref[k] and S[k] = sum |A w| (the sum of the magnitudes).

Bar: |h - h_ref|[k] <= 4e-6 S[k] + 1e-9, derived, not measured: the delay x is split into integer and fraction in fp64, so every fp32
contribution carries a few ulp (<= 1e-6 relative without fast-math), and a fixed-order fp32 sum of n terms adds at most n 6e-8 S (the kernel
accumulates in fp64, which only lowers that share).  Every case prints its worst ratio |h - h_ref| / (4e-6 S + 1e-9).

The LDS image list holds 256 threads x 8 slots = 2048 images per pass (RIR_TILE x RIR_SLOTS in rir.hip); `test_list_overflow` puts 4096 images
into one tile and 16 images into one thread's (nx, ny) pair, so both the pass loop and a thread's resumption run."""
import functools
import math

import numpy as np
import pytest
import torch

from nbss_amd import ops
from nbss_amd._lib import NbssError

LIST_CAPACITY = 2048
ROOM = (3.2, 4.1, 2.6)
BETA = (0.9, 0.7, 0.8, 0.6, 0.5, 0.85)
SRC = [[1.0, 1.5, 1.2], [2.2, 3.0, 0.9], [0.7, 3.6, 1.8]]
RCV = [[1.6, 2.0, 1.3], [1.7, 2.0, 1.3], [1.6, 2.1, 1.3], [2.5, 0.8, 1.1]]
C = 343.0
TW = 8e-3


def reflections(n):
    a = abs(n)
    return (a // 2, (a + 1) // 2) if n >= 0 else ((a + 1) // 2, a // 2)


def image_coord(n, L, s):
    return n * L + s if n % 2 == 0 else (n + 1) * L - s


def window(u, Tk):
    return np.where(np.abs(u) < Tk / 2, 0.5 * (1.0 + np.cos(2.0 * np.pi * u / Tk)) * np.sinc(u), 0.0)  # np.sinc(u) = sin(pi u) / (pi u), 1 at 0


def ref_rir(room, beta, src, rcv, nb, n_samples, fs, c=C, tw=TW, x_max=math.inf):
    """-> (h [S,M,n], S [S,M,n]) in fp64"""
    src, rcv = np.asarray(src, dtype=np.float64), np.asarray(rcv, dtype=np.float64)
    Tk = tw * fs
    h = np.zeros((len(src), len(rcv), n_samples))
    mag = np.zeros_like(h)
    k = np.arange(n_samples, dtype=np.float64)
    for ix in range(nb[0]):
        nx = ix - nb[0] // 2
        for iy in range(nb[1]):
            ny = iy - nb[1] // 2
            for iz in range(nb[2]):
                nz = iz - nb[2] // 2
                amp = 1.0
                for a, n in enumerate((nx, ny, nz)):
                    r0, r1 = reflections(n)
                    amp *= float(beta[2 * a]) ** r0 * float(beta[2 * a + 1]) ** r1  # python: 0.0 ** 0 = 1.0
                for s in range(len(src)):
                    img = np.array([image_coord(n, room[a], src[s, a]) for a, n in enumerate((nx, ny, nz))])
                    for m in range(len(rcv)):
                        d = max(float(np.linalg.norm(img - rcv[m])), 1e-3)
                        x = fs * d / c
                        if not x < x_max:
                            continue
                        lo, hi = max(0, int(x - Tk / 2) - 1), min(n_samples, int(x + Tk / 2) + 2)
                        if lo >= hi:
                            continue
                        t = amp / (4.0 * math.pi * d) * window(k[lo:hi] - x, Tk)
                        h[s, m, lo:hi] += t
                        mag[s, m, lo:hi] += np.abs(t)
    return h, mag


@functools.lru_cache(maxsize=None)
def ref_cached(room, beta, src, rcv, nb, n_samples, fs, x_max=math.inf):
    return ref_rir(room, beta, src, rcv, nb, n_samples, fs, x_max=x_max)


def tup(v):
    return tuple(tuple(r) for r in v)


def run(backend, room, beta, src, rcv, nb, n_samples, fs, **kw):
    """one room -> [S,M,n] fp32 on the CPU"""
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=backend.device)
    return ops.rir_ism(backend.lib, t([room]), t([beta]), t([src]), t([rcv]), nb, n_samples, fs, **kw)[0].cpu()


def check_bar(h, h_ref, mag, what):
    err = np.abs(h.double().numpy() - h_ref)
    ratio = float((err / (4e-6 * mag + 1e-9)).max())
    print(f"{what}: worst |h - h_ref| / (4e-6 S + 1e-9) = {ratio:.3f}")
    assert np.isfinite(h.numpy()).all()
    assert ratio <= 1.0, (what, ratio)


BASE = [((1, 1, 1), 1, 1), ((2, 3, 1), 2, 3), ((3, 2, 4), 3, 4), ((5, 4, 3), 2, 2), ((8, 7, 6), 1, 4)]


@pytest.mark.parametrize("nb,S,M", BASE, ids=lambda v: str(v).replace(" ", ""))
def test_base_cases(backend, nb, S, M):
    h = run(backend, ROOM, BETA, SRC[:S], RCV[:M], nb, 700, 8000)
    h_ref, mag = ref_cached(ROOM, BETA, tup(SRC[:S]), tup(RCV[:M]), nb, 700, 8000)
    check_bar(h, h_ref, mag, f"{backend.name} nb_img {nb} S {S} M {M}")


@pytest.mark.parametrize("n_samples", [1, 65, 255, 256, 257, 700])
def test_output_lengths(backend, n_samples):
    """below one window, and on, before and after a tile edge (the tile is 256 samples)"""
    h = run(backend, ROOM, BETA, SRC[:2], RCV[:2], (3, 2, 4), n_samples, 8000)
    h_ref, mag = ref_cached(ROOM, BETA, tup(SRC[:2]), tup(RCV[:2]), (3, 2, 4), n_samples, 8000)
    assert h.shape == (2, 2, n_samples)
    check_bar(h, h_ref, mag, f"{backend.name} n_samples {n_samples}")


def test_window_clipped_at_both_ends(backend):
    """a source 5 cm from a receiver (x = 1.17: the window starts at k < 0) and an output that ends inside the last image's window"""
    src, rcv = [[1.0, 1.5, 1.2]], [[1.05, 1.5, 1.2], [2.5, 0.8, 1.1]]
    x_far = 8000 * math.dist(src[0], rcv[1]) / C
    for n in (40, int(x_far) + 5):
        h = run(backend, ROOM, BETA, src, rcv, (1, 1, 1), n, 8000)
        h_ref, mag = ref_cached(ROOM, BETA, tup(src), tup(rcv), (1, 1, 1), n, 8000)
        assert abs(h_ref[0, 0, 0]) > 1e-3 and (n == 40 or abs(h_ref[0, 1, -1]) > 1e-4)  # the cuts go through the windows
        check_bar(h, h_ref, mag, f"{backend.name} clipped n {n}")


def test_zero_beta(backend):
    """0^0 = 1: walls that reflect nothing silence exactly the images that touch them"""
    beta = (0.0, 0.7, 0.8, 0.0, 0.5, 0.85)
    h = run(backend, ROOM, beta, SRC[:2], RCV[:2], (5, 4, 3), 500, 8000)
    h_ref, mag = ref_cached(ROOM, beta, tup(SRC[:2]), tup(RCV[:2]), (5, 4, 3), 500, 8000)
    assert np.abs(h_ref).max() > 1e-2
    check_bar(h, h_ref, mag, f"{backend.name} zero beta")


def test_rooms_of_a_batch_are_independent(backend):
    """three rooms with different nb_img in one launch: each bitwise equal to its launch alone"""
    rooms = [ROOM, (4.0, 3.3, 2.9), (3.0, 5.2, 3.1)]
    betas = [BETA, (0.6, 0.65, 0.7, 0.75, 0.8, 0.85), (0.95, 0.9, 0.0, 0.8, 0.75, 0.7)]
    nbs = [(3, 2, 4), (8, 7, 6), (1, 1, 1)]
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=backend.device)
    src, rcv = t([SRC[:2]] * 3), t([RCV[:2]] * 3)
    h = ops.rir_ism(backend.lib, t(rooms), t(betas), src, rcv, nbs, 600, 8000).cpu()
    for b in range(3):
        alone = run(backend, rooms[b], betas[b], SRC[:2], RCV[:2], nbs[b], 600, 8000)
        assert torch.equal(h[b], alone), b
    h_ref, mag = ref_cached(rooms[1], betas[1], tup(SRC[:2]), tup(RCV[:2]), nbs[1], 600, 8000)
    check_bar(h[1], h_ref, mag, f"{backend.name} room 1 of 3")


def test_fs_16000(backend):
    """K = Tw fs = 128"""
    h = run(backend, ROOM, BETA, SRC[:2], RCV[:3], (3, 2, 4), 600, 16000)
    h_ref, mag = ref_cached(ROOM, BETA, tup(SRC[:2]), tup(RCV[:3]), (3, 2, 4), 600, 16000)
    check_bar(h, h_ref, mag, f"{backend.name} fs 16000")


def test_list_overflow(backend):
    """4096 images, nearly all within the first tile: more than the LIST_CAPACITY = 2048 images of one pass, and 16 images per (nx, ny) pair
    against the 8 slots of a thread"""
    room, nb = (0.8, 0.9, 0.7), (16, 16, 16)
    beta = (0.97, 0.95, 0.96, 0.94, 0.93, 0.98)
    src, rcv = [[0.3, 0.5, 0.2]], [[0.6, 0.3, 0.45]]
    assert nb[0] * nb[1] * nb[2] > LIST_CAPACITY and nb[2] > LIST_CAPACITY // 256
    h = run(backend, room, beta, src, rcv, nb, 300, 8000)
    h_ref, mag = ref_cached(room, beta, tup(src), tup(rcv), nb, 300, 8000)
    far = 8000 * math.sqrt(sum((8 * L) ** 2 for L in room)) / C
    assert far < 256 + 64  # every image reaches the first tile's pass loop or the second's
    check_bar(h, h_ref, mag, f"{backend.name} list overflow")


# ---------------------------------------------------------------- known answers
def test_single_image_on_a_sample(backend):
    """d = 1.715 m: x = 40 exactly at fs = 8000, c = 343"""
    h = run(backend, ROOM, (0.0,) * 6, [[1.0, 1.0, 1.0]], [[2.715, 1.0, 1.0]], (1, 1, 1), 128, 8000)[0, 0].double()
    peak = 1.0 / (4.0 * math.pi * 1.715)
    assert abs(float(h[40]) - peak) <= 4e-6 * peak + 1e-9
    rest = torch.cat([h[:40], h[41:]]).abs().max()
    assert float(rest) < 1e-5 * peak, float(rest) / peak


@pytest.mark.parametrize("nb,S,M", BASE, ids=lambda v: str(v).replace(" ", ""))
def test_direct_path_peak(backend, nb, S, M):
    h = run(backend, ROOM, (0.0,) * 6, SRC[:S], RCV[:M], (1, 1, 1), 700, 8000)
    for s in range(S):
        for m in range(M):
            assert int(h[s, m].abs().argmax()) == round(8000 * math.dist(SRC[s], RCV[m]) / C), (s, m)


def test_mirror_symmetry(backend):
    """odd N_x: mirroring source and receiver about x = L_x / 2 and swapping the two x walls gives the same room"""
    nb = (5, 4, 3)
    mir = lambda pts: [[ROOM[0] - p[0], p[1], p[2]] for p in pts]
    beta_m = (BETA[1], BETA[0]) + BETA[2:]
    h = run(backend, ROOM, beta_m, mir(SRC[:2]), mir(RCV[:2]), nb, 700, 8000)
    h_ref, mag = ref_cached(ROOM, BETA, tup(SRC[:2]), tup(RCV[:2]), nb, 700, 8000)
    check_bar(h, h_ref, mag, f"{backend.name} mirrored")


# ---------------------------------------------------------------- contract
def test_repeatable_and_fully_written(backend):
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=backend.device)
    args = (t([ROOM]), t([BETA]), t([SRC[:2]]), t([RCV[:3]]), (8, 7, 6), 300, 8000)
    a = ops.rir_ism(backend.lib, *args)
    out = torch.full((1, 2, 3, 300), float("nan"), dtype=torch.float32, device=backend.device)
    b = ops.rir_ism(backend.lib, *args, out=out)
    assert b.data_ptr() == out.data_ptr()
    assert torch.isfinite(out).all()
    assert torch.equal(a, out)
    # with the tail as well
    out2 = torch.full((1, 2, 3, 300), float("nan"), dtype=torch.float32, device=backend.device)
    c1 = ops.rir_ism(backend.lib, *args, t_diff=0.02, rt60=0.3, seed=3)
    c2 = ops.rir_ism(backend.lib, *args, t_diff=0.02, rt60=0.3, seed=3, out=out2)
    assert torch.isfinite(out2).all() and torch.equal(c1, c2)


def test_workspace_size_is_exact(backend):
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=backend.device)
    nbs = [(3, 2, 4), (8, 7, 6)]
    nb = torch.tensor(nbs, dtype=torch.int32)
    need = backend.lib.nbss_rir_ism_ws_bytes(2, nb.data_ptr())
    assert need == 2 * 16 + 8 * (9 + 21)
    args = (t([ROOM] * 2), t([BETA] * 2), t([SRC[:1]] * 2), t([RCV[:1]] * 2), nbs, 100, 8000)
    ops.rir_ism(backend.lib, *args, ws=ops.scratch(need, backend.device))
    with pytest.raises(NbssError, match="NBSS_EINVAL"):
        ops.rir_ism(backend.lib, *args, ws=ops.scratch(need - 1, backend.device))


def raw_ism(backend, B=1, S=1, M=1, n_samples=100, fs=8000.0, tw=TW, k_d=0, nb=(2, 2, 2)):
    """nbss_rir_ism itself with buffers that are large enough for one room, one source, one receiver whatever the counts say"""
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=backend.device)
    room, beta, src, rcv = t([ROOM]), t([BETA]), t([SRC[:1]]), t([RCV[:1]])
    nbt = torch.tensor([nb], dtype=torch.int32)
    h = torch.zeros(1, 1, 1, 65536, dtype=torch.float32, device=backend.device)
    ws = ops.scratch(1 << 16, backend.device)
    stream = None if backend.name == "emu" else torch.cuda.current_stream().cuda_stream
    return backend.lib.nbss_rir_ism(B, S, M, n_samples, fs, C, tw, k_d, room.data_ptr(), beta.data_ptr(), src.data_ptr(), rcv.data_ptr(), nbt.data_ptr(),
                                    h.data_ptr(), ws.data_ptr(), ws.numel(), stream)


def raw_tail(backend, B=1, S=1, M=1, n_samples=100, fs=8000.0, tw=TW, k_d=64):
    rt = torch.tensor([0.3], dtype=torch.float64, device=backend.device)
    h = torch.zeros(1, 1, 1, 65536, dtype=torch.float32, device=backend.device)
    stream = None if backend.name == "emu" else torch.cuda.current_stream().cuda_stream
    return backend.lib.nbss_rir_tail(B, S, M, n_samples, fs, tw, k_d, rt.data_ptr(), 0, h.data_ptr(), stream)


UNSUPPORTED = -2


def test_limits_are_refused(backend):
    assert raw_ism(backend) == 0
    assert raw_ism(backend, n_samples=65536, nb=(1, 1, 1)) == 0
    assert raw_ism(backend, tw=256 / 8000.0, n_samples=300, nb=(1, 1, 1)) == 0  # Tw fs + 1 = 257
    for kw in (dict(nb=(0, 2, 2)), dict(nb=(2, 513, 2)), dict(nb=(2, 2, -1)), dict(n_samples=0), dict(n_samples=65537), dict(tw=257 / 8000.0),
               dict(B=0), dict(S=0), dict(M=0), dict(k_d=63), dict(k_d=100), dict(k_d=200)):
        assert raw_ism(backend, **kw) == UNSUPPORTED, kw
    assert raw_ism(backend, nb=(512, 1, 1)) == 0
    assert raw_ism(backend, k_d=64) == 0 and raw_ism(backend, k_d=99) == 0
    assert raw_tail(backend) == 0 and raw_tail(backend, k_d=99) == 0
    for kw in (dict(k_d=63), dict(k_d=100), dict(n_samples=0), dict(n_samples=65537), dict(tw=257 / 8000.0), dict(B=0), dict(S=0), dict(M=0)):
        assert raw_tail(backend, **kw) == UNSUPPORTED, kw
    nb = torch.tensor([[2, 2, 513]], dtype=torch.int32)
    assert backend.lib.nbss_rir_ism_ws_bytes(1, nb.data_ptr()) == UNSUPPORTED


# ---------------------------------------------------------------- the diffuse tail
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return z ^ (z >> 31)


def gauss(seed, b, s, m, k):
    key = mix64(mix64(mix64(seed + b) + s) + m)
    h1 = mix64((key + k) & (2 ** 64 - 1))
    h2 = mix64(h1)
    u1, u2 = ((h1 >> 41) + 1) / 2.0 ** 23, (h2 >> 40) / 2.0 ** 24
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)


def test_tail(backend):
    B, S, M, n, fs, t_diff, K = 2, 2, 2, 700, 8000, 0.03, 64
    k_d = 240
    rooms, betas, nbs, rt60 = [ROOM, (4.0, 3.3, 2.9)], [BETA, (0.6, 0.65, 0.7, 0.75, 0.8, 0.85)], [(8, 7, 6), (5, 4, 3)], [0.3, 0.45]
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=backend.device)
    args = (t(rooms), t(betas), t([SRC[:S]] * B), t([RCV[:M]] * B), nbs, n, fs)
    h = ops.rir_ism(backend.lib, *args, t_diff=t_diff, rt60=rt60, seed=11).cpu()
    h2 = ops.rir_ism(backend.lib, *args, t_diff=t_diff, rt60=t(rt60), seed=12).cpu()
    assert torch.equal(h[..., :k_d], h2[..., :k_d]) and not torch.equal(h[..., k_d:], h2[..., k_d:])  # the seed changes the tail only
    worst, worst_g = 0.0, 0.0
    for b in range(B):
        h_ref, mag = ref_cached(rooms[b], betas[b], tup(SRC[:S]), tup(RCV[:M]), nbs[b], n, fs, x_max=k_d + K / 2)
        check_bar(h[b, ..., :k_d], h_ref[..., :k_d], mag[..., :k_d], f"{backend.name} early part of room {b}")
        for s in range(S):
            for m in range(M):
                row = h[b, s, m].double().numpy()
                g = math.sqrt(float(np.mean(row[k_d - K:k_d] ** 2)))  # fp64 mean square of the kernel's own early part
                assert g > 0
                xi = np.array([gauss(11, b, s, m, k) for k in range(k_d, n)])
                want = g * 10.0 ** (-3.0 * np.arange(n - k_d) / (fs * rt60[b])) * xi
                worst = max(worst, float(np.abs(row[k_d:] - want).max()) / g)
                j = int(np.abs(xi[:64]).argmax())  # g as the kernel used it, from its largest early tail sample (fp32 rounding: 6e-8)
                g_kernel = row[k_d + j] / (10.0 ** (-3.0 * j / (fs * rt60[b])) * xi[j])
                worst_g = max(worst_g, abs(g_kernel ** 2 / g ** 2 - 1.0))
    print(f"{backend.name} tail: worst |h - closed form| / g = {worst:.3e}, worst relative error of g^2 = {worst_g:.3e}")
    assert worst <= 1e-5 and worst_g <= 1e-6
