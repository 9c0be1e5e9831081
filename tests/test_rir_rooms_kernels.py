"""The per-room switch to the diffuse tail (nbss_amd/csrc/rir.hip: nbss_rir_ism_rooms, nbss_rir_tail_rooms; include/nbss_hip.h), on the emulator
and, under -m gpu, on the device.

The acceptance bar has tolerance zero: room b of a `_rooms` call is BITWISE what the scalar entry point gives for that room with k_d = k_d[b].
The scalar tail draws xi(seed, b, s, m, k) with the room's index in its own call, so the single-room result comes from the scalar entry on the
leading b + 1 rooms, of which the last is compared.

Against the host fp64 closed form (nbss_amd.rir.simulate_rir with a per-room t_diff) the bars are those of tests/test_rir_kernels.py, restated here:
the early part |h - h_ref|[k] <= 4e-6 S[k] + 1e-9 with S = sum |A w| (a few fp32 ulp per image, fixed-order sum), the tail within 1e-5 g of the
closed form, and g^2 as the kernel used it within 1e-6 relative of the fp64 mean square of the kernel's own early part.

RIR_ROOMS_PER_LAUNCH = 256 in rir.hip: the k_d of 256 rooms travel in one launch's arguments; `test_more_rooms_than_one_launch` takes 259."""
import functools
import math

import numpy as np
import torch

from nbss_amd import ops
from nbss_amd.rir import simulate_rir, tail_gauss

FS, C, TW, K, N, S, M = 8000, 343.0, 8e-3, 64, 300, 2, 3
ROOMS_PER_LAUNCH = 256
NB = [(3, 3, 3), (5, 4, 3), (4, 5, 2), (5, 5, 3)]
K_D = [0, K, 150, N - 1]  # no cut, the lowest legal value, a mid value, a tail of one sample
UNSUPPORTED, EINVAL = -2, -1


@functools.lru_cache(maxsize=None)
def scene(B, seed=0, S=S, M=M):
    """B rooms of 3-5 m (fp64, host): room_sz [B,3], beta [B,6], pos_src [B,S,3], pos_rcv [B,M,3], rt60 [B]"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    room = 3.0 + 2.0 * u(B, 3)
    beta = 0.6 + 0.35 * u(B, 6)
    src = 0.3 + (room[:, None, :] - 0.6) * u(B, S, 3)
    rcv = 0.5 + (room[:, None, :] - 1.0) * u(B, M, 3)
    return room, beta, src, rcv, 0.2 + 0.3 * u(B)


def stream(backend):
    return None if backend.name == "emu" else torch.cuda.current_stream().cuda_stream


def i32(v):
    return torch.tensor(v, dtype=torch.int32).reshape(-1).contiguous()


def ism(backend, geo, nbs, n, k_d, ws_short=0, h=None):
    """nbss_rir_ism_rooms for a list of k_d, nbss_rir_ism for one number -> (return code, h [B,S,M,n] on the device)"""
    room, beta, src, rcv = [t.to(backend.device).contiguous() for t in geo[:4]]
    B, nb = room.shape[0], i32(nbs)
    ws = ops.scratch(backend.lib.nbss_rir_ism_ws_bytes(B, nb.data_ptr()) - ws_short, backend.device)
    if h is None:
        h = torch.full((B, src.shape[1], rcv.shape[1], n), float("nan"), dtype=torch.float32, device=backend.device)
    rooms = isinstance(k_d, (list, tuple))
    kd = i32(k_d) if rooms else None
    fn = backend.lib.nbss_rir_ism_rooms if rooms else backend.lib.nbss_rir_ism
    rc = fn(B, src.shape[1], rcv.shape[1], n, float(FS), C, TW, kd.data_ptr() if rooms else int(k_d), room.data_ptr(), beta.data_ptr(), src.data_ptr(),
            rcv.data_ptr(), nb.data_ptr(), h.data_ptr(), ws.data_ptr(), ws.numel(), stream(backend))
    return rc, h


def tail(backend, h, k_d, rt60, seed):
    """nbss_rir_tail_rooms / nbss_rir_tail in place on h -> return code"""
    B, S_, M_, n = h.shape
    rt = rt60.to(backend.device).contiguous()
    if isinstance(k_d, (list, tuple)):
        kd = i32(k_d)
        return backend.lib.nbss_rir_tail_rooms(B, S_, M_, n, float(FS), TW, kd.data_ptr(), rt.data_ptr(), seed, h.data_ptr(), stream(backend))
    return backend.lib.nbss_rir_tail(B, S_, M_, n, float(FS), TW, int(k_d), rt.data_ptr(), seed, h.data_ptr(), stream(backend))


def both(backend, geo, nbs, n, k_d, seed):
    """(early part alone, early part and tail) on the CPU; a scalar k_d = 0 has no tail call"""
    rc, h = ism(backend, geo, nbs, n, k_d)
    assert rc == 0
    early = h.clone()
    if isinstance(k_d, (list, tuple)) or k_d > 0:
        assert tail(backend, h, k_d, geo[4], seed) == 0
    return early.cpu(), h.cpu()


def lead(geo, b):
    return tuple(t[:b + 1] for t in geo)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def test_mixed_batch_is_bitwise_the_scalar_entry_points(backend):
    geo = scene(4)
    early, full = both(backend, geo, NB, N, K_D, seed=7)
    assert torch.isfinite(full).all()
    for b, k_d in enumerate(K_D):
        e1, f1 = both(backend, lead(geo, b), NB[:b + 1], N, k_d, seed=7)
        assert same(early[b], e1[b]), ("early part", b)
        assert same(full[b], f1[b]), ("with the tail", b)
    uncut = ism(backend, geo, NB, N, 0)[1].cpu()
    assert same(early[0], uncut[0]) and same(full[0], uncut[0])  # k_d = 0: every image, no tail
    for b in (1, 2):  # the cut removes images, and the tail replaces what follows k_d
        assert not same(early[b], uncut[b]) and not same(full[b, ..., K_D[b]:], early[b, ..., K_D[b]:])
    assert same(full[1, ..., :K], early[1, ..., :K]) and float(full[3, ..., N - 1].abs().min()) > 0.0  # the tail of one sample is written


def test_equal_k_d_is_bitwise_the_scalar_call_on_the_batch(backend):
    geo = scene(4)
    for k_d in (0, 150):
        e_r, f_r = both(backend, geo, NB, N, [k_d] * 4, seed=3)
        e_s, f_s = both(backend, geo, NB, N, k_d, seed=3)
        assert same(e_r, e_s) and same(f_r, f_s), k_d


def test_room_without_tail_is_untouched(backend):
    geo = scene(4)
    rc, h = ism(backend, geo, NB, N, K_D)
    assert rc == 0
    h[0] = torch.arange(h[0].numel(), dtype=torch.float32, device=h.device).reshape(h[0].shape)  # anything: the call may not read or write it
    before = h.cpu().clone()
    assert tail(backend, h, K_D, geo[4], 5) == 0
    after = h.cpu()
    assert same(after[0], before[0])
    for b in (1, 2, 3):
        assert same(after[b, ..., :K_D[b]], before[b, ..., :K_D[b]]) and not same(after[b, ..., K_D[b]:], before[b, ..., K_D[b]:])
    none = before.clone().to(backend.device)
    assert tail(backend, none, [0] * 4, geo[4], 5) == 0 and same(none.cpu(), before)  # no room has a tail: nothing to do


def test_repeatable_and_independent_of_the_order_of_the_rooms(backend):
    geo = scene(4)
    e1, f1 = both(backend, geo, NB, N, K_D, seed=11)
    e2, f2 = both(backend, geo, NB, N, K_D, seed=11)
    assert same(e1, e2) and same(f1, f2)
    perm = [2, 0, 3, 1]
    rc, hp = ism(backend, tuple(t[perm] for t in geo), [NB[p] for p in perm], N, [K_D[p] for p in perm])
    assert rc == 0 and same(hp.cpu(), e1[perm])  # the tail depends on the room's index by definition: the image-source part only


def ref_magnitudes(room, beta, src, rcv, nb, n, x_max):
    """S[s][m][k] = sum over the admitted images of |A w(k - x)|, fp64, by the definition of include/nbss_hip.h"""
    Tk = TW * FS
    k = np.arange(n, dtype=np.float64)
    idx = [np.arange(N_) - N_ // 2 for N_ in nb]
    refl = lambda i: (np.where(i >= 0, np.abs(i) // 2, (np.abs(i) + 1) // 2), np.where(i >= 0, (np.abs(i) + 1) // 2, np.abs(i) // 2))
    fac = [beta[2 * a] ** refl(idx[a])[0] * beta[2 * a + 1] ** refl(idx[a])[1] for a in range(3)]
    amp = (fac[0][:, None, None] * fac[1][None, :, None] * fac[2][None, None, :]).reshape(-1)
    mag = np.zeros((len(src), len(rcv), n))
    for s in range(len(src)):
        co = [np.where(idx[a] % 2 == 0, idx[a] * room[a] + src[s][a], (idx[a] + 1) * room[a] - src[s][a]) for a in range(3)]
        for m in range(len(rcv)):
            d = np.sqrt((co[0][:, None, None] - rcv[m][0]) ** 2 + (co[1][None, :, None] - rcv[m][1]) ** 2 + (co[2][None, None, :] - rcv[m][2]) ** 2)
            d = np.maximum(d.reshape(-1), 1e-3)
            x = FS * d / C
            keep = x < x_max
            u = k[None, :] - x[keep, None]
            w = np.where(np.abs(u) < Tk / 2, 0.5 * (1.0 + np.cos(2.0 * np.pi * u / Tk)) * np.sinc(u), 0.0)
            mag[s, m] = np.abs((amp[keep] / (4.0 * np.pi * d[keep]))[:, None] * w).sum(0)
    return mag


def test_against_the_host_closed_form(backend):
    """rooms 1 .. 3 of the mixed batch (a per-room t_diff has no entry for "no tail"), k_d = K, 150, N - 1"""
    geo = tuple(t[1:] for t in scene(4))
    nbs, k_ds, seed = NB[1:], K_D[1:], 9
    t_diff = [k / FS for k in k_ds]
    host = simulate_rir(*geo[:4], nbs, N, FS, t_diff=t_diff, rt60=geo[4], seed=seed)
    assert host.dtype == torch.float64
    dev = ops.rir_ism(backend.lib, *[t.to(backend.device) for t in geo[:4]], nbs, N, FS, t_diff=torch.tensor(t_diff, dtype=torch.float64), rt60=geo[4], seed=seed).cpu()
    _, raw = both(backend, geo, nbs, N, k_ds, seed)
    assert same(dev, raw)  # ops.rir_ism with a per-room t_diff is the two _rooms calls
    worst, worst_t, worst_g = 0.0, 0.0, 0.0
    for b, k_d in enumerate(k_ds):
        mag = ref_magnitudes(geo[0][b].numpy(), geo[1][b].numpy(), geo[2][b].numpy(), geo[3][b].numpy(), nbs[b], N, k_d + K / 2)
        err = np.abs(dev[b, ..., :k_d].double().numpy() - host[b, ..., :k_d].numpy())
        worst = max(worst, float((err / (4e-6 * mag[..., :k_d] + 1e-9)).max()))
        for s in range(S):
            for m in range(M):
                row = dev[b, s, m].double().numpy()
                g = math.sqrt(float(np.mean(row[k_d - K:k_d] ** 2)))  # fp64 mean square of the kernel's own early part
                assert g > 0
                kk = np.arange(k_d, N)
                xi = tail_gauss(seed, b, s, m, kk)
                decay = 10.0 ** (-3.0 * (kk - k_d) / (FS * float(geo[4][b])))
                worst_t = max(worst_t, float(np.abs(row[k_d:] - g * decay * xi).max()) / g, float(np.abs(row[k_d:] - host[b, s, m, k_d:].numpy()).max()) / g)
                j = int(np.abs(xi[:64]).argmax())  # g as the kernel used it, from its largest early tail sample (fp32 rounding: 6e-8)
                worst_g = max(worst_g, abs((row[k_d + j] / (decay[j] * xi[j])) ** 2 / g ** 2 - 1.0))
    print(f"{backend.name} per-room switch: worst early |h - h_host| / (4e-6 S + 1e-9) = {worst:.3f}, worst tail |h - closed form| / g = {worst_t:.3e}, "
          f"worst relative error of g^2 = {worst_g:.3e}")
    assert worst <= 1.0 and worst_t <= 1e-5 and worst_g <= 1e-6


def test_refusals(backend):
    geo = scene(4)
    sentinel = lambda: torch.full((4, S, M, N), 123.0, dtype=torch.float32, device=backend.device)
    for bad in (1, K - 1, N):
        for b in (0, 2, 3):
            k_ds = [K, 0, 150, N - 1]
            k_ds[b] = bad
            h = sentinel()
            assert ism(backend, geo, NB, N, k_ds, h=h)[0] == UNSUPPORTED, (bad, b)
            assert tail(backend, h, k_ds, geo[4], 0) == UNSUPPORTED, (bad, b)
            assert float((h - 123.0).abs().max()) == 0.0  # refused before anything is launched
    assert ism(backend, geo, NB, N, [K, -1, 150, 0])[0] == EINVAL
    assert ism(backend, geo, NB, N, K_D, ws_short=1)[0] == EINVAL
    assert ism(backend, geo, NB, N, K_D)[0] == 0
    null = backend.lib.nbss_rir_tail_rooms(4, S, M, N, float(FS), TW, None, geo[4].to(backend.device).data_ptr(), 0, sentinel().data_ptr(), stream(backend))
    assert null == EINVAL


def test_more_rooms_than_one_launch(backend):
    """259 rooms against the 256 whose k_d one launch carries: rooms on both sides of the seam against single-room calls"""
    B, n = ROOMS_PER_LAUNCH + 3, 128
    geo = scene(B, seed=1, S=1, M=2)
    geo = (geo[0], geo[1], geo[2], geo[2] + torch.tensor([[[0.9, 0.4, 0.2], [-0.5, 0.8, -0.1]]], dtype=torch.float64), geo[4])  # delays of 15 - 25 samples
    nbs = [(1, 1, 1)] * B
    k_ds = [(0, K, 80, n - 1)[b % 4] for b in range(B)]
    early, full = both(backend, geo, nbs, n, k_ds, seed=2)
    assert torch.isfinite(full).all()
    picked = (0, 1, ROOMS_PER_LAUNCH - 1, ROOMS_PER_LAUNCH, ROOMS_PER_LAUNCH + 1, B - 1)
    assert {k_ds[b] for b in picked} == {0, K, 80, n - 1}
    for b in picked:
        alone = ism(backend, tuple(t[b:b + 1] for t in geo), nbs[:1], n, k_ds[b])[1].cpu()
        assert same(early[b], alone[0]), b
        f1 = both(backend, lead(geo, b), nbs[:b + 1], n, k_ds[b], seed=2)[1]
        assert same(full[b], f1[b]), b
        assert float(early[b].abs().max()) > 1e-2  # the direct path is there


def test_scalar_entry_points_split_their_launches(backend):
    """259 rooms through nbss_rir_ism and nbss_rir_tail with one k_d: the scalar entry points are the per-room launches with every cut equal, so
    they too take a second launch after 256 rooms.  Rooms on both sides of the seam are the bits of the _rooms entry points; rooms of the second
    launch meet the bars of this file against the host closed form."""
    B, k_d, seed = ROOMS_PER_LAUNCH + 3, 150, 4
    geo = scene(B, seed=2, S=1, M=1)
    nbs = [(3, 3, 3)] * B
    e_s, f_s = both(backend, geo, nbs, N, k_d, seed)
    e_r, f_r = both(backend, geo, nbs, N, [k_d] * B, seed)
    assert torch.isfinite(f_s).all()
    for b in (0, ROOMS_PER_LAUNCH - 1, ROOMS_PER_LAUNCH, B - 1):
        assert same(e_s[b], e_r[b]) and same(f_s[b], f_r[b]), b
        assert not same(f_s[b, ..., k_d:], e_s[b, ..., k_d:])  # the tail is written
    host = simulate_rir(*geo[:4], nbs, N, FS, t_diff=k_d / FS, rt60=geo[4], seed=seed)
    worst, worst_t = 0.0, 0.0
    for b in (ROOMS_PER_LAUNCH, B - 1):
        mag = ref_magnitudes(geo[0][b].numpy(), geo[1][b].numpy(), geo[2][b].numpy(), geo[3][b].numpy(), nbs[b], N, k_d + K / 2)
        err = np.abs(f_s[b, ..., :k_d].double().numpy() - host[b, ..., :k_d].numpy())
        worst = max(worst, float((err / (4e-6 * mag[..., :k_d] + 1e-9)).max()))
        row = f_s[b, 0, 0].double().numpy()
        g = math.sqrt(float(np.mean(row[k_d - K:k_d] ** 2)))  # fp64 mean square of the kernel's own early part
        assert g > 0
        kk = np.arange(k_d, N)
        closed = g * 10.0 ** (-3.0 * (kk - k_d) / (FS * float(geo[4][b]))) * tail_gauss(seed, b, 0, 0, kk)
        worst_t = max(worst_t, float(np.abs(row[k_d:] - closed).max()) / g, float(np.abs(row[k_d:] - host[b, 0, 0, k_d:].numpy()).max()) / g)
    print(f"{backend.name} scalar k_d over two launches: worst early |h - h_host| / (4e-6 S + 1e-9) = {worst:.3f}, worst tail |h - closed form| / g = {worst_t:.3e}")
    assert worst <= 1.0 and worst_t <= 1e-5
