"""nbss_amd.rir: simulate_rir on the host (fp64 closed form) against the restatement of tests/test_rir_kernels.py, on the device against the host
path, and the closed-form helpers around it (beta_sabine, t2n, att2t, the array geometries, the rotation about z)."""
import math

import numpy as np
import pytest
import torch

from nbss_amd.rir import array_geometry, att2t, beta_sabine, rotate_z, simulate_rir, t2n, tail_gauss
from test_rir_kernels import BETA, RCV, ROOM, SRC, gauss, ref_cached, tup

T64 = lambda v: torch.tensor(v, dtype=torch.float64)


@pytest.mark.parametrize("nb,fs,beta", [((1, 1, 1), 8000, BETA), ((5, 4, 3), 8000, BETA), ((8, 7, 6), 8000, BETA), ((3, 2, 4), 16000, BETA),
                                        ((5, 4, 3), 8000, (0.0, 0.7, 0.8, 0.0, 0.5, 0.85))], ids=str)
def test_host_path_against_restatement(nb, fs, beta):
    n = 500
    h = simulate_rir(T64(ROOM), T64(beta), T64(SRC[:2]), T64(RCV[:2]), nb, n, fs)
    h_ref, _ = ref_cached(ROOM, beta, tup(SRC[:2]), tup(RCV[:2]), nb, n, fs)
    assert h.dtype == torch.float64 and h.shape == (2, 2, n)
    assert np.abs(h.numpy() - h_ref).max() <= 1e-12 * np.abs(h_ref).max()


def test_host_batch_and_tail():
    """a batch with per-room nb_img equals its rooms alone; the tail follows the definition"""
    rooms, betas, nbs = [ROOM, (4.0, 3.3, 2.9)], [BETA, (0.6, 0.65, 0.7, 0.75, 0.8, 0.85)], [(5, 4, 3), (8, 7, 6)]
    args = (T64(rooms), T64(betas), T64([SRC[:2]] * 2), T64([RCV[:2]] * 2))
    h = simulate_rir(*args, nbs, 600, 8000)
    for b in range(2):
        assert torch.equal(h[b], simulate_rir(args[0][b], args[1][b], args[2][b], args[3][b], nbs[b], 600, 8000))
    k_d, K, rt60 = 240, 64, [0.3, 0.45]
    ht = simulate_rir(*args, nbs, 600, 8000, t_diff=0.03, rt60=rt60, seed=5)
    for b in range(2):
        h_ref, _ = ref_cached(rooms[b], betas[b], tup(SRC[:2]), tup(RCV[:2]), nbs[b], 600, 8000, x_max=k_d + K / 2)
        assert np.abs(ht[b, ..., :k_d].numpy() - h_ref[..., :k_d]).max() <= 1e-12 * np.abs(h_ref).max()
        g = math.sqrt(float(np.mean(h_ref[1, 0, k_d - K:k_d] ** 2)))
        want = [g * 10.0 ** (-3.0 * (k - k_d) / (8000 * rt60[b])) * gauss(5, b, 1, 0, k) for k in range(k_d, 600)]
        assert np.abs(ht[b, 1, 0, k_d:].numpy() - np.array(want)).max() <= 1e-12 * g
    xi = tail_gauss(0, 0, 0, 0, np.arange(200000))  # a unit Gaussian
    assert abs(xi.mean()) < 0.01 and abs(xi.std() - 1.0) < 0.01


@pytest.mark.gpu
def test_device_against_host():
    """the kernel bar of tests/test_rir_kernels.py, with the host path as the reference and its own sum of magnitudes"""
    dev = torch.device("cuda:0")
    rooms, betas, nbs = [ROOM, (4.0, 3.3, 2.9)], [BETA, (0.6, 0.65, 0.7, 0.75, 0.8, 0.85)], [(5, 4, 3), (8, 7, 6)]
    args = (T64(rooms), T64(betas), T64([SRC[:2]] * 2), T64([RCV[:3]] * 2))
    host = simulate_rir(*args, nbs, 600, 8000)
    got = simulate_rir(*[a.to(dev) for a in args], nbs, 600, 8000)
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == host.shape
    for b in range(2):
        mag = ref_cached(rooms[b], betas[b], tup(SRC[:2]), tup(RCV[:3]), nbs[b], 600, 8000)[1]
        ratio = float((np.abs(got[b].double().cpu().numpy() - host[b].numpy()) / (4e-6 * mag + 1e-9)).max())
        print(f"room {b}: worst |device - host| / (4e-6 S + 1e-9) = {ratio:.3f}")
        assert ratio <= 1.0
    one = simulate_rir(*[a[0].to(dev) for a in args], nbs[0], 600, 8000)  # one room
    assert torch.equal(one, got[0])
    tail_h = simulate_rir(*args, nbs, 600, 8000, t_diff=0.03, rt60=[0.3, 0.45], seed=5)
    tail_d = simulate_rir(*[a.to(dev) for a in args], nbs, 600, 8000, t_diff=0.03, rt60=[0.3, 0.45], seed=5)
    g = tail_h[..., 240 - 64:240].pow(2).mean(-1).sqrt()
    assert float(((tail_d.double().cpu() - tail_h)[..., 240:].abs().amax(-1) / g).max()) <= 1e-5  # host and device tails agree to fp32 rounding


def test_beta_sabine():
    """Sabine by hand for a 5 x 4 x 3 m room: V = 60, walls 12, 12, 15, 15, 20, 20 m^2 (S = 94)"""
    beta, err = beta_sabine([5.0, 4.0, 3.0], 0.5)
    alpha = 0.161 * 60.0 / (0.5 * 94.0)
    assert torch.allclose(beta, torch.full((6,), math.sqrt(1.0 - alpha), dtype=torch.float64), rtol=0, atol=1e-14) and abs(float(err)) < 1e-14
    # unequal weights: the floor absorbs twice as much as every other wall; sum w S = 0.5 (12 + 12 + 15 + 15 + 20) + 20 = 57
    beta, err = beta_sabine([5.0, 4.0, 3.0], 0.5, [1, 1, 1, 1, 2, 1])
    x = 0.161 * 60.0 / (0.5 * 57.0)
    want = [math.sqrt(1.0 - 0.5 * x)] * 4 + [math.sqrt(1.0 - x), math.sqrt(1.0 - 0.5 * x)]
    assert torch.allclose(beta, T64(want), rtol=0, atol=1e-14) and abs(float(err)) < 1e-14
    # out of reach: fully absorbing walls give 0.161 V / S = 0.1028 s, not 0.05 s
    beta, err = beta_sabine([5.0, 4.0, 3.0], 0.05)
    assert float(beta.abs().max()) == 0.0 and abs(float(err) - (0.161 * 60.0 / 94.0 - 0.05)) < 1e-14
    # batched
    beta, err = beta_sabine(T64([[5.0, 4.0, 3.0], [6.0, 5.0, 3.0]]), T64([0.5, 0.4]))
    assert beta.shape == (2, 6) and err.shape == (2,) and abs(float(beta[0, 0]) - math.sqrt(1.0 - alpha)) < 1e-14


def test_t2n_att2t():
    assert att2t(15.0, 0.6) == pytest.approx(0.15) and att2t(60.0, 0.4) == pytest.approx(0.4)
    # 2 T c = 2 * 0.15 * 343 = 102.9 m of path: / 5 = 20.58, / 4 = 25.7, / 3 = 34.3
    assert t2n(0.15, [5.0, 4.0, 3.0]).tolist() == [21, 26, 35]
    assert t2n(T64([0.15, 0.3]), T64([[5.0, 4.0, 3.0], [5.0, 4.0, 3.0]])).tolist() == [[21, 26, 35], [42, 52, 69]]


def test_array_geometries():
    c = array_geometry("circular", 6, 0.05)
    assert c.shape == (6, 3) and torch.allclose(c.norm(dim=1), T64([0.05] * 6)) and float(c[:, 2].abs().max()) == 0.0
    assert torch.allclose(c[0], T64([0.05, 0.0, 0.0])) and float(c[1, 1]) > 0
    assert torch.allclose((c[0] - c[1]).norm(), T64(0.05))  # a hexagon's side is its radius
    cm = array_geometry("circular+cm", 7, 0.05)
    assert cm.shape == (7, 3) and float(cm[0].abs().max()) == 0.0 and torch.allclose(cm[1:], c)
    lin = array_geometry("linear", 4, spacing=0.03)
    assert torch.allclose(lin[:, 0], T64([-0.045, -0.015, 0.015, 0.045])) and float(lin[:, 1:].abs().max()) == 0.0
    with pytest.raises(ValueError, match="chime3"):
        array_geometry("chime3", 6)
    rot = rotate_z(cm, 0.7)
    assert torch.allclose(torch.cdist(rot, rot), torch.cdist(cm, cm), atol=1e-15)
    assert torch.allclose(rot[1], T64([0.05 * math.cos(0.7), 0.05 * math.sin(0.7), 0.0]))
    many = rotate_z(cm.expand(3, 7, 3), T64([0.0, 0.7, math.pi]))
    assert many.shape == (3, 7, 3) and torch.allclose(many[0], cm) and torch.allclose(many[1], rot) and torch.allclose(many[2, :, :2], -cm[:, :2], atol=1e-15)
