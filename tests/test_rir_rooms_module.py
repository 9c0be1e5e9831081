"""simulate_rir / ops.rir_ism with one t_diff per room (nbss_amd/rir.py, nbss_amd/ops.py): the host fp64 closed form, the emulator library and,
under -m gpu, the device.  Room b of a per-room call is the scalar call with t_diff[b]: for b = 0 on that room alone, for b > 0 on the leading
b + 1 rooms (the tail's xi(seed, b, s, m, k) takes the room's index), of which the last is compared — bitwise on every path."""
import math

import pytest
import torch

from nbss_amd import ops
from nbss_amd.rir import simulate_rir

FS, N, K = 8000, 300, 64
NB = [(5, 4, 3), (4, 5, 2), (3, 3, 3)]
T_DIFF = [K / FS, 150 / FS, (N - 1) / FS]  # k_d = 64 (the lowest legal value), 150, 299 (a tail of one sample)
RT60 = [0.25, 0.4, 0.3]


def scene(B=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    room = 3.0 + 2.0 * u(B, 3)
    return (room, 0.6 + 0.35 * u(B, 6), 0.3 + (room[:, None, :] - 0.6) * u(B, 2, 3), 0.5 + (room[:, None, :] - 1.0) * u(B, 3, 3))


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("kind", ["tensor", "list"])
def test_per_room_t_diff_is_the_scalar_call_per_room(device, kind):
    geo = [t.to(device) for t in scene()]
    t_diff = torch.tensor(T_DIFF, dtype=torch.float64, device=device) if kind == "tensor" else list(T_DIFF)
    h = simulate_rir(*geo, NB, N, FS, t_diff=t_diff, rt60=RT60, seed=4)
    assert h.shape == (3, 2, 3, N) and h.dtype == (torch.float64 if device == "cpu" else torch.float32) and torch.isfinite(h).all()
    alone = simulate_rir(*[t[0] for t in geo], NB[0], N, FS, t_diff=T_DIFF[0], rt60=RT60[0], seed=4)  # one room, no batch dimension
    assert same(h[0], alone)
    for b in (1, 2):
        lead = simulate_rir(*[t[:b + 1] for t in geo], NB[:b + 1], N, FS, t_diff=T_DIFF[b], rt60=RT60[:b + 1], seed=4)
        assert same(h[b], lead[b]), b
    full = simulate_rir(*geo, NB, N, FS)
    assert same(h[1, ..., :150], full[1, ..., :150]) and not same(h[1, ..., 150:], full[1, ..., 150:])  # the full sum up to the switch, the tail after it
    one = simulate_rir(*[t[0] for t in geo], NB[0], N, FS, t_diff=[T_DIFF[0]], rt60=RT60[0], seed=4)  # a single room takes a list of one
    assert same(one, alone)


def test_scalar_t_diff_keeps_the_scalar_entry_points(backend, monkeypatch):
    """the names that reach the library, and a scalar t_diff against the per-room path with that value in every room"""
    geo = [t.to(backend.device) for t in scene()]
    names = []
    call = backend.lib.call
    monkeypatch.setattr(backend.lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    h_s = ops.rir_ism(backend.lib, *geo, NB, N, FS, t_diff=0.02, rt60=RT60, seed=1)
    assert names == ["nbss_rir_ism", "nbss_rir_tail"]
    del names[:]
    h_0 = ops.rir_ism(backend.lib, *geo, NB, N, FS, t_diff=torch.tensor(0.02), rt60=RT60, seed=1)  # a tensor without a dimension is a number
    assert names == ["nbss_rir_ism", "nbss_rir_tail"] and same(h_0, h_s)
    del names[:]
    h_r = ops.rir_ism(backend.lib, *geo, NB, N, FS, t_diff=[0.02] * 3, rt60=RT60, seed=1)
    assert names == ["nbss_rir_ism_rooms", "nbss_rir_tail_rooms"] and same(h_r, h_s)
    del names[:]
    ops.rir_ism(backend.lib, *geo, NB, N, FS)
    assert names == ["nbss_rir_ism"]


@pytest.mark.parametrize("device", ["cpu", "emu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
def test_errors_name_the_room(device, request):
    if device == "emu":
        lib = request.getfixturevalue("emu_lib")
        run = lambda geo, **kw: ops.rir_ism(lib, *geo, NB, N, FS, rt60=RT60, **kw)
        dev = "cpu"
    else:
        run = lambda geo, **kw: simulate_rir(*geo, NB, N, FS, rt60=RT60, **kw)
        dev = device
    geo = [t.to(dev) for t in scene()]
    for bad, k_d in ((1 / FS, 1), ((K - 1) / FS, K - 1), (N / FS, N)):
        with pytest.raises(ValueError, match=rf"{K} <= k_d < {N}, got {k_d} for room 1"):
            run(geo, t_diff=[T_DIFF[0], bad, T_DIFF[2]])
    for bad in (None, float("nan"), 0.0, -0.01, math.inf):
        with pytest.raises(ValueError, match=r"room 2 must be a positive number"):
            run(geo, t_diff=[T_DIFF[0], T_DIFF[1], bad])
    with pytest.raises(ValueError, match="one value per room, B = 3, got 2"):
        run(geo, t_diff=torch.tensor(T_DIFF[:2], dtype=torch.float64))
    assert torch.isfinite(run(geo, t_diff=T_DIFF)).all()
