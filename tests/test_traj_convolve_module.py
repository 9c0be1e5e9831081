"""Moving sources through data_loaders/gpu_simulation.py: traj_weights, convolve_traj_aligned ('fft' on the host, 'native' on the emulator and, under
-m gpu, on the device) and mix_batch(traj_hop=...).

The host path is pinned to the reference's own convolve_traj_with_win(..., 'trapezium20') and convolve_traj (utils/mix.py) through
tests/golden/traj_convolve.npz (tests/golden/make_golden_traj.py).  Bar of the native path, as in tests/test_traj_convolve_kernels.py: rel-L2 against an
fp64 comparator (the 'fft' path run in fp64: the functions follow the dtype of their inputs) no larger than the larger of twice the error of the fp32 'fft'
path on the same inputs and eps_fp32 sqrt(2 L)."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from data_loaders.gpu_simulation import (convolve_aligned, convolve_traj_aligned, diffuse_mixing_matrices, mix_batch, traj_rirs_needed, traj_weights)

GOLDEN = Path(__file__).parent / "golden" / "traj_convolve.npz"
EPS = float(np.finfo(np.float32).eps)
B, S, M, N, L, RAMP = 2, 2, 3, 601, 97, 20
HOP = [[100, 64], [257, 21]]  # H - ramp even and odd, above the kernel's tile, just above the ramp


def rel_l2(y, ref):
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(y - ref) / max(np.linalg.norm(ref), 1e-300))


def within_bar(name, native, fft, ref, taps=L):
    e_nat, e_fft = rel_l2(native, ref), rel_l2(fft, ref)
    bar = max(2.0 * e_fft, EPS * (2 * taps) ** 0.5)
    print(f"{name}: native {e_nat:.3e} fft {e_fft:.3e} bar {bar:.3e}")
    assert e_nat <= bar, (name, e_nat, e_fft, bar)


def golden_cases():
    g = np.load(GOLDEN)
    for i, (n, hop, taps) in enumerate(g["cases"].tolist()):
        yield n, hop, taps, g[f"x16_{i}"] / 16.0, g[f"h16_{i}"] / 16.0, g[f"win_{i}"], g[f"switch_{i}"]


def test_traj_weights_are_the_reference_windows_laid_along_the_source():
    """at the fixture's (N, hop): the window as the reference builds it (mix.py:219-225, restated here), laid over [(p - 1) hop, (p + 1) hop) for point p
    and cut to [0, N).  The recorded reference OUTPUTS pin the same weights through test_fft_path_on_the_host_against_the_reference_fixture"""
    for n, hop, _, _, _, _, _ in golden_cases():
        P = traj_rirs_needed(n, hop)
        w = traj_weights(n, hop, "trapezium", RAMP, dtype=torch.float64).numpy()
        assert w.shape == (P, n)
        z = (hop - RAMP) // 2
        o = hop - RAMP - z
        win = np.concatenate([np.zeros(z), np.arange(RAMP) / (RAMP - 1), np.ones(2 * o), np.arange(RAMP - 1, -1, -1) / (RAMP - 1), np.zeros(z)])
        want = np.zeros((P, (P + 1) * hop))
        for p in range(P):  # the window of point p covers the samples [(p - 1) hop, (p + 1) hop)
            want[p, p * hop: (p + 2) * hop] = win
        assert np.array_equal(w, want[:, hop: hop + n])
        sw = traj_weights(n, hop, "switch").numpy()
        assert sw.shape == (traj_rirs_needed(n, hop, "switch"), n) and np.array_equal(sw.sum(0), np.ones(n))
        assert np.array_equal(sw.argmax(0), np.arange(n) // hop)
    w = traj_weights(50, torch.tensor([[21, 30]]), P=5)  # a hop per item, surplus rows are zero
    assert w.shape == (1, 2, 5, 50) and float(w[0, 1, 3:].abs().max()) == 0.0
    assert torch.equal(w[0, 0, :4], traj_weights(50, 21, P=4)) and torch.equal(w[0, 1, :3], traj_weights(50, 30))


def test_fft_path_on_the_host_against_the_reference_fixture():
    """convolve_traj_aligned('fft') = the reference's full output cut at the argmax of the first trajectory point's reference channel
    (chime3_moving.py:204, mix.py:247-252); fp64 inputs, so what remains is the reference's float32 accumulation: <= 1e-5 absolute"""
    for n, hop, taps, x, h, win, switch in golden_cases():
        wav, rir, hp = torch.tensor(x)[None, None], torch.tensor(h)[None, None], torch.tensor([[hop]])
        for ref_channel in (0, 1):
            d = int(np.argmax(h[0, ref_channel]))
            pad = lambda a: np.concatenate([a, np.zeros((2, taps))], -1)[:, d: d + n]
            got, tgt = convolve_traj_aligned(wav, rir, hp, ramp=RAMP, ref_channel=ref_channel)
            assert tgt is got and got.shape == (1, 1, 2, n)
            assert np.abs(got[0, 0].numpy() - pad(win)).max() <= 1e-5
            P0 = traj_rirs_needed(n, hop, "switch")
            got0, _ = convolve_traj_aligned(wav, rir[:, :, :P0], hp, mode="switch", ref_channel=ref_channel)
            assert np.abs(got0[0, 0].numpy() - pad(switch)).max() <= 1e-5


@functools.lru_cache(maxsize=None)
def scene():
    """dry sources, a trajectory of RIRs per (b, s) whose direct path wanders by a sample per point, direct-path-only targets"""
    g = torch.Generator().manual_seed(21)
    P = traj_rirs_needed(N, 21)
    wav = torch.randn(B, S, N, generator=g)
    k = torch.arange(L)
    onset = torch.tensor([[20, 37], [5, 64]])[:, :, None, None, None] + (torch.arange(P)[None, None, :, None, None] % 4) + (torch.arange(M)[None, None, None, :, None] % 3)
    rir = 0.2 * torch.randn(B, S, P, M, L, generator=g) * torch.exp(-k / 30.0) * (k >= onset)
    rir.scatter_(-1, onset, 1.0)
    dp = torch.zeros_like(rir).scatter_(-1, onset, 1.0)
    return wav, rir, dp, torch.tensor(HOP, dtype=torch.int32)


@pytest.mark.parametrize("mode", ["trapezium", "switch"])
@pytest.mark.parametrize("with_target", [False, True], ids=["no_target", "rir_target"])
def test_native_against_fft(backend, with_target, mode):
    wav, rir, dp, hop = scene()
    dev = backend.device
    tgt = dp.to(dev) if with_target else None
    full_n, tgt_n = convolve_traj_aligned(wav.to(dev), rir.to(dev), hop.to(dev), tgt, mode=mode, convolve="native", lib=backend.lib)
    full_f, tgt_f = convolve_traj_aligned(wav.to(dev), rir.to(dev), hop.to(dev), tgt, mode=mode)
    full_64, tgt_64 = convolve_traj_aligned(wav.double(), rir.double(), hop, dp.double() if with_target else None, mode=mode)
    assert full_n.shape == full_f.shape == (B, S, M, N) and tgt_n.shape == (B, S, M, N) and full_n.device.type == dev.type
    within_bar(f"{backend.name} {mode} reverberant", full_n.cpu(), full_f.cpu(), full_64)
    if with_target:
        within_bar(f"{backend.name} {mode} target", tgt_n.cpu(), tgt_f.cpu(), tgt_64)
        assert tgt_n.data_ptr() != full_n.data_ptr()
    else:
        assert tgt_n is full_n
    full_1, _ = convolve_traj_aligned(wav.to(dev), rir.to(dev), hop.to(dev), tgt, mode=mode, ref_channel=1, convolve="native", lib=backend.lib)
    within_bar(f"{backend.name} {mode} ref_channel 1", full_1.cpu(), convolve_traj_aligned(wav.to(dev), rir.to(dev), hop.to(dev), tgt, mode=mode, ref_channel=1)[0].cpu(),
               convolve_traj_aligned(wav.double(), rir.double(), hop, dp.double() if with_target else None, mode=mode, ref_channel=1)[0])
    assert rel_l2(full_1.cpu(), full_64) > 1e-3  # another channel, another delay


@functools.lru_cache(maxsize=None)
def mix_inputs():
    ang = torch.arange(M) * (2 * np.pi / M)
    pos = torch.stack([0.1 * torch.cos(ang), 0.1 * torch.sin(ang), torch.zeros(M)], 1)
    Cs = diffuse_mixing_matrices(pos, 8000)[1]
    white = torch.randn(B, M, N, generator=torch.Generator().manual_seed(22))
    return Cs, white, torch.tensor([-3.0, 4.0]), torch.tensor([5.0, 15.0])


def test_mix_batch_with_a_trajectory(backend):
    wav, rir, dp, hop = scene()
    Cs, white, sir, snr = mix_inputs()
    dev = backend.device
    args = (wav.to(dev), rir.to(dev), Cs.to(torch.complex64).to(dev), sir.to(dev), snr.to(dev), None)
    kw = dict(rir_target=dp.to(dev), white=white.to(dev), traj_hop=hop.to(dev))
    mix_n, tgt_n, par_n = mix_batch(*args, **kw, convolve="native", lib=backend.lib)
    mix_f, tgt_f, par_f = mix_batch(*args, **kw)
    mix64, tgt64, par64 = mix_batch(wav.double(), rir.double(), Cs, sir.double(), snr.double(), None, rir_target=dp.double(), white=white.double(), traj_hop=hop)
    assert mix_n.shape == (B, M, N) and tgt_n.shape == (B, S, M, N)
    within_bar(f"{backend.name} mix", mix_n.cpu(), mix_f.cpu(), mix64)
    within_bar(f"{backend.name} targets", tgt_n.cpu(), tgt_f.cpu(), tgt64)
    for key in ("snr", "scale"):
        within_bar(f"{backend.name} paras[{key}]", par_n[key].cpu(), par_f[key].cpu(), par64[key])


@pytest.mark.parametrize("convolve", ["fft", "native"])
def test_a_constant_trajectory_is_the_static_mix_batch(backend, convolve):
    """all P responses equal and H - ramp even (z = o: down(r) + up(r) = 1 at every r): the static mix_batch within fp32 round-off.  Measured against the
    static batch in fp64; the allowance is the fp32 'fft' static batch's own error plus eps sqrt(2 L) for the second rounding of x w"""
    wav, rir, dp, _ = scene()
    Cs, white, sir, snr = mix_inputs()
    dev = backend.device
    P = traj_rirs_needed(N, 64)
    hop = torch.tensor([[100, 64], [256, 64]], dtype=torch.int32)
    assert all((h - RAMP) % 2 == 0 for row in hop.tolist() for h in row)
    r0, d0 = rir[:, :, 0].contiguous(), dp[:, :, 0].contiguous()
    rP, dP = r0[:, :, None].expand(B, S, P, M, L).contiguous(), d0[:, :, None].expand(B, S, P, M, L).contiguous()
    common = (Cs.to(torch.complex64).to(dev), sir.to(dev), snr.to(dev), None)
    lib = dict(convolve=convolve, lib=backend.lib) if convolve == "native" else {}
    mov = mix_batch(wav.to(dev), rP.to(dev), *common, rir_target=dP.to(dev), white=white.to(dev), traj_hop=hop.to(dev), **lib)
    sta = mix_batch(wav.to(dev), r0.to(dev), *common, rir_target=d0.to(dev), white=white.to(dev))
    s64 = mix_batch(wav.double(), r0.double(), Cs, sir.double(), snr.double(), None, rir_target=d0.double(), white=white.double())
    for name, a, b, c in (("mix", mov[0], sta[0], s64[0]), ("targets", mov[1], sta[1], s64[1]), ("snr", mov[2]["snr"], sta[2]["snr"], s64[2]["snr"])):
        e_mov, e_sta = rel_l2(a.cpu(), c), rel_l2(b.cpu(), c)
        print(f"{backend.name} {convolve} {name}: moving {e_mov:.3e} static {e_sta:.3e}")
        assert e_mov <= 2.0 * e_sta + EPS * (2 * L) ** 0.5


def test_value_errors():
    wav, rir, dp, hop = scene()
    Cs, white, sir, snr = mix_inputs()
    args = (wav, rir, Cs.to(torch.complex64), sir, snr, None)
    with pytest.raises(ValueError, match="'fft' or 'native'"):
        convolve_traj_aligned(wav, rir, hop, convolve="direct")
    with pytest.raises(ValueError, match="'fft'"):  # host tensors, no library handed in
        convolve_traj_aligned(wav, rir, hop, convolve="native")
    with pytest.raises(ValueError, match="'fft'"):
        mix_batch(*args, white=white, traj_hop=hop, convolve="native")
    with pytest.raises(ValueError, match="'switch' or 'trapezium'"):
        convolve_traj_aligned(wav, rir, hop, mode="hann")
    with pytest.raises(ValueError, match="'switch' or 'trapezium'"):
        traj_weights(100, 30, "tri")
    with pytest.raises(ValueError, match="too few"):
        convolve_traj_aligned(wav, rir[:, :, :-1], hop)
    with pytest.raises(ValueError, match="ramp"):
        convolve_traj_aligned(wav, rir, torch.tensor([[100, 64], [257, 20]]))
    with pytest.raises(ValueError, match="hop"):
        convolve_traj_aligned(wav, rir, torch.tensor([[100, 64], [0, 21]]), mode="switch")
    with pytest.raises(ValueError, match=r"\[B,S,P,M,L\]"):
        convolve_traj_aligned(wav, rir[:, :, 0], hop)
    with pytest.raises(ValueError, match="traj_hop"):  # a trajectory without hops, hops without a trajectory
        mix_batch(*args, white=white)
    with pytest.raises(ValueError, match="traj_hop"):
        mix_batch(wav, rir[:, :, 0], *args[2:], white=white, traj_hop=hop)
    with pytest.raises(ValueError, match="rir_target"):
        convolve_traj_aligned(wav, rir, hop, dp[:, :, :-1])


def test_native_reports_invalid_items_as_value_errors(backend):
    wav, rir, dp, hop = scene()
    dev = backend.device
    with pytest.raises(ValueError, match="too few"):
        convolve_traj_aligned(wav.to(dev), rir[:, :, :-1].to(dev), hop.to(dev), convolve="native", lib=backend.lib)
