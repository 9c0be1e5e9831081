"""convolve='native' through data_loaders/gpu_simulation.py: convolve_aligned_native, mix_batch, SimulatedRoomDataModule and its YAML, on the emulator
and, under -m gpu, on the device.

Bar (as in tests/test_fir_convolve_kernels.py), rel-L2 against an fp64 comparator: the larger of twice the error of the shipped fp32 'fft' path on the
same inputs and eps_fp32 sqrt(L).  The comparator of convolve_aligned is numpy.convolve in fp64; the comparator of mix_batch is mix_batch itself
run in fp64 with convolve='fft' on the host (the function follows the dtype of its inputs)."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from data_loaders.gpu_simulation import SimulatedRoomDataModule, convolve_aligned, convolve_aligned_native, diffuse_mixing_matrices, mix_batch

ROOT = Path(__file__).resolve().parent.parent
EPS = float(np.finfo(np.float32).eps)
B, S, M, N, L = 2, 2, 6, 1201, 401


def rel_l2(y, ref):
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(y - ref) / max(np.linalg.norm(ref), 1e-300))


@functools.lru_cache(maxsize=None)
def scene():
    """dry sources, RIRs with one clear direct path per (b, s) and a decaying tail, direct-path-only targets"""
    g = torch.Generator().manual_seed(11)
    wav = torch.randn(B, S, N, generator=g)
    rir = 0.2 * torch.randn(B, S, M, L, generator=g) * torch.exp(-torch.arange(L) / 80.0)
    onset = torch.tensor([[20, 37], [5, 64]])
    k = torch.arange(L)
    rir = rir * (k >= onset[:, :, None, None])
    rir.scatter_(-1, (onset[:, :, None, None] + torch.arange(M)[None, None, :, None] % 3), 1.0)  # channel 0 peaks at the onset, others up to 2 later
    dp = torch.zeros_like(rir).scatter_(-1, (onset[:, :, None, None] + torch.arange(M)[None, None, :, None] % 3), 1.0)
    return wav, rir, dp, onset


def ref_aligned(wav, rir, delay):
    wav, rir = wav.double().numpy(), rir.double().numpy()
    out = np.zeros(rir.shape[:3] + (wav.shape[-1],))
    for b in range(rir.shape[0]):
        for s in range(rir.shape[1]):
            for m in range(rir.shape[2]):
                full = np.concatenate([np.convolve(wav[b, s], rir[b, s, m]), np.zeros(rir.shape[-1])])
                out[b, s, m] = full[delay[b, s]: delay[b, s] + wav.shape[-1]]
    return out


def within_bar(name, native, fft, ref, taps=L):
    e_nat, e_fft = rel_l2(native, ref), rel_l2(fft, ref)
    bar = max(2.0 * e_fft, EPS * taps ** 0.5)
    print(f"{name}: native {e_nat:.3e} fft {e_fft:.3e} bar {bar:.3e}")
    assert e_nat <= bar, (name, e_nat, e_fft, bar)


@pytest.mark.parametrize("with_target", [False, True], ids=["no_target", "rir_target"])
def test_convolve_aligned_native_against_convolve_aligned(backend, with_target):
    wav, rir, dp, onset = scene()
    dev = backend.device
    tgt_rir = dp.to(dev) if with_target else None
    full_n, tgt_n = convolve_aligned_native(wav.to(dev), rir.to(dev), tgt_rir, lib=backend.lib)
    full_f, tgt_f = convolve_aligned(wav.to(dev), rir.to(dev), tgt_rir)
    assert full_n.shape == full_f.shape == (B, S, M, N) and tgt_n.shape == (B, S, M, N) and full_n.device.type == dev.type
    within_bar(f"{backend.name} reverberant", full_n.cpu(), full_f.cpu(), ref_aligned(wav, rir, onset.numpy()))
    if with_target:
        within_bar(f"{backend.name} target", tgt_n.cpu(), tgt_f.cpu(), ref_aligned(wav, dp, onset.numpy()))
        assert tgt_n.data_ptr() != full_n.data_ptr()
    else:
        assert tgt_n is full_n  # the same tensor twice, no second convolution
    # another reference channel: channel 1 peaks one sample later
    full_1, _ = convolve_aligned_native(wav.to(dev), rir.to(dev), None, ref_channel=1, lib=backend.lib)
    within_bar(f"{backend.name} ref_channel 1", full_1.cpu(), convolve_aligned(wav.to(dev), rir.to(dev), None, 1)[0].cpu(), ref_aligned(wav, rir, onset.numpy() + 1))


@functools.lru_cache(maxsize=None)
def mix_inputs():
    wav, rir, dp, _ = scene()
    ang = torch.arange(M) * (2 * np.pi / M)
    pos = torch.stack([0.1 * torch.cos(ang), 0.1 * torch.sin(ang), torch.zeros(M)], 1)
    Cs = diffuse_mixing_matrices(pos, 8000)[1]  # complex128
    white = torch.randn(B, M, N, generator=torch.Generator().manual_seed(12))
    sir, snr = torch.tensor([-3.0, 4.0]), torch.tensor([5.0, 15.0])
    want = mix_batch(wav.double(), rir.double(), Cs, sir.double(), snr.double(), None, rir_target=dp.double(), white=white.double())  # the fp64 comparator
    return Cs, white, sir, snr, want


def test_mix_batch_native_against_fft(backend):
    wav, rir, dp, _ = scene()
    Cs, white, sir, snr, (mix64, tgt64, paras64) = mix_inputs()
    dev = backend.device
    args = (wav.to(dev), rir.to(dev), Cs.to(torch.complex64).to(dev), sir.to(dev), snr.to(dev), None)
    kw = dict(rir_target=dp.to(dev), white=white.to(dev))
    mix_n, tgt_n, par_n = mix_batch(*args, **kw, convolve="native", lib=backend.lib)
    mix_f, tgt_f, par_f = mix_batch(*args, **kw, convolve="fft")
    assert mix_n.shape == (B, M, N) and tgt_n.shape == (B, S, M, N)
    within_bar(f"{backend.name} mix", mix_n.cpu(), mix_f.cpu(), mix64)
    within_bar(f"{backend.name} targets", tgt_n.cpu(), tgt_f.cpu(), tgt64)
    for key in ("snr", "scale"):
        within_bar(f"{backend.name} paras[{key}]", par_n[key].cpu(), par_f[key].cpu(), paras64[key])


def test_default_is_fft_bit_for_bit():
    wav, rir, dp, _ = scene()
    Cs, white, sir, snr, _ = mix_inputs()
    args = (wav, rir, Cs.to(torch.complex64), sir, snr, None)
    a = mix_batch(*args, rir_target=dp, white=white)
    b = mix_batch(*args, rir_target=dp, white=white, convolve="fft")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert SimulatedRoomDataModule(device="cpu").convolve == "fft"


def test_value_errors():
    wav, rir, dp, _ = scene()
    Cs, white, sir, snr, _ = mix_inputs()
    args = (wav, rir, Cs.to(torch.complex64), sir, snr, None)
    with pytest.raises(ValueError, match="'fft' or 'native'"):
        mix_batch(*args, white=white, convolve="direct")
    with pytest.raises(ValueError, match="'fft'"):  # host tensors, no library handed in
        mix_batch(*args, white=white, convolve="native")
    with pytest.raises(ValueError, match="'fft'"):
        convolve_aligned_native(wav, rir)
    with pytest.raises(ValueError, match="'fft' or 'native'"):
        SimulatedRoomDataModule(device="cpu", convolve="rocfft")
    with pytest.raises(ValueError, match="'fft'"):
        SimulatedRoomDataModule(device="cpu", convolve="native")


# small, dead rooms as in tests/test_rir_datamodule.py, a quarter of a second of audio (one workgroup along n): the emulator convolves a batch in about a second
SMALL = dict(batch_size=[2, 2], num_samples=[4, 2, 2], audio_time_len=[0.25, 0.25, 0.25], num_channels=3, num_speakers=2, rt60=(0.10, 0.12),
             room_size_lims=((3.0, 3.4), (3.0, 3.4), (3.0, 3.2)))


def test_datamodule_native_batch_keeps_the_contract(backend):
    kw = dict(SMALL, device=str(backend.device), rir="ism", convolve="native", conv_lib=backend.lib if backend.name == "emu" else None)
    x, ys, paras = next(iter(SimulatedRoomDataModule(**kw).batches(0)))
    assert x.shape == (2, 3, 2000) and ys.shape == (2, 2, 3, 2000) and len(paras) == 2 and x.device.type == backend.device.type
    assert torch.isfinite(x).all() and torch.isfinite(ys).all() and float(ys.abs().max()) > 0.05
    assert {"index", "seed", "sample_rate", "snr", "sir"} <= set(paras[0])
    assert max(float(x.abs().max()), float(ys.abs().max())) == pytest.approx(0.9, abs=1e-3)  # mix_batch's peak scaling
    # and the 'fft' module draws the same scene: the two batches agree to fp32 convolution error
    kw_f = {k: v for k, v in kw.items() if k not in ("convolve", "conv_lib")}
    xf, ysf, _ = next(iter(SimulatedRoomDataModule(**kw_f).batches(0)))
    assert rel_l2(x.cpu(), xf.cpu()) < 1e-4 and rel_l2(ys.cpu(), ysf.cpu()) < 1e-4


def test_native_yaml_instantiates():
    from SharedTrainer import _instantiate
    cfg = yaml.safe_load((ROOT / "configs" / "datasets" / "simulated_room_native.yaml").read_text())
    init = cfg["data"]["init_args"]
    assert init["rir"] == "ism" and init["convolve"] == "native"
    ism = yaml.safe_load((ROOT / "configs" / "datasets" / "simulated_room_ism.yaml").read_text())["data"]["init_args"]
    assert {k: v for k, v in init.items() if k != "convolve"} == ism  # the ism configuration, plus the switch
    init["device"] = "cpu"
    with pytest.raises(ValueError, match="'fft'"):  # the switch reaches the class: no HIP device, no native convolution
        _instantiate(cfg["data"])
    init["convolve"] = "fft"
    assert _instantiate(cfg["data"]).convolve == "fft"
