"""diffuse='native' through data_loaders/gpu_simulation.py: gen_diffuse_noise_native, mix_batch, SimulatedRoomDataModule and its YAML, on the emulator
and, under -m gpu, on the device.

gen_diffuse_noise_native is held to the bar of tests/test_diffuse_noise_kernels.py (rel-L2 against gen_diffuse_noise in fp64: the larger of twice the
fp32 torch path's error and eps_fp32 sqrt(2 nfft + M)); mix_batch to the bars of tests/test_gpu_simulation.py's device test against the fp64 host
pipeline on the same sources, RIRs, SIR / SNR draws and sensor noises: rel 1e-4 on mix and targets, snr within 1e-3 dB, scale within rtol 1e-4."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

import data_loaders.gpu_simulation as gs
from data_loaders.gpu_simulation import SimulatedRoomDataModule, diffuse_mixing_matrices, gen_diffuse_noise, gen_diffuse_noise_native, mix_batch

ROOT = Path(__file__).resolve().parent.parent
EPS = float(np.finfo(np.float32).eps)
B, S, M, N, L = 2, 2, 6, 1201, 401


def rel_l2(y, ref):
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(y - ref) / max(np.linalg.norm(ref), 1e-300))


@functools.lru_cache(maxsize=None)
def array_cs(m=M):
    ang = torch.arange(m) * (2 * np.pi / m)
    pos = torch.stack([0.1 * torch.cos(ang), 0.1 * torch.sin(ang), torch.zeros(m)], 1)
    return diffuse_mixing_matrices(pos, 8000)[1]  # complex128


def test_gen_diffuse_noise_native_against_gen_diffuse_noise(backend):
    dev = backend.device
    white = torch.randn(2, 6, 2100, generator=torch.Generator().manual_seed(3))
    Cs = array_cs()
    ref = gen_diffuse_noise(white.double(), 2000, Cs).numpy()
    got = gen_diffuse_noise_native(white.to(dev), 2000, Cs.to(torch.complex64).to(dev), lib=backend.lib)  # the first 2000 of 2100 samples, as gen_diffuse_noise
    fft = gen_diffuse_noise(white.to(dev), 2000, Cs.to(torch.complex64).to(dev))
    assert got.shape == (2, 6, 2000) and got.dtype == torch.float32 and got.device.type == dev.type
    e_nat, e_fft = rel_l2(got.cpu().numpy(), ref), rel_l2(fft.cpu().numpy(), ref)
    bar = max(2.0 * e_fft, EPS * (2 * 256 + 6) ** 0.5)
    print(f"{backend.name} [2, 6, 2000]: native {e_nat:.3e} torch {e_fft:.3e} bar {bar:.3e}")
    assert e_nat <= bar
    one = gen_diffuse_noise_native(white[0].to(dev), 2000, Cs.to(dev), lib=backend.lib)  # no batch dimension, complex128 matrices: converted
    assert one.shape == (6, 2000) and torch.equal(one, got[0])


@functools.lru_cache(maxsize=None)
def scene():
    """dry sources, RIRs with a clear direct path and a decaying tail, SIR / SNR draws, sensor noises, and the fp64 host pipeline on them"""
    g = torch.Generator().manual_seed(21)
    wav = torch.randn(B, S, N, generator=g)
    rir = 0.2 * torch.randn(B, S, M, L, generator=g) * torch.exp(-torch.arange(L) / 80.0)
    rir[..., 10] = 1.0
    white = torch.randn(B, M, N, generator=g)
    sir, snr = torch.tensor([-3.0, 4.0]), torch.tensor([5.0, 15.0])
    want = mix_batch(wav.double(), rir.double(), array_cs(), sir.double(), snr.double(), None, white=white.double())
    return wav, rir, white, sir, snr, want


@pytest.mark.parametrize("convolve", ["fft", "native"])
def test_mix_batch_native_against_fp64_host(backend, convolve):
    wav, rir, white, sir, snr, (mix64, tgt64, par64) = scene()
    dev = backend.device
    mix, tgt, par = mix_batch(wav.to(dev), rir.to(dev), array_cs().to(torch.complex64).to(dev), sir.to(dev), snr.to(dev), None, white=white.to(dev),
                              convolve=convolve, diffuse="native", lib=backend.lib)
    assert mix.shape == (B, M, N) and tgt.shape == (B, S, M, N) and mix.device.type == dev.type
    e_mix, e_tgt = rel_l2(mix.cpu(), mix64), rel_l2(tgt.cpu(), tgt64)
    print(f"{backend.name} convolve {convolve}: mix {e_mix:.3e} targets {e_tgt:.3e}")
    assert e_mix < 1e-4 and e_tgt < 1e-4
    assert torch.allclose(par["snr"].double().cpu(), par64["snr"], atol=1e-3) and torch.allclose(par["scale"].double().cpu(), par64["scale"], rtol=1e-4)


def test_default_is_fft_bit_for_bit():
    wav, rir, white, sir, snr, _ = scene()
    args = (wav, rir, array_cs().to(torch.complex64), sir, snr, None)
    a = mix_batch(*args, white=white)
    b = mix_batch(*args, white=white, diffuse="fft")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    # and what 'fft' computes is the chain of today: the same ops, written out
    rvbt, _ = gs.convolve_aligned(wav, rir)
    coeff = gs.energy_ratio_coeff(rvbt[:, 0], rvbt[:, 1], sir)
    mix = (rvbt * torch.stack([torch.ones_like(coeff), coeff], 1)[:, :, None, None]).sum(1)
    noise = gen_diffuse_noise(white, N, array_cs().to(torch.complex64), 256)
    noise = noise * gs.energy_ratio_coeff(mix, noise, snr)[:, None, None]
    assert torch.equal(b[2]["snr"], 10 * torch.log10(mix.pow(2).sum((1, 2)) / noise.pow(2).sum((1, 2))))
    dm = SimulatedRoomDataModule(device="cpu")
    assert dm.diffuse == "fft" and dm.convolve == "fft"
    # the draws do not move: a module with the switch spelled out yields the default module's batch
    kw = dict(batch_size=[2, 2], num_samples=[2, 2, 2], audio_time_len=[0.25, 0.25, 0.25], device="cpu")
    x0, y0, _ = next(iter(SimulatedRoomDataModule(**kw).batches(0)))
    x1, y1, _ = next(iter(SimulatedRoomDataModule(**kw, diffuse="fft").batches(0)))
    assert torch.equal(x0, x1) and torch.equal(y0, y1)


def test_value_errors():
    wav, rir, white, sir, snr, _ = scene()
    args = (wav, rir, array_cs().to(torch.complex64), sir, snr, None)
    with pytest.raises(ValueError, match="'fft' or 'native'"):
        mix_batch(*args, white=white, diffuse="wav")
    with pytest.raises(ValueError, match="'fft'"):  # host tensors, no library handed in
        mix_batch(*args, white=white, diffuse="native")
    with pytest.raises(ValueError, match="'fft'"):
        gen_diffuse_noise_native(white, N, array_cs())
    with pytest.raises(ValueError, match="'fft' or 'native'"):
        SimulatedRoomDataModule(device="cpu", diffuse="wav")
    with pytest.raises(ValueError, match="'fft'"):
        SimulatedRoomDataModule(device="cpu", diffuse="native")


def test_native_needs_fp32(emu_lib):
    wav, rir, white, sir, snr, _ = scene()
    with pytest.raises(ValueError, match="fp32"):
        gen_diffuse_noise_native(white.double(), N, array_cs(), lib=emu_lib)


SMALL = dict(batch_size=[2, 2], num_samples=[4, 2, 2], audio_time_len=[0.25, 0.25, 0.25], num_channels=3, num_speakers=2)


def test_datamodule_native_keeps_the_contract_and_is_deterministic(emu_lib):
    dm = SimulatedRoomDataModule(**SMALL, device="cpu", diffuse="native", conv_lib=emu_lib)
    a, b = list(dm.batches(0, 0, 1, 0)), list(dm.batches(0, 0, 1, 0))
    x, ys, paras = a[0]
    assert len(a) == 2 and x.shape == (2, 3, 2000) and ys.shape == (2, 2, 3, 2000) and len(paras) == 2
    assert torch.isfinite(x).all() and torch.isfinite(ys).all()
    assert {"index", "seed", "sample_rate", "snr", "sir"} <= set(paras[0])
    assert max(float(x.abs().max()), float(ys.abs().max())) == pytest.approx(0.9, abs=1e-3)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[1][0], b[1][0]) and not torch.equal(a[0][0], a[1][0])  # per (index, seed)
    # the 'fft' module draws the same scene and the same white noise: the batches agree to fp32 error
    xf, ysf, pf = next(iter(SimulatedRoomDataModule(**SMALL, device="cpu").batches(0, 0, 1, 0)))
    assert rel_l2(x, xf) < 1e-4 and rel_l2(ys, ysf) < 1e-4 and abs(paras[0]["snr"] - pf[0]["snr"]) < 1e-3


def test_all_native_yaml_instantiates():
    from SharedTrainer import _instantiate
    cfg = yaml.safe_load((ROOT / "configs" / "datasets" / "simulated_room_all_native.yaml").read_text())
    init = cfg["data"]["init_args"]
    assert init["rir"] == "ism" and init["convolve"] == "native" and init["diffuse"] == "native"
    nat = yaml.safe_load((ROOT / "configs" / "datasets" / "simulated_room_native.yaml").read_text())["data"]["init_args"]
    assert {k: v for k, v in init.items() if k != "diffuse"} == nat  # the native-convolution configuration, plus the switch
    init["device"], init["convolve"] = "cpu", "fft"
    with pytest.raises(ValueError, match="diffuse='native'"):  # the switch reaches the class: no HIP device, no native kernel
        _instantiate(cfg["data"])
    init["diffuse"] = "fft"
    assert _instantiate(cfg["data"]).diffuse == "fft"


@pytest.mark.gpu
def test_datamodule_all_native_on_the_device():
    dm = SimulatedRoomDataModule(batch_size=[2, 2], num_samples=[4, 2, 2], audio_time_len=[1.0, 1.0, 1.0], device="cuda:0", rir="ism", convolve="native",
                                 diffuse="native", rt60=(0.10, 0.15), room_size_lims=((3.0, 3.4), (3.0, 3.4), (3.0, 3.2)))
    x, ys, paras = next(iter(dm.batches(0)))
    assert x.is_cuda and x.shape == (2, 6, 8000) and ys.shape == (2, 2, 6, 8000)
    assert torch.isfinite(x).all() and torch.isfinite(ys).all()
    assert max(float(x.abs().max()), float(ys.abs().max())) == pytest.approx(0.9, abs=1e-3)
    for p in paras:  # the SNR that mix_batch reports is the one drawn (snr in [0, 20] dB, met by the energy-ratio scaling)
        assert 0.0 - 1e-3 <= p["snr"] <= 20.0 + 1e-3
    fft = SimulatedRoomDataModule(batch_size=[2, 2], num_samples=[4, 2, 2], audio_time_len=[1.0, 1.0, 1.0], device="cuda:0", rir="ism", convolve="native",
                                  rt60=(0.10, 0.15), room_size_lims=((3.0, 3.4), (3.0, 3.4), (3.0, 3.2)))
    xf, _, pf = next(iter(fft.batches(0)))
    assert all(abs(a["snr"] - b["snr"]) < 1e-3 for a, b in zip(paras, pf)) and rel_l2(x.cpu(), xf.cpu()) < 1e-4


@pytest.mark.gpu
def test_coherence_of_the_close_pair_follows_sinc(hip_lib):
    pos = torch.tensor([[0.0, 0, 0], [0.05, 0, 0], [0.2, 0, 0]])
    dsc, Cs = diffuse_mixing_matrices(pos, 8000)
    white = torch.randn(3, 40000, generator=torch.Generator().manual_seed(2)).to("cuda:0")
    x = gen_diffuse_noise_native(white, 40000, Cs.to("cuda:0")).double().cpu()
    X = gs._stft_scipy(x, 256)
    psd = (X.abs() ** 2).mean(-1)
    coh01 = ((X[0] * X[1].conj()).mean(-1) / torch.sqrt(psd[0] * psd[1])).real
    k = torch.arange(4, 60)
    err = float((coh01[k] - dsc[0, 1, k]).abs().mean())
    print(f"mean |coherence - sinc| over bins 4-59: {err:.4f}")
    assert err < 0.05
