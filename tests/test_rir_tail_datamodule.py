"""SimulatedRoomDataModule(rir='ism', rir_att_diff=...): per room the images are summed to rir_att_diff dB of that room's decay and the response
continues with the diffuse tail (nbss_amd/rir.py: simulate_rir with a per-room t_diff).  On the host path, and under -m gpu on the device."""
from pathlib import Path

import pytest
import torch
import yaml

from data_loaders.gpu_simulation import SimulatedRoomDataModule, mix_batch
from nbss_amd.rir import att2t, simulate_rir, t2n

ROOT = Path(__file__).resolve().parent.parent
TINY = dict(batch_size=[2, 2], num_samples=[4, 2, 2], audio_time_len=[0.25, 0.25, 0.25], num_channels=3, num_speakers=2, rt60=(0.2, 0.3),
            room_size_lims=((3.0, 4.0), (3.0, 4.0), (3.0, 4.0)), rir="ism")
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]


def first(dm, stage=0):
    return next(iter(dm.batches(stage)))


def batch_generator(dm, paras):
    return torch.Generator(device=dm.device).manual_seed(int(paras[0]["seed"]) * 1000003 + int(paras[0]["index"]))


def draw_sources(dm, stage, gen):
    """the draws of SimulatedRoomDataModule.batches in front of the RIRs"""
    N, bs = int(dm.audio_time_len[stage] * dm.sr), dm.batch_size[min(stage, len(dm.batch_size) - 1)]
    k = torch.hann_window(33, device=dm.device)
    src = torch.randn(bs * dm.S, 1, N, generator=gen, device=dm.device)
    src = torch.nn.functional.conv1d(src, (k / k.sum())[None, None], padding=16).reshape(bs, dm.S, N) * 3.0
    sir = dm.sir[0] + (dm.sir[1] - dm.sir[0]) * torch.rand(bs, generator=gen, device=dm.device)
    snr = dm.snr[0] + (dm.snr[1] - dm.snr[0]) * torch.rand(bs, generator=gen, device=dm.device)
    return bs, src, sir, snr


@pytest.fixture(scope="module", params=DEVICES)
def batches(request):
    """per device: the module with rir_att_diff = 15 and its first batch, and the first batch of the module built without the argument (the host
    path sums 69 images per axis down to 60 dB: two seconds a batch, so it is made once)"""
    dm = SimulatedRoomDataModule(rir_att_diff=15, device=request.param, **TINY)
    return request.param, dm, first(dm), first(SimulatedRoomDataModule(device=request.param, **TINY))


@pytest.fixture
def tail_batch(batches):
    return batches[1], batches[2]


def test_none_is_the_module_without_the_argument(batches):
    device, _, _, (x, ys, paras) = batches
    x2, ys2, paras2 = first(SimulatedRoomDataModule(rir_att_diff=None, device=device, **TINY))
    assert torch.equal(x, x2) and torch.equal(ys, ys2) and paras == paras2


def test_batches_keep_the_contract_and_repeat(batches):
    device, dm, (x, ys, paras), plain = batches
    assert x.device.type == dm.device.type and x.shape == (2, 3, 2000) and ys.shape == (2, 2, 3, 2000) and len(paras) == 2
    assert torch.isfinite(x).all() and torch.isfinite(ys).all() and float(ys.abs().max()) > 0.05
    assert set(paras[0]) == {"index", "seed", "sample_rate", "snr", "sir"}
    assert max(float(x.abs().max()), float(ys.abs().max())) == pytest.approx(0.9, abs=1e-3)  # mix_batch's peak scaling
    x2, ys2, paras2 = first(SimulatedRoomDataModule(rir_att_diff=15, device=device, **TINY))  # the same (index, seed): the same batch
    assert torch.equal(x, x2) and torch.equal(ys, ys2) and paras == paras2
    assert not torch.equal(x, plain[0]) and [p["index"] for p in paras] == [p["index"] for p in plain[2]]


def test_responses_are_simulate_rir_with_the_rooms_own_switch(tail_batch):
    dm, (x, ys, paras) = tail_batch
    gen = batch_generator(dm, paras)
    bs, src, sir, snr = draw_sources(dm, 0, gen)
    rir, rir_dp = dm._ism_rirs(bs, gen)
    mix, tgt, _ = mix_batch(src, rir, dm.Cs, sir, snr, gen, rir_target=rir_dp)
    assert torch.equal(mix, x) and torch.equal(tgt, ys)  # these are the responses the batch was made of
    # the same draws again: the scene, then one integer for the tail's seed, after every draw of the scene
    gen = batch_generator(dm, paras)
    draw_sources(dm, 0, gen)
    sc = dm._ism_scene(bs, gen)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen, device=dm.device))
    n = sc["n_samples"]
    assert n == int((float(sc["rt60"].max()) + 0.1) * 8000) and rir.shape == (2, 2, 3, n)
    t_diff = att2t(15.0, sc["rt60"])
    nb = t2n(t_diff, sc["room_sz"]).cpu()
    assert (nb < sc["nb_img"]).all()  # fewer images than down to 60 dB
    for b in range(bs):  # room b is simulate_rir with t_diff = att2t(15, rt60[b]): the leading rooms, so that the tail's noise is room b's
        lead = simulate_rir(sc["room_sz"][:b + 1], sc["beta"][:b + 1], sc["pos_src"][:b + 1], sc["pos_rcv"][:b + 1], nb[:b + 1], n, 8000,
                            t_diff=float(t_diff[b]), rt60=sc["rt60"][:b + 1], seed=seed)
        assert torch.equal(rir[b], lead[b].float()), b
        k_d = int(torch.ceil(t_diff[b] * 8000 - 1e-9))
        assert float(rir[b, ..., k_d:].abs().min()) > 0.0  # the tail reaches the end of every response
    dp = simulate_rir(sc["room_sz"], torch.zeros_like(sc["beta"]), sc["pos_src"], sc["pos_rcv"], (1, 1, 1), n, 8000).float()
    assert torch.equal(rir_dp, dp)  # the direct-path call is unchanged


@pytest.mark.parametrize("device", DEVICES)
def test_moving_speakers_with_the_switch(device):
    dm = SimulatedRoomDataModule(moving=(0.12, 0.4), rir_att_diff=15, device=device, **TINY)
    x, ys, paras = first(dm)
    assert x.shape == (2, 3, 2000) and ys.shape == (2, 2, 3, 2000) and torch.isfinite(x).all() and torch.isfinite(ys).all()
    assert all(len(p["speed"]) == 2 and all(0.12 <= v <= 0.4 for v in p["speed"]) for p in paras)
    x2, ys2, _ = first(SimulatedRoomDataModule(moving=(0.12, 0.4), rir_att_diff=15, device=device, **TINY))
    assert torch.equal(x, x2) and torch.equal(ys, ys2)


def test_refusals():
    kw = {k: v for k, v in TINY.items() if k != "rir"}
    with pytest.raises(ValueError, match="rir must be 'ism'"):
        SimulatedRoomDataModule(rir="synthetic", rir_att_diff=15, device="cpu", **kw)
    with pytest.raises(ValueError, match="rir must be 'ism'"):
        SimulatedRoomDataModule(rir_att_diff=15, device="cpu", **kw)  # the default is synthetic
    # 1 dB of an RT60 of 0.2 - 0.3 s is 3.3 - 5 ms: 27 - 40 samples, below the K = 64 of the windowed sinc
    dm = SimulatedRoomDataModule(rir_att_diff=1.0, device="cpu", **TINY)
    with pytest.raises(ValueError, match=r"room 0 \(RT60 0\.\d+ s\).*outside 64 <= k_d"):
        first(dm)


@pytest.mark.parametrize("name,base", [("simulated_room_ism_tail", "simulated_room_ism"), ("simulated_room_moving_tail", "simulated_room_moving")])
def test_yamls_instantiate(name, base):
    from SharedTrainer import _instantiate
    cfg = yaml.safe_load((ROOT / "configs" / "datasets" / f"{name}.yaml").read_text())
    init = cfg["data"]["init_args"]
    parent = yaml.safe_load((ROOT / "configs" / "datasets" / f"{base}.yaml").read_text())["data"]["init_args"]
    assert init["rir_att_diff"] == 15 and {k: v for k, v in init.items() if k != "rir_att_diff"} == parent  # the existing configuration, plus the switch
    init["device"], init["convolve"] = "cpu", "fft"
    dm = _instantiate(cfg["data"])
    assert isinstance(dm, SimulatedRoomDataModule) and dm.rir == "ism" and dm.rir_att_diff == 15.0
    assert (dm.moving == (0.12, 0.4, 1.0)) == ("moving" in name)
