"""SimulatedRoomDataModule(moving=...): trajectories of image-source responses, cross-faded along the sources (data_loaders/gpu_simulation.py), and its
YAML.  The convolution itself is tested in tests/test_traj_convolve_kernels.py and tests/test_traj_convolve_module.py; here the draws, the trajectories and
the batch contract, on the host with convolve='fft', and under -m gpu one batch of configs/datasets/simulated_room_moving.yaml against convolve='fft'."""
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from data_loaders.gpu_simulation import SimulatedRoomDataModule, traj_rirs_needed

ROOT = Path(__file__).resolve().parent.parent
# small, dead rooms as in tests/test_rir_datamodule.py, an eighth of a second of audio; at 1 to 2 m/s a trajectory point lasts 200 to 400 samples: 4 to 6 points
SMALL = dict(batch_size=[2, 2], num_samples=[4, 2, 2], audio_time_len=[0.125, 0.125, 0.125], num_channels=3, num_speakers=2, rt60=(0.10, 0.12),
             room_size_lims=((3.0, 3.4), (3.0, 3.4), (3.0, 3.2)), device="cpu", rir="ism")


def rel_l2(y, ref):
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(y - ref) / max(np.linalg.norm(ref), 1e-300))


def first(dm, stage=0):
    return next(iter(dm.batches(stage)))


def test_batch_contract_and_repeatability():
    dm = SimulatedRoomDataModule(**SMALL, moving=(1.0, 2.0))
    x, ys, paras = first(dm)
    assert x.shape == (2, 3, 1000) and ys.shape == (2, 2, 3, 1000) and len(paras) == 2
    assert torch.isfinite(x).all() and torch.isfinite(ys).all() and float(ys.abs().max()) > 0.05
    assert {"index", "seed", "sample_rate", "snr", "sir", "speed"} <= set(paras[0])
    assert all(len(p["speed"]) == 2 and all(1.0 <= v <= 2.0 for v in p["speed"]) for p in paras)
    assert len({v for p in paras for v in p["speed"]}) == 4  # every speaker of every item draws its own speed
    assert max(float(x.abs().max()), float(ys.abs().max())) == pytest.approx(0.9, abs=1e-3)  # mix_batch's peak scaling
    x2, ys2, paras2 = first(SimulatedRoomDataModule(**SMALL, moving=(1.0, 2.0)))
    assert torch.equal(x, x2) and torch.equal(ys, ys2) and paras == paras2
    # the static module is what it was: no 'speed', and another mixture
    xs, _, ps = first(SimulatedRoomDataModule(**SMALL))
    assert "speed" not in ps[0] and not torch.equal(xs, x)


def test_trajectories_stay_in_the_box_and_step_by_traj_dist():
    dm = SimulatedRoomDataModule(**dict(SMALL, room_size_lims=((1.2, 1.5), (1.2, 1.5), (3.0, 3.2))), moving=(1.0, 2.0), traj_dist=0.05)
    gen = torch.Generator(device="cpu").manual_seed(3)
    N, B = 16000, 4  # two seconds at up to 2 m/s in a box under a metre wide: every trajectory is folded several times
    sc, hop, speed, pts = dm._traj_draws(B, N, gen)  # the draws alone: no responses are computed
    P = traj_rirs_needed(N, int(hop.min()))
    assert pts.shape == (B, 2, P, 3) and hop.dtype == torch.int32 and hop.shape == speed.shape == (B, 2)
    assert torch.equal(hop.long(), torch.round(0.05 / speed * 8000).long())
    step = (pts[:, :, 1:] - pts[:, :, :-1]).norm(dim=-1)
    assert float(step.max()) <= 1.5 * 0.05 and float(step.min()) > 0.0
    assert P * 0.05 > 4 * 0.9  # the walk is several boxes long
    room = sc["room_sz"]
    for ax in range(2):
        assert float(pts[..., ax].min()) >= 0.3 - 1e-9 and bool((pts[..., ax] <= room[:, None, None, ax] - 0.3 + 1e-9).all())
    assert float((pts[..., 2] - pts[:, :, :1, 2]).abs().max()) == 0.0  # the height stays


def test_prob_zero_is_a_standing_speaker():
    """(vmin, vmax, 0): nobody walks; all P responses of a speaker are equal, and the batch is the static convolution with the first of them"""
    from data_loaders.gpu_simulation import mix_batch
    dm = SimulatedRoomDataModule(**SMALL, moving=(1.0, 2.0, 0.0))
    gen = torch.Generator(device="cpu").manual_seed(5)
    rir, rir_dp, hop, speed = dm._ism_traj_rirs(2, 1000, gen)
    assert float(speed.abs().max()) == 0.0 and rir.shape[:4] == (2, 2, traj_rirs_needed(1000, int(hop.min())), 3) and rir_dp.shape == rir.shape
    assert torch.equal(rir, rir[:, :, :1].expand_as(rir)) and float(rir.abs().max()) > 0
    # 'switch' through equal responses IS the static convolution
    g = torch.Generator().manual_seed(6)
    wav, white = torch.randn(2, 2, 1000, generator=g), torch.randn(2, 3, 1000, generator=g)
    sir, snr = torch.tensor([1.0, -2.0]), torch.tensor([10.0, 5.0])
    mov = mix_batch(wav, rir, dm.Cs, sir, snr, None, rir_target=rir_dp, white=white, traj_hop=hop, traj_mode="switch")
    sta = mix_batch(wav, rir[:, :, 0].contiguous(), dm.Cs, sir, snr, None, rir_target=rir_dp[:, :, 0].contiguous(), white=white)
    assert rel_l2(mov[0], sta[0]) < 1e-5 and rel_l2(mov[1], sta[1]) < 1e-5
    # prob = 0.5: some stand (speed 0, one point), some walk
    some = SimulatedRoomDataModule(**SMALL, moving=(1.0, 2.0, 0.5))
    _, _, sp, pts = some._traj_draws(8, 1000, torch.Generator(device="cpu").manual_seed(7))
    still = (pts - pts[:, :, :1]).abs().amax((2, 3)) == 0
    assert bool(still.any()) and bool((~still).any()) and torch.equal(still, sp == 0)


def test_value_errors():
    with pytest.raises(ValueError, match="'ism'"):
        SimulatedRoomDataModule(device="cpu", moving=(0.12, 0.4))
    with pytest.raises(ValueError, match="'ism'"):
        SimulatedRoomDataModule(device="cpu", rir="synthetic", moving=(0.12, 0.4))
    for bad in ((0.4,), (0.4, 0.12), (0.0, 0.4), (0.12, 0.4, 1.5), (0.12, 0.4, 0.5, 1.0)):
        with pytest.raises(ValueError, match="moving"):
            SimulatedRoomDataModule(device="cpu", rir="ism", moving=bad)
    with pytest.raises(ValueError, match="ramp"):  # 0.05 m at 25 m/s: 16 samples per point, below the window's ramp
        first(SimulatedRoomDataModule(**SMALL, moving=(25.0, 25.0)))
    assert SimulatedRoomDataModule(device="cpu").moving is None


def test_moving_yaml_instantiates():
    from SharedTrainer import _instantiate
    cfg = yaml.safe_load((ROOT / "configs" / "datasets" / "simulated_room_moving.yaml").read_text())
    init = cfg["data"]["init_args"]
    assert init["rir"] == "ism" and init["convolve"] == "native" and init["moving"] == [0.12, 0.4]
    nat = yaml.safe_load((ROOT / "configs" / "datasets" / "simulated_room_native.yaml").read_text())["data"]["init_args"]
    assert {k: v for k, v in init.items() if k != "moving"} == nat  # the native configuration, plus the speeds
    init["device"] = "cpu"
    with pytest.raises(ValueError, match="'fft'"):  # no HIP device, no native convolution
        _instantiate(cfg["data"])
    init["convolve"] = "fft"
    assert _instantiate(cfg["data"]).moving == (0.12, 0.4, 1.0)


@pytest.mark.gpu
def test_one_batch_of_the_moving_config_against_fft():
    """B = 2, one second, the speeds, rooms and microphones of the YAML: convolve='native' against convolve='fft' on the same draws"""
    init = yaml.safe_load((ROOT / "configs" / "datasets" / "simulated_room_moving.yaml").read_text())["data"]["init_args"]
    kw = dict(init, batch_size=[2, 2], num_samples=[2, 2, 2], audio_time_len=[1.0, 1.0, 1.0], device="cuda")
    x, ys, paras = first(SimulatedRoomDataModule(**kw))
    xf, ysf, parasf = first(SimulatedRoomDataModule(**dict(kw, convolve="fft")))
    assert x.shape == (2, init.get("num_channels", 6), 8000) and x.is_cuda and torch.isfinite(x).all() and torch.isfinite(ys).all()
    assert [p["speed"] for p in paras] == [p["speed"] for p in parasf] and all(0.12 <= v <= 0.4 for p in paras for v in p["speed"])
    print(f"moving batch, native against fft: mix {rel_l2(x.cpu(), xf.cpu()):.3e} targets {rel_l2(ys.cpu(), ysf.cpu()):.3e}")
    assert rel_l2(x.cpu(), xf.cpu()) < 1e-4 and rel_l2(ys.cpu(), ysf.cpu()) < 1e-4  # the bound of tests/test_fir_convolve_module.py for the static pair
