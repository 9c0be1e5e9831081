"""SimulatedRoomDataModule(rir='ism'), its YAML, and tools/generate_rirs.py."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from data_loaders.gpu_simulation import SimulatedRoomDataModule, mix_batch
from nbss_amd.rir import simulate_rir

ROOT = Path(__file__).resolve().parent.parent
# small, dead rooms: a CPU batch in well under a second (the images are summed down to 60 dB: about 28 per axis)
SMALL = dict(batch_size=[2, 2], num_samples=[4, 2, 2], audio_time_len=[0.5, 0.5, 0.5], num_channels=3, num_speakers=2, rt60=(0.10, 0.12),
             room_size_lims=((3.0, 3.4), (3.0, 3.4), (3.0, 3.2)), device="cpu")


def first_batch(dm, stage=0):
    return next(iter(dm.batches(stage)))


def draw_sources(dm, stage, gen):
    """the draws of SimulatedRoomDataModule.batches in front of the RIRs"""
    N, bs = int(dm.audio_time_len[stage] * dm.sr), dm.batch_size[min(stage, len(dm.batch_size) - 1)]
    k = torch.hann_window(33, device=dm.device)
    src = torch.randn(bs * dm.S, 1, N, generator=gen, device=dm.device)
    src = torch.nn.functional.conv1d(src, (k / k.sum())[None, None], padding=16).reshape(bs, dm.S, N) * 3.0
    sir = dm.sir[0] + (dm.sir[1] - dm.sir[0]) * torch.rand(bs, generator=gen, device=dm.device)
    snr = dm.snr[0] + (dm.snr[1] - dm.snr[0]) * torch.rand(bs, generator=gen, device=dm.device)
    return bs, src, sir, snr


@pytest.fixture(scope="module")
def ism_batch():
    dm = SimulatedRoomDataModule(rir="ism", **SMALL)
    return dm, first_batch(dm)


def test_ism_batches_keep_the_contract(ism_batch):
    dm, (x, ys, paras) = ism_batch
    assert x.shape == (2, 3, 4000) and ys.shape == (2, 2, 3, 4000) and len(paras) == 2
    assert torch.isfinite(x).all() and torch.isfinite(ys).all() and float(ys.abs().max()) > 0
    assert {"index", "seed", "sample_rate", "snr", "sir"} <= set(paras[0])
    x2, ys2, paras2 = first_batch(SimulatedRoomDataModule(rir="ism", **SMALL))  # the same (index, seed): the same batch
    assert torch.equal(x, x2) and torch.equal(ys, ys2) and paras == paras2


def test_ism_targets_are_direct_path_images(ism_batch):
    dm, (x, ys, paras) = ism_batch
    gen = torch.Generator(device=dm.device).manual_seed(int(paras[0]["seed"]) * 1000003 + int(paras[0]["index"]))
    bs, src, sir, snr = draw_sources(dm, 0, gen)
    sc = dm._ism_scene(bs, gen)
    lims = torch.tensor(SMALL["room_size_lims"], dtype=torch.float64)
    assert ((sc["room_sz"] >= lims[:, 0]) & (sc["room_sz"] <= lims[:, 1])).all()
    assert (sc["pos_rcv"][..., 2] >= 1.0).all() and (sc["pos_rcv"][..., 2] <= 1.5).all() and (sc["pos_src"][..., 2] <= 1.8).all()
    assert ((sc["pos_src"] > 0) & (sc["pos_src"] < sc["room_sz"][:, None])).all() and ((sc["pos_rcv"] > 0) & (sc["pos_rcv"] < sc["room_sz"][:, None])).all()
    V, S = sc["room_sz"].prod(-1), 2 * (sc["room_sz"][:, 0] * sc["room_sz"][:, 1] + sc["room_sz"][:, 0] * sc["room_sz"][:, 2] + sc["room_sz"][:, 1] * sc["room_sz"][:, 2])
    assert (sc["rt60"] >= 0.161 * V / S).all() and sc["n_samples"] == int((float(sc["rt60"].max()) + 0.1) * 8000)
    assert torch.equal(sc["nb_img"], torch.ceil(2 * sc["rt60"][:, None] * 343.0 / sc["room_sz"]).long())
    d = torch.cdist(sc["pos_rcv"], sc["pos_rcv"])
    assert torch.allclose(d, torch.cdist(dm.pos_mics.double(), dm.pos_mics.double()).expand_as(d), atol=1e-12)  # a rigid copy of the array
    rir = simulate_rir(sc["room_sz"], sc["beta"], sc["pos_src"], sc["pos_rcv"], sc["nb_img"], sc["n_samples"], 8000).float()
    dp = simulate_rir(sc["room_sz"], torch.zeros_like(sc["beta"]), sc["pos_src"], sc["pos_rcv"], (1, 1, 1), sc["n_samples"], 8000).float()
    mix, tgt, _ = mix_batch(src, rir, dm.Cs, sir, snr, gen, rir_target=dp)
    assert torch.equal(mix, x) and torch.equal(tgt, ys)
    # and the direct-path RIR is one windowed sinc at the distance's delay
    delay = 8000 * (sc["pos_src"][0, 1] - sc["pos_rcv"][0, 2]).norm() / 343.0
    assert int(dp[0, 1, 2].argmax()) == round(float(delay))
    k0 = round(float(delay))
    assert float(dp[0, 1, 2, :k0 - 33].abs().max()) == 0.0 and float(dp[0, 1, 2, k0 + 33:].abs().max()) == 0.0  # nothing outside its 64-sample window
    assert float(rir[0, 1, 2, k0 + 33:].abs().max()) > 0.0  # the reflections follow


@pytest.mark.gpu
def test_ism_batches_on_the_device():
    """the same module with the rooms simulated by the HIP kernels: contract shapes, finite, repeatable, and close to the host path's batch"""
    kw = dict(SMALL, device="cuda:0")
    x, ys, paras = first_batch(SimulatedRoomDataModule(rir="ism", **kw))
    assert x.is_cuda and x.shape == (2, 3, 4000) and ys.shape == (2, 2, 3, 4000) and torch.isfinite(x).all() and torch.isfinite(ys).all()
    x2, ys2, _ = first_batch(SimulatedRoomDataModule(rir="ism", **kw))
    assert torch.equal(x, x2) and torch.equal(ys, ys2)
    assert max(float(x.abs().max()), float(ys.abs().max())) == pytest.approx(0.9, abs=1e-3) and float(ys.abs().max()) > 0.05  # mix_batch's peak scaling


def test_synthetic_default_is_unchanged():
    """the default path against a recording made here from the class's own pieces: the sources, then `_rirs`, then mix_batch, on one generator"""
    kw = {k: v for k, v in SMALL.items() if k != "room_size_lims"}
    dm = SimulatedRoomDataModule(**kw)
    assert dm.rir == "synthetic"
    for stage in (0, 1):
        x, ys, paras = first_batch(dm, stage)
        gen = torch.Generator(device=dm.device).manual_seed(int(paras[0]["seed"]) * 1000003 + int(paras[0]["index"]))
        bs, src, sir, snr = draw_sources(dm, stage, gen)
        mix, tgt, _ = mix_batch(src, dm._rirs(bs, gen), dm.Cs, sir, snr, gen)
        assert torch.equal(mix, x) and torch.equal(tgt, ys)
    with pytest.raises(ValueError, match="rir"):
        SimulatedRoomDataModule(rir="measured", **kw)


def test_yaml_instantiates():
    from SharedTrainer import _instantiate
    cfg = yaml.safe_load((ROOT / "configs" / "datasets" / "simulated_room_ism.yaml").read_text())
    cfg["data"]["init_args"]["device"] = "cpu"
    dm = _instantiate(cfg["data"])
    assert isinstance(dm, SimulatedRoomDataModule) and dm.rir == "ism" and dm.C == 6 and dm.S == 2
    assert dm.room_size_lims == [(3.0, 8.0), (3.0, 8.0), (3.0, 4.0)] and dm.mic_zlim == (1.0, 1.5) and dm.spk_zlim == (1.0, 1.8) and tuple(dm.rt60) == (0.2, 0.6)
    default = SimulatedRoomDataModule(device="cpu")
    assert default.room_size_lims == dm.room_size_lims and default.mic_zlim == dm.mic_zlim and default.spk_zlim == dm.spk_zlim


KEYS = {"fs", "RT60", "room_sz", "pos_src", "pos_rcv", "pos_noise", "rir", "rir_dp", "rir_noise", "arr_geometry", "selected_channels", "beta"}


def test_generate_rirs_tool(tmp_path):
    cmd = [sys.executable, str(ROOT / "tools" / "generate_rirs.py"), "--rir_dir", str(tmp_path), "--rir_nums", "[2,1,1]", "--device", "cpu", "--fs", "8000",
           "--mic_num", "3", "--spk_num", "2", "--noise_num", "1", "--RT60_lim", "[0.2,0.3]", "--attn_diff", "15", "--arr_geometry", "circular+cm", "--seed", "7"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    files = sorted(p.relative_to(tmp_path).as_posix() for p in tmp_path.rglob("*.npz"))
    assert files == ["test/0.npz", "train/0.npz", "train/1.npz", "validation/0.npz"]
    for f in files:
        z = np.load(tmp_path / f)
        assert set(z.files) == KEYS
        L = int((float(z["RT60"]) + 0.1) * 8000)
        assert int(z["fs"]) == 8000 and 0.2 <= float(z["RT60"]) <= 0.3
        assert z["rir"].shape == (2, 3, L) and z["rir_dp"].shape == (2, 3, L) and z["rir_noise"].shape == (1, 3, L)
        assert z["pos_src"].shape == (2, 3) and z["pos_rcv"].shape == (3, 3) and z["pos_noise"].shape == (1, 3) and z["beta"].shape == (6,)
        assert str(z["arr_geometry"]) == "circular+cm" and z["selected_channels"].tolist() == [0, 1, 2]
        assert np.isfinite(z["rir"]).all() and np.abs(z["rir"][..., -1]).max() > 0  # the diffuse tail reaches the end
        d = np.linalg.norm(z["pos_src"][0] - z["pos_rcv"][0])
        assert int(np.abs(z["rir_dp"][0, 0]).argmax()) == round(8000 * d / 343.0) == int(z["rir"][0, 0].argmax())


def test_generate_rirs_refuses_what_is_out_of_scope(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("generate_rirs_tool", ROOT / "tools" / "generate_rirs.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for flag, word, why in (("--arr_geometry", "chime3", "out of scope"), ("--arr_geometry", "libricss", "out of scope"), ("--arr_geometry", "audiowu", "out of scope"),
                            ("--trajectory", "line", "out of scope"), ("--directivity", "card", "only omnidirectional")):
        with pytest.raises(SystemExit):
            tool.parse_args([flag, word])
        err = capsys.readouterr().err
        assert word in err or flag in err
        assert why in err, (flag, err)
