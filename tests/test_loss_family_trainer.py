"""The loss family through the trainer: the command line selects it, the fused step (`fit`, engine.TrainStep) trains with neg_snr / neg_sa_sdr,
the module path (TrainModule.training_step) computes the same thing, cc_mse takes the module sequence and is refused by the fused step."""
from pathlib import Path

import pytest
import torch

from SharedTrainer import TrainCLI, TrainModule, build_module, parse_cli

ROOT = Path(__file__).resolve().parent.parent
SYN = str(ROOT / "configs" / "datasets" / "synthetic.yaml")
ONLINE = ["fit", "--config", str(ROOT / "configs" / "onlineSpatialNet.yaml"), "--config", SYN, "--model.arch.dim_input=12", "--model.arch.dim_output=4",
          "--model.arch.num_freqs=129", "--model.arch.num_layers=1"]


def test_cli_selects_neg_snr_for_online_spatialnet():
    """7. the reference's onlineSpatialNet.yaml trains with neg_snr: one override gives its objective"""
    _, c = parse_cli(ONLINE + ["--model.loss.init_args.loss_func=models.io.loss.neg_snr"])
    m = build_module(c)
    assert m.loss.name == "neg_snr" and m.loss.pit and m.loss.is_scale_invariant_loss is False
    assert "loss_func=neg_snr()" in repr(m.loss)
    _, c = parse_cli(ONLINE + ["--model.loss.init_args.loss_func=models.io.loss.neg_sa_sdr", "--model.loss.init_args.loss_func_kwargs={scale_invariant: true}"])
    m = build_module(c)
    assert m.loss.name == "neg_sa_sdr" and m.loss.is_scale_invariant_loss is True and "neg_sa_sdr(scale_invariant=True,)" in repr(m.loss)


def _tiny_online(loss):
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    from models.io.norm import Norm
    from models.io.stft import STFT
    torch.manual_seed(0)
    arch = OnlineSpatialNet(dim_input=4, dim_output=4, num_layers=1, dim_squeeze=8, num_freqs=9, encoder_kernel_size=5, dim_hidden=32, dim_ffn=64, num_heads=4,
                            dropout=(0, 0, 0), kernel_size=(5, 3), conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], full_share=0,
                            attention="ret(2)", decay=[4, 5, 9, 10], rope=False)
    return TrainModule(arch=arch, channels=[0, 1], ref_channel=0, stft=STFT(n_fft=16, n_hop=8), norm=Norm(mode="frequency", online=True), loss=loss)


def _tiny_batch(B=2, C=2, S=2, N=400, seed=1):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(B, S, N, generator=g)
    ys = torch.stack([src * (0.6 + 0.1 * c) for c in range(C)], 2)  # [B,S,C,N]
    return ys.sum(1) + 0.05 * torch.randn(B, C, N, generator=g), ys


@pytest.mark.parametrize("loss_func", ["neg_snr", "neg_sa_sdr", "cc_mse"])
def test_training_step_passes_loss_paras_on_the_host(loss_func):
    """training_step hands the forward's loss_paras to the loss (cc_mse needs out / XrMM / stft): the host path runs every loss and differentiates"""
    from models.io.loss import Loss
    m = _tiny_online(Loss(f"models.io.loss.{loss_func}", pit=True))
    x, ys = _tiny_batch()
    loss = m.training_step((x, ys, None))
    loss.backward()
    assert loss.shape == () and torch.isfinite(loss)
    gn = [p.grad.norm() for p in m.arch.parameters() if p.grad is not None]
    assert gn and all(torch.isfinite(v) for v in gn) and sum(float(v) for v in gn) > 0
    if loss_func == "cc_mse":  # what it computed: the MSE between the network output and the normalised target spectrum, best pairing
        with torch.no_grad():
            yr = ys[:, :, 0]
            _, paras = m.forward(x)
            tgt = torch.view_as_real(m.stft.stft(yr)[0] / paras["XrMM"])
            out = torch.view_as_real(paras["out"])
            want = torch.stack([torch.stack([((out[:, list(pm)] - tgt) ** 2).reshape(2, -1).mean(1) for pm in ((0, 1), (1, 0))]).min(0).values]).mean()
        assert abs(float(loss.detach()) - float(want)) < 1e-5 * max(1.0, abs(float(want)))


def test_cc_mse_is_not_fusable_and_the_fused_step_refuses_it_by_name():
    from SharedTrainer import _fused_step_for
    base = ["fit", "--config", str(ROOT / "configs" / "SpatialNet.yaml"), "--config", SYN, "--model.arch.dim_input=12", "--model.arch.dim_output=4",
            "--model.arch.num_freqs=129"]
    _, c = parse_cli(base + ["--model.loss.init_args.loss_func=models.io.loss.cc_mse"])
    m = build_module(c)
    assert m.loss.name == "cc_mse" and not m._fusable()  # TrainModule.forward takes the module sequence, whose loss_paras carry out / stft
    with pytest.raises(NotImplementedError, match="cc_mse"):
        _fused_step_for(m, c, torch.device("cpu"))
    _, c = parse_cli(base + ["--model.loss.init_args.loss_func=models.io.loss.neg_snr"])
    assert build_module(c)._fusable()
    from nbss_amd.engine import TrainStep
    with pytest.raises(NotImplementedError, match="cc_mse"):
        TrainStep(None, loss="cc_mse")


@pytest.mark.gpu
@pytest.mark.parametrize("loss_func", ["neg_snr", "neg_sa_sdr"])
def test_fit_two_epochs_with_the_family_on_gpu(loss_func):
    """8. a two-epoch fit of a 1-layer SpatialNet-small through the fused step: the logged train/<name> is finite and falls.  The training split has the
    synthetic data module's own default size (64 items = 32 steps an epoch): these losses are not scale-invariant, single mixtures score many dB
    off the rest, and an epoch mean over a handful of steps is decided by which mixtures it drew rather than by the weights."""
    argv = ["fit", "--config", str(ROOT / "configs" / "SpatialNet.yaml"), "--config", SYN, "--model.arch.dim_input=12", "--model.arch.dim_output=4",
            "--trainer.precision=bf16-mixed", "--trainer.max_epochs=2", "--data.num_samples=[64,4,4]", "--data.audio_time_len=[1.0,1.0,1.0]",
            "--model.arch.num_layers=1", f"--model.loss.init_args.loss_func=models.io.loss.{loss_func}"]
    log = TrainCLI(argv=argv).result["log"]
    tk, vk = f"train/{loss_func}", f"val/{loss_func}"
    print(log)
    assert len(log) == 2 and all(torch.isfinite(torch.tensor(r[tk])) and torch.isfinite(torch.tensor(r[vk])) for r in log)
    assert "train/neg_si_sdr" not in log[0]
    assert log[1][tk] < log[0][tk]


@pytest.mark.gpu
def test_fused_step_matches_module_path_with_neg_snr(hip_lib):
    """8. TrainStep(loss="neg_snr").forward_loss + engine.backward against TrainModule.training_step with Loss(neg_snr, pit=True) + autograd on the
    same weights (the bars of tests/test_train_module.py: loss 1e-5 relative, gradients 1e-4 relative L2)"""
    from models.arch.SpatialNet import SpatialNet
    from models.io.loss import Loss, neg_snr
    from models.io.norm import Norm
    from models.io.stft import STFT
    from nbss_amd._lib import NBSS_F32
    from nbss_amd.engine import TrainStep
    dev = torch.device("cuda:0")
    torch.manual_seed(2)
    arch = SpatialNet(dim_input=12, dim_output=4, num_layers=1, encoder_kernel_size=5, dim_hidden=96, dim_ffn=192, num_heads=4, dropout=(0, 0, 0),
                      kernel_size=(5, 3), conv_groups=(8, 8), norms=("LN", "LN", "GN", "LN", "LN", "LN"), dim_squeeze=8, num_freqs=129, full_share=0)
    m = TrainModule(arch, channels=[0, 1, 2, 3, 4, 5], ref_channel=0, stft=STFT(256, 128, 256), norm=Norm("frequency", online=True),
                    loss=Loss(neg_snr, pit=True)).to(dev)
    m.precision = "32"
    x, ys = _tiny_batch(B=2, C=6, S=2, N=8000, seed=5)
    loss = m.training_step((x.to(dev), ys.to(dev), None))
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.arch.named_parameters()}
    assert all(torch.isfinite(gv).all() for gv in grads.values())
    eng = m.arch._engine_for(dev)
    eng.dtype = NBSS_F32
    ts = TrainStep(eng, loss="neg_snr")
    l2, _, dout, xin, _ = ts.forward_loss(x.to(dev), ys[:, :, 0].contiguous().to(dev))
    eng.grads.zero_()
    eng.backward(xin, dout)
    views = eng.param_views(eng.grads)
    print("module path", float(loss), "fused step", float(l2))
    assert abs(float(loss) - float(l2)) <= 1e-5 * max(1.0, abs(float(l2)))
    for k, gv in grads.items():
        ref = views[k]
        assert float((gv - ref).norm()) / (float(ref.norm()) + 1e-30) <= 1e-4, k


@pytest.mark.gpu
def test_online_spatialnet_training_step_with_neg_snr_on_gpu(hip_lib):
    """9. the configuration the reference ships: OnlineSpatialNet (ret(2), 1 layer) with Loss(neg_snr, pit=True) on the device kernel"""
    from models.io.loss import Loss, neg_snr
    dev = torch.device("cuda:0")
    m = _tiny_online(Loss(neg_snr, pit=True)).to(dev)
    x, ys = _tiny_batch()
    loss = m.training_step((x.to(dev), ys.to(dev), None))
    loss.backward()
    gn = [p.grad.norm() for p in m.arch.parameters() if p.grad is not None]
    assert torch.isfinite(loss) and gn and all(torch.isfinite(v) for v in gn) and sum(float(v) for v in gn) > 0
    # the same step on the host: the kernel and the closed forms agree
    mh = _tiny_online(Loss(neg_snr, pit=True))
    lh = mh.training_step((x, ys, None))
    print("device", float(loss), "host", float(lh))
    assert abs(float(loss) - float(lh)) < 1e-3 * max(1.0, abs(float(lh)))
