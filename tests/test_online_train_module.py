"""The native T-ConvFFN inside models.arch.OnlineSpatialNet (nbss_amd/online_train.py): the switch NBSS_ONLINE_NATIVE_TRAIN, the autograd Function in the
graph, every p.grad of a model against the switch-off run in fp64 on the CPU (the project's fp32 bars: forward <= 2e-5, gradients <= 1e-4 rel-L2), the
refusals, and one `TrainCLI fit` on the device."""
import copy
from pathlib import Path

import pytest
import torch

from nbss_amd import online_train
from util import rel_l2

ROOT = Path(__file__).resolve().parent.parent
FWD_TOL, GRAD_TOL = 2e-5, 1e-4
F, T = 5, 20


def _net(**kw):
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    torch.manual_seed(11)
    args = dict(dim_input=4, dim_output=4, num_layers=1, dim_squeeze=8, num_freqs=F, dim_hidden=96, dim_ffn=192, num_heads=4, attention="ret(2)")
    args.update(kw)
    net = OnlineSpatialNet(**args).train()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.2 * torch.randn_like(p))
    return net


def _grad_fns(t):
    """names of every node of the autograd graph behind t"""
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo += [g for g, _ in f.next_functions]
    return names


@pytest.fixture(scope="module")
def reference():
    """the switch-off run in fp64 on the CPU: computed once"""
    net = _net()
    x, r = torch.randn(2, F, T, 4), torch.randn(2, F, T, 4)
    n64 = copy.deepcopy(net).double()
    y = n64(x.double())
    (y * r.double()).sum().backward()
    return net, x, r, y.detach(), {k: p.grad for k, p in n64.named_parameters()}


def test_switch_on_matches_switch_off_fp64(backend, reference, monkeypatch):
    net, x, r, wy, wg = reference
    net = copy.deepcopy(net).to(backend.device)
    xd, rd = x.to(backend.device), r.to(backend.device)
    monkeypatch.delenv("NBSS_ONLINE_NATIVE_TRAIN", raising=False)
    with online_train.use_lib(backend.lib):
        y_off = net(xd)
        assert "OnlineTConvFFNFnBackward" not in _grad_fns(y_off)  # off by default
        monkeypatch.setenv("NBSS_ONLINE_NATIVE_TRAIN", "1")
        y = net(xd)
        assert "OnlineTConvFFNFnBackward" in _grad_fns(y)
        (y * rd).sum().backward()
        with pytest.raises(RuntimeError, match="second time|retain_graph"):
            (y * rd).sum().backward()
        with torch.no_grad():  # inference obeys the same switch: the forward entry alone, nothing kept
            y_inf = net(xd)
    assert torch.equal(y_inf, y.detach())
    ey = rel_l2(y.detach().cpu(), wy)
    errs = {k: rel_l2(p.grad.cpu(), wg[k]) for k, p in net.named_parameters()}
    print(f"y {ey:.1e}; worst grad {max(errs, key=errs.get)} {max(errs.values()):.1e}")
    assert set(errs) == set(wg) and ey <= FWD_TOL, ey
    assert max(errs.values()) <= GRAD_TOL, {k: v for k, v in errs.items() if v > GRAD_TOL}


def test_unsupported_geometry_warns_once_and_runs_torch(backend, monkeypatch):
    net = _net(dim_ffn=256).to(backend.device)
    x = torch.randn(1, F, 6, 4, device=backend.device)
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_TRAIN", "1")
    with online_train.use_lib(backend.lib):
        with pytest.warns(RuntimeWarning, match="dim_ffn must be 192"):
            y = net(x)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # once per module and reason
            y2 = net(x)
    assert "OnlineTConvFFNFnBackward" not in _grad_fns(y) and torch.equal(y, y2)


def test_streaming_call_never_takes_the_native_block(backend, monkeypatch):
    net = _net().to(backend.device)
    x = torch.randn(1, F, 8, 4, device=backend.device)
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_TRAIN", "1")
    with online_train.use_lib(backend.lib):
        assert online_train.eligible(net.layers[0], torch.zeros(1, F, 8, 96, device=backend.device), {}) == "streaming call"
        st = net.init_stream(1, device=backend.device)
        y = torch.cat([net.forward_stream(x[:, :, :4], st), net.forward_stream(x[:, :, 4:], st)], 2)
        assert "OnlineTConvFFNFnBackward" not in _grad_fns(y)
        whole = net(x)
    assert "OnlineTConvFFNFnBackward" in _grad_fns(whole)
    assert rel_l2(y.detach(), whole.detach()) < 1e-4  # (the streamed frames are the whole-utterance ones)


@pytest.mark.gpu
def test_fit_on_the_device_with_the_switch(monkeypatch):
    """TrainCLI fit, configs/onlineSpatialNet.yaml, synthetic data, 2 layers, 1-s segments, two epochs of two steps: the first step's loss is the switch-off
    run's to 1e-4 relative, and the loss decreases"""
    import SharedTrainer
    from SharedTrainer import TrainCLI
    argv = ["fit", "--config", str(ROOT / "configs" / "onlineSpatialNet.yaml"), "--config", str(ROOT / "configs" / "datasets" / "synthetic.yaml"),
            "--model.arch.dim_input=12", "--model.arch.dim_output=4", "--model.arch.num_freqs=129", "--model.arch.num_layers=2", "--data.num_samples=[4,2,2]",
            "--data.audio_time_len=[1.0,1.0,1.0]", "--data.batch_size=[2,1]", "--trainer.max_epochs=2"]
    steps = []
    orig = SharedTrainer.TrainModule.training_step

    def recording(self, *a, **k):
        loss = orig(self, *a, **k)
        steps.append((float(loss.detach()), "OnlineTConvFFNFnBackward" in _grad_fns(loss)))
        return loss

    monkeypatch.setattr(SharedTrainer.TrainModule, "training_step", recording)
    monkeypatch.delenv("NBSS_ONLINE_NATIVE_TRAIN", raising=False)
    TrainCLI(argv=argv)
    off, steps[:] = list(steps), []
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_TRAIN", "1")
    log = TrainCLI(argv=argv).result["log"]
    on = list(steps)
    print("switch off:", off, "\nswitch on: ", on)
    assert len(log) == 2 and len(on) == len(off) == 4 and log[0]["device"].startswith("cuda")
    assert not any(n for _, n in off) and all(n for _, n in on)
    assert abs(on[0][0] - off[0][0]) <= 1e-4 * abs(off[0][0]), (on[0], off[0])
    key = next(k for k in log[0] if k.startswith("train/"))
    assert log[1][key] < log[0][key], log
