"""The native T-ConvFFN inside models.arch.OnlineSpatialNet (nbss_amd/online_train.py): the switch NBSS_ONLINE_NATIVE_TRAIN, the autograd Function in the
graph, every p.grad of a model against the switch-off run in fp64 on the CPU (the project's fp32 bars: forward <= 2e-5, gradients <= 1e-4 rel-L2), the
refusals, and one `TrainCLI fit` on the device."""
import copy
import types
import warnings
from pathlib import Path

import pytest
import torch

from nbss_amd import online_train, ops
from util import ONLINE_SWITCHES, check_against_fp64, fit_with_switch, fp64_reference, grad_fns, online_net, rel_l2

ROOT = Path(__file__).resolve().parent.parent
FWD_TOL, GRAD_TOL = 2e-5, 1e-4
F, T = 5, 20


def _net(**kw):
    return online_net(11, F, **kw)


@pytest.fixture(scope="module")
def reference():
    """the switch-off run in fp64 on the CPU: computed once"""
    return fp64_reference(_net(), 2, F, T)


def test_switch_on_matches_switch_off_fp64(backend, reference, monkeypatch):
    net, x, r, wy, wg = reference
    net = copy.deepcopy(net).to(backend.device)
    xd, rd = x.to(backend.device), r.to(backend.device)
    monkeypatch.delenv("NBSS_ONLINE_NATIVE_TRAIN", raising=False)
    with online_train.use_lib(backend.lib):
        y_off = net(xd)
        assert "OnlineTConvFFNFnBackward" not in grad_fns(y_off)  # off by default
        monkeypatch.setenv("NBSS_ONLINE_NATIVE_TRAIN", "1")
        y = net(xd)
        assert "OnlineTConvFFNFnBackward" in grad_fns(y)
        (y * rd).sum().backward()
        with pytest.raises(RuntimeError, match="second time|retain_graph"):
            (y * rd).sum().backward()
        with torch.no_grad():  # inference obeys the same switch: the forward entry alone, nothing kept
            y_inf = net(xd)
    assert torch.equal(y_inf, y.detach())
    check_against_fp64(y, {k: p.grad for k, p in net.named_parameters()}, wy, wg, FWD_TOL, GRAD_TOL)


def test_unsupported_geometry_warns_once_and_runs_torch(backend, monkeypatch):
    net = _net(dim_ffn=256).to(backend.device)
    x = torch.randn(1, F, 6, 4, device=backend.device)
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_TRAIN", "1")
    with online_train.use_lib(backend.lib):
        with pytest.warns(RuntimeWarning, match="dim_ffn must be 192"):
            y = net(x)
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # once per module and reason
            y2 = net(x)
    assert "OnlineTConvFFNFnBackward" not in grad_fns(y) and torch.equal(y, y2)


def test_streaming_call_never_takes_the_native_block(backend, monkeypatch):
    net = _net().to(backend.device)
    x = torch.randn(1, F, 8, 4, device=backend.device)
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_TRAIN", "1")
    with online_train.use_lib(backend.lib):
        assert online_train.eligible(net.layers[0], torch.zeros(1, F, 8, 96, device=backend.device), {}) == "streaming call"
        st = net.init_stream(1, device=backend.device)
        y = torch.cat([net.forward_stream(x[:, :, :4], st), net.forward_stream(x[:, :, 4:], st)], 2)
        assert "OnlineTConvFFNFnBackward" not in grad_fns(y)
        whole = net(x)
    assert "OnlineTConvFFNFnBackward" in grad_fns(whole)
    assert rel_l2(y.detach(), whole.detach()) < 1e-4  # (the streamed frames are the whole-utterance ones)


def test_library_for_another_device_goes_to_torch_silently(backend, monkeypatch):
    """all three blocks: under a `use_lib` override whose backend does not match the tensor's device the gate says so, the layer runs torch.nn — the bits
    of the switch-off run — and nothing warns.  The override is the backend's library and the tensors are on the other kind of device; where no HIP device
    exists the emulator backend takes the other direction instead: CPU tensors under a stand-in for a library that is not the emulator (the gate asks the
    library nothing else)."""
    if backend.device.type == "cpu" and not torch.cuda.is_available():
        lib, dev = types.SimpleNamespace(_is_emu=False), torch.device("cpu")
    else:
        lib, dev = backend.lib, torch.device("cuda" if backend.device.type == "cpu" else "cpu")
    net = _net().to(dev)
    layer, x = net.layers[0], torch.randn(1, F, 6, 4, device=dev)
    h, pos = torch.zeros(1, F, 6, 96, device=dev), net.get_causal_mask(slen=6, device=dev)
    why = "no library for the tensor's device"
    for s in ONLINE_SWITCHES:
        monkeypatch.delenv(s, raising=False)
    with online_train.use_lib(lib), warnings.catch_warnings():
        warnings.simplefilter("error")
        y_off = net(x)
        for s in ONLINE_SWITCHES:
            monkeypatch.setenv(s, "1")
        assert online_train.eligible(layer, h, None) == why and online_train.xband_eligible(layer, h, None) == why
        assert online_train.ret_eligible(layer, h[0], pos, True, False, None, False) == why
        y = net(x)
    assert not {n for n in grad_fns(y) if n.startswith("Online")} and torch.equal(y, y_off)


@pytest.mark.parametrize("block", ["tconvffn", "retention"])
def test_no_grad_forward_keeps_nothing(backend, monkeypatch, block):
    """under no_grad, with parameters that require gradients, the block's forward entry runs alone (keep=False), its output has no grad_fn and the bits of
    the training output; T 70 spans two 64-frame chunks of the retention kernels"""
    entry, switch, frames = {"tconvffn": ("online_tconvffn_train_fwd", "NBSS_ONLINE_NATIVE_TRAIN", T),
                             "retention": ("online_ret_train_fwd", "NBSS_ONLINE_NATIVE_RET", 70)}[block]
    net = _net().to(backend.device)
    layer, h = net.layers[0], torch.randn(2, F, frames, 96, device=backend.device)
    pos = net.get_causal_mask(slen=frames, device=backend.device)
    run = (lambda: layer._tconvffn(h, residual=True)) if block == "tconvffn" else (lambda: layer._tsa(h, pos, True, net.rope)[0])
    keeps, orig = [], getattr(ops, entry)
    monkeypatch.setattr(ops, entry, lambda *a, **k: (keeps.append(k.get("keep")), orig(*a, **k))[1])
    monkeypatch.setenv(switch, "1")
    with online_train.use_lib(backend.lib):
        y_train = run()
        with torch.no_grad():
            y_inf = run()
    assert all(p.requires_grad for p in layer.parameters()) and keeps == [True, False]
    assert y_train.grad_fn is not None and y_inf.grad_fn is None and torch.equal(y_inf, y_train.detach())


@pytest.mark.gpu
def test_fit_on_the_device_with_the_switch(monkeypatch):
    """TrainCLI fit, configs/onlineSpatialNet.yaml, synthetic data, 2 layers, 1-s segments, two epochs of two steps: the first step's loss is the switch-off
    run's to 1e-4 relative, and the loss decreases"""
    argv = ["fit", "--config", str(ROOT / "configs" / "onlineSpatialNet.yaml"), "--config", str(ROOT / "configs" / "datasets" / "synthetic.yaml"),
            "--model.arch.dim_input=12", "--model.arch.dim_output=4", "--model.arch.num_freqs=129", "--model.arch.num_layers=2", "--data.num_samples=[4,2,2]",
            "--data.audio_time_len=[1.0,1.0,1.0]", "--data.batch_size=[2,1]", "--trainer.max_epochs=2"]
    fit_with_switch(monkeypatch, argv, ["NBSS_ONLINE_NATIVE_TRAIN"], "OnlineTConvFFNFnBackward")
