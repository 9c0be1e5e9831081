"""The native Mamba core inside models.arch.OnlineSpatialNet (nbss_amd/online_train.py: MAMBA, NBSS_ONLINE_NATIVE_MAMBA; the variant itself behind
NBSS_ONLINE_MAMBA): a 2-layer width-96 'mamba(16,4)' net with the switch on — the output and every p.grad against the same module's torch path in fp64 on
the CPU (the project's fp32 bars: forward <= 2e-5, gradients <= 1e-4 rel-L2) at T = 21 and T = MAMBA_CKPT + 5, alone and together with the native cross-band
trio — and the switch's behaviour: off by default, one warning for a module that does not fit, streaming and inference calls never taken, nothing kept
under no_grad."""
import copy
import warnings

import pytest
import torch

from nbss_amd import online_train, ops
from nbss_amd.online_train import MAMBA_CKPT
from util import check_against_fp64, fp64_reference, grad_fns, rel_l2

FWD_TOL, GRAD_TOL = 2e-5, 1e-4
F = 9
NODE = "OnlineMambaFnBackward"


def _net(monkeypatch, attention="mamba(16,4)", seed=13):
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    monkeypatch.setenv("NBSS_ONLINE_MAMBA", "1")
    torch.manual_seed(seed)
    net = OnlineSpatialNet(dim_input=4, dim_output=4, num_layers=2, dim_squeeze=8, num_freqs=F, dim_hidden=96, dim_ffn=192, num_heads=4,
                           attention=attention).train()
    with torch.no_grad():
        for n, p in net.named_parameters():
            if p.dim() == 1 and not n.endswith("dt_proj.bias"):
                p.add_(0.2 * torch.randn_like(p))
            if n.endswith("A_log"):
                p.add_(0.3 * torch.randn_like(p))
    return net


@pytest.fixture(scope="module")
def references():
    """the torch path in fp64 on the CPU at the two lengths: computed once"""
    mp = pytest.MonkeyPatch()
    try:
        return {T: fp64_reference(_net(mp), 2, F, T) for T in (21, MAMBA_CKPT + 5)}
    finally:
        mp.undo()


@pytest.mark.parametrize("T,xband", [(21, False), (MAMBA_CKPT + 5, False), (21, True)])
def test_switch_on_matches_torch_path_fp64(backend, references, monkeypatch, T, xband):
    net, x, r, wy, wg = references[T]
    net = copy.deepcopy(net).to(backend.device)
    xd, rd = x.to(backend.device), r.to(backend.device)
    monkeypatch.delenv("NBSS_ONLINE_NATIVE_MAMBA", raising=False)
    with online_train.use_lib(backend.lib):
        assert NODE not in grad_fns(net(xd))  # off by default: the torch module
        monkeypatch.setenv("NBSS_ONLINE_NATIVE_MAMBA", "1")
        if xband:
            monkeypatch.setenv("NBSS_ONLINE_NATIVE_XBAND", "1")
        y = net(xd)
        names = grad_fns(y)
        assert NODE in names and ("OnlineXBandFnBackward" in names) == xband
        (y * rd).sum().backward()
    check_against_fp64(y, {k: p.grad for k, p in net.named_parameters()}, wy, wg, FWD_TOL, GRAD_TOL)


def test_bf16_autocast_takes_the_node(backend, monkeypatch):
    net = _net(monkeypatch).to(backend.device)
    x = torch.randn(1, F, 12, 4, device=backend.device)
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_MAMBA", "1")
    with online_train.use_lib(backend.lib):
        y32 = net(x)
        with torch.autocast(backend.device.type, dtype=torch.bfloat16):
            y = net(x)
        assert NODE in grad_fns(y)
        y.float().sum().backward()
    assert rel_l2(y.float().detach(), y32.detach()) < 3e-2 and all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


def test_unsupported_module_warns_once_and_runs_torch(backend, monkeypatch):
    net = _net(monkeypatch, "mamba(8,4)").to(backend.device)
    x = torch.randn(1, F, 6, 4, device=backend.device)
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_MAMBA", "1")
    with online_train.use_lib(backend.lib):
        with pytest.warns(RuntimeWarning, match="d_state must be 16") as rec:
            y = net(x)
        assert len([w for w in rec if "d_state" in str(w.message)]) == 4  # one per Mamba module: two layers of two
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # once per module and reason
            y2 = net(x)
    assert NODE not in grad_fns(y) and torch.equal(y, y2)


def test_streaming_and_inference_calls_never_take_the_native_core(backend, monkeypatch):
    net = _net(monkeypatch).to(backend.device)
    x = torch.randn(1, F, 8, 4, device=backend.device)
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_MAMBA", "1")
    with online_train.use_lib(backend.lib):
        st = net.init_stream(1, device=backend.device)
        ys = torch.cat([net.forward_stream(x[:, :, :4], st), net.forward_stream(x[:, :, 4:], st)], 2)
        yi = net(x, inference=True)
        whole = net(x)
    assert NODE not in grad_fns(ys) and NODE not in grad_fns(yi) and NODE in grad_fns(whole)
    assert rel_l2(ys.detach(), whole.detach()) < 1e-4 and rel_l2(yi.detach(), whole.detach()) < 1e-4


def test_no_grad_forward_keeps_nothing(backend, monkeypatch):
    net = _net(monkeypatch).to(backend.device)
    layer, h = net.layers[0], torch.randn(2, F, MAMBA_CKPT + 5, 96, device=backend.device)
    run = lambda: layer._mamba(h, layer.tconvffn, layer.norm_tconvffn, layer.dropout_tconvffn)  # noqa: E731
    keeps, orig = [], ops.online_mamba_train_fwd
    monkeypatch.setattr(ops, "online_mamba_train_fwd", lambda *a, **k: (keeps.append(k.get("keep")), orig(*a, **k))[1])
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_MAMBA", "1")
    with online_train.use_lib(backend.lib):
        y_train = run()
        with torch.no_grad():
            y_inf = run()
    assert all(p.requires_grad for p in layer.parameters()) and keeps == [True, False]
    assert y_train.grad_fn is not None and y_inf.grad_fn is None and torch.equal(y_inf, y_train.detach())
