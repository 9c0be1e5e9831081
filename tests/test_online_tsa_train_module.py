"""The whole retention block as one native node inside models.arch.OnlineSpatialNet (nbss_amd/online_train.py): the switch NBSS_ONLINE_NATIVE_TSA, the
autograd Function in the graph, every p.grad of a model against the switch-off run in fp64 on the CPU (the project's fp32 bars: forward <= 2e-5, gradients
<= 1e-4 rel-L2), alone and with NBSS_ONLINE_NATIVE_RET (TSA wins), both key forms, the layers and calls that never take it, all four switches on a
two-layer net, and one `TrainCLI fit` on the device.  T = 70 crosses a chunk boundary of the core (64 frames); 2 x 5 x 70 = 700 rows are no whole 128-row
tile of the projection kernels."""
import copy
import warnings
from pathlib import Path

import pytest
import torch

from nbss_amd import online_train
from util import check_against_fp64, fit_with_switch, fp64_reference, grad_fns, online_net, rel_l2

ROOT = Path(__file__).resolve().parent.parent
FWD_TOL, GRAD_TOL = 2e-5, 1e-4
F, T, B = 5, 70, 2
SWITCH = "NBSS_ONLINE_NATIVE_TSA"
ALL = ("NBSS_ONLINE_NATIVE_XBAND", "NBSS_ONLINE_NATIVE_TRAIN", "NBSS_ONLINE_NATIVE_RET", SWITCH)
TSA, RET, TCF, XB = "OnlineTSAFnBackward", "OnlineRetentionFnBackward", "OnlineTConvFFNFnBackward", "OnlineXBandFnBackward"


def _net(**kw):
    return online_net(17, F, **{"decay": [4, 5, 9, 10], **kw})


def _all_off(monkeypatch):
    for s in ALL:
        monkeypatch.delenv(s, raising=False)


@pytest.fixture(scope="module", params=["ret(2)", "ret(2,not_share_qk)"])
def reference(request):
    """a 1-layer model ('ret(2)' with rope=False shares q and k; the other form has a k_proj) and its switch-off run in fp64 on the CPU: computed once"""
    net = _net(attention=request.param)
    assert net.layers[0].mhsa.share_qk == (request.param == "ret(2)") and net.rope is False
    return fp64_reference(net, B, F, T)


@pytest.mark.parametrize("both", [False, True], ids=["tsa", "tsa+ret"])
def test_switch_on_matches_switch_off_fp64(backend, reference, monkeypatch, both):
    net, x, r, wy, wg = reference
    net = copy.deepcopy(net).to(backend.device)
    xd, rd = x.to(backend.device), r.to(backend.device)
    _all_off(monkeypatch)
    with online_train.use_lib(backend.lib):
        assert TSA not in grad_fns(net(xd))  # off by default
        monkeypatch.setenv(SWITCH, "0")
        assert TSA not in grad_fns(net(xd))
        monkeypatch.setenv(SWITCH, "true")  # off unless exactly '1'
        assert TSA not in grad_fns(net(xd))
        monkeypatch.setenv(SWITCH, "1")
        if both:
            monkeypatch.setenv("NBSS_ONLINE_NATIVE_RET", "1")
        y = net(xd)
        fns = grad_fns(y)
        assert TSA in fns and RET not in fns  # with both on, TSA takes the call
        (y * rd).sum().backward()
        grads = {k: p.grad.clone() for k, p in net.named_parameters()}  # (the refused second backward below may reach some leaves before it is refused)
        with pytest.raises(RuntimeError, match="second time|retain_graph"):
            (y * rd).sum().backward()
        # inference obeys the same switch: the forward entry alone, nothing kept (compared on the block this switch governs)
        layer, h = net.layers[0], torch.randn(B, F, T, 96, device=backend.device)
        pos = net.get_causal_mask(slen=T, device=backend.device)
        y_train = online_train.tsa_residual(layer, h.requires_grad_(True), pos, True, net.rope)
        with torch.no_grad():
            y_inf = online_train.tsa_residual(layer, h, pos, True, net.rope)
            assert TSA not in grad_fns(net(xd))
    assert TSA in grad_fns(y_train) and y_inf.grad_fn is None and torch.equal(y_inf, y_train.detach())
    check_against_fp64(y, grads, wy, wg, FWD_TOL, GRAD_TOL)


def test_a_training_layer_is_three_native_nodes_and_all_four_switches_match_fp64(backend, monkeypatch):
    """two layers, every switch on: loss and every parameter gradient against fp64; nothing of torch.nn is left between the encoder and the decoder"""
    net, x, r, wy, wg = fp64_reference(_net(num_layers=2), B, F, T)
    net = copy.deepcopy(net).to(backend.device)
    for s in ALL:
        monkeypatch.setenv(s, "1")
    with online_train.use_lib(backend.lib):
        y = net(x.to(backend.device))
        loss = (y * r.to(backend.device)).sum()
        fns = grad_fns(loss)
        loss.backward()
    assert {TSA, TCF, XB} <= fns and RET not in fns
    assert not {n for n in fns if "LayerNorm" in n or "GroupNorm" in n or "Silu" in n or "Prelu" in n}, fns
    want = float((wy * r.double()).sum())
    got = float(loss.detach())
    assert abs(got - want) <= FWD_TOL * float((wy.abs() * r.double().abs()).sum()), (got, want)
    check_against_fp64(y, {k: p.grad for k, p in net.named_parameters()}, wy, wg, FWD_TOL, GRAD_TOL)


def _with_bias(net):
    net.layers[0].mhsa.q_proj = torch.nn.Linear(96, 96, bias=True)
    return net


@pytest.mark.parametrize("make,reason", [(lambda: _with_bias(_net()), "projections must have no bias"), (lambda: _net(dropout=(0.1, 0, 0)).eval(), "dropout"),
                                         (lambda: _net(rope=True), "rope must be False")], ids=["bias", "dropout", "rope"])
def test_unsupported_layer_or_call_warns_once_and_runs_torch(backend, monkeypatch, make, reason):
    """the switch is on and the layer (bias, dropout) or — the layer fits — the call (rope) does not fit: the torch path, and one warning that names the reason"""
    net = make().to(backend.device)
    x = torch.randn(1, F, 6, 4, device=backend.device)
    _all_off(monkeypatch)
    y_off = net(x)
    monkeypatch.setenv(SWITCH, "1")
    with online_train.use_lib(backend.lib):
        with pytest.warns(RuntimeWarning, match=reason):
            y = net(x)
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # once per module and reason
            y2 = net(x)
    assert TSA not in grad_fns(y) and torch.equal(y, y2) and torch.equal(y, y_off)


def test_mhsa_recurrent_and_streaming_calls_never_take_the_node(backend, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    with online_train.use_lib(backend.lib), warnings.catch_warnings():
        warnings.simplefilter("error")  # ordinary torch.nn cases: no warning
        mh = _net(attention="mhsa(7)").to(backend.device)
        x = torch.randn(1, F, 8, 4, device=backend.device)
        assert TSA not in grad_fns(mh(x))
        net = _net().to(backend.device)
        layer, h = net.layers[0], torch.zeros(1, F, 8, 96, device=backend.device)
        pos = net.get_causal_mask(slen=8, device=backend.device)
        assert online_train.tsa_eligible(layer, h, pos, True, False, None, False) is None
        assert online_train.tsa_eligible(layer, h, pos, True, False, {}, False) == "streaming or recurrent call"
        assert online_train.tsa_eligible(layer, h, pos, True, False, None, True) == "streaming or recurrent call"
        assert TSA not in grad_fns(net(x, inference=True))
        st = net.init_stream(1, device=backend.device)
        y = torch.cat([net.forward_stream(x[:, :, :4], st), net.forward_stream(x[:, :, 4:], st)], 2)
        assert TSA not in grad_fns(y)
        whole = net(x)
    assert TSA in grad_fns(whole)
    assert rel_l2(y.detach(), whole.detach()) < 1e-4  # (the streamed frames are the whole-utterance ones)


def test_supported_names_the_layer():
    assert online_train.tsa_supported(_net().layers[0]) is None
    assert online_train.tsa_supported(_net(attention="ret(2,not_share_qk)").layers[0]) is None
    assert "no bias" in online_train.tsa_supported(_with_bias(_net()).layers[0])
    assert "dropout" in online_train.tsa_supported(_net(dropout=(0.1, 0, 0)).layers[0])
    assert "retention" in online_train.tsa_supported(_net(attention="mhsa(7)").layers[0])
    net = _net()
    net.layers[0].norm_mhsa = torch.nn.LayerNorm(96, eps=1e-6)
    assert "norm_mhsa" in online_train.tsa_supported(net.layers[0])
    assert online_train.tsa_enabled() in (False, True)


@pytest.mark.gpu
def test_fit_on_the_device_with_the_switch(monkeypatch):
    """TrainCLI fit, configs/onlineSpatialNet.yaml, synthetic data, 2 layers, 1.1-s segments (69 frames: two chunks), two epochs of two steps: the first
    step's loss is the switch-off run's to 1e-4 relative, and the loss decreases"""
    argv = ["fit", "--config", str(ROOT / "configs" / "onlineSpatialNet.yaml"), "--config", str(ROOT / "configs" / "datasets" / "synthetic.yaml"),
            "--model.arch.dim_input=12", "--model.arch.dim_output=4", "--model.arch.num_freqs=129", "--model.arch.num_layers=2", "--data.num_samples=[4,2,2]",
            "--data.audio_time_len=[1.1,1.1,1.1]", "--data.batch_size=[2,1]", "--trainer.max_epochs=2"]
    monkeypatch.delenv(SWITCH, raising=False)
    fit_with_switch(monkeypatch, argv, [SWITCH], TSA)
