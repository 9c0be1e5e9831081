"""The native retention core inside models.arch.OnlineSpatialNet (nbss_amd/online_train.py): the switch NBSS_ONLINE_NATIVE_RET, the autograd Function in the
graph, every p.grad of a model against the switch-off run in fp64 on the CPU (the project's fp32 bars: forward <= 2e-5, gradients <= 1e-4 rel-L2), alone
and together with NBSS_ONLINE_NATIVE_TRAIN, both key forms, the calls that never take it, and one `TrainCLI fit` on the device.  T = 70 crosses a chunk
boundary of the kernels (64 frames)."""
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
RET, TCF = "OnlineRetentionFnBackward", "OnlineTConvFFNFnBackward"


def _net(**kw):
    return online_net(13, F, **{"decay": [4, 5, 9, 10], **kw})


@pytest.fixture(scope="module", params=["ret(2)", "ret(2,not_share_qk)"])
def reference(request):
    """a 1-layer model ('ret(2)' with rope=False shares q and k; the other form has a k_proj) and its switch-off run in fp64 on the CPU: computed once"""
    net = _net(attention=request.param)
    assert net.layers[0].mhsa.share_qk == (request.param == "ret(2)") and net.rope is False
    return fp64_reference(net, B, F, T)


@pytest.mark.parametrize("both", [False, True], ids=["ret", "ret+tconvffn"])
def test_switch_on_matches_switch_off_fp64(backend, reference, monkeypatch, both):
    net, x, r, wy, wg = reference
    net = copy.deepcopy(net).to(backend.device)
    xd, rd = x.to(backend.device), r.to(backend.device)
    monkeypatch.delenv("NBSS_ONLINE_NATIVE_RET", raising=False)
    monkeypatch.delenv("NBSS_ONLINE_NATIVE_TRAIN", raising=False)
    with online_train.use_lib(backend.lib):
        assert RET not in grad_fns(net(xd))  # off by default
        monkeypatch.setenv("NBSS_ONLINE_NATIVE_RET", "0")
        assert RET not in grad_fns(net(xd))
        monkeypatch.setenv("NBSS_ONLINE_NATIVE_RET", "1")
        if both:
            monkeypatch.setenv("NBSS_ONLINE_NATIVE_TRAIN", "1")
        y = net(xd)
        fns = grad_fns(y)
        assert RET in fns and (TCF in fns) == both
        (y * rd).sum().backward()
        grads = {k: p.grad.clone() for k, p in net.named_parameters()}  # (the refused second backward below may reach some leaves before it is refused)
        with pytest.raises(RuntimeError, match="second time|retain_graph"):
            (y * rd).sum().backward()
        # inference obeys the same switch: the forward entry alone, nothing kept.  Compared on the block this switch governs (LayerNorm, projections, the native
        # core, out_proj): around it torch picks its own convolution kernels, and not the same ones with and without autograd on every device
        layer, h = net.layers[0], torch.randn(B, F, T, 96, device=backend.device)
        pos = net.get_causal_mask(slen=T, device=backend.device)
        a_train = layer._tsa(h, pos, True, net.rope)[0]
        with torch.no_grad():
            a_inf = layer._tsa(h, pos, True, net.rope)[0]
            assert RET not in grad_fns(net(xd))
    assert RET in grad_fns(a_train) and a_inf.grad_fn is None and torch.equal(a_inf, a_train.detach())
    check_against_fp64(y, grads, wy, wg, FWD_TOL, GRAD_TOL)


@pytest.mark.parametrize("kw,reason", [(dict(rope=True), "rope must be False"), (dict(num_heads=2, decay=[4, 5]), "num_heads must be 4")], ids=["rope", "heads"])
def test_unsupported_call_warns_once_and_runs_torch(backend, monkeypatch, kw, reason):
    net = _net(**kw).to(backend.device)
    x = torch.randn(1, F, 6, 4, device=backend.device)
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_RET", "1")
    with online_train.use_lib(backend.lib):
        with pytest.warns(RuntimeWarning, match=reason):
            y = net(x)
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # once per module and reason
            y2 = net(x)
    assert RET not in grad_fns(y) and torch.equal(y, y2)


def test_recurrent_and_streaming_calls_never_take_the_native_core(backend, monkeypatch):
    net = _net().to(backend.device)
    x = torch.randn(1, F, 8, 4, device=backend.device)
    monkeypatch.setenv("NBSS_ONLINE_NATIVE_RET", "1")
    with online_train.use_lib(backend.lib), warnings.catch_warnings():
        warnings.simplefilter("error")  # ordinary torch.nn cases: no warning
        layer, u = net.layers[0], torch.zeros(F, 8, 96, device=backend.device)
        pos = net.get_causal_mask(slen=8, device=backend.device)
        assert online_train.ret_eligible(layer, u, pos, True, False, None, False) is None
        assert online_train.ret_eligible(layer, u, pos, True, False, {}, False) == "streaming or recurrent call"
        assert online_train.ret_eligible(layer, u, pos, True, False, None, True) == "streaming or recurrent call"
        assert RET not in grad_fns(net(x, inference=True))
        st = net.init_stream(1, device=backend.device)
        y = torch.cat([net.forward_stream(x[:, :, :4], st), net.forward_stream(x[:, :, 4:], st)], 2)
        assert RET not in grad_fns(y)
        whole = net(x)
    assert RET in grad_fns(whole)
    assert rel_l2(y.detach(), whole.detach()) < 1e-4  # (the streamed frames are the whole-utterance ones)


def test_supported_names_the_geometry():
    from models.arch.base.retention import MultiScaleRetention
    assert online_train.ret_supported(MultiScaleRetention(96, 4, share_qk=True)) is None
    assert online_train.ret_supported(MultiScaleRetention(96, 4, share_qk=False)) is None
    assert "value_dim" in online_train.ret_supported(MultiScaleRetention(96, 4, value_factor=1))
    assert "embed_dim" in online_train.ret_supported(MultiScaleRetention(192, 4))
    assert "look_ahead" in online_train.ret_supported(MultiScaleRetention(96, 4, look_ahead=1))
    assert "swish" in online_train.ret_supported(MultiScaleRetention(96, 4, gate_fn="gelu"))
    assert "retention" in online_train.ret_supported(torch.nn.MultiheadAttention(96, 4))


@pytest.mark.gpu
def test_fit_on_the_device_with_the_switch(monkeypatch):
    """TrainCLI fit, configs/onlineSpatialNet.yaml, synthetic data, 2 layers, 1.1-s segments (69 frames: two chunks), two epochs of two steps: the first
    step's loss is the switch-off run's to 1e-4 relative, and the loss decreases"""
    argv = ["fit", "--config", str(ROOT / "configs" / "onlineSpatialNet.yaml"), "--config", str(ROOT / "configs" / "datasets" / "synthetic.yaml"),
            "--model.arch.dim_input=12", "--model.arch.dim_output=4", "--model.arch.num_freqs=129", "--model.arch.num_layers=2", "--data.num_samples=[4,2,2]",
            "--data.audio_time_len=[1.1,1.1,1.1]", "--data.batch_size=[2,1]", "--trainer.max_epochs=2"]
    fit_with_switch(monkeypatch, argv, ["NBSS_ONLINE_NATIVE_RET"], RET)
