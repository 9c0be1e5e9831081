"""models/arch/base/mamba.py (the Mamba block in plain torch: mamba_ssm's interface and state_dict keys, written from the published equations; parity with
mamba_ssm itself is not pinned — the package is not installed) and the 'mamba(N,K)' variants of models/arch/OnlineSpatialNet.py behind NBSS_ONLINE_MAMBA=1:
parameters and their initialisation, the forward against an fp64 loop over the equations, the step form, a closed-form known answer, and the model's
state_dict keys, causality, `inference=True`, the streaming interface and the gates of the native paths."""
import math

import pytest
import torch
import torch.nn.functional as F

from util import rel_l2

KW = dict(dim_input=4, dim_output=4, num_layers=2, dim_squeeze=8, num_freqs=9, encoder_kernel_size=5, dim_hidden=32, dim_ffn=64, num_heads=4,
          dropout=(0, 0, 0), kernel_size=(5, 3), conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], full_share=0)
MAMBA_KEYS = ("in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "A_log", "D", "out_proj.weight")


def _mamba(seed=0, **kw):
    from models.arch.base.mamba import Mamba
    torch.manual_seed(seed)
    args = dict(d_model=96, d_state=16, d_conv=4, layer_idx=0)
    args.update(kw)
    return Mamba(**args)


@pytest.mark.parametrize("D,N,K", [(96, 16, 4), (32, 8, 3), (40, 16, 4)])
def test_parameters_and_init(D, N, K):
    m = _mamba(d_model=D, d_state=N, d_conv=K)
    E, R = 2 * D, math.ceil(D / 16)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {"in_proj.weight": (2 * E, D), "conv1d.weight": (E, 1, K), "conv1d.bias": (E,), "x_proj.weight": (R + 2 * N, E), "dt_proj.weight": (E, R),
                      "dt_proj.bias": (E,), "A_log": (E, N), "D": (E,), "out_proj.weight": (D, E)}
    assert set(shapes) == set(MAMBA_KEYS) and all(p.requires_grad for p in m.parameters())
    w = m.dt_proj.weight.detach().abs()
    assert float(w.max()) <= R ** -0.5 and float(w.max()) > 0.5 * R ** -0.5
    dt = F.softplus(m.dt_proj.bias.detach().double())
    assert float(dt.min()) >= 1e-3 * (1 - 1e-5) and float(dt.max()) <= 0.1 * (1 + 1e-5) and float(dt.max() / dt.min()) > 5  # log-uniform over [1e-3, 0.1]
    assert torch.allclose(m.A_log, torch.log(torch.arange(1, N + 1.0)).expand(E, N)) and torch.equal(m.D, torch.ones(E))
    assert float(m.in_proj.weight.detach().abs().max()) <= D ** -0.5 and float(m.conv1d.weight.detach().abs().max()) <= K ** -0.5  # torch's defaults


def _loop64(m, u):
    """the block's equations as an fp64 loop over frames, channels vectorised"""
    p = {k: v.detach().double() for k, v in m.state_dict().items()}
    E, R, N, K = m.d_inner, m.dt_rank, m.d_state, m.d_conv
    u = u.double()
    BF, T, _ = u.shape
    xz = u @ p["in_proj.weight"].T
    xr, z = xz[..., :E], xz[..., E:]
    A = -torch.exp(p["A_log"])
    h = torch.zeros(BF, E, N, dtype=torch.float64)
    out = []
    for t in range(T):
        acc = p["conv1d.bias"].expand(BF, E).clone()
        for k in range(K):
            if t - (K - 1) + k >= 0:
                acc = acc + p["conv1d.weight"][:, 0, k] * xr[:, t - (K - 1) + k]
        x = acc / (1 + torch.exp(-acc))
        dbc = x @ p["x_proj.weight"].T
        dt = torch.log1p(torch.exp(dbc[:, :R] @ p["dt_proj.weight"].T + p["dt_proj.bias"]))
        Bt, Ct = dbc[:, R:R + N], dbc[:, R + N:]
        h = torch.exp(dt[:, :, None] * A) * h + dt[:, :, None] * Bt[:, None, :] * x[:, :, None]
        y = (h * Ct[:, None, :]).sum(-1) + p["D"] * x
        out.append((y * (z[:, t] / (1 + torch.exp(-z[:, t])))) @ p["out_proj.weight"].T)
    return torch.stack(out, 1)


@pytest.mark.parametrize("D,N,K,T", [(96, 16, 4, 21), (32, 8, 3, 2), (40, 16, 4, 1)])
def test_forward_against_fp64_loop(D, N, K, T):
    m = _mamba(1, d_model=D, d_state=N, d_conv=K)
    with torch.no_grad():
        m.A_log.add_(0.3 * torch.randn_like(m.A_log))
        m.D.add_(0.3 * torch.randn_like(m.D))
    u = torch.randn(3, T, D)
    want = _loop64(m, u)
    assert rel_l2(m(u), want) < 2e-6 and rel_l2(m.double()(u.double()), want) < 1e-12


def test_forward_is_differentiable():
    m = _mamba(2).double()
    u = torch.randn(2, 6, 96, dtype=torch.float64, requires_grad=True)
    m(u).square().sum().backward()
    assert u.grad is not None and all(p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.norm()) > 0 for p in m.parameters())


def test_step_form_equals_forward():
    m = _mamba(3)
    u = torch.randn(3, 19, 96)
    with torch.no_grad():
        y = m(u)
        st = m.init_state(3)
        assert {k: tuple(v.shape) for k, v in st.items()} == {"conv": (3, 192, 3), "ssm": (3, 192, 16)}
        ys = torch.cat([m.step(u[:, t:t + 1], st) for t in range(19)], 1)
    assert rel_l2(ys, y) < 2e-6


def test_known_answer_geometric_series():
    """with dt_proj.weight and the dt rows of x_proj zeroed, dt = softplus(dt_proj.bias) is a constant; with the convolution reduced to its last tap a
    constant input u makes x_t = x, B_t = B and C_t = C constant from frame 0 on, so h is a geometric series: after T frames
    h = dt B x (1 - a^T) / (1 - a) with a = exp(dt A).  (With ALL of x_proj zeroed B = C = 0 and only the D skip would be left.)  y of the last frame
    against that closed form."""
    m = _mamba(4).double()
    E, R, N = m.d_inner, m.dt_rank, m.d_state
    with torch.no_grad():
        m.dt_proj.weight.zero_()
        m.x_proj.weight[:R].zero_()
        m.conv1d.weight[:, :, :-1].zero_()
    T = 40
    u = torch.randn(1, 1, 96, dtype=torch.float64).expand(2, T, 96).contiguous()
    with torch.no_grad():
        xz = m.in_proj(u[:, 0])
        x = F.silu(m.conv1d.weight[:, 0, -1] * xz[:, :E] + m.conv1d.bias)
        dbc = x @ m.x_proj.weight.T
        Bc, Cc = dbc[:, R:R + N], dbc[:, R + N:]
        dt = F.softplus(m.dt_proj.bias)
        a = torch.exp(dt[:, None] * -torch.exp(m.A_log))  # [E,N]
        h = (dt * x)[:, :, None] * Bc[:, None, :] * (1 - a ** T) / (1 - a)  # after T frames: sum_{i<T} a^i
        y = (h * Cc[:, None, :]).sum(-1) + m.D * x
        want = m.out_proj(y * F.silu(xz[:, E:]))
        got = m(u)[:, -1]
    assert rel_l2(got, want) < 1e-12


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------------
def _net(monkeypatch, attention="mamba(16,4)", seed=11, **kw):
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    monkeypatch.setenv("NBSS_ONLINE_MAMBA", "1")
    torch.manual_seed(seed)
    return OnlineSpatialNet(**{**KW, **kw}, attention=attention).eval()


def _common_keys(i):
    q = f"layers.{i}."
    keys = [q + f"{f}.{j}.{a}" for f in ("fconv1", "fconv2") for j, a in ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias"), (2, "weight"))]
    keys += [q + k for k in ("norm_full.weight", "norm_full.bias", "squeeze.0.weight", "squeeze.0.bias", "full.weight", "full.bias", "unsqueeze.0.weight",
                             "unsqueeze.0.bias", "norm_mhsa.weight", "norm_mhsa.bias")]
    return keys + [q + "mhsa." + k for k in MAMBA_KEYS]


def test_state_dict_keys(monkeypatch):
    base = {"encoder.weight", "encoder.bias", "decoder.weight", "decoder.bias"}
    net = _net(monkeypatch)
    want = set(base)
    for i in range(2):
        want |= set(_common_keys(i)) | {f"layers.{i}.norm_tconvffn.weight", f"layers.{i}.norm_tconvffn.bias"} | {f"layers.{i}.tconvffn.{k}" for k in MAMBA_KEYS}
    assert set(net.state_dict()) == want and net.attn_scope == 1 and net.pos is None
    assert tuple(net.state_dict()["layers.1.tconvffn.in_proj.weight"].shape) == (128, 32)
    net = _net(monkeypatch, "mamba(16,4,not_replace_ffn)")
    want = set(base)
    for i in range(2):
        want |= set(_common_keys(i)) | {f"layers.{i}.tconvffn.{j}.{a}" for j in (0, 1, 3, 5, 6, 8, 10) for a in ("weight", "bias")}
    assert set(net.state_dict()) == want and not hasattr(net.layers[0], "norm_tconvffn")
    assert net.layers[0].mhsa.d_state == 16 and net.layers[0].mhsa.d_conv == 4


@pytest.mark.parametrize("attention", ["mamba(16,4)", "mamba(8,3,not_replace_ffn)"])
def test_causal_inference_and_streaming(monkeypatch, attention):
    from models.arch.OnlineSpatialNet import OnlineStreamer
    net = _net(monkeypatch, attention)
    x = torch.randn(2, 9, 48, 4)
    with torch.no_grad():
        y = net(x)
        assert float((y[:, :, :25] - net(x[:, :, :25])).abs().max()) < 1e-5  # the reference's causality property
        assert rel_l2(net(x, inference=True), y) < 1e-5
        for chunk in (4, 16):
            st = net.init_stream(2)
            ys = torch.cat([net.forward_stream(x[:, :, c:c + chunk], st) for c in range(0, 48, chunk)], 2)
            s = OnlineStreamer(net, 2, chunk, use_graph=False)
            yz = torch.cat([s.step(x[:, :, c:c + chunk]) for c in range(0, 48, chunk)], 2)
            assert rel_l2(ys, y) < 1e-5 and rel_l2(yz, y) < 1e-5, chunk
        s.reset()
        assert rel_l2(s.step(x[:, :, :16]), y[:, :, :16]) < 1e-5  # a new utterance from the empty state


@pytest.mark.parametrize("attention", ["mamba(16,4)", "mamba(16,4,not_replace_ffn)"])
def test_native_gates_give_reasons(monkeypatch, attention, emu_lib):
    """everything that walks layer.tconvffn as a ModuleList, or expects retention, answers with a reason for a mamba layer; the cross-band gate accepts it"""
    from nbss_amd import online, online_train
    from nbss_amd.online import NativeOnlineStreamer
    net = _net(monkeypatch, attention, dim_hidden=96, dim_ffn=192).train()
    layer, h = net.layers[0], torch.zeros(1, 9, 6, 96)
    assert "mamba" in online.supported(net)
    with pytest.raises(NotImplementedError, match="mamba"):
        NativeOnlineStreamer(net, 1, 4, lib=emu_lib)
    replaced = "not_replace_ffn" not in attention
    assert (online_train.supported(layer) is not None) == replaced
    assert "Mamba" in online_train.ret_supported(layer.mhsa) and "Mamba" in online_train.tsa_supported(layer)
    assert online_train.xband_supported(layer) is None and online_train.mamba_supported(layer.mhsa) is None
    for s in ("NBSS_ONLINE_NATIVE_TRAIN", "NBSS_ONLINE_NATIVE_RET", "NBSS_ONLINE_NATIVE_TSA", "NBSS_ONLINE_NATIVE_XBAND", "NBSS_ONLINE_NATIVE_MAMBA"):
        monkeypatch.setenv(s, "1")
    with online_train.use_lib(emu_lib):
        if replaced:
            assert online_train.eligible(layer, h, None).startswith("!the T-ConvFFN must be")
        assert online_train.ret_eligible(layer, h[0], None, True, False, None, False).startswith("!the attention must be retention")
        assert online_train.tsa_eligible(layer, h, None, True, False, None, False).startswith("!the attention must be retention")
        assert online_train.xband_eligible(layer, h, None) is None and online_train.mamba_eligible(layer.mhsa, h[0], None, False) is None
        assert online_train.mamba_eligible(layer.mhsa, h[0], {}, False) == online_train.mamba_eligible(layer.mhsa, h[0], None, True) == "streaming or inference call"


def test_constructor_names_the_switch(monkeypatch):
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    for value in (None, "0", "true", "11"):
        monkeypatch.delenv("NBSS_ONLINE_MAMBA", raising=False)
        if value is not None:
            monkeypatch.setenv("NBSS_ONLINE_MAMBA", value)
        with pytest.raises(NotImplementedError, match="mamba.*NBSS_ONLINE_MAMBA=1.*parity with mamba_ssm is not pinned"):
            OnlineSpatialNet(**KW, attention="mamba(16,4)")
