"""NBC2 / NBC inference beyond 256 frames on the native path (NBSS_NB_LONG=1): the key-blocked forward attention kernels behind
nbss_nb_attention_long_fwd (csrc/attn_kb.hip, head widths 24 / 48 / 96) and nbss_nb_attention_relpos_long_fwd (csrc/attn_relpos_kb.hip, 24 / 48) against
the fp64 formulas, the runners against the reference's own NBC2 / NBC on 300 frames (tests/golden/nb_long.npz, written by
tests/golden/make_golden_nb_long.py), the switch, the refusals that remain and the modules' dispatch on the device."""
import math
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32, NbssError
from util import rel_l2

DTYPES = [pytest.param(NBSS_F32, id="f32"), pytest.param(NBSS_BF16, id="bf16")]
# block - 1 / block / block + 1 of the 64-key blocks, the old cap and its neighbours, more than four key blocks and query blocks
LENGTHS = [1, 63, 64, 65, 129, 256, 257, 300, 321]
RELPOS_LENGTHS = [1, 2, 17, 64, 65, 129, 257, 300]
GOLDEN = Path(__file__).resolve().parent / "golden" / "nb_long.npz"
UNSUPPORTED = "-2|UNSUPPORTED|unsupported"


def _td(dtype):
    return torch.bfloat16 if dtype == NBSS_BF16 else torch.float32


def _tol(dtype):
    return 2e-5 if dtype == NBSS_F32 else 1.5e-2  # (the bars of tests/test_nbc2_large.py / test_relpos_attention_and_group_norm_blocks)


# ---- 1, 2: softmax(q k^T / sqrt(dh)) v ---------------------------------------------------------------------------------------------------------------
def _attn64(qkv64, nseq, T, heads, dh):
    H = heads * dh
    q, k, v = [t.reshape(nseq, T, heads, dh).transpose(1, 2) for t in qkv64.split(H, dim=-1)]
    return (torch.softmax(q @ k.transpose(-1, -2) / dh ** 0.5, -1) @ v).transpose(1, 2).reshape(nseq, T, H)


def _long_fwd(backend, dtype, qkv, heads, entry="nbss_nb_attention_long_fwd"):
    """qkv: stream-dtype host tensor -> o on the backend's device (the output buffer starts as NaN: every element must be written)"""
    lib, dev = backend.lib, backend.device
    nseq, T, H3 = qkv.shape
    qd = qkv.to(dev).contiguous()
    o = torch.full((nseq, T, H3 // 3), float("nan"), dtype=qd.dtype, device=dev)
    lib.call(entry, dtype, nseq, T, H3 // 3, heads, ops._ptr(lib, qd), ops._ptr(lib, o), ops._stream(lib, qd))
    return o


def _check_plain(backend, dtype, qkv, nseq, T, heads, dh):
    qs = qkv.to(_td(dtype))  # (the fp64 formula on the inputs as the stream holds them)
    got = _long_fwd(backend, dtype, qs, heads)
    assert torch.equal(got, _long_fwd(backend, dtype, qs, heads)), "the forward is not repeatable"
    e = rel_l2(got, _attn64(qs.double(), nseq, T, heads, dh))
    print(f"long attention {backend.name} dtype={dtype} dh={dh} heads={heads} T={T}: rel_l2 {e:.3e}")
    assert e < _tol(dtype), (dh, heads, T, e)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("dh", [24, 48, 96])
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_attention_forward(backend, dtype, dh, heads, T):
    """nbss_nb_attention_long_fwd at the three head widths against fp64 torch on the stream-rounded inputs: 2e-5 fp32, 1.5e-2 bf16; two runs bit-equal"""
    g = torch.Generator().manual_seed(1000 * dh + 100 * heads + T)
    nseq = 2
    _check_plain(backend, dtype, torch.randn(nseq, T, 3 * heads * dh, generator=g), nseq, T, heads, dh)


@pytest.mark.parametrize("dh", [24, 48])
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_attention_logit_range(backend, dtype, dh):
    """the construction of test_nbc2_large.py::test_attention96_logit_range at the narrow widths and 300 frames: scores beyond +- 30 and row maxima that
    rise after the first key block in most rows — a wrong rescale of O or of the running sum cannot pass.  Same bars."""
    g = torch.Generator().manual_seed(42 + dh)
    nseq, T, heads = 2, 300, 2
    H = heads * dh
    qkv = torch.randn(nseq, T, 3 * H, generator=g)
    qkv[..., :H] *= 10.0
    qs = qkv.to(_td(dtype)).double()
    q, k = [t.reshape(nseq, T, heads, dh).transpose(1, 2) for t in qs.split(H, dim=-1)[:2]]
    s = q @ k.transpose(-1, -2) / dh ** 0.5
    assert s.max() >= 30 and s.min() <= -30
    bmax = torch.stack([s[..., b:b + 64].amax(-1) for b in range(0, T, 64)], -1)  # row maximum inside each key block
    assert ((bmax[..., 1:].amax(-1) - bmax[..., 0]) > 1).float().mean() > 0.5     # most rows: the running maximum moves after the first block
    _check_plain(backend, dtype, qkv, nseq, T, heads, dh)


# ---- 3: the relative-position attention ---------------------------------------------------------------------------------------------------------------
def _relpos64(qkv, pos, u, v, scale, heads):
    """the gather formula of tests/test_nbc_native.py::test_relpos_attention_and_group_norm_blocks (= the reference's NBC.py:106-143), fp64"""
    nseq, T, H3 = qkv.shape
    H, dh = H3 // 3, H3 // 3 // heads
    q, k, vv = [t.double().view(nseq, T, heads, dh).transpose(1, 2) for t in qkv.split(H, -1)]
    P = pos.double().view(2 * T - 1, heads, dh).permute(1, 2, 0)
    content = (q + u.double()[None, :, None]) @ k.transpose(-1, -2)
    qp = (q + v.double()[None, :, None]) @ P
    idx = torch.arange(T)
    rel = (idx[:, None] - idx[None, :] + T - 1).expand(nseq, heads, T, T)
    return (torch.softmax((content + qp.gather(-1, rel)) * scale, -1) @ vv).transpose(1, 2).reshape(nseq, T, H)


def _relpos_fwd(backend, dtype, entry, qkv, pos, u, v, scale, heads):
    lib, dev = backend.lib, backend.device
    nseq, T, H3 = qkv.shape
    qd, pd, ud, vd = qkv.to(dev).contiguous(), pos.to(dev).contiguous(), u.to(dev).contiguous(), v.to(dev).contiguous()
    o = torch.full((nseq, T, H3 // 3), float("nan"), dtype=qd.dtype, device=dev)
    lib.call(entry, dtype, nseq, T, H3 // 3, heads, ops._ptr(lib, qd), ops._ptr(lib, pd), ops._ptr(lib, ud), ops._ptr(lib, vd), scale, ops._ptr(lib, o),
             ops._stream(lib, qd))
    return o


@pytest.mark.parametrize("T", RELPOS_LENGTHS)
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("dh", [24, 48])
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_relpos_attention_forward(backend, dtype, dh, heads, T):
    """nbss_nb_attention_relpos_long_fwd against the fp64 gather formula (non-zero u / v, a random table): 2e-5 fp32, 1.5e-2 bf16; two runs bit-equal; up
    to 256 frames also against the whole-head kernel (nbss_nb_attention_relpos_fwd) on the same inputs: rel_l2 below the fp32 bar in the fp32 stream.  In
    the bf16 stream both kernels round their output (and their probabilities, one before and one after the normalisation) to bf16, 2^-9 relative per
    element: two correct results differ by about 3e-3 (measured on the emulator: 2.5e-3 .. 3.4e-3 from 2 frames on, 0 at one frame), so there the
    comparison holds the bf16 bar."""
    g = torch.Generator().manual_seed(1000 * dh + 100 * heads + T + 1)
    nseq, H, td = 2, heads * dh, _td(dtype)
    qkv = torch.randn(nseq, T, 3 * H, generator=g).to(td)
    pos = torch.randn(2 * T - 1, H, generator=g).to(td)
    u, v = torch.randn(heads, dh, generator=g) * 0.5, torch.randn(heads, dh, generator=g) * 0.5
    scale = 1.0 / math.sqrt(H)
    got = _relpos_fwd(backend, dtype, "nbss_nb_attention_relpos_long_fwd", qkv, pos, u, v, scale, heads)
    assert torch.equal(got, _relpos_fwd(backend, dtype, "nbss_nb_attention_relpos_long_fwd", qkv, pos, u, v, scale, heads)), "the forward is not repeatable"
    e = rel_l2(got, _relpos64(qkv, pos, u, v, scale, heads))
    print(f"long relpos attention {backend.name} dtype={dtype} dh={dh} heads={heads} T={T}: rel_l2 {e:.3e}")
    assert e < _tol(dtype), (dh, heads, T, e)
    if T <= 256:
        whole = _relpos_fwd(backend, dtype, "nbss_nb_attention_relpos_fwd", qkv, pos, u, v, scale, heads)
        ew = rel_l2(got, whole)
        print(f"    against the whole-head kernel: rel_l2 {ew:.3e}")
        assert ew < (2e-5 if dtype == NBSS_F32 else 1.5e-2), (dh, heads, T, ew)


# ---- 4: refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_long_refusals(backend):
    """4097 frames, head width 64 and head width 96 on the relative-position entry: NBSS_EUNSUPPORTED; the whole-head entry points still refuse 257 frames"""
    lib, dev = backend.lib, backend.device

    def plain(entry, T, H, heads):
        qkv, o = torch.zeros(1, T, 3 * H, device=dev), torch.zeros(1, T, H, device=dev)
        lib.call(entry, NBSS_F32, 1, T, H, heads, ops._ptr(lib, qkv), ops._ptr(lib, o), ops._stream(lib, qkv))

    def relpos(entry, T, H, heads):
        qkv, o, pos = torch.zeros(1, T, 3 * H, device=dev), torch.zeros(1, T, H, device=dev), torch.zeros(2 * T - 1, H, device=dev)
        u = torch.zeros(heads, H // heads, device=dev)
        lib.call(entry, NBSS_F32, 1, T, H, heads, ops._ptr(lib, qkv), ops._ptr(lib, pos), ops._ptr(lib, u), ops._ptr(lib, u), 1.0, ops._ptr(lib, o),
                 ops._stream(lib, qkv))

    for T, H, heads in ((4097, 48, 2), (4097, 96, 1), (16, 128, 2)):
        with pytest.raises(NbssError, match=UNSUPPORTED):
            plain("nbss_nb_attention_long_fwd", T, H, heads)
    for T, H, heads in ((4097, 48, 2), (16, 128, 2), (16, 96, 1), (300, 192, 2)):
        with pytest.raises(NbssError, match=UNSUPPORTED):
            relpos("nbss_nb_attention_relpos_long_fwd", T, H, heads)
    for H, heads in ((48, 2), (96, 2), (192, 2)):
        with pytest.raises(NbssError, match=UNSUPPORTED):
            plain("nbss_nb_attention_fwd", 257, H, heads)
    with pytest.raises(NbssError, match=UNSUPPORTED):
        relpos("nbss_nb_attention_relpos_fwd", 257, 48, 2)


# ---- 5, 6: the runners against the reference, and the switch -----------------------------------------------------------------------------------------
_GOLD = {}


def _case(name):
    """(x, y, params, the reference's own fp32 error) of one network of the fixture (loaded once)"""
    if not _GOLD:
        d = np.load(GOLDEN)
        _GOLD.update({k: torch.from_numpy(np.asarray(d[k]).astype(np.float32) if d[k].dtype == np.float16 else np.asarray(d[k])) for k in d.files})
    pre = name + "/"
    t = {k[len(pre):]: v for k, v in _GOLD.items() if k.startswith(pre)}
    return t["x"], t["y"], {k[len("param/"):]: v for k, v in t.items() if k.startswith("param/")}, float(t["ref32/y"])


def _nbc2(dh, params, dev):
    from models.arch.NBC2 import NBC2
    bk = {"n_heads": 1, "dropout": 0, "conv_kernel_size": 3, "n_conv_groups": 4, "norms": ("LN", "GBN", "GBN"),
          "group_batch_norm_kwargs": {"share_along_sequence_dim": False}}
    net = NBC2(dim_input=4, dim_output=4, n_layers=1, dim_hidden=dh, dim_ffn=32, num_freqs=5, block_kwargs=bk)
    assert set(net.state_dict()) == set(params)
    net.load_state_dict(params)
    return net.float().to(dev).eval()


def _nbc(params, dev):
    from models.arch.NBC import NBC
    net = NBC(dim_input=4, dim_output=4, n_layers=1, encoder_kernel_size=4, n_heads=2, hidden_size=48, ffn_size=64)
    assert {k for k in net.state_dict() if not k.endswith("rel_pos.pe")} == set(params)
    net.load_state_dict(params, strict=False)
    return net.float().to(dev).eval()


@pytest.mark.parametrize("dh", [24, 48, 96])
def test_native_nbc2_long_equals_the_reference(backend, monkeypatch, dh):
    """NativeNBC2.forward with NBSS_NB_LONG=1 on 1 x 5 x 300 frames against the REFERENCE's own NBC2 run in fp64 (one layer, one head of width dh): the bar
    of test_native_nbc2_head96_equals_the_reference, 5e-6; the reference itself in fp32 on the same data (stored in the fixture) lies under it.
    Without the switch the same call is refused, naming the frame count; forward_train refuses 300 frames whatever the switch says."""
    from nbss_amd.nbc2 import NativeNBC2, supported
    x, y_ref, params, e32 = _case(f"nbc2_{dh}")
    assert x.shape == (1, 5, 300, 4) and e32 < 5e-6
    net = _nbc2(dh, params, backend.device)
    assert supported(net) is None
    run, xd = NativeNBC2(net, backend.lib), x.to(backend.device)
    monkeypatch.delenv("NBSS_NB_LONG", raising=False)
    with pytest.raises(NbssError, match="300 frames"):
        run.forward(xd)
    monkeypatch.setenv("NBSS_NB_LONG", "1")
    with torch.no_grad():
        y = run.forward(xd)
    e = rel_l2(y, y_ref)
    print(f"nbc2 long dh={dh} {backend.name}: forward rel_l2 {e:.3e} (reference in fp32: {e32:.3e})")
    assert y.shape == y_ref.shape and e < 5e-6
    with pytest.raises(NbssError, match="300 frames"):
        run.forward_train(xd)


def test_native_nbc_long_equals_the_reference(backend, monkeypatch):
    """NativeNBC.forward with NBSS_NB_LONG=1 on 1 x 5 x 300 frames against the REFERENCE's own NBC run in fp64 (one layer, hidden 48 / 2 heads): the bar of
    test_native_nbc_forward_fp32, 2e-5; the reference itself in fp32 lies under it.  Without the switch: refused, naming the frame count; forward_train
    refuses whatever the switch says."""
    from nbss_amd.nbc import NativeNBC, supported
    x, y_ref, params, e32 = _case("nbc")
    assert x.shape == (1, 5, 300, 4) and e32 < 2e-5
    net = _nbc(params, backend.device)
    assert supported(net) is None
    run, xd = NativeNBC(net, backend.lib), x.to(backend.device)
    monkeypatch.delenv("NBSS_NB_LONG", raising=False)
    with pytest.raises(NbssError, match="300 frames"):
        run.forward(xd)
    monkeypatch.setenv("NBSS_NB_LONG", "1")
    y = run.forward(xd)
    e = rel_l2(y, y_ref)
    print(f"nbc long {backend.name}: forward rel_l2 {e:.3e} (reference in fp32: {e32:.3e})")
    assert y.shape == y_ref.shape and e < 2e-5
    with pytest.raises(NbssError, match="300 frames"):
        run.forward_train(xd)


def test_long_limits_of_the_runners(emu_lib, monkeypatch):
    """with the switch on: 4097 frames, and NBC beyond its sinusoid table (T - K + 1 > max_len + 1 = 1001), are refused before any launch"""
    from nbss_amd.nbc import NativeNBC
    from nbss_amd.nbc2 import NativeNBC2
    from nbss_amd.nb import long_enabled
    monkeypatch.delenv("NBSS_NB_LONG", raising=False)
    assert not long_enabled()
    monkeypatch.setenv("NBSS_NB_LONG", "1")
    assert long_enabled()
    net2, net = _nbc2(24, _case("nbc2_24")[2], "cpu"), _nbc(_case("nbc")[2], "cpu")  # (the runners hold their modules weakly)
    nbc2, nbc = NativeNBC2(net2, emu_lib), NativeNBC(net, emu_lib)
    with pytest.raises(NbssError, match="4097 frames"):
        nbc2.forward(torch.zeros(1, 5, 4097, 4))
    with pytest.raises(NbssError, match="4097 frames"):
        nbc.forward(torch.zeros(1, 1, 4097, 4))
    with pytest.raises(NbssError, match="1005 frames.*sinusoid"):
        nbc.forward(torch.zeros(1, 1, 1005, 4))


# ---- 7: the modules on the device ---------------------------------------------------------------------------------------------------------------------
def _dispatch(net, x, monkeypatch, off_switch, label):
    """no_grad + NBSS_NB_LONG=1: silent, another implementation than the torch.nn modules, equal to 1e-4; train mode with grad: the "300 frames" warning"""
    monkeypatch.setenv("NBSS_NB_LONG", "1")
    with torch.no_grad():
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the native path is silent
            got = net(x)
        monkeypatch.setenv(off_switch, "0")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = net(x)
        monkeypatch.delenv(off_switch)
    assert got.shape == want.shape and not torch.equal(got, want)  # (another implementation ran)
    e = rel_l2(got, want)
    print(f"{label} 1x9x300 on the device: native vs torch.nn {e:.3e}")
    assert e < 1e-4
    net.train()
    with pytest.warns(RuntimeWarning, match="300 frames"):
        y = net(x)
    assert y.requires_grad and "TrainFn" not in type(y.grad_fn).__name__
    if label == "NBC2":  # (no dropout: the torch.nn modules give the eval result; NBC's train mode draws dropout masks)
        assert rel_l2(y.detach(), want) < 1e-5


@pytest.mark.gpu
def test_nbc2_module_takes_the_long_path_on_the_device(hip_lib, monkeypatch):
    from models.arch.NBC2 import NBC2
    torch.manual_seed(11)
    net = NBC2(dim_input=12, dim_output=4, n_layers=1, dim_hidden=96, dim_ffn=192, num_freqs=9).cuda().eval()
    _dispatch(net, torch.randn(1, 9, 300, 12).cuda(), monkeypatch, "NBSS_NBC2_NATIVE", "NBC2")


@pytest.mark.gpu
def test_nbc_module_takes_the_long_path_on_the_device(hip_lib, monkeypatch):
    from models.arch.NBC import NBC
    torch.manual_seed(12)
    net = NBC(dim_input=12, dim_output=4, n_layers=1, encoder_kernel_size=4, n_heads=2, hidden_size=96, ffn_size=192).cuda().eval()
    with torch.no_grad():  # (biases and the position biases away from their zero / symmetric initial values)
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    _dispatch(net, torch.randn(1, 9, 300, 12).cuda(), monkeypatch, "NBSS_NBC_NATIVE", "NBC")
