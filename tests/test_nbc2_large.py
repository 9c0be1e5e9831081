"""NBC2-large (dim_hidden 192, dim_ffn 384, 2 heads: attention head width 96) on the native path: the key-blocked attention of csrc/attn_kb.hip
(forward and backward, block of 64 keys / queries) against fp64 torch, the module against the reference's own NBC2 (tests/golden/nbc2_head96.npz,
written by tests/golden/make_golden_nbc2_wide.py), the shipped geometry on the device, and the refusals that remain."""
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32, NbssError
from util import rel_l2

DTYPES = [pytest.param(NBSS_F32, id="f32"), pytest.param(NBSS_BF16, id="bf16")]
DH = 96
NARROW = [24, 48]  # the whole-head kernels behind the same two entry points
# the lengths the narrow heads are tested at, plus those that straddle the 64-row block: block - 1, block, block + 1, two blocks + 1
LENGTHS = [1, 2, 15, 16, 17, 31, 33, 48, 100, 255, 256, 63, 64, 65, 129]
GOLDEN = Path(__file__).resolve().parent / "golden" / "nbc2_head96.npz"


def _td(dtype):
    return torch.bfloat16 if dtype == NBSS_BF16 else torch.float32


def _attn64(qkv64, nseq, T, heads):
    H = qkv64.shape[-1] // 3
    dh = H // heads
    q, k, v = [t.reshape(nseq, T, heads, dh).transpose(1, 2) for t in qkv64.split(H, dim=-1)]
    return (torch.softmax(q @ k.transpose(-1, -2) / dh ** 0.5, -1) @ v).transpose(1, 2).reshape(nseq, T, H)


def _fwd(backend, dtype, qkv, heads):
    """qkv: stream-dtype host tensor -> o on the backend's device"""
    lib, dev = backend.lib, backend.device
    nseq, T, H3 = qkv.shape
    qd = qkv.to(dev).contiguous()
    o = torch.full((nseq, T, H3 // 3), float("nan"), dtype=qd.dtype, device=dev)
    lib.call("nbss_nb_attention_fwd", dtype, nseq, T, H3 // 3, heads, ops._ptr(lib, qd), ops._ptr(lib, o), ops._stream(lib, qd))
    return o


def _bwd(backend, dtype, qkv, do, heads):
    lib, dev = backend.lib, backend.device
    nseq, T, H3 = qkv.shape
    H = H3 // 3
    qd, dd = qkv.to(dev).contiguous(), do.to(dev).contiguous()
    dqkv = torch.full((nseq, T, H3), float("nan"), dtype=qd.dtype, device=dev)
    ws = torch.empty(lib._dll.nbss_nb_attention_bwd_ws_bytes(dtype, nseq, T, H, heads), dtype=torch.uint8, device=dev)
    lib.call("nbss_nb_attention_bwd", dtype, nseq, T, H, heads, ops._ptr(lib, qd), ops._ptr(lib, dd), ops._ptr(lib, dqkv), ops._ptr(lib, ws), ops._stream(lib, qd))
    return dqkv


def _grad64(qkv, do, nseq, T, heads):
    q64 = qkv.double().requires_grad_(True)
    (_attn64(q64, nseq, T, heads) * do.double()).sum().backward()
    return q64.grad


def _torch_bf16_grad(qkv, do, nseq, T, heads):
    """torch's own bf16 computation (host, bf16 tensors throughout) of the same forward + autograd backward"""
    H = qkv.shape[-1] // 3
    dh = H // heads
    qb = qkv.to(torch.bfloat16).requires_grad_(True)
    q, k, v = [t.reshape(nseq, T, heads, dh).transpose(1, 2) for t in qb.split(H, dim=-1)]
    o = (torch.softmax(q @ k.transpose(-1, -2) / dh ** 0.5, -1) @ v).transpose(1, 2).reshape(nseq, T, H)
    o.backward(do.to(torch.bfloat16))
    return qb.grad


def _check_fwd(backend, dtype, qkv, nseq, T, heads):
    qs = qkv.to(_td(dtype))
    e = rel_l2(_fwd(backend, dtype, qs, heads), _attn64(qs.double(), nseq, T, heads))
    print(f"attention fwd {backend.name} dtype={dtype} dh={qkv.shape[-1] // 3 // heads} heads={heads} T={T}: rel_l2 {e:.3e}")
    assert e < (2e-5 if dtype == NBSS_F32 else 1.5e-2), (T, heads, e)


def _check_bwd(backend, dtype, qkv, do, nseq, T, heads):
    qs, ds = qkv.to(_td(dtype)), do.to(_td(dtype))
    want = _grad64(qs, ds, nseq, T, heads)  # (the fp64 formula on the inputs as the stream holds them)
    got = _bwd(backend, dtype, qs, ds, heads)
    again = _bwd(backend, dtype, qs, ds, heads)
    assert torch.equal(got, again), "the backward is not repeatable"
    e = rel_l2(got, want)
    if dtype == NBSS_F32:
        print(f"attention bwd {backend.name} f32 dh={qkv.shape[-1] // 3 // heads} heads={heads} T={T}: rel_l2 {e:.3e}")
        assert e < 5e-5, (T, heads, e)
    else:
        e_torch = rel_l2(_torch_bf16_grad(qs, ds, nseq, T, heads), want)
        print(f"attention bwd {backend.name} bf16 dh={qkv.shape[-1] // 3 // heads} heads={heads} T={T}: torch-bf16 {e_torch:.3e}  kernel {e:.3e}")
        assert e <= 1.5 * e_torch, (T, heads, e, e_torch)


def _forward_case(backend, dtype, dh, heads, T):
    g = torch.Generator().manual_seed(100 * T + heads)
    nseq = 2
    _check_fwd(backend, dtype, torch.randn(nseq, T, 3 * heads * dh, generator=g), nseq, T, heads)


def _backward_case(backend, dtype, dh, heads, T):
    g = torch.Generator().manual_seed(100 * T + heads + 7)
    nseq = 2
    qkv = torch.randn(nseq, T, 3 * heads * dh, generator=g)
    do = torch.randn(nseq, T, heads * dh, generator=g)
    _check_bwd(backend, dtype, qkv, do, nseq, T, heads)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention96_forward(backend, dtype, heads, T):
    """softmax(q k^T / sqrt(96)) v of nbss_nb_attention_fwd at head width 96 against fp64 torch: the bars the block meets at widths 24 / 48"""
    _forward_case(backend, dtype, DH, heads, T)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention96_backward(backend, dtype, heads, T):
    """nbss_nb_attention_bwd at head width 96 against torch autograd in fp64; run twice: bitwise repeatable.  fp32: rel_l2(dqkv) < 5e-5 (the bar of widths
    24 / 48).  bf16: the comparator is the fp64 formula on the bf16-rounded inputs and the allowance 1.5 x the error torch's own bf16 forward + autograd
    backward (host) shows against it on the same inputs (the margin of tests/test_bf16_vs_reference.py: accumulation order differs, precision class
    does not).  Largest case (T = 256, 2 heads), measured: torch-bf16 error 5.69e-03, kernel error 2.35e-03 on the emulator and 2.35e-03 on the MI355X
    (T = 1 is the exact case: one key, softmax == 1, torch's error is 0 and so must the kernel's be: D = rowsum(P dP) equals dP bit for bit, dS == 0)."""
    _backward_case(backend, dtype, DH, heads, T)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("dh", NARROW)
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_narrow_forward(backend, dtype, dh, heads, T):
    """the same entry point, cases, fp64 reference and bars at head widths 24 / 48: the whole-head kernels of csrc/gb_attn.hip"""
    _forward_case(backend, dtype, dh, heads, T)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("dh", NARROW)
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_narrow_backward(backend, dtype, dh, heads, T):
    """nbss_nb_attention_bwd at head widths 24 / 48 (gb_attn_q_kernel / gb_attn_k_kernel): the references and bars of test_attention96_backward"""
    _backward_case(backend, dtype, dh, heads, T)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention96_logit_range(backend, dtype):
    """scores spanning more than +- 30, with row maxima that rise from key block to key block: a wrong running-max rescale of O or of the running sum
    cannot pass.  Same bars as the two tests above."""
    g = torch.Generator().manual_seed(42)
    nseq, T, heads = 2, 200, 2
    H = heads * DH
    qkv = torch.randn(nseq, T, 3 * H, generator=g)
    qkv[..., :H] *= 10.0
    do = torch.randn(nseq, T, H, generator=g)
    qs = qkv.to(_td(dtype)).double()
    q, k = [t.reshape(nseq, T, heads, DH).transpose(1, 2) for t in qs.split(H, dim=-1)[:2]]
    s = q @ k.transpose(-1, -2) / DH ** 0.5
    assert s.max() >= 30 and s.min() <= -30
    bmax = torch.stack([s[..., b:b + 64].amax(-1) for b in range(0, T, 64)], -1)  # row maximum inside each key block
    assert ((bmax[..., 1:].amax(-1) - bmax[..., 0]) > 1).float().mean() > 0.5     # most rows: the running maximum moves after the first block
    _check_fwd(backend, dtype, qkv, nseq, T, heads)
    _check_bwd(backend, dtype, qkv, do, nseq, T, heads)


def test_refusals_that_remain(backend):
    """head widths 12 and 64 are still named by supported(); the C entry points still refuse H / heads = 64 and 257 frames at any width"""
    from models.arch.NBC2 import NBC2
    from nbss_amd.nbc2 import supported
    lib, dev = backend.lib, backend.device
    for hidden, heads in ((96, 8), (128, 2)):
        bk = {"n_heads": heads, "dropout": 0, "conv_kernel_size": 3, "n_conv_groups": 8, "norms": ("LN", "GBN", "GBN"),
              "group_batch_norm_kwargs": {"share_along_sequence_dim": False}}
        assert "head width" in supported(NBC2(dim_input=12, dim_output=4, n_layers=1, dim_hidden=hidden, dim_ffn=192, num_freqs=9, block_kwargs=bk))
    for T, H, heads in ((16, 128, 2), (257, 48, 2), (257, 96, 2), (257, 192, 2)):
        qkv = torch.zeros(1, T, 3 * H, device=dev)
        o, do, dqkv = torch.zeros(1, T, H, device=dev), torch.zeros(1, T, H, device=dev), torch.zeros(1, T, 3 * H, device=dev)
        ws = torch.empty(lib._dll.nbss_nb_attention_bwd_ws_bytes(NBSS_F32, 1, T, H, heads), dtype=torch.uint8, device=dev)
        with pytest.raises(NbssError, match="-2|UNSUPPORTED|unsupported"):
            lib.call("nbss_nb_attention_fwd", NBSS_F32, 1, T, H, heads, ops._ptr(lib, qkv), ops._ptr(lib, o), ops._stream(lib, qkv))
        with pytest.raises(NbssError, match="-2|UNSUPPORTED|unsupported"):
            lib.call("nbss_nb_attention_bwd", NBSS_F32, 1, T, H, heads, ops._ptr(lib, qkv), ops._ptr(lib, do), ops._ptr(lib, dqkv), ops._ptr(lib, ws), ops._stream(lib, qkv))


def _golden():
    d = np.load(GOLDEN)
    t = {k: torch.from_numpy(np.asarray(d[k]).astype(np.float32) if d[k].dtype == np.float16 else np.asarray(d[k])) for k in d.files}
    params = {k[len("param/"):]: v for k, v in t.items() if k.startswith("param/")}
    grads = {k[len("grad/"):]: v for k, v in t.items() if k.startswith("grad/")}
    return t, params, grads


def test_native_nbc2_head96_equals_the_reference(backend):
    """the native forward and forward_train + backward at head width 96 against the REFERENCE's own NBC2 run in fp64 (tests/golden/nbc2_head96.npz:
    dim_hidden 192, 2 heads, dim_ffn 64 in 4 conv groups, 1 layer, 2 x 5 x 33): output and every parameter gradient of sum(y * r), with the bars of
    tests/test_nb_native_vs_reference.py::test_native_nbc2_equals_the_reference (5e-6 output, 2e-5 + floor 1e-7 gradients).  The fixture also holds the
    error of the reference module itself in fp32 on the same data (output 3.1e-7, gradients 6.0e-7): the wider contraction needs no wider bar.
    (in_proj_weight's gradient is stored every second row.)"""
    from models.arch.NBC2 import NBC2
    from nbss_amd.nbc2 import NativeNBC2, supported
    lib, dev = backend.lib, backend.device
    t, params, grads = _golden()
    x, r, y_ref = t["x"].to(dev), t["r"].to(dev), t["y"]
    bk = {"n_heads": 2, "dropout": 0, "conv_kernel_size": 3, "n_conv_groups": 4, "norms": ("LN", "GBN", "GBN"),
          "group_batch_norm_kwargs": {"share_along_sequence_dim": False}}
    net = NBC2(dim_input=4, dim_output=4, n_layers=1, dim_hidden=192, dim_ffn=64, num_freqs=5, block_kwargs=bk)
    assert set(net.state_dict()) == set(params)
    net.load_state_dict(params)
    net = net.float().to(dev).train()
    assert supported(net) is None
    run = NativeNBC2(net, lib)
    e = rel_l2(run.forward(x), y_ref)
    print(f"nbc2 head96 {backend.name}: forward rel_l2 {e:.3e} (reference in fp32: {float(t['ref32/y']):.3e})")
    assert e < 5e-6
    y = run.forward_train(x)
    (y.float() * r).sum().backward()
    assert y.shape == y_ref.shape and rel_l2(y.detach(), y_ref) < 5e-6
    top = max(float(g.norm()) for g in grads.values())
    bad, seen, worst = {}, set(), 0.0
    for n, p in net.named_parameters():
        assert p.grad is not None and n in grads, n
        g = p.grad.detach().float().cpu()
        if g.dim() == 2 and g.shape[0] >= 512:
            g = g[::2]
        want = grads[n]
        assert g.shape == want.shape, (n, g.shape, want.shape)
        err = float((g.double() - want.double()).norm())
        worst = max(worst, err / float(want.norm()))
        if err > 2e-5 * float(want.norm()) + 1e-7 * top:
            bad[n] = (err, float(want.norm()))
        seen.add(n)
    print(f"nbc2 head96 {backend.name}: worst gradient rel_l2 {worst:.3e} (reference in fp32: {float(t['ref32/grad']):.3e})")
    assert seen == set(grads) and not bad, bad


def _large(n_layers=12, F=129):
    from models.arch.NBC2 import NBC2
    return NBC2(dim_input=12, dim_output=4, n_layers=n_layers, dim_hidden=192, dim_ffn=384, num_freqs=F)


def test_supported_admits_nbc2_large():
    from nbss_amd.nbc2 import _train_supported, supported
    net = _large()
    assert supported(net) is None and _train_supported(net) is None


@pytest.mark.gpu
def test_nbc2_large_module_takes_the_native_path_on_the_device(hip_lib, monkeypatch):
    """NBC2-large as configs/NBC2.yaml names it (12 layers, 192 / 384, 2 heads) at B = 1, F = 129, T = 251 under no_grad: the module on a HIP tensor is
    silent (native path), differs bit-wise from and agrees to rel_l2 < 1e-4 (fp32) with the same module under NBSS_NBC2_NATIVE=0.  bf16: the distance of
    the torch.nn modules run in bf16 (NBSS_NBC2_NATIVE=0) from the fp32 torch.nn output on the same input is measured here, the native bf16 output gets
    1.5 x that (the precedent of tests/test_bf16_vs_reference.py).  Measured on the MI355X: fp32 native vs torch.nn 5.9e-07; bf16 torch.nn 7.95e-03,
    native 7.71e-03."""
    import copy
    torch.manual_seed(21)
    net = _large().cuda().eval()
    x = torch.randn(1, 129, 251, 12).bfloat16().float().cuda()  # (values both precisions hold exactly: the same input everywhere)
    with torch.no_grad():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y = net(x)
            yb = net(x.bfloat16())
        monkeypatch.setenv("NBSS_NBC2_NATIVE", "0")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            y_nn = net(x)
            yb_nn = copy.deepcopy(net).bfloat16()(x.bfloat16())
        monkeypatch.delenv("NBSS_NBC2_NATIVE")
    assert y.shape == (1, 129, 251, 4) and y.dtype == torch.float32 and yb.dtype == torch.bfloat16
    assert not torch.equal(y, y_nn)
    e = rel_l2(y, y_nn)
    e_nn, e_nat = rel_l2(yb_nn, y_nn), rel_l2(yb, y_nn)
    print(f"nbc2-large 1x129x251: fp32 native vs torch.nn {e:.3e}; bf16 vs fp32 torch.nn: torch.nn {e_nn:.3e}  native {e_nat:.3e}")
    assert e < 1e-4
    assert e_nat <= 1.5 * e_nn, (e_nat, e_nn)


@pytest.mark.gpu
def test_nbc2_large_trains_natively_on_the_device(hip_lib):
    """training mode at the large widths (2 layers, 192 / 384, 2 heads) on 1 x 129 x 64: the output's grad_fn is the native autograd.Function, every
    parameter gets a finite gradient, and the gradients agree with fp64 autograd through the torch.nn module on the host within 2e-4 (fp32: the bar of
    tests/test_nbc2_native.py)."""
    torch.manual_seed(22)
    net = _large(n_layers=2)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(1, 129, 251, 12)[:, :, :64].contiguous()
    r = torch.randn(1, 129, 64, 4)
    ref = _large(n_layers=2).double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    y64 = ref(x.double())
    (y64 * r.double()).sum().backward()
    net = net.cuda().train()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y = net(x.cuda())
    assert type(y.grad_fn).__name__ == "_NBC2TrainFnBackward"
    (y * r.cuda()).sum().backward()
    assert rel_l2(y.detach(), y64.detach()) < 1e-4
    bad = {}
    for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        e = rel_l2(p.grad, q.grad)
        if e > 2e-4:
            bad[n] = e
    assert not bad, bad
