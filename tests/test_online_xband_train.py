"""nbss_online_xband_train_fwd / _bwd (csrc/online_xband_train.hip) through the C ABI: the cross-band trio of an OnlineSpatialNet layer
(x + fconv1, + full-band, + fconv2) against fp64 torch autograd of the repository's own SpatialNetLayer._fconv / _full chain on the CPU, and bit
for bit against chaining the per-block entry points nbss_fconv_fwd / nbss_full_fwd / nbss_fconv_fwd (and their _bwd) on a one-layer SpatialNet
that holds the same parameters — the same launches run, so a difference there is a gather, pack or scatter bug.

Shapes (B, F, T): (1,1,1) the one-workgroup grid (where the full-band fold scratch once overlapped the partial tiles); (2,17,3) a single bin in the
second frequency tile and a half-empty last workgroup of the bf16 forward's two-frames-per-workgroup grid; (2,33,40) of tests/test_kernels_bwd.py; on
the device also (1,129,251), the model's own grid.

Bars: fp32 — the project's per-block bars against fp64: forward <= 2e-5, dx and the 18 gradients <= 1e-4 rel-L2.  bf16 (the reference sees the
bf16-rounded input and cotangent) — the bars of tests/test_kernels_bwd.py for these blocks: 5e-2 for the F-conv tensors (PReLU kink: bf16 rounding
flips the sign of ~1 % of the pre-activations), 3e-2 for the rest, dx included; forward 1.5e-2 (tests/util.py: Case.tol)."""
import copy
import ctypes as C
import functools

import pytest
import torch

from nbss_amd import online_train, ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32, make_cfg
from nbss_amd.params import _LAYER, param_table
from util import Case, rel_l2

FWD_TOL, GRAD_TOL = 2e-5, 1e-4
BF16_FWD_TOL, BF16_FCONV_TOL, BF16_TOL = 1.5e-2, 5e-2, 3e-2
EINVAL, EUNSUPPORTED = -1, -2
NAMES = [n for n, _ in _LAYER[:18]]  # fconv1.0.weight .. fconv2.2.weight: the order of the C ABI
SHAPES = [(1, 1, 1), (2, 17, 3), (2, 33, 40)]
DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16")]
GUARD = 4096


def shapes_for(backend):
    return SHAPES + ([(1, 129, 251)] if backend.name == "hip" else [])


def _layer(F, seed=0):
    from models.arch.OnlineSpatialNet import SpatialNetLayer
    torch.manual_seed(2000 + seed)
    layer = SpatialNetLayer(dim_hidden=96, dim_ffn=192, dim_squeeze=8, num_freqs=F, num_heads=4, attention="ret(2,share_qk)").eval()
    with torch.no_grad():  # non-trivial gamma, beta, biases and PReLU slopes
        for p in online_train.xband_params(layer):
            if p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))
    return layer


def _trio(layer, x):
    x = x + layer._fconv(layer.fconv1, x)
    x = x + layer._full(x)
    return x + layer._fconv(layer.fconv2, x)


def _autograd64(layer, x, r):
    """(y, dx, {name: grad}) of the module's own chain, loss = sum(y r), in fp64 on the CPU"""
    lay = copy.deepcopy(layer).double()
    xx = x.double().clone().requires_grad_(True)
    y = _trio(lay, xx)
    (y * r.double()).sum().backward()
    return y.detach(), xx.grad, {n: p.grad.reshape(p.shape) for n, p in zip(NAMES, online_train.xband_params(lay))}


KINK = 2e-6


def _clear_of_the_kink(layer, x, g):
    """fp32 cases only.  PReLU' jumps at 0, so a pre-activation that fp64 puts closer to 0 than fp32 can resolve takes either slope in a correct fp32
    kernel, and ONE such element moves the gradients of its frame by more than the 1e-4 bar (seen: a 4.6e-8 pre-activation among 253 440 at (2,33,40), dx
    2.8e-4, fconv1.0.bias 8.6e-4, confined to its frame and the five bins around it).  A pre-activation is a 60-term dot product of LayerNorm outputs of
    order 1 with weights of order 60^-1/2: its fp32 error stays below 60 x 0.13 x 2^-23 ~ 1e-6.  The frames whose fp64 pre-activations (of either F-conv)
    come closer to 0 than KINK = 2e-6 are drawn again; the three blocks work frame by frame, so the other frames are not touched.  Decided by the fp64
    reference alone.  The bf16 bars contain the kink (5e-2) and those cases keep their draw."""
    lay = copy.deepcopy(layer).double()
    pre = []
    hooks = [ml[2].register_forward_pre_hook(lambda m, a: pre.append(a[0])) for ml in (lay.fconv1, lay.fconv2)]
    B, F, T, H = x.shape
    for _ in range(20):
        pre.clear()
        with torch.no_grad():
            _trio(lay, x.double())
        near = sum((p.abs() < KINK).reshape(B, T, -1).any(-1) for p in pre) > 0  # [B][T]
        if not near.any():
            for h in hooks:
                h.remove()
            return x
        for b, t in near.nonzero().tolist():
            x[b, :, t] = torch.randn(F, H, generator=g)
    raise AssertionError("no draw clear of the PReLU kink")


@functools.lru_cache(maxsize=None)
def _case(B, F, T, bf16=False, grads=True):
    """layer, inputs and the fp64 reference of one shape: computed once, shared by every test (and backend) that uses the shape, never modified"""
    layer = _layer(F)
    g = torch.Generator().manual_seed(11 * T + F)
    x, r = torch.randn(B, F, T, 96, generator=g), 0.5 * torch.randn(B, F, T, 96, generator=g)
    if bf16:  # the reference sees the rounded input and cotangent, as the stream does
        x, r = x.bfloat16().float(), r.bfloat16().float()
    elif grads:
        x = _clear_of_the_kink(layer, x, g)
    if grads:
        return layer, x, r, _autograd64(layer, x, r)
    with torch.no_grad():
        return layer, x, r, (_trio(copy.deepcopy(layer).double(), x.double()), None, None)


def _params(backend, layer):
    return [p.to(backend.device) for p in online_train._xband_kernel_params(online_train.xband_params(layer))]


def _run(backend, layer, x, r, dtype=torch.float32):
    """-> y, dx, {name: grad} through the two entry points; scratch and save start as NaN bytes (tests/conftest.py) and so do the 18 gradient
    buffers: they are WRITTEN, so nothing of that survives"""
    p = _params(backend, layer)
    xs, rs = x.to(dtype).to(backend.device), r.to(dtype).to(backend.device)
    y, save = ops.online_xband_train_fwd(backend.lib, p, xs)
    grads = [torch.full_like(q, float("nan")) for q in p]
    dx, gr = ops.online_xband_train_bwd(backend.lib, p, xs, save, rs, grads)
    return y.cpu(), dx.cpu(), {n: g.cpu().reshape(q.shape) for n, g, q in zip(NAMES, gr, online_train.xband_params(layer))}


def _errors(got, want):
    (y, dx, g), (wy, wdx, wg) = got, want
    return {"y": rel_l2(y, wy), "dx": rel_l2(dx, wdx), **{n: rel_l2(g[n], wg[n]) for n in NAMES}}


def test_fp32_against_fp64_autograd(backend):
    for B, F, T in shapes_for(backend):
        layer, x, r, want = _case(B, F, T)
        errs = _errors(_run(backend, layer, x, r), want)
        print(f"{(B, F, T)}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert errs["y"] <= FWD_TOL, ((B, F, T), errs)
        assert all(v <= GRAD_TOL for k, v in errs.items() if k != "y"), ((B, F, T), errs)


def test_bf16_against_fp64_autograd(backend):
    for B, F, T in shapes_for(backend):
        layer, x, r, want = _case(B, F, T, True)
        errs = _errors(_run(backend, layer, x, r, torch.bfloat16), want)
        print(f"{(B, F, T)}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        bars = {k: BF16_FWD_TOL if k == "y" else BF16_FCONV_TOL if k.startswith("fconv") else BF16_TOL for k in errs}
        assert not {k: v for k, v in errs.items() if not v <= bars[k]}, ((B, F, T), errs)


def _chained(backend, layer, x, r, dtype):
    """the same computation through the per-block entry points on a one-layer SpatialNet (another C_in / C_out than the trio's internal configuration:
    the flat offsets differ, the launches do not) -> y, dx, {name: grad}"""
    B, F, T = x.shape[:3]
    cs = Case(backend, B, F, T, NBSS_BF16 if dtype == torch.bfloat16 else NBSS_F32)
    p = dict(cs.p)
    for n, t in zip(NAMES, online_train.xband_params(layer)):
        p["layers.0." + n] = t.detach()
    flat = ops.flatten_params(cs.lib, cs.cfg, p, backend.device)
    packed = ops.pack_params(cs.lib, cs.cfg, flat)
    xs, rs = x.to(dtype).to(backend.device), r.to(dtype).to(backend.device)
    x1 = ops.fconv_fwd(cs.lib, cs.cfg, flat, packed, 0, 0, xs)
    x2 = ops.full_fwd(cs.lib, cs.cfg, flat, packed, 0, x1)
    y = ops.fconv_fwd(cs.lib, cs.cfg, flat, packed, 0, 1, x2)
    G = torch.zeros_like(flat)
    ws = ops.workspace(cs.lib, cs.cfg, backend.device)
    g2 = ops.fconv_bwd(cs.lib, cs.cfg, flat, G, packed, 0, 1, x2, rs, ws)
    g1 = ops.full_bwd(cs.lib, cs.cfg, flat, G, packed, 0, x1, g2, ws)
    dx = ops.fconv_bwd(cs.lib, cs.cfg, flat, G, packed, 0, 0, xs, g1, ws)
    table, G = param_table(cs.lib, cs.cfg), G.cpu()
    grads = {}
    for n in NAMES:
        off, shape = table["layers.0." + n]
        numel = int(torch.Size(shape).numel())
        grads[n] = G[off:off + numel].reshape(shape)
    return y.cpu(), dx.cpu(), grads


@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_equal_to_the_chained_block_entry_points(backend, dtype):
    for B, F, T in shapes_for(backend):
        layer, x, r, _ = _case(B, F, T, dtype == torch.bfloat16)
        y, dx, g = _run(backend, layer, x, r, dtype)
        wy, wdx, wg = _chained(backend, layer, x, r, dtype)
        assert torch.equal(y, wy) and torch.equal(dx, wdx), (B, F, T)
        for n in NAMES:
            assert torch.equal(g[n].reshape(-1), wg[n].reshape(-1)), ((B, F, T), n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_are_written_and_calls_repeat_bitwise(backend, dtype):
    """the 18 gradient buffers start as NaN (`_run`), the shared workspace holds the previous call's data: two calls give the same, finite, bits"""
    layer, x, r, _ = _case(2, 17, 3, dtype == torch.bfloat16)
    a, b = _run(backend, layer, x, r, dtype), _run(backend, layer, x, r, dtype)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    for n in NAMES:
        assert torch.isfinite(a[2][n]).all(), n
        assert torch.equal(a[2][n], b[2][n]), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_without_save(backend, dtype):
    """save = NULL: the bits of the saving forward; and forward only beyond the training limit (T = 300) against fp64"""
    layer, x, r, _ = _case(2, 17, 3, dtype == torch.bfloat16)
    p = _params(backend, layer)
    xs = x.to(dtype).to(backend.device)
    y_keep, save = ops.online_xband_train_fwd(backend.lib, p, xs, keep=True)
    y, none = ops.online_xband_train_fwd(backend.lib, p, xs, keep=False)
    assert none is None and save is not None and torch.equal(y, y_keep)
    layer, x, _, (wy, _, _) = _case(1, 5, 300, dtype == torch.bfloat16, False)
    y = ops.online_xband_train_fwd(backend.lib, _params(backend, layer), x.to(dtype).to(backend.device), keep=False)[0]
    err = rel_l2(y.cpu(), wy)
    print(f"T = 300 forward: {err:.1e}")
    assert err <= (FWD_TOL if dtype == torch.float32 else BF16_FWD_TOL)


def _align(n):
    return (n + 255) & ~255


@pytest.mark.parametrize("dtype", DTYPES)
def test_size_functions_are_exact(backend, dtype):
    """save = the two block inputs; ws = flat parameters | packed fragments | two stream tensors | flat gradients | the backward kernels' workspace of the
    one-layer configuration; a guard band behind either buffer stays intact through a forward and a backward"""
    lib, dt = backend.lib, NBSS_BF16 if dtype == torch.bfloat16 else NBSS_F32
    for B, F, T in [(1, 1, 1), (2, 17, 3)]:
        sb = _align(B * F * T * 96 * (2 if dt == NBSS_BF16 else 4))
        save_bytes, ws_bytes = ops.online_xband_save_bytes(lib, dt, B, F, T), ops.online_xband_ws_bytes(lib, dt, B, F, T)
        assert save_bytes == 2 * sb
        cfg = make_cfg(B, F, T, 4, 2, L=1, dtype=dt)
        flat_bytes = _align(4 * lib.nbss_param_count(C.byref(cfg)))
        assert ws_bytes == 2 * flat_bytes + _align(lib.nbss_packed_bytes(C.byref(cfg))) + 2 * sb + lib.nbss_workspace_bytes(C.byref(cfg))
        # forward-only shapes carry neither the gradients nor the backward workspace
        cfg_long = make_cfg(B, F, 300, 4, 2, L=1, dtype=dt)
        assert ops.online_xband_ws_bytes(lib, dt, B, F, 300) == flat_bytes + _align(lib.nbss_packed_bytes(C.byref(cfg_long))) + 2 * _align(B * F * 300 * 96 * (2 if dt == NBSS_BF16 else 4))
        layer, x, r, _ = _case(B, F, T, dtype == torch.bfloat16)
        p = _params(backend, layer)
        xs, rs = x.to(dtype).to(backend.device), r.to(dtype).to(backend.device)
        save = torch.full((save_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=backend.device)
        ws = torch.full((ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=backend.device)
        y, dx, grads = torch.empty_like(xs), torch.empty_like(xs), [torch.empty_like(q) for q in p]
        st = ops._stream(lib, xs)
        ptr = lambda t: ops._ptr(lib, t)  # noqa: E731
        lib.call("nbss_online_xband_train_fwd", dt, B, F, T, *map(ptr, p), ptr(xs), ptr(y), ptr(save), ptr(ws), st)
        lib.call("nbss_online_xband_train_bwd", dt, B, F, T, *map(ptr, p), ptr(xs), ptr(save), ptr(rs), ptr(dx), *map(ptr, grads), ptr(ws), st)
        assert bool((save[save_bytes:] == 0xA5).all()) and bool((ws[ws_bytes:] == 0xA5).all()), (B, F, T)
        want = _run(backend, layer, x, r, dtype)
        assert torch.equal(y.cpu(), want[0]) and torch.equal(dx.cpu(), want[1])


def test_refusals(backend):
    """every refusal returns its code and launches nothing.  (The buffer is large enough for the workspace of the single-token shape the pointer
    refusals use, with every other operand behind it.)"""
    lib = backend.lib
    ws_bytes = ops.online_xband_ws_bytes(lib, NBSS_F32, 1, 1, 1)
    buf = torch.zeros(ws_bytes // 4 + (1 << 18), device=backend.device)
    ws = ops._ptr(lib, buf)
    o = ws + ws_bytes  # operands: 4 KB apart
    st = ops._stream(lib, buf)
    P, X, Y, SAVE, DY, DX, GR = [o] * 18, o + 4096, o + 8192, o + 12288, o + 16384, o + 20480, [o + 24576] * 18

    def fwd(dt=NBSS_F32, B=1, F=1, T=1, p=P, x=X, y=Y, save=None, w=ws):
        return lib.nbss_online_xband_train_fwd(dt, B, F, T, *p, x, y, save, w, st)

    def bwd(dt=NBSS_F32, B=1, F=1, T=1, p=P, x=X, save=SAVE, dy=DY, dx=DX, g=GR, w=ws):
        return lib.nbss_online_xband_train_bwd(dt, B, F, T, *p, x, save, dy, dx, *g, w, st)

    # a null pointer
    for i in range(18):
        assert fwd(p=P[:i] + [None] + P[i + 1:]) == EINVAL and bwd(p=P[:i] + [None] + P[i + 1:]) == EINVAL, i
        assert bwd(g=GR[:i] + [None] + GR[i + 1:]) == EINVAL, i
    assert fwd(x=None) == EINVAL and fwd(y=None) == EINVAL and fwd(w=None) == EINVAL
    assert bwd(x=None) == EINVAL and bwd(save=None) == EINVAL and bwd(dy=None) == EINVAL and bwd(dx=None) == EINVAL and bwd(w=None) == EINVAL
    # aliasing
    assert fwd(y=X) == EINVAL and bwd(dx=DY) == EINVAL
    # dtype, batch
    assert fwd(dt=2) == EINVAL and bwd(dt=2) == EINVAL and fwd(B=0) == EINVAL
    # F > 272, T > 4096: every call
    for kw in (dict(F=273), dict(T=4097)):
        assert fwd(**kw) == EUNSUPPORTED and fwd(save=SAVE, **kw) == EUNSUPPORTED and bwd(**kw) == EUNSUPPORTED, kw
        assert lib.nbss_online_xband_save_bytes(NBSS_F32, 1, kw.get("F", 1), kw.get("T", 1)) == EUNSUPPORTED
        assert lib.nbss_online_xband_ws_bytes(NBSS_F32, 1, kw.get("F", 1), kw.get("T", 1)) == EUNSUPPORTED
    # backward, or a forward that saves: T > 256, or fp32 with F > 160
    for kw in (dict(T=257), dict(F=161), dict(dt=NBSS_BF16, T=257)):
        assert fwd(save=SAVE, **kw) == EUNSUPPORTED and bwd(**kw) == EUNSUPPORTED, kw
        assert lib.nbss_online_xband_save_bytes(kw.get("dt", NBSS_F32), 1, kw.get("F", 1), kw.get("T", 1)) == EUNSUPPORTED
        assert lib.nbss_online_xband_ws_bytes(kw.get("dt", NBSS_F32), 1, kw.get("F", 1), kw.get("T", 1)) > 0  # (forward only: served)
    assert lib.nbss_online_xband_save_bytes(NBSS_BF16, 1, 161, 256) > 0  # bf16 trains up to F = 272
    assert lib.nbss_online_xband_save_bytes(7, 1, 1, 1) == EINVAL and lib.nbss_online_xband_ws_bytes(7, 1, 1, 1) == EINVAL
    assert not buf.any()  # nothing ran, nothing was written
