"""nbss_online_tsa_train_fwd / _bwd (csrc/online_tsa_train.hip) through the C ABI: y = x + out_proj(SiLU(g) * RMSNorm_head(chunk_retention(q, k, v))) on
u = LayerNorm(x), forward and backward, against fp64 torch autograd of the repository's own LayerNorm + MultiScaleRetention + residual (whose forward the
online_* golden fixtures pin to the reference), loss = sum(y r).  y, dx and all seven parameter gradients are checked.

Shapes: BF = 3 with T in {1, 63, 64, 65, 130} — the chunk edges of the core; 3 x 65 = 195 and 3 x 130 = 390 tokens are no whole 128-row tile of the two
projection kernels, 3 x 1 is a tile with three live rows — and one case with BF = 1.  Both key forms, fp32 and bf16.  The projection kernels do not cap their
grid (one workgroup per 128 rows), so there is no case above a cap.

Bars: fp32 — the project's per-block bars against fp64, forward <= 2e-5, gradients <= 1e-4 rel-L2.  bf16 — x and the cotangent rounded to bf16 for both
sides; tensor by tensor at most 1.5 x what the PARENT's path — the bf16-autocast module with NBSS_ONLINE_NATIVE_RET=1, i.e. torch's LayerNorm and GEMMs around
the native core, through the same library — loses against fp64 on the same inputs (the margin of tests/test_bf16_vs_reference.py: two correct bf16
evaluations differ in rounding order).  One thing is made like for like: the node's y and dx ARE bf16 tensors — the stream between the native blocks is
bf16, as for the T-ConvFFN and cross-band nodes — while the autocast module adds its bf16 block output to an fp32 x (1.5e-4 / 3e-4 against fp64); no bf16
tensor can hold y closer than its own rounding, 1.7e-3 rel-L2.  The parent's y and dx are therefore rounded to bf16, as the next native block of the
parent's fastest setting rounds them on entry, before their error is taken; the seven parameter gradients are compared as they come.
Measured pairs (new node / parent's path; emulator, BF 3, T 65, not_share_qk; every case prints its own):
    y 1.664e-3 / 1.663e-3   dx 1.723e-3 / 1.725e-3   ln.weight 9.10e-3 / 9.15e-3   ln.bias 7.47e-3 / 7.67e-3   q_proj 8.08e-3 / 8.28e-3
    k_proj 8.11e-3 / 8.25e-3   v_proj 6.39e-3 / 6.61e-3   g_proj 6.16e-3 / 6.37e-3   out_proj 6.06e-3 / 6.29e-3
(the parent rounds q, k, v, g and their gradients to bf16 on the way through torch's GEMMs, and so does the node: the same places, hence the same sizes)."""
import copy
import functools

import pytest
import torch

from nbss_amd import online_train, ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32
from util import rel_l2

FWD_TOL, GRAD_TOL = 2e-5, 1e-4
BF16_FACTOR = 1.5
EINVAL, EUNSUPPORTED = -1, -2
T_MAX = 4096
TS = (1, 63, 64, 65, 130)
NAMES = ("ln.weight", "ln.bias", "q_proj", "k_proj", "v_proj", "g_proj", "out_proj")
DECAYS = [1 - 2.0 ** -d for d in (4, 5, 9, 10)]
KEYS = pytest.mark.parametrize("share", [False, True], ids=["not_share_qk", "share_qk"])


class _Block(torch.nn.Module):
    """norm_mhsa + mhsa of a SpatialNetLayer with attention 'ret(2,*)' at the kernels' geometry, plus the residual of its caller"""

    def __init__(self, share):
        super().__init__()
        from models.arch.base.retention import MultiScaleRetention
        self.norm_mhsa = torch.nn.LayerNorm(96, eps=1e-5)
        self.mhsa = MultiScaleRetention(embed_dim=96, num_heads=4, value_factor=2, share_qk=share)
        self.dropout_mhsa = torch.nn.Dropout(0.0)

    def params(self):
        m = self.mhsa
        return [self.norm_mhsa.weight, self.norm_mhsa.bias, m.q_proj.weight, None if m.k_proj is None else m.k_proj.weight, m.v_proj.weight, m.g_proj.weight,
                m.out_proj.weight]

    def rel_pos(self, dtype=torch.float32):
        return (None, None), ("chunk", 64, torch.tensor(DECAYS, dtype=dtype))

    def forward(self, x, native_core=False):
        u = self.norm_mhsa(x)
        if native_core:  # the parent's path: the module's LayerNorm and nn.Linear's around the native core
            return x + online_train.retention_forward(self.mhsa, u, self.rel_pos())
        return x + self.mhsa(u, rel_pos=self.rel_pos(x.dtype), chunkwise_recurrent=True, rope=False)


def _grads(block):
    return [None if p is None else p.grad.detach().double() for p in block.params()]


@functools.lru_cache(maxsize=None)
def _case(BF, T, share, bf16=False):
    """the block, x, r and the fp64 reference (y, dx, the seven gradients) of one case: computed once, shared, never modified"""
    torch.manual_seed(100 * T + 10 * BF + share)
    block = _Block(share)
    with torch.no_grad():
        block.norm_mhsa.weight.add_(0.2 * torch.randn(96))
        block.norm_mhsa.bias.add_(0.2 * torch.randn(96))
        # q_proj and k_proj four times their initial size: scores on both sides of the clamp of the absolute row sums.  At T = 1 a fifth of it instead: a
        # sequence's frame 0 sees one key, o_0 = s v_0 with the single score s, and the RMSNorm leaves of d out / d s only what its eps lets through — a
        # factor eps / (mean(o_0^2) + eps), the rest cancels — so every fp32 evaluation of d q_proj and d k_proj has its rounding amplified by the inverse of
        # that factor (tests/test_online_ret_train.py: torch's own fp32 is 0.07 - 0.24 off on dq at T = 1), and with T = 1 there is no other frame for the
        # gradient to come from.  With shared keys s = |q_0|^2 ~ 0.8 at the initial size and the factor is ~1e-4; at a fifth, s ~ 0.03 and the factor ~0.05.
        for lin in (block.mhsa.q_proj, block.mhsa.k_proj):
            if lin is not None:
                lin.weight.mul_(4.0 if T > 1 else 0.2)
    x = torch.randn(BF, T, 96) * (1 + 0.5 * torch.arange(BF).view(BF, 1, 1)) + 0.3
    r = torch.randn(BF, T, 96)
    if bf16:  # the reference sees the rounded input and cotangent, as the stream does
        x, r = x.bfloat16().float(), r.bfloat16().float()
    b64 = copy.deepcopy(block).double()
    x64 = x.double().requires_grad_(True)
    y = b64(x64)
    (y * r.double()).sum().backward()
    return block, x, r, (y.detach(), x64.grad, *_grads(b64))


def _kparams(block, device):
    gamma = torch.tensor(DECAYS, dtype=torch.float32)
    return [None if p is None else p.detach().float().contiguous().to(device) for p in block.params() + [gamma]]


def _run(backend, block, x, r, dtype=torch.float32, keep=True, bwd=True, nan_grads=False, want_save=False):
    """-> (y, dx, *the seven gradients) through the two entry points (ws and save start as NaN bytes: tests/conftest.py)"""
    params = _kparams(block, backend.device)
    xs, rs = x.to(backend.device, dtype), r.to(backend.device, dtype)
    y, save = ops.online_tsa_train_fwd(backend.lib, params, xs, keep=keep)
    if not bwd:
        return (y.cpu(), save) if want_save else (y.cpu(),)
    grads = None
    if nan_grads:
        grads = [None if p is None else torch.full_like(p, float("nan")) for p in params[:7]] + [None]
    dx, grads = ops.online_tsa_train_bwd(backend.lib, params, xs, save, rs, grads)
    return tuple(None if t is None else t.cpu() for t in (y, dx, *grads[:7]))


def _errors(got, want):
    errs = {}
    for name, a, b in zip(("y", "dx") + NAMES, got, want):
        if b is None:
            assert a is None, name
            continue
        assert torch.isfinite(a).all(), name
        errs[name] = rel_l2(a, b)
    return errs


@KEYS
@pytest.mark.parametrize("BF,T", [(3, T) for T in TS] + [(1, 65)])
def test_fp32_against_fp64_autograd(backend, BF, T, share):
    block, x, r, want = _case(BF, T, share)
    errs = _errors(_run(backend, block, x, r), want)
    print(f"BF {BF} T {T} share {share}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert errs["y"] <= FWD_TOL, errs
    assert all(v <= GRAD_TOL for k, v in errs.items() if k != "y"), errs


def _parent_bf16(backend, block, x, r):
    """the parent's path on the same library: bf16 autocast of LayerNorm and the nn.Linear's, NBSS_ONLINE_NATIVE_RET's core between them"""
    b = copy.deepcopy(block).to(backend.device)
    xs = x.to(backend.device).requires_grad_(True)
    with online_train.use_lib(backend.lib), torch.autocast(backend.device.type, dtype=torch.bfloat16):
        y = b(xs, native_core=True)
    (y.float() * r.to(backend.device)).sum().backward()
    # y and dx as the bf16 stream carries them (the module docstring: why)
    return (y.detach().bfloat16().cpu(), xs.grad.bfloat16().cpu(), *(None if g is None else g.cpu() for g in _grads(b)))


@KEYS
@pytest.mark.parametrize("BF,T", [(3, T) for T in TS] + [(1, 65)])
def test_bf16_against_the_parents_path(backend, BF, T, share):
    block, x, r, want = _case(BF, T, share, True)
    lost = _errors(_parent_bf16(backend, block, x, r), want)
    errs = _errors(_run(backend, block, x, r, torch.bfloat16), want)
    for k in errs:
        print(f"BF {BF} T {T} share {share} {k}: node {errs[k]:.3e}  parent's path {lost[k]:.3e}")
    worse = {k: (errs[k], lost[k]) for k in errs if errs[k] > BF16_FACTOR * lost[k]}
    assert not worse, worse


# ---- consistency with the existing entry points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@KEYS
def test_saved_projections_reproduce_the_core_and_out_proj(backend, dtype, share):
    """q, k, v, g of `save` through nbss_online_ret_train_fwd give the saved core output bit for bit; nbss_nb_conv_t on it, with x as residual, gives y"""
    block, x, r, _ = _case(3, 65, share)
    y, save = _run(backend, block, x, r, dtype, bwd=False, want_save=True)
    xs = x.to(backend.device, dtype)
    v = ops.online_tsa_save_views(backend.lib, save, xs, share)
    gamma = torch.tensor(DECAYS, dtype=torch.float32, device=backend.device)
    out, _ = ops.online_ret_train_fwd(backend.lib, v["q"].clone(), None if share else v["k"].clone(), v["v"].clone(), v["g"].clone(), 24 ** -0.5, gamma,
                                      keep=False)
    assert torch.equal(out, v["go"])
    wo = _kparams(block, backend.device)[6]
    lib, y2 = backend.lib, torch.empty_like(xs)
    ws = ops.scratch(lib.nbss_nb_ws_bytes(96, 192, 1, 1), backend.device)
    lib.call("nbss_nb_conv_t", NBSS_BF16 if dtype == torch.bfloat16 else NBSS_F32, 3, 65, 192, 192, 96, 1, 1, ops._ptr(lib, out), ops._ptr(lib, wo), None,
             ops._ptr(lib, y2), ops._ptr(lib, xs), 0, 0, ops._ptr(lib, ws), ops._stream(lib, xs))
    assert torch.equal(y2.cpu(), y)
    mean = x.to(dtype).double().mean(-1)
    assert rel_l2(v["stats"][..., 0].cpu(), mean) <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_batch_invariant(backend, dtype):
    """every sequence alone has the bits of its rows (y and dx) in the three-sequence launch"""
    block, x, r, _ = _case(3, 65, False)
    three = _run(backend, block, x, r, dtype)
    for n in range(3):
        alone = _run(backend, block, x[n:n + 1].contiguous(), r[n:n + 1].contiguous(), dtype)
        assert torch.equal(three[0][n:n + 1], alone[0]) and torch.equal(three[1][n:n + 1], alone[1]), n


# ---- the contract --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@KEYS
def test_bitwise_repeatable_and_gradients_written(backend, dtype, share):
    """two calls give the same bits, forward and backward; the second starts from gradient buffers full of NaN"""
    block, x, r, _ = _case(3, 130, share)
    a, b = _run(backend, block, x, r, dtype), _run(backend, block, x, r, dtype, nan_grads=True)
    assert all(p is None and q is None or (torch.isfinite(q).all() and torch.equal(p, q)) for p, q in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_forward_only_keeps_nothing_and_is_the_same(backend, dtype):
    block, x, r, _ = _case(3, 130, True)
    assert torch.equal(_run(backend, block, x, r, dtype, keep=False, bwd=False)[0], _run(backend, block, x, r, dtype, keep=True, bwd=False)[0])


def test_4d_input_is_the_flattened_one(backend):
    block, x, r, _ = _case(3, 65, False)
    params = _kparams(block, backend.device)
    y3 = ops.online_tsa_train_fwd(backend.lib, params, x.to(backend.device), keep=False)[0]
    y4 = ops.online_tsa_train_fwd(backend.lib, params, x.to(backend.device).view(1, 3, 65, 96), keep=False)[0]
    assert y4.shape == (1, 3, 65, 96) and torch.equal(y4.view(3, 65, 96), y3)


def test_refusals(backend):
    lib = backend.lib
    buf = torch.zeros(1 << 20, device=backend.device)
    p = ops._ptr(lib, buf)
    st = ops._stream(lib, buf)
    o = p + 4 * 65536
    ins = dict(ln_w=p, ln_b=p + 512, wq=p + 4096, wk=p + 65536, wv=p + 2 * 65536, wg=p + 3 * 65536, wo=p + 4 * 65536, decay=p + 1024)
    order = ("ln_w", "ln_b", "wq", "wk", "wv", "wg", "wo", "decay")
    gnames = ("d_ln_w", "d_ln_b", "d_wq", "d_wk", "d_wv", "d_wg", "d_wo")

    def fwd(T=4, dt=NBSS_F32, BF=1, x=p, y=o, save=None, ws=p, **kw):
        a = {**ins, **kw}
        return lib.nbss_online_tsa_train_fwd(dt, BF, T, *(a[n] for n in order), x, y, save, ws, st)

    def bwd(T=4, dt=NBSS_F32, BF=1, x=p, save=p, dy=p + 2048, dx=o, ws=p, **kw):
        a = {**ins, **{n: o + 4096 * (i + 1) for i, n in enumerate(gnames)}, **kw}
        return lib.nbss_online_tsa_train_bwd(dt, BF, T, *(a[n] for n in order), x, save, dy, dx, *(a[n] for n in gnames), ws, st)

    for T in (0, T_MAX + 1):
        assert fwd(T=T) == EUNSUPPORTED and bwd(T=T) == EUNSUPPORTED, T
        assert lib.nbss_online_tsa_save_bytes(NBSS_F32, 1, T, 0) == EUNSUPPORTED and lib.nbss_online_tsa_ws_bytes(NBSS_F32, 1, T, 0) == EUNSUPPORTED
    assert fwd(BF=(1 << 28) // 4 + 1) == EUNSUPPORTED and lib.nbss_online_tsa_save_bytes(NBSS_F32, (1 << 28) // 4 + 1, 4, 0) == EUNSUPPORTED
    assert fwd(dt=2) == EINVAL and bwd(dt=2) == EINVAL and fwd(BF=0) == EINVAL and bwd(BF=0) == EINVAL
    assert lib.nbss_online_tsa_save_bytes(7, 1, 4, 0) == EINVAL and lib.nbss_online_tsa_ws_bytes(7, 1, 4, 0) == EINVAL
    for name in ("ln_w", "ln_b", "wq", "wv", "wg", "wo", "decay", "x", "y", "ws"):
        assert fwd(**{name: None}) == EINVAL, name
    for name in ("ln_w", "ln_b", "wq", "wv", "wg", "wo", "decay", "x", "save", "dy", "dx", "ws", "d_ln_w", "d_ln_b", "d_wq", "d_wv", "d_wg", "d_wo"):
        assert bwd(**{name: None}) == EINVAL, name
    assert bwd(wk=None) == EINVAL and bwd(d_wk=None) == EINVAL  # d_wk without wk, wk without d_wk
    assert fwd(y=p) == EINVAL and bwd(dx=p + 2048) == EINVAL and bwd(dx=p) == EINVAL  # y == x, dx == dy, dx == x
    assert not buf.any()  # nothing ran: the buffers are untouched
    k, s = lib.nbss_online_tsa_save_bytes(NBSS_BF16, 3, 65, 0), lib.nbss_online_tsa_save_bytes(NBSS_BF16, 3, 65, 1)
    assert k - s == (3 * 65 * 96 * 2 + 255) // 256 * 256 and s >= 3 * 65 * (480 + 192) * 2 + 3 * 65 * 8 + 3 * 4 * 2 * 24 * 48 * 4
    assert lib.nbss_online_tsa_ws_bytes(NBSS_BF16, 3, 65, 0) > 0


def test_ops_refuse_mismatched_tensors(backend):
    block, x, r, _ = _case(3, 65, True)
    params = _kparams(block, backend.device)
    xs = x.to(backend.device)
    y, save = ops.online_tsa_train_fwd(backend.lib, params, xs)
    with pytest.raises(ops.NbssError, match="grads must match"):  # wk = None with d_wk given
        ops.online_tsa_train_bwd(backend.lib, params, xs, save, xs, [torch.empty_like(params[2]) if i < 7 else None for i in range(8)])
    with pytest.raises(ops.NbssError, match="params must be"):
        ops.online_tsa_train_fwd(backend.lib, params[:7], xs)
    with pytest.raises(ops.NbssError, match="does not match"):
        ops.online_tsa_train_bwd(backend.lib, params, xs, save, xs[:, :1].contiguous())


@pytest.mark.gpu
def test_host_tensor_is_refused_by_the_device_library(hip_lib):
    """a CPU tensor handed to the gfx950 library is refused before any launch"""
    block, x, r, _ = _case(3, 65, False)
    with pytest.raises(ops.NbssError, match="HIP device"):
        ops.online_tsa_train_fwd(hip_lib, _kparams(block, torch.device("cpu")), x)
