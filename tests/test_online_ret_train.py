"""nbss_online_ret_train_fwd / _bwd (csrc/online_ret_train.hip) through the C ABI against fp64 torch autograd of the repository's own
MultiScaleRetention: chunk_recurrent_forward -> group_norm -> SiLU(g) * (whose forward the online_* golden fixtures pin to the reference), loss = sum(out r).

Shapes are the kernel's edges: chunks of 64 frames (CHUNK) — T = 1, 2, 3 (one frame, a partial first chunk), 63 / 64 / 65 (one frame below, exactly one chunk,
one frame into the second), 127 / 128 / 130 (the state carried once and twice, a ragged last chunk), 257 (no whole-sequence cap).  BF in {1, 3, 10}.  Both key
forms (k with k_scale = 24^-0.5, and k = NULL: 'share_qk'), the shipped decays [4, 5, 9, 10] and decay = False (gamma = 1), and three input levels: at
0.05 every clamped absolute score sum sits on its clamp and the RMSNorm's eps weighs in, at 4 none does, at 1 both occur.

Bars: fp32 — the project's per-block bars against fp64, forward <= 2e-5, gradients <= 1e-4 rel-L2.  For dq and dk the denominator is
max(|ref|, |dv_ref| |v| / |q|): at T = 1, and at frame 0 of every sequence, the true q / k gradient is a cancellation that survives only through the eps
of the RMSNorm (torch's own fp32 evaluation shows 0.07 - 0.24 plain relative error on dq at T = 1), so a plain relative error measures nothing there.
bf16 — inputs and cotangent rounded to bf16 for both sides; tensor by tensor at most 1.5 x what torch's own bf16-autocast evaluation of the same function
loses against fp64 on the CPU, with the 5e-3 floor (the convention of tests/test_bf16_vs_reference.py and tests/test_online_tconvffn_train.py)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32
from util import rel_l2

CHUNK = 64
GRID_CAP = 4096  # workgroups of a launch (csrc/online_ret_train.hip: RT_GRID_CAP), one per (sequence, head)
FWD_TOL, GRAD_TOL = 2e-5, 1e-4
BF16_FACTOR, BF16_FLOOR = 1.5, 5e-3
EINVAL, EUNSUPPORTED = -1, -2
K_SCALE = 24 ** -0.5
BFS = (1, 3, 10)
TS = (1, 2, 3, 63, 64, 65, 127, 128, 130, 257)
LEVELS = (0.05, 1.0, 4.0)
DECAYS = {"shipped": [1 - 2.0 ** -d for d in (4, 5, 9, 10)], "none": [1.0] * 4}


def _module(share):
    from models.arch.base.retention import MultiScaleRetention
    return MultiScaleRetention(embed_dim=96, num_heads=4, value_factor=2, share_qk=share)


def _function(q, k, v, g, gamma):
    """the module's own methods between the projections and out_proj; k None: shared with q"""
    m = _module(k is None)
    BF, T, _ = q.shape
    qr = q.view(BF, T, 4, 24).transpose(1, 2)
    kr = qr if k is None else (k * m.scaling).view(BF, T, 4, 24).transpose(1, 2)
    o = m.chunk_recurrent_forward(qr, kr, v, ("chunk", CHUNK, gamma.to(v.dtype)))
    return F.silu(g) * m.group_norm(o).reshape(BF, T, 192)


def _autograd(q, k, v, g, r, gamma, dtype, autocast=False):
    """(out, dq, dk, dv, dg) in `dtype` on the CPU, as fp64 tensors"""
    leaves = [None if t is None else t.to(dtype).clone().requires_grad_(True) for t in (q, k, v, g)]
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = _function(*leaves, gamma)
    (out.double() * r.double()).sum().backward()
    return (out.detach().double(), *(None if t is None else t.grad.double() for t in leaves))


@functools.lru_cache(maxsize=None)
def _case(BF, T, share, decay, level, bf16=False):
    """inputs and the fp64 reference of one case: computed once, shared by every test (and backend) that uses it, never modified.  BF = 10 is five
    frequencies for each of two batch items (the second item at another level, so rows leaking between sequences would show)."""
    gen = torch.Generator().manual_seed(1000 * T + 10 * BF + share)
    item = 1 + 0.5 * (torch.arange(BF) >= 5).view(BF, 1, 1)
    q = level * item * torch.randn(BF, T, 96, generator=gen)
    k = None if share else level * item * torch.randn(BF, T, 96, generator=gen)
    v, g, r = (torch.randn(BF, T, 192, generator=gen) for _ in range(3))
    if k is not None:
        # Frame 0 sees one key, so o_0 = s v_0 / ab_0 with the single score s = q_0 . k'_0, and the RMSNorm leaves of d out / d s only what its eps lets
        # through: a factor eps / (s^2 + eps)^1.5, up to 1 / sqrt(eps) = 1e3 for |s| <~ 1e-2.  When s is also a cancelling dot product, |s| << |q_0| |k'_0|,
        # that factor multiplies the rounding of the dot product itself (relative 6e-8 |q_0| |k'_0| / |s|) and the one row outweighs the whole tensor: with
        # such a draw (BF 3, T 64, level 4: cosine 1e-5) torch's own fp32 evaluation is 2.3e-4 off the fp64 dq and dk, any fp32 evaluation is.  The bars
        # are about the kernel, not about the conditioning of a draw: a frame-0 pair whose cosine is below 0.02 gets 0.2 of its key's direction added to
        # the query (every level, sequence and head alike; 'share_qk' has s = |q_0|^2 and no cancellation).
        q0, k0 = q[:, 0].view(BF, 4, 24), k[:, 0].view(BF, 4, 24)
        ratio = q0.norm(dim=-1, keepdim=True) / k0.norm(dim=-1, keepdim=True)
        flat = ((q0 * k0).sum(-1, keepdim=True) / (q0.norm(dim=-1, keepdim=True) * k0.norm(dim=-1, keepdim=True))).abs() < 0.02
        q0 += flat * 0.2 * ratio * k0
    if bf16:  # the reference sees the rounded inputs and cotangent, as the stream does
        q, k, v, g, r = (None if t is None else t.bfloat16().float() for t in (q, k, v, g, r))
    gamma = torch.tensor(DECAYS[decay], dtype=torch.float32)
    return (q, k, v, g, r, gamma), _autograd(q, k, v, g, r, gamma.double(), torch.float64)


def _run(backend, inputs, dtype=torch.float32, keep=True, bwd=True):
    """-> (out, dq, dk, dv, dg) through the two entry points (ws and save start as NaN bytes: tests/conftest.py)"""
    q, k, v, g, r, gamma = (None if t is None else t.to(backend.device) for t in inputs)
    q, k, v, g, r = (None if t is None else t.to(dtype) for t in (q, k, v, g, r))
    out, save = ops.online_ret_train_fwd(backend.lib, q, k, v, g, K_SCALE, gamma, keep=keep)
    if not bwd:
        return (out.cpu(),)
    return tuple(None if t is None else t.cpu() for t in (out, *ops.online_ret_train_bwd(backend.lib, q, k, v, g, K_SCALE, gamma, save, r)))


def _errors(got, want, inputs):
    """rel-L2 per tensor; dq / dk over max(|ref|, |dv_ref| |v| / |q|)"""
    q, _, v = inputs[:3]
    floor = float(want[3].norm() * v.double().norm() / q.double().norm())
    errs = {}
    for name, a, b in zip(("out", "dq", "dk", "dv", "dg"), got, want):
        if b is None:
            assert a is None, name
            continue
        if name in ("dq", "dk"):
            errs[name] = float((a.double() - b).norm() / max(float(b.norm()), floor))
        else:
            errs[name] = rel_l2(a, b)
        assert torch.isfinite(a).all(), name
    return errs


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("decay", list(DECAYS))
@pytest.mark.parametrize("share", [False, True], ids=["k", "share_qk"])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("BF", BFS)
def test_fp32_against_fp64_autograd(backend, BF, T, share, decay, level):
    inputs, want = _case(BF, T, share, decay, level)
    errs = _errors(_run(backend, inputs), want, inputs)
    print(f"BF {BF} T {T} share {share} decay {decay} level {level}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert errs["out"] <= FWD_TOL, errs
    assert all(v <= GRAD_TOL for k, v in errs.items() if k != "out"), errs


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("share", [False, True], ids=["k", "share_qk"])
@pytest.mark.parametrize("T", [3, CHUNK + 1, 2 * CHUNK + 2])
def test_bf16_against_torch_autocast(backend, T, share, level):
    inputs, want = _case(3, T, share, "shipped", level, True)
    auto = _autograd(*inputs[:5], inputs[5], torch.float32, autocast=True)
    lost = _errors(auto, want, inputs)
    errs = _errors(_run(backend, inputs, torch.bfloat16), want, inputs)
    for k in errs:
        print(f"T {T} share {share} level {level} {k}: kernel {errs[k]:.3e}  torch bf16 autocast {lost[k]:.3e}")
    worse = {k: (errs[k], lost[k]) for k in errs if errs[k] > max(BF16_FACTOR * lost[k], BF16_FLOOR)}
    assert not worse, worse


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("share", [False, True], ids=["k", "share_qk"])
def test_bitwise_repeatable(backend, dtype, share):
    inputs, _ = _case(3, 2 * CHUNK + 2, share, "shipped", 1.0)
    a, b = _run(backend, inputs, dtype), _run(backend, inputs, dtype)
    assert all(x is None and y is None or torch.equal(x, y) for x, y in zip(a, b))


def test_batch_invariant(backend):
    """sequence 0 of a BF = 10 launch has the bits of the BF = 1 launch of that sequence"""
    inputs, _ = _case(10, CHUNK + 1, False, "shipped", 1.0)
    one = tuple(t if t.dim() == 1 else t[:1].contiguous() for t in inputs)
    ten, alone = _run(backend, inputs), _run(backend, one)
    assert all(torch.equal(x[:1], y) for x, y in zip(ten, alone))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inference_forward_keeps_nothing_and_is_the_same(backend, dtype):
    inputs, _ = _case(3, 2 * CHUNK + 2, True, "shipped", 1.0)
    assert torch.equal(_run(backend, inputs, dtype, keep=False, bwd=False)[0], _run(backend, inputs, dtype, keep=True, bwd=False)[0])


def test_more_sequences_than_one_grid_pass(backend):
    """the grid is capped at GRID_CAP workgroups, one per (sequence, head): BF just above GRID_CAP / 4 makes the first workgroup walk a second pair"""
    BF = GRID_CAP // 4 + 1
    inputs, want = _case(BF, 2, False, "shipped", 1.0)
    errs = _errors(_run(backend, inputs), want, inputs)
    print(errs)
    assert errs["out"] <= FWD_TOL and all(v <= GRAD_TOL for k, v in errs.items() if k != "out"), errs


def test_refusals(backend):
    lib = backend.lib
    buf = torch.zeros(1 << 20, device=backend.device)
    p = ops._ptr(lib, buf)
    st = ops._stream(lib, buf)
    o = p + 4 * 65536
    ins = dict(q=p, k=p + 4096, v=p + 8192, g=p + 16384)

    def fwd(T=4, dt=NBSS_F32, BF=1, out=o, save=None, ws=p, decay=p, **kw):
        a = {**ins, **kw}
        return lib.nbss_online_ret_train_fwd(dt, BF, T, a["q"], a["k"], a["v"], a["g"], K_SCALE, decay, out, save, ws, st)

    def bwd(T=4, dt=NBSS_F32, BF=1, save=p, d_out=p, dq=o, dk=o + 4096, dv=o + 8192, dg=o + 16384, ws=p, decay=p, **kw):
        a = {**ins, **kw}
        return lib.nbss_online_ret_train_bwd(dt, BF, T, a["q"], a["k"], a["v"], a["g"], K_SCALE, decay, save, d_out, dq, dk, dv, dg, ws, st)

    for T in (0, 4097):
        assert fwd(T=T) == EUNSUPPORTED and bwd(T=T) == EUNSUPPORTED, T
        assert lib.nbss_online_ret_train_save_bytes(NBSS_F32, 1, T) == EUNSUPPORTED and lib.nbss_online_ret_train_ws_bytes(NBSS_F32, 1, T) == EUNSUPPORTED
    assert fwd(BF=(1 << 28) // 4 + 1) == EUNSUPPORTED and lib.nbss_online_ret_train_save_bytes(NBSS_F32, (1 << 28) // 4 + 1, 4) == EUNSUPPORTED
    assert fwd(dt=2) == EINVAL and bwd(dt=2) == EINVAL and fwd(BF=0) == EINVAL and bwd(BF=0) == EINVAL
    assert lib.nbss_online_ret_train_save_bytes(7, 1, 4) == EINVAL and lib.nbss_online_ret_train_ws_bytes(7, 1, 4) == EINVAL
    assert lib.nbss_online_ret_train_save_bytes(NBSS_F32, 0, 4) == EINVAL
    for name in ("q", "v", "g", "out", "ws", "decay"):
        assert fwd(**{name: None}) == EINVAL, name
    for name in ("q", "v", "g", "save", "d_out", "dq", "dv", "dg", "ws", "decay"):
        assert bwd(**{name: None}) == EINVAL, name
    assert bwd(k=None) == EINVAL and bwd(dk=None) == EINVAL  # dk without k, k without dk
    for name in ("q", "k", "v", "g"):
        assert fwd(out=ins[name]) == EINVAL, name
    assert not buf.any()  # nothing ran: the output buffers are untouched
    assert lib.nbss_online_ret_train_save_bytes(NBSS_BF16, 3, 65) >= 3 * 4 * 2 * 24 * 48 * 4 and lib.nbss_online_ret_train_ws_bytes(NBSS_BF16, 3, 65) > 0
