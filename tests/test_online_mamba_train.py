"""nbss_online_mamba_train_fwd / _bwd (csrc/online_mamba_train.hip) through the C ABI against fp64 torch autograd of the repository's own Mamba.core
(models/arch/base/mamba.py: everything between in_proj and out_proj), loss = sum(out r).

Shapes are the kernel's edges: runs of MAMBA_CKPT frames (c) — T = 1 .. 5 (the convolution's left edge, K - 1 = 3), c - 1 / c / c + 1 (one frame below, exactly
one run, one frame into the second), 2 c + 2 (the state and its gradient carried twice, a ragged last run), 257 (33 runs).  BF in {1, 3, 10}; BF = 10 is
five frequencies for each of two items at different levels.  Input levels 0.05, 1 and 4.  A_log and D are drawn at random so that every channel differs.
Three parameter sets: 'default' (the module's init otherwise), 'fast' (dt_proj.bias = 5: exp(dt A) underflows to 0 for the high states) and 'slow'
(dt_proj.bias = -9: dt ~ 1.2e-4, the decay is ~ 1 and the memory spans all 257 frames).

Bars: fp32 — the project's per-block bars against fp64, forward <= 2e-5, every gradient <= 1e-4 rel-L2; torch's own fp32 evaluation of the function loses
at most 1.2e-7 / 1.1e-6 of that with default-style parameters.  For the two extreme sets torch's fp32 evaluation is measured in the test, and where it
exceeds half a bar for a tensor, 2 x the measured value is that tensor's bar (measured on the CPU at BF 3, T in {2 c + 2, 257}, all three levels: 'fast'
at most 1.0e-7 forward and 3.5e-6 on a gradient (dt_proj.weight), 'slow' at most 9.1e-8 and 2.9e-6 (dt_proj.bias): neither reaches half a bar, so the
plain bars hold; the kernels on the host emulator: 1.4e-7 / 1.9e-6 and 1.4e-7 / 1.8e-6).  The true A_log gradient at T = 1
is exactly zero (h_{-1} = 0): bounded absolutely there, <= 1e-6 x the largest gradient norm.  bf16 — inputs and cotangent rounded to bf16 for both
sides; tensor by tensor at most 1.5 x what torch's own bf16-autocast evaluation of the same function loses against fp64 on the CPU, with the 5e-3 floor
(the convention of tests/test_online_ret_train.py)."""
import functools

import pytest
import torch

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32
from nbss_amd.online_train import MAMBA_CKPT, MAMBA_GRID_CAP
from util import rel_l2

C = MAMBA_CKPT
FWD_TOL, GRAD_TOL = 2e-5, 1e-4
BF16_FACTOR, BF16_FLOOR = 1.5, 5e-3
EINVAL, EUNSUPPORTED = -1, -2
BFS = (1, 3, 10)
TS = (1, 2, 3, 4, 5, C - 1, C, C + 1, 2 * C + 2, 257)
LEVELS = (0.05, 1.0, 4.0)
NAMES = ("out", "dxz", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "A_log", "D")


@functools.lru_cache(maxsize=None)
def _module(kind):
    """the fp32 module of a parameter set (never modified)"""
    from models.arch.base.mamba import Mamba
    torch.manual_seed({"default": 3, "fast": 4, "slow": 5}[kind])
    m = Mamba(d_model=96, d_state=16, d_conv=4, layer_idx=0)
    with torch.no_grad():
        m.A_log.add_(0.3 * torch.randn_like(m.A_log))
        m.D.add_(0.3 * torch.randn_like(m.D))
        if kind != "default":
            m.dt_proj.bias.fill_(5.0 if kind == "fast" else -9.0)
    return m


def _params(m):
    return [m.conv1d.weight, m.conv1d.bias, m.x_proj.weight, m.dt_proj.weight, m.dt_proj.bias, m.A_log, m.D]


def _autograd(kind, xz, r, dtype, autocast=False):
    """(out, dxz, the seven parameter gradients) of Mamba.core in `dtype` on the CPU, as fp64 tensors"""
    import copy
    m = copy.deepcopy(_module(kind)).to(dtype)
    x = xz.to(torch.bfloat16 if autocast else dtype).clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = m.core(x)
    (out.double() * r.double()).sum().backward()
    return (out.detach().double(), x.grad.double(), *(p.grad.double() for p in _params(m)))


@functools.lru_cache(maxsize=None)
def _case(BF, T, level, kind="default", bf16=False):
    """inputs and the fp64 reference of one case: computed once, shared by every test (and backend) that uses it, never modified"""
    gen = torch.Generator().manual_seed(1000 * T + 10 * BF)
    item = 1 + 0.5 * (torch.arange(BF) >= 5).view(BF, 1, 1)
    xz = level * item * torch.randn(BF, T, 384, generator=gen)
    r = torch.randn(BF, T, 192, generator=gen)
    if bf16:  # the reference sees the rounded inputs and cotangent, as the stream does
        xz, r = xz.bfloat16().float(), r.bfloat16().float()
    return (xz, r), _autograd(kind, xz, r, torch.float64)


def _run(backend, kind, inputs, dtype=torch.float32, keep=True, bwd=True):
    """-> (out, dxz, the seven gradients) through the two entry points (ws and save start as NaN bytes: tests/conftest.py)"""
    xz, r = (t.to(backend.device).to(dtype) for t in inputs)
    params = [p.detach().float().contiguous().to(backend.device) for p in _params(_module(kind))]
    out, save = ops.online_mamba_train_fwd(backend.lib, params, xz, keep=keep)
    assert (save is None) == (not keep)
    if not bwd:
        return (out.cpu(),)
    dxz, grads = ops.online_mamba_train_bwd(backend.lib, params, xz, save, r)
    return tuple(t.cpu() for t in (out, dxz, *grads))


def _errors(got, want, T):
    """rel-L2 per tensor; at T = 1 the A_log gradient (exactly zero) over the largest gradient norm"""
    errs = {}
    top = max(float(w.norm()) for w in want[2:])
    for name, a, b in zip(NAMES, got, want):
        assert torch.isfinite(a).all(), name
        if name == "A_log" and T == 1:
            assert float(b.abs().max()) == 0.0
            errs[name] = float(a.double().norm()) / top
        else:
            errs[name] = rel_l2(a, b.reshape(a.shape))
    return errs


def _bars(errs, lost=None, T=0):
    """the bar of each tensor: the project's, or 2 x torch's own fp32 loss where that exceeds half of it"""
    bars = {}
    for k in errs:
        bar = FWD_TOL if k == "out" else 1e-6 if (k == "A_log" and T == 1) else GRAD_TOL
        bars[k] = 2 * lost[k] if lost is not None and lost[k] > bar / 2 else bar
    return bars


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("BF", BFS)
def test_fp32_against_fp64_autograd(backend, BF, T, level):
    inputs, want = _case(BF, T, level)
    errs = _errors(_run(backend, "default", inputs), want, T)
    print(f"BF {BF} T {T} level {level}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    bars = _bars(errs, T=T)
    assert all(errs[k] <= bars[k] for k in errs), {k: (errs[k], bars[k]) for k in errs if errs[k] > bars[k]}


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("T", [2 * C + 2, 257])
@pytest.mark.parametrize("kind", ["fast", "slow"])
def test_fp32_extreme_parameters(backend, kind, T, level):
    inputs, want = _case(3, T, level, kind)
    lost = _errors(_autograd(kind, *inputs, torch.float32), want, T)
    errs = _errors(_run(backend, kind, inputs), want, T)
    for k in errs:
        print(f"{kind} T {T} level {level} {k}: kernel {errs[k]:.3e}  torch fp32 {lost[k]:.3e}")
    bars = _bars(errs, lost, T)
    assert all(errs[k] <= bars[k] for k in errs), {k: (errs[k], bars[k]) for k in errs if errs[k] > bars[k]}


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("T", [3, C + 1, 2 * C + 2])
def test_bf16_against_torch_autocast(backend, T, level):
    inputs, want = _case(3, T, level, "default", True)
    lost = _errors(_autograd("default", *inputs, torch.float32, autocast=True), want, T)
    errs = _errors(_run(backend, "default", inputs, torch.bfloat16), want, T)
    for k in errs:
        print(f"T {T} level {level} {k}: kernel {errs[k]:.3e}  torch bf16 autocast {lost[k]:.3e}")
    worse = {k: (errs[k], lost[k]) for k in errs if errs[k] > max(BF16_FACTOR * lost[k], BF16_FLOOR)}
    assert not worse, worse


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bitwise_repeatable(backend, dtype):
    inputs, _ = _case(3, 2 * C + 2, 1.0)
    a, b = _run(backend, "default", inputs, dtype), _run(backend, "default", inputs, dtype)
    assert len(a) == 9 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_batch_invariant(backend):
    """a sequence's rows of out and dxz in a BF = 10 launch have the bits of the BF = 1 launch of that sequence"""
    inputs, _ = _case(10, C + 1, 1.0)
    ten = _run(backend, "default", inputs)
    for n in (0, 7):
        alone = _run(backend, "default", tuple(t[n:n + 1].contiguous() for t in inputs))
        assert torch.equal(ten[0][n:n + 1], alone[0]) and torch.equal(ten[1][n:n + 1], alone[1]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inference_forward_keeps_nothing_and_is_the_same(backend, dtype):
    inputs, _ = _case(3, 2 * C + 2, 1.0)
    assert torch.equal(_run(backend, "default", inputs, dtype, keep=False, bwd=False)[0], _run(backend, "default", inputs, dtype, keep=True, bwd=False)[0])


def test_more_sequences_than_one_grid_pass(backend):
    """the grid is capped at MAMBA_GRID_CAP workgroups, one per sequence: one sequence more makes the first workgroup walk a second one"""
    BF = MAMBA_GRID_CAP + 1
    inputs, want = _case(BF, 2, 1.0)
    errs = _errors(_run(backend, "default", inputs), want, 2)
    print(errs)
    assert errs["out"] <= FWD_TOL and all(v <= GRAD_TOL for k, v in errs.items() if k != "out"), errs


@pytest.mark.parametrize("BF,T", [(1, 1), (3, C + 1), (MAMBA_GRID_CAP + 1, 2), (10, 257)])
def test_buffer_sizes_are_exact(backend, BF, T):
    """save: the checkpoints [BF][ceil(T / c)][16][192] fp32 and the x_proj rows [BF][T][38] fp32, each piece 256-byte aligned; ws: one row of 67 x 192
    fp32 partial sums per workgroup.  (Every other test allocates exactly these sizes, filled with NaN bytes, and checks that every output is finite.)"""
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for dt in (NBSS_F32, NBSS_BF16):
        assert backend.lib.nbss_online_mamba_train_save_bytes(dt, BF, T) == al(BF * ((T + C - 1) // C) * 16 * 192 * 4) + al(BF * T * 38 * 4)
        assert backend.lib.nbss_online_mamba_train_ws_bytes(dt, BF, T) == al(min(BF, MAMBA_GRID_CAP) * 67 * 192 * 4)


def test_refusals(backend):
    lib = backend.lib
    buf = torch.zeros(1 << 20, device=backend.device)
    p = ops._ptr(lib, buf)
    st = ops._stream(lib, buf)
    o = p + 4 * 524288
    names = ("conv_w", "conv_b", "xproj_w", "dt_w", "dt_b", "A_log", "D")
    ins = dict(xz=p, **{n: p + 4 * 32768 * (i + 1) for i, n in enumerate(names)})
    gr = {"d_" + n: o + 4 * 32768 * (i + 1) for i, n in enumerate(names)}

    def fwd(T=4, dt=NBSS_F32, BF=1, y=o, save=None, ws=p + 4 * 300000, **kw):
        a = {**ins, **kw}
        return lib.nbss_online_mamba_train_fwd(dt, BF, T, a["xz"], *(a[n] for n in names), y, save, ws, st)

    def bwd(T=4, dt=NBSS_F32, BF=1, save=p, dy=p, dxz=o, ws=p + 4 * 300000, **kw):
        a = {**ins, **gr, **kw}
        return lib.nbss_online_mamba_train_bwd(dt, BF, T, a["xz"], *(a[n] for n in names), save, dy, dxz, *(a["d_" + n] for n in names), ws, st)

    for T in (0, -1, 4097):
        assert fwd(T=T) == EINVAL and bwd(T=T) == EINVAL, T
        assert lib.nbss_online_mamba_train_save_bytes(NBSS_F32, 1, T) == EINVAL and lib.nbss_online_mamba_train_ws_bytes(NBSS_F32, 1, T) == EINVAL
    assert fwd(dt=2) == EUNSUPPORTED and bwd(dt=2) == EUNSUPPORTED
    assert lib.nbss_online_mamba_train_save_bytes(7, 1, 4) == EUNSUPPORTED and lib.nbss_online_mamba_train_ws_bytes(7, 1, 4) == EUNSUPPORTED
    assert fwd(BF=0) == EINVAL and bwd(BF=0) == EINVAL and lib.nbss_online_mamba_train_save_bytes(NBSS_F32, 0, 4) == EINVAL
    assert fwd(BF=(1 << 28) // 4 + 1) == EUNSUPPORTED
    for name in ("xz", *names, "y", "ws"):
        assert fwd(**{name: None}) == EINVAL, name
    for name in ("xz", *names, "save", "dy", "dxz", *gr, "ws"):
        assert bwd(**{name: None}) == EINVAL, name
    assert fwd(y=ins["xz"]) == EINVAL and bwd(dxz=ins["xz"]) == EINVAL
    assert not buf.any()  # nothing ran: the output buffers are untouched
