"""The narrow-band building blocks of the C ABI (nbss_nb_conv_t, _conv_t_train, _conv_t_bwd, _layernorm, _layernorm_bwd, _group_batch_norm, _group_batch_norm_bwd,
_group_norm, _group_norm_train, _group_norm_bwd), one call per case, on the emulator AND on the device, one explicit case per branch of the launch code
(csrc/nb_blocks.hip over gb_gemm.hip, gemm_g.hip, wgrad.hip, gb_rows.hip), against plain torch in fp64 on the CPU fed the SAME rounded tensors the kernel reads.
Outputs start as NaN; accumulated outputs (dw, dbias, dgamma, dbeta) start from seeded non-zero values and must come back as prefill + gradient."""
# Case -> kernel branch.  Every row was confirmed once with a temporary print in the launchers of a scratch emulator build (gb_gemm, wgrad_launch_t,
# gb_ln_fwd, gb_ln_bwd); the first word of a case id is the row's tag.
#   gb_gemm (forward, and the data gradient = the same kernels on re-laid weights)
#     lds-*                    gb_tap_gemm_lds_kernel<f32 | bf16>; under test_conv_t_bwd_data with pre = 1: its Dact epilogue; *-y2: its Y2 epilogue
#     nolds-fallback[-dense]   gb_tap_gemm_kernel (taps 64 (Kp + 8) sizeof(T) = 174 080 / 168 960 / 157 696 bytes > 150 KiB); pre = 1: with Dact
#     gl-gemm                  gl_gemm_kernel (bf16, K = Kp >= 64, M >= 64), pre = 1: its Dact epilogue; also the dx of tr3-64x5 / x10 / x14 "both"
#     lds-dense-cout40         K = 40 != Kp = 64: gl_gemm_takes refuses, gb_tap_gemm_lds_kernel<bf16> with Dact
#     not reached: gb_tap_store's store1 tail (m0 + 3 >= Mg).  gb_gemm wants ldy % 4 == 0 and ygs % 4 == 0, so Mg % 4 == 0 for every call this ABI
#       can make and a 4-output piece is whole or absent.  gl_gemm_kernel's forward epilogues are tests/test_gemm_g.py's.
#   wgrad_launch_t (test_conv_t_bwd_weight; "both" adds the data gradient in the same call)
#     tr3-128x2-skinny         wgrad_tr3_kernel<128, 2>, 127 / 128 / 129 tokens = 1, 1, 2 chunks
#     tr3-64x2-tconv           wgrad_tr3_kernel<64, 2>, per-sequence chunks: T = 63, 64 -> 2 chunks, T = 65 -> 4
#     tr3-64x5, -64x10, -64x14 wgrad_tr3_kernel<64, 5 | 10 | 14> (36, 72, 96 tiles), 65 / 63 / 64 and 129 tokens
#     tr3-32x27-tconv          wgrad_tr3_kernel<32, 27> (8 groups x 27 tiles), T = 31, 32 -> 2 chunks, T = 33 -> 4
#     wk-bf16-cw4-*            wgrad_kernel<bf16, 4, 4> (NB % 8 != 0, resp. Cout / groups % 8 != 0); -tpw14: wgrad_kernel<bf16, 4, 14> (48 tiles)
#     wk-f32-all-groups        wgrad_kernel<float, 4, 14>, all = 1 (both groups in one workgroup), 38 / 64 tokens of 32-token chunks
#     wk-f32-group-per-y       wgrad_kernel<float, 4, 14>, all = 0, gridDim.y = 8
#     nz2-grouped-linear       gridDim.z = 2, atomic flush (no partial tiles): wgrad_kernel<float, 4, 14> and wgrad_kernel<bf16, 8, 14>
#     dense-row-slices-144+64  nb_conv_t_bwd's slice loop, last slice partial: f32 2 x wgrad_kernel<float, 4, 14>; bf16 wgrad_tr3_kernel<64, 14> then <64, 10>
#     not reached: wgrad_kernel<bf16, 8, 4> (8-wide staging AND <= 32 tiles AND refused by the tr3 branch: that needs taps > 1 on a layout that is neither
#       per-sequence nor per-frequency, or a_gw / b_gw / stats, none of which nb_conv_t_bwd sets); wgrad_tr3_kernel<96, *> (F-convs: shift_dim = 1);
#       the a.part = nullptr fallbacks of the tr3 branch (more than WGPART_BYTES of partial tiles: > 512 x 112 tiles); FoldScope batching (g_fold).
#   gb_ln_fwd / gb_ln_bwd:  C = 192, 384 -> gb_ln_fwd8_kernel / gb_ln_bwd8_kernel<3 | 6> (atomic flush); others -> gb_ln_fwd_kernel / gb_ln_bwd_kernel.
#     not reached: gb_ln_bwd's `part` rows + affine_reduce_launch (nb_layernorm_bwd_impl passes no partial buffer), and the refusals (C > 384).
#
# Tolerances
#   rel-L2 against fp64, fp32 stream:        2e-5 forward and conv gradients, 5e-5 norm gradients (tests/test_nbc2_native.py's emulator values)
#   rel-L2 against fp64, bf16 stored output: 1.5e-2 (util.Case.tol)
#   fp32 outputs computed from bf16 inputs (dw, dbias, dgamma, dbeta, LayerNorm / GroupNorm statistics): TOL_F32_FROM_BF16 = 4 x the worst value measured over
#     all cases on both backends (2.22e-5; the condition was <= 1e-4).  Measured worst rel-L2 (emulator / MI355X):
#       dw 7.8e-8 / 6.5e-8, dbias 3.1e-8 / 3.1e-8, LayerNorm dgamma 3.2e-6 / 5.5e-6 (the worst: the 100 + randn case), dbeta 4.7e-8 / 4.7e-8,
#       GroupBatchNorm dgamma 1.9e-6 / 1.8e-6, dbeta 8.5e-7 / 8.4e-7, GroupNorm dgamma 2.8e-6 / 2.8e-6, dbeta 1.4e-6 / 1.4e-6,
#       LayerNorm mean 7.2e-8 / 7.3e-8, rstd 8.3e-8 / 7.3e-8, GroupNorm mean 6.0e-8 / 1.0e-7, rstd 6.4e-8 / 6.9e-8
#     (the fp32 stream's own: dw 1.1e-7, dbias 1.2e-7, norm affine gradients <= 7.7e-6 on both)
#   every element of y / dx:  |got - want| <= u |want| + (n + 8) 2^-24 S   (forward error of an n-term fp32 dot product + one output rounding), where
#     S = the same convolution of |x| and |w| (+ |bias| + |residual|), times 1.1 behind SiLU / SiLU' (max |SiLU'| < 1.1); n = taps K; u = 2^-8 (bf16) / 2^-22 (fp32).
#     Nothing measured; the fast exp of silu_f / dsilu_f needed no wider u (worst error / bound on the MI355X: fp32 0.11, bf16 0.99 = the output rounding).
#     Two roundings the kernels make BEFORE the output rounding are part of their contract and get their own terms, derived, not measured:
#       bf16, act_in:   the MFMA operand SiLU(x) is rounded to bf16 (relative 2^-8 per term: bf16 keeps 8 significant bits) -> + 2^-8 S
#       bf16, residual: y = residual + round_bf16(conv) (what a separate add over the stored conv gives)                    -> + 2^-8 |conv|
#   every element of y_silu against SiLU of the STORED y: U_SILU |want| — silu_f alone: v_exp_f32 and v_rcp_f32 (1 ulp each), the exponent's scaling, one add and
#     one multiply.  fp32: 2^-21; measured worst 1.18 * 2^-22 on the MI355X (0.58 * 2^-22 on the emulator).  bf16: the output rounding, 2^-8.
import ctypes as C
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as Fn

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32, NbssError
from util import rel_l2

F32, BF16 = "f32", "bf16"
BOTH = (F32, BF16)
_DT = {F32: (NBSS_F32, torch.float32), BF16: (NBSS_BF16, torch.bfloat16)}
TOL = {F32: 2e-5, BF16: 1.5e-2}              # stream outputs, conv gradients
TOL_NORM_GRAD = {F32: 5e-5, BF16: 1.5e-2}    # dx of the norms
TOL_F32_FROM_BF16 = 2.22e-5                  # 4 x 5.55e-6 (header)
U = {F32: 2.0 ** -22, BF16: 2.0 ** -8}
U_SILU = {F32: 2.0 ** -21, BF16: 2.0 ** -8}
EPS24 = 2.0 ** -24


def _f32_out_tol(dt, f32_tol):
    return f32_tol if dt == F32 else TOL_F32_FROM_BF16


class Env:
    """one (backend, dtype, seed): tensors on the backend's device in the stream dtype next to their fp64 CPU twins"""

    def __init__(self, backend, dt, seed):
        self.lib, self.dev, self.be, self.dt = backend.lib, backend.device, backend.name, dt
        self.code, self.td = _DT[dt]
        self.g = torch.Generator().manual_seed(seed)

    def randn(self, *shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=self.g) * scale + shift

    def stream(self, t):
        r = t.to(self.td)
        return r.to(self.dev).contiguous(), r.double()

    def f32(self, t):
        r = t.float().contiguous()
        return r.to(self.dev), r.double()

    def nan(self, *shape, dtype=None):
        return torch.full(shape, float("nan"), dtype=dtype or self.td, device=self.dev)

    def P(self, t):
        return ops._ptr(self.lib, t)

    def st(self, t):
        return ops._stream(self.lib, t)

    def ws(self, nbytes):
        assert nbytes > 0
        return torch.empty(nbytes, dtype=torch.uint8, device=self.dev)

    def note(self, kind, err):
        """every figure is printed before it is asserted on (pytest -s): `NBB <output class> <dtype> <backend> <value>`"""
        print(f"NBB {kind} {self.dt} {self.be} {err:.3e}")
        return err


def _silu64(x):
    return x * torch.sigmoid(x)


def _dsilu64(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def _elementwise(env, kind, got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0: an element whose bound is zero has to be exact)"""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{kind}: NaN / inf left in the output"
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = env.note(kind + "-elem/bound", float(ratio.max()))
    i = int(ratio.argmax())
    assert worst <= 1.0, f"{kind}: element {i}: got {got.flatten()[i]}, want {want.flatten()[i]}, bound {bound.flatten()[i]}"


class Sh(NamedTuple):
    """y [nseq][T][groups mg] = conv_t(x [nseq][T][ldx], valid columns groups kg), kernel size taps"""
    nseq: int
    T: int
    groups: int
    kg: int
    mg: int
    taps: int
    ldx: int = 0
    dts: tuple = BOTH

    @property
    def cin(self):
        return self.groups * self.kg

    @property
    def cout(self):
        return self.groups * self.mg

    @property
    def ld(self):
        return self.ldx or self.cin

    def __str__(self):
        return f"{self.nseq}x{self.T}-g{self.groups}-{self.kg}to{self.mg}-k{self.taps}" + (f"-ld{self.ldx}" if self.ldx else "")


def _conv64(x, w, b, groups):
    return Fn.conv1d(x.transpose(1, 2), w, b, padding=w.shape[-1] // 2, groups=groups).transpose(1, 2)


def _params(cases, arity):
    """(tag, shape, *flags) -> one pytest.param per dtype the case runs in; the id names the branch the case is there for"""
    out = []
    for c in cases:
        tag, s, rest = c[0], c[1], tuple(c[2:])
        assert len(rest) == arity, c
        for dt in s.dts:
            flags = "".join(f"-{int(r)}" if not isinstance(r, str) else f"-{r}" for r in rest)
            out.append(pytest.param(s, *rest, dt, id=f"{tag}-{s}{flags}-{dt}"))
    return out


# ---- 1. tap-GEMM forward -------------------------------------------------------------------------------------------------------------------------------
ROWS = (1, 15, 16, 17, 255, 256, 257)   # around the 16-row wave tile and the 64 * GT_R = 256-row workgroup of gb_tap_gemm_lds_kernel
G24 = lambda nseq, T, taps=3: Sh(nseq, T, 2, 24, 24, taps)  # noqa: E731
FWD = (
    [(f"lds-rows{r}", G24(1, r), 0, 0, 0) for r in ROWS]
    + [("lds-tile-spans-3-seqs", G24(3, 5, 3), 0, 0, 0), ("lds-tile-spans-3-seqs", G24(3, 5, 5), 0, 0, 0),
       ("lds-more-taps-than-frames", G24(2, 1, 5), 0, 0, 0), ("lds-more-taps-than-frames", G24(2, 2, 5), 0, 0, 0)]
    + [(f"lds-out{mg}", Sh(2, 19, 2, 8, mg, 3), 0, 0, 0) for mg in (4, 20, 24, 72, 80)]   # partial 16-tile / second 64-chunk with one valid tile (Mp = 80)
    + [(f"lds-grouped-g{g}-k{kg}", Sh(2, 19, g, kg, 16, 3), 0, 0, 1) for g in (2, 8) for kg in (8, 24, 40)]
    + [("lds-dense-12of16", Sh(2, 19, 1, 12, 40, 5, ldx=16), 0, 0, 0), ("lds-dense-12of16", Sh(2, 19, 1, 12, 40, 1, ldx=16), 1, 1, 1)]
    + [("lds-act-res", G24(2, 19), ai, ao, r) for ai in (0, 1) for ao in (0, 1) for r in (0, 1)]
    + [("nolds-fallback", Sh(2, 19, 1, 128, 40, 5, dts=(F32,)), 0, 0, 0), ("nolds-fallback", Sh(2, 19, 1, 128, 40, 5, dts=(F32,)), 1, 1, 1),
       ("nolds-fallback", Sh(2, 19, 1, 256, 40, 5, dts=(BF16,)), 0, 0, 0), ("nolds-fallback", Sh(2, 19, 1, 256, 40, 5, dts=(BF16,)), 1, 1, 1),
       ("nolds-fallback-dense", Sh(1, 33, 1, 608, 24, 1, dts=(F32,)), 0, 1, 1)]
)


def _conv_operands(env, s):
    """x (zero in the padding columns), w [Cout][Kg][taps] ~ N(0, 1 / fan-in), bias; w64 is what the GEMM reads: the weight rounded to the stream dtype by the re-lay"""
    x = torch.zeros(s.nseq, s.T, s.ld)
    x[..., :s.cin] = env.randn(s.nseq, s.T, s.cin)
    w = env.randn(s.cout, s.kg, s.taps, scale=(s.kg * s.taps) ** -0.5)
    b = env.randn(s.cout, scale=0.1)
    return x, w, b


def _forward(env, s, act_in, act_out, res, train):
    lib = env.lib
    x, w, b = _conv_operands(env, s)
    xd, x64 = env.stream(x)
    wd, _ = env.f32(w)
    w64 = w.to(env.td).double()
    bd, b64 = env.f32(b)
    rd, r64 = env.stream(env.randn(s.nseq, s.T, s.cout)) if res else (None, None)
    y = env.nan(s.nseq, s.T, s.cout)
    xin = x64[..., :s.cin]
    xin = _silu64(xin) if act_in else xin
    z = _conv64(xin, w64, b64, s.groups)
    S = _conv64(xin.abs(), w64.abs(), b64.abs(), s.groups)
    core = _silu64(z) if act_out else z
    want = core + r64 if res else core
    if train:
        h = env.nan(s.nseq, s.T, s.cout)
        ws = env.ws(lib._dll.nbss_nb_bwd_ws_bytes(s.cout, s.cin, s.groups, s.taps))
        lib.call("nbss_nb_conv_t_train", env.code, s.nseq, s.T, s.cin, s.ld, s.cout, s.groups, s.taps, env.P(xd), env.P(wd), env.P(bd), env.P(y), env.P(h),
                 env.P(rd), env.P(ws), env.st(xd))
    else:
        ws = env.ws(lib._dll.nbss_nb_ws_bytes(s.cout, s.cin, s.groups, s.taps))
        lib.call("nbss_nb_conv_t", env.code, s.nseq, s.T, s.cin, s.ld, s.cout, s.groups, s.taps, env.P(xd), env.P(wd), env.P(bd), env.P(y), env.P(rd),
                 act_in, act_out, env.P(ws), env.st(xd))
    bound = U[env.dt] * want.abs() + (1.1 if act_out else 1.0) * (s.taps * s.kg + 8) * EPS24 * (S + (r64.abs() if res else 0))
    if env.dt == BF16 and act_in:
        bound = bound + 2.0 ** -8 * S
    if env.dt == BF16 and res:
        bound = bound + 2.0 ** -8 * core.abs()
    e = env.note("y", rel_l2(y, want))
    _elementwise(env, "y", y, want, bound)
    assert e < TOL[env.dt]
    if train:
        ys = y.double().cpu()
        e2 = env.note("y_silu", rel_l2(h, _silu64(want)))
        _elementwise(env, "y_silu", h, _silu64(ys), U_SILU[env.dt] * _silu64(ys).abs())  # (the activation of the STORED y)
        assert e2 < TOL[env.dt]


@pytest.mark.parametrize("s,act_in,act_out,res,dt", _params(FWD, 3))
def test_conv_t(backend, s, act_in, act_out, res, dt):
    _forward(Env(backend, dt, 100 + s.T + s.kg), s, act_in, act_out, res, train=False)


TRAIN = [("lds-grouped-y2", Sh(2, 19, 2, 24, 24, 3), 0), ("lds-grouped-y2", Sh(2, 19, 2, 24, 24, 3), 1),
         ("lds-dense-12of16-y2", Sh(3, 17, 1, 12, 40, 1, ldx=16), 0), ("lds-dense-12of16-y2", Sh(3, 17, 1, 12, 40, 1, ldx=16), 1)]


@pytest.mark.parametrize("s,res,dt", _params(TRAIN, 1))
def test_conv_t_train(backend, s, res, dt):
    _forward(Env(backend, dt, 200 + s.T), s, 0, 0, res, train=True)


# ---- 2. / 3. data, weight and bias gradient --------------------------------------------------------------------------------------------------------------
def _backward(env, s, pre, need_dx, need_dw):
    """nbss_nb_conv_t_bwd on x = SiLU(x_pre) (pre) or a plain x: dx (times SiLU'(x_pre)), dw, dbias against autograd in fp64"""
    lib = env.lib
    a = env.randn(s.nseq, s.T, s.ld)
    ad, a64 = env.stream(a)  # (the padding columns of x_pre hold values: dx there is SiLU'(.) times an exact zero)
    _, w, _ = _conv_operands(env, s)
    x = torch.zeros(s.nseq, s.T, s.ld, dtype=torch.float64)
    x[..., :s.cin] = (_silu64(a64) if pre else a64)[..., :s.cin]
    xd, x64 = env.stream(x)
    wd, _ = env.f32(w)
    w64 = w.to(env.td).double()
    dyd, dy64 = env.stream(env.randn(s.nseq, s.T, s.cout))
    xr, wr = x64[..., :s.cin].clone().requires_grad_(True), w64.clone().requires_grad_(True)
    (_conv64(xr, wr, None, s.groups) * dy64).sum().backward()
    xs = x64[..., :s.cin].abs().requires_grad_(True)
    (_conv64(xs, w64.abs(), None, s.groups) * dy64.abs()).sum().backward()
    dx_want, S = torch.zeros_like(x64), torch.zeros_like(x64)
    dx_want[..., :s.cin] = xr.grad * (_dsilu64(a64[..., :s.cin]) if pre else 1.0)
    S[..., :s.cin] = xs.grad * (1.1 if pre else 1.0)
    dx = env.nan(s.nseq, s.T, s.ld) if need_dx else None
    dw0, db0 = env.randn(s.cout * s.kg * s.taps), env.randn(s.cout)
    dw, db = (dw0.to(env.dev, copy=True), db0.to(env.dev, copy=True)) if need_dw else (None, None)
    ws = env.ws(lib._dll.nbss_nb_bwd_ws_bytes(s.cout, s.cin, s.groups, s.taps))
    lib.call("nbss_nb_conv_t_bwd", env.code, s.nseq, s.T, s.cin, s.ld, s.cout, s.groups, s.taps, env.P(xd), env.P(wd), env.P(dyd), env.P(ad) if pre else None,
             env.P(dx), env.P(dw), env.P(db), env.P(ws), env.st(xd))
    errs = {}
    if need_dx:
        errs["dx"] = (env.note("dx", rel_l2(dx, dx_want)), TOL[env.dt])
        bound = U[env.dt] * dx_want.abs() + (s.taps * s.mg + 8) * EPS24 * S
        _elementwise(env, "dx", dx, dx_want, bound)
        if s.ld > s.cin:
            assert (dx[..., s.cin:] == 0).all(), "padding columns of dx"
    if need_dw:
        tol = _f32_out_tol(env.dt, 2e-5)
        errs["dw"] = (env.note("dw", rel_l2(dw.double().cpu() - dw0.double(), wr.grad.reshape(-1))), tol)
        errs["dbias"] = (env.note("dbias", rel_l2(db.double().cpu() - db0.double(), dy64.sum((0, 1)))), tol)
    bad = {k: v for k, v in errs.items() if not v[0] < v[1]}
    assert not bad, bad


DGRAD = (
    [(f"lds-rows{r}", G24(1, r)) for r in ROWS]
    + [("lds-tile-spans-3-seqs", G24(3, 5, 3)), ("lds-tile-spans-3-seqs", G24(3, 5, 5)), ("lds-more-taps-than-frames", G24(2, 1, 5)), ("lds-more-taps-than-frames", G24(2, 2, 5))]
    + [(f"lds-out{kg}", Sh(2, 19, 2, kg, 8, 3)) for kg in (8, 24, 40, 72, 80)]                       # the transposed map's outputs are the forward's inputs
    + [(f"lds-grouped-g{g}-k{mg}", Sh(2, 19, g, 16, mg, 3)) for g in (2, 8) for mg in (8, 24, 40)]   # ... and its K the forward's outputs
    + [("lds-dense-12of16", Sh(2, 19, 1, 12, 40, 5, ldx=16)), ("lds-dense-12of16", Sh(2, 19, 1, 12, 40, 1, ldx=16)), ("lds-dense-20of24", Sh(1, 17, 1, 20, 24, 1, ldx=24)),
       ("gl-gemm", Sh(1, 129, 1, 64, 64, 1, dts=(BF16,))), ("gl-gemm", Sh(3, 43, 1, 192, 384, 1, dts=(BF16,))),
       ("lds-dense-cout40", Sh(1, 257, 1, 64, 40, 1)),                                               # gl_gemm_takes refuses K = 40: the LDS kernel, with Dact under pre
       ("nolds-fallback", Sh(2, 19, 1, 40, 128, 5, dts=(F32,))), ("nolds-fallback", Sh(2, 19, 1, 40, 256, 5, dts=(BF16,))),
       ("nolds-fallback-dense", Sh(1, 33, 1, 24, 608, 1, dts=(F32,)))]
)


@pytest.mark.parametrize("s,pre,dt", _params([c + (p,) for c in DGRAD for p in (0, 1)], 1))
def test_conv_t_bwd_data(backend, s, pre, dt):
    _backward(Env(backend, dt, 300 + s.T + s.mg), s, pre, need_dx=True, need_dw=False)


T3 = (BF16,)
WGRAD = (
    [("tr3-128x2-skinny", Sh(1, n, 1, 16, 16, 1, dts=T3)) for n in (127, 128, 129)]
    + [("tr3-64x2-tconv", Sh(2, t, 1, 16, 16, 3, dts=T3)) for t in (63, 64, 65)]
    + [("tr3-64x5", Sh(1, 65, 1, 96, 96, 1, dts=T3)), ("tr3-64x10", Sh(1, 63, 1, 96, 192, 1, dts=T3)), ("tr3-64x14", Sh(1, 64, 1, 128, 192, 1, dts=T3)),
       ("tr3-64x14", Sh(3, 43, 1, 128, 192, 1, dts=T3))]
    + [("tr3-32x27-tconv", Sh(2, t, 8, 48, 48, 3, dts=T3)) for t in (31, 32, 33)]
    + [("wk-bf16-cw4-12of16", Sh(2, 19, 1, 12, 40, 5, ldx=16, dts=T3)), ("wk-bf16-cw4-12of16", Sh(3, 11, 1, 12, 40, 1, ldx=16, dts=T3)),
       ("wk-bf16-cw4-cout20", Sh(2, 19, 1, 16, 20, 1, dts=T3)), ("wk-bf16-cw4-tpw14", Sh(2, 19, 1, 12, 192, 5, ldx=16, dts=T3)),  # 48 tiles: more than 4 per wave
       ("wk-f32-all-groups", Sh(2, 19, 2, 8, 8, 3, dts=(F32,))), ("wk-f32-all-groups", Sh(2, 32, 2, 8, 8, 3, dts=(F32,))),
       ("wk-f32-group-per-y", Sh(2, 19, 8, 48, 48, 3, dts=(F32,))), ("wk-f32-group-per-y", Sh(2, 33, 8, 48, 48, 3, dts=(F32,))),
       ("nz2-grouped-linear", Sh(1, 31, 2, 192, 192, 1)), ("nz2-grouped-linear", Sh(1, 65, 2, 192, 192, 1)),
       ("dense-row-slices-144+64", Sh(1, 65, 1, 192, 208, 1)), ("dense-row-slices-144+64", Sh(2, 19, 1, 192, 208, 1))]
)


# (dx needs Cout / groups % 8 == 0: the Cout = 20 case has no "both")
@pytest.mark.parametrize("s,mode,dt", _params([c + (m,) for c in WGRAD for m in ("dw", "both") if m == "dw" or c[1].mg % 8 == 0], 1))
def test_conv_t_bwd_weight(backend, s, mode, dt):
    _backward(Env(backend, dt, 400 + s.T + s.kg), s, 0, need_dx=mode == "both", need_dw=True)


# ---- 4. row norms ------------------------------------------------------------------------------------------------------------------------------------------
def _affine(env, Cc):
    gam, bet = torch.rand(Cc, generator=env.g) + 0.5, env.randn(Cc, scale=0.3)
    return env.f32(gam) + env.f32(bet)


def _check(errs):
    bad = {k: v for k, v in errs.items() if not v[0] < v[1]}
    assert not bad, bad


def _layernorm(env, rows, Cc, dres, shift=0.5, scale=2.0):
    lib = env.lib
    xd, x64 = env.stream(env.randn(rows, Cc, scale=scale, shift=shift))
    gd, g64, bd, b64 = _affine(env, Cc)
    y, stats = env.nan(rows, Cc), env.nan(rows, 2, dtype=torch.float32)
    lib.call("nbss_nb_layernorm", env.code, rows, Cc, env.P(xd), env.P(gd), env.P(bd), env.P(y), env.P(stats), env.st(xd))
    xr, gr, br = x64.clone().requires_grad_(True), g64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    want = Fn.layer_norm(xr, (Cc,), gr, br, 1e-5)
    var, mean = torch.var_mean(x64, dim=-1, unbiased=False)
    errs = {"y": (env.note("ln-y", rel_l2(y, want)), TOL[env.dt]),
            "mean": (env.note("ln-mean", rel_l2(stats[:, 0], mean)), _f32_out_tol(env.dt, 2e-5)),
            "rstd": (env.note("ln-rstd", rel_l2(stats[:, 1], torch.rsqrt(var + 1e-5))), _f32_out_tol(env.dt, 2e-5))}
    dyd, dy64 = env.stream(env.randn(rows, Cc))
    drd, dr64 = env.stream(env.randn(rows, Cc) if dres else torch.zeros(rows, Cc))
    (want * dy64).sum().backward()
    dx = env.nan(rows, Cc)
    dg0, db0 = env.randn(Cc), env.randn(Cc)
    dg, db = dg0.to(env.dev, copy=True), db0.to(env.dev, copy=True)
    lib.call("nbss_nb_layernorm_bwd", env.code, rows, Cc, env.P(xd), env.P(stats), env.P(gd), env.P(dyd), env.P(drd), env.P(dx), env.P(dg), env.P(db), env.st(xd))
    errs["dx"] = (env.note("ln-dx", rel_l2(dx, xr.grad + dr64)), TOL_NORM_GRAD[env.dt])
    errs["dgamma"] = (env.note("ln-dgamma", rel_l2(dg.double().cpu() - dg0.double(), gr.grad)), _f32_out_tol(env.dt, 5e-5))
    errs["dbeta"] = (env.note("ln-dbeta", rel_l2(db.double().cpu() - db0.double(), br.grad)), _f32_out_tol(env.dt, 5e-5))
    _check(errs)


def _ln_kernel(Cc):
    return "fwd8-bwd8" if Cc in (192, 384) else "generic"


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("dres", [0, 1], ids=["dres0", "dres"])
@pytest.mark.parametrize("rows", [1, 3, 63, 64, 65, 129])
@pytest.mark.parametrize("Cc", [8, 40, 96, 192, 384], ids=lambda c: f"{_ln_kernel(c)}-C{c}")
def test_layernorm_fwd_bwd(backend, Cc, rows, dres, dt):
    """(dres0: a tensor of zeros: the ABI takes no NULL there, see test_layernorm_bwd_refuses_null_dres)"""
    _layernorm(Env(backend, dt, 500 + rows + Cc), rows, Cc, dres)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("Cc", [96, 192], ids=lambda c: f"{_ln_kernel(c)}-C{c}")
def test_layernorm_offset_mean(backend, Cc, dt):
    """input 100 + randn: the statistics are two-pass (sum of squared deviations from the mean), so the tolerances hold"""
    _layernorm(Env(backend, dt, 510 + Cc), 65, Cc, 1, shift=100.0, scale=1.0)


def test_layernorm_bwd_refuses_null_dres(backend):
    env = Env(backend, F32, 0)
    xd, _ = env.stream(env.randn(3, 8))
    gd, _, _, _ = _affine(env, 8)
    st, dg, db = torch.zeros(3, 2, device=env.dev), torch.zeros(8, device=env.dev), torch.zeros(8, device=env.dev)
    dx = env.nan(3, 8)
    with pytest.raises(NbssError, match="EINVAL"):
        env.lib.call("nbss_nb_layernorm_bwd", env.code, 3, 8, env.P(xd), env.P(st), env.P(gd), env.P(xd), None, env.P(dx), env.P(dg), env.P(db), env.st(xd))
    assert torch.isnan(dx).all()  # nothing was launched


def _gbn(env, B, F, T, Cc, act, affine, alias=False, shift=0.3, scale=2.0):
    lib = env.lib
    xd, x64 = env.stream(env.randn(B * F, T, Cc, scale=scale, shift=shift))
    gd, g64, bd, b64 = _affine(env, Cc) if affine else (None,) * 4
    y = env.nan(B * F, T, Cc)
    lib.call("nbss_nb_group_batch_norm", env.code, B, F, T, Cc, env.P(xd), env.P(gd), env.P(bd), C.c_float(1e-5), act, env.P(y), env.st(xd))
    xr = x64.clone().requires_grad_(True)
    gr, br = (g64.clone().requires_grad_(True), b64.clone().requires_grad_(True)) if affine else (None, None)
    v = xr.reshape(B, F, T, Cc)
    var, mean = torch.var_mean(v, dim=(1, 3), unbiased=False, keepdim=True)  # per (utterance, frame) over (sequence, feature)
    want = (v - mean) * torch.rsqrt(var + 1e-5)
    if affine:
        want = want * gr + br
    want = (_silu64(want) if act else want).reshape(B * F, T, Cc)
    errs = {"y": (env.note("gbn-y", rel_l2(y, want)), TOL[env.dt])}
    dyd, dy64 = env.stream(env.randn(B * F, T, Cc))
    (want * dy64).sum().backward()
    dx = dyd if alias else env.nan(B * F, T, Cc)
    dg0, db0 = env.randn(Cc), env.randn(Cc)
    dg, db = (dg0.to(env.dev, copy=True), db0.to(env.dev, copy=True)) if affine else (None, None)
    lib.call("nbss_nb_group_batch_norm_bwd", env.code, B, F, T, Cc, env.P(xd), env.P(gd), env.P(bd), C.c_float(1e-5), act, env.P(dyd), env.P(dx), env.P(dg), env.P(db),
             env.st(xd))
    errs["dx"] = (env.note("gbn-dx", rel_l2(dx, xr.grad)), TOL_NORM_GRAD[env.dt])
    if affine:
        errs["dgamma"] = (env.note("gbn-dgamma", rel_l2(dg.double().cpu() - dg0.double(), gr.grad)), _f32_out_tol(env.dt, 5e-5))
        errs["dbeta"] = (env.note("gbn-dbeta", rel_l2(db.double().cpu() - db0.double(), br.grad)), _f32_out_tol(env.dt, 5e-5))
    _check(errs)


GBN_SHAPES = [(1, 1, 1, 8), (2, 3, 5, 96), (1, 5, 9, 192), (2, 2, 3, 384)]  # 384: more channels than threads (two rounds of the per-channel sums)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("affine", [1, 0], ids=["affine", "plain"])
@pytest.mark.parametrize("act", [0, 1], ids=["id", "silu"])
@pytest.mark.parametrize("shape", GBN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_group_batch_norm_fwd_bwd(backend, shape, act, affine, dt):
    _gbn(Env(backend, dt, 600 + sum(shape)), *shape, act, affine)


@pytest.mark.parametrize("dt", BOTH)
def test_group_batch_norm_bwd_in_place(backend, dt):
    """dx aliasing dy (the kernel reads every dy of a frame before it stores, twice)"""
    _gbn(Env(backend, dt, 620), 2, 3, 5, 96, 1, 1, alias=True)


@pytest.mark.parametrize("dt", BOTH)
def test_group_batch_norm_offset_mean(backend, dt):
    _gbn(Env(backend, dt, 630), 2, 3, 5, 96, 1, 1, shift=100.0, scale=1.0)


def _group_norm(env, nseq, T, Cc, groups, shift=0.3, scale=2.0):
    """group_norm (no SiLU), group_norm_train (SiLU, keeps the statistics) and group_norm_bwd (in place) against nn.functional.group_norm"""
    lib = env.lib
    xd, x64 = env.stream(env.randn(nseq, T, Cc, scale=scale, shift=shift))
    gd, g64, bd, b64 = _affine(env, Cc)
    y0, y = env.nan(nseq, T, Cc), env.nan(nseq, T, Cc)
    stats = env.nan(nseq * groups, 2, dtype=torch.float32)
    lib.call("nbss_nb_group_norm", env.code, nseq, T, Cc, groups, env.P(xd), env.P(gd), env.P(bd), 0, env.P(y0), env.st(xd))
    lib.call("nbss_nb_group_norm_train", env.code, nseq, T, Cc, groups, env.P(xd), env.P(gd), env.P(bd), 1, env.P(y), env.P(stats), env.st(xd))
    xr, gr, br = x64.clone().requires_grad_(True), g64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    plain = Fn.group_norm(xr.transpose(1, 2), groups, gr, br, 1e-5).transpose(1, 2)
    want = _silu64(plain)
    var, mean = torch.var_mean(x64.reshape(nseq, T, groups, Cc // groups), dim=(1, 3), unbiased=False)  # [nseq][groups]
    errs = {"y-plain": (env.note("gn-y", rel_l2(y0, plain)), TOL[env.dt]), "y": (env.note("gn-y", rel_l2(y, want)), TOL[env.dt]),
            "mean": (env.note("gn-mean", rel_l2(stats[:, 0], mean.reshape(-1))), _f32_out_tol(env.dt, 2e-5)),
            "rstd": (env.note("gn-rstd", rel_l2(stats[:, 1], torch.rsqrt(var + 1e-5).reshape(-1))), _f32_out_tol(env.dt, 2e-5))}
    dyd, dy64 = env.stream(env.randn(nseq, T, Cc))
    (want * dy64).sum().backward()
    dg0, db0 = env.randn(Cc), env.randn(Cc)
    dg, db = dg0.to(env.dev, copy=True), db0.to(env.dev, copy=True)
    lib.call("nbss_nb_group_norm_bwd", env.code, nseq, T, Cc, groups, env.P(xd), env.P(stats), env.P(gd), env.P(bd), env.P(dyd), env.P(dg), env.P(db), env.st(xd))
    errs["dx"] = (env.note("gn-dx", rel_l2(dyd, xr.grad)), TOL_NORM_GRAD[env.dt])
    errs["dgamma"] = (env.note("gn-dgamma", rel_l2(dg.double().cpu() - dg0.double(), gr.grad)), _f32_out_tol(env.dt, 5e-5))
    errs["dbeta"] = (env.note("gn-dbeta", rel_l2(db.double().cpu() - db0.double(), br.grad)), _f32_out_tol(env.dt, 5e-5))
    _check(errs)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("T", [1, 7, 33, 130])
@pytest.mark.parametrize("Cg", [(64, 4), (96, 2), (192, 8)], ids=lambda c: f"C{c[0]}-width{c[0] // c[1]}")  # group widths 16, 48 and 24 (256 % 24 != 0)
def test_group_norm_fwd_bwd(backend, Cg, T, dt):
    _group_norm(Env(backend, dt, 700 + T + Cg[0]), 2, T, *Cg)


@pytest.mark.parametrize("dt", BOTH)
def test_group_norm_offset_mean(backend, dt):
    _group_norm(Env(backend, dt, 730), 2, 33, 192, 8, shift=100.0, scale=1.0)
