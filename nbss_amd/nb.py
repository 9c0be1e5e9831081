"""What the three native narrow-band paths (nbc2.py, nbc.py, blstm.py) share: the one place that talks to the generic `nbss_nb_*` building blocks of the C ABI.

`Launcher`      one per forward / backward call: stream dtype, device, stream, workspace, and one method per building block (allocate the outputs, convert
                the parameters, launch).  The arch files keep what differs: which blocks in which order, and their own kernels (attention, recurrence).
`NativeRunner`  base of NativeNBC2 / NativeNBC / NativeBLSTM: the weak reference to the module, `forward_train` as one autograd.Function (`TrainFn`) over
                the subclass's `_forward_train(x) -> (out, saved)` and `_backward_train(saved, dout) -> parameter gradients in param_list order`."""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import Optional

import torch
from torch import Tensor

from . import ops
from ._lib import NBSS_BF16, NBSS_F32, Lib, NbssError


T_WHOLE = 256  # frames per sequence of the whole-head attention kernels: the training paths' limit
T_LONG = 4096  # ... of the key-blocked forward kernels behind nbss_nb_attention_long_fwd / nbss_nb_attention_relpos_long_fwd


def long_enabled() -> bool:
    """NBSS_NB_LONG=1: inference (`NativeNBC2.forward`, `NativeNBC.forward`) beyond 256 frames runs natively, through the key-blocked attention kernels.
    Read at call time, like NBSS_NBC2_NATIVE; off by default (then such calls are refused, and the modules take their torch.nn path with a warning)."""
    return os.environ.get("NBSS_NB_LONG", "0") == "1"


def pad8(c: int) -> int:
    return (c + 7) // 8 * 8


def ws_bytes(lib: Lib, shapes, bwd: bool = False) -> int:
    """workspace of the largest tap-GEMM among `shapes` = (M, K, groups, taps) per launch; bwd: the training entry points (forward and backward)"""
    fn = lib._dll.nbss_nb_bwd_ws_bytes if bwd else lib._dll.nbss_nb_ws_bytes
    return max(fn(*s) for s in shapes)


class Launcher:
    """The launches of ONE forward or backward call.  `like` (the input, or the output gradient) gives stream dtype, device and stream.

    Lifetime rule: a kernel reads its arguments when it runs, not when it is enqueued, and the caching allocator hands a freed block to the next
    request on the same stream — so a converted copy (`f32`) must outlive the enqueue of the kernel that reads it: a temporary freed before its kernel
    is enqueued could be re-used by the next one.  Every copy therefore goes into `keep` and lives as long as this object, which the caller drops when
    its call returns.  The launcher must NOT be reachable from the state saved for backward, nor from the runner: every fp32 copy and padded weight of
    the forward would then live until backward."""

    def __init__(self, lib: Lib, like: Tensor, ws: Optional[Tensor] = None):
        self.lib, self.dev, self.st, self.ws, self.keep = lib, like.device, ops._stream(lib, like), ws, []
        self.dt = NBSS_BF16 if like.dtype == torch.bfloat16 else NBSS_F32
        self.td = like.dtype if self.dt == NBSS_BF16 else torch.float32

    def p(self, t: Optional[Tensor]):
        return ops._ptr(self.lib, t)  # (checks that the tensor lives where the library computes: HIP device — or host for the test emulator)

    def f32(self, t: Tensor) -> Tensor:
        """a parameter as an fp32 contiguous device tensor (no copy for the fp32 parameters of an nn.Module), alive until this launcher goes"""
        v = t.detach().to(device=self.dev, dtype=torch.float32).contiguous()
        self.keep.append(v)
        return v

    def _f32(self, t: Optional[Tensor]):
        return self.p(self.f32(t)) if t is not None else None

    def zeros(self, *shape) -> Tensor:
        return torch.zeros(*shape, dtype=torch.float32, device=self.dev)

    def alloc_ws(self, shapes, bwd: bool = False, at_least: int = 0) -> Tensor:
        self.ws = torch.empty(max(ws_bytes(self.lib, shapes, bwd), at_least), dtype=torch.uint8, device=self.dev)
        return self.ws

    # ---- padding to the kernels' multiples of 8, and back ----------------------------------------------------------------------------------------------
    def pad_cols(self, x: Tensor, n: int, rows: int, c: int) -> Tensor:
        """x [.., c] -> [n, rows, pad8(c)] in the stream dtype, zero columns behind"""
        out = torch.zeros(n, rows, pad8(c), dtype=self.td, device=self.dev)
        out[..., :c] = x.reshape(n, rows, c).to(self.td)
        return out

    def padded(self, t: Optional[Tensor], *shape) -> Tensor:
        """fp32 zeros of `shape` with the parameter `t` in the leading corner (decoder rows beyond dim_output, input columns beyond dim_input, taps)"""
        out = self.zeros(*shape)
        if t is not None:
            out[tuple(slice(0, s) for s in t.shape)] = t
        return out

    @staticmethod
    def unpad(y: Tensor, B: int, F: int, T: int, cout: int, dtype) -> Tensor:
        return y[..., :cout].reshape(B, F, T, cout).to(dtype).contiguous()

    # ---- tap-GEMMs: y[n][rows][cout] = conv along the rows of x[n][rows][ldx] (first cin columns), w [cout][cin / groups][taps] ---------------------------
    def conv(self, xin, n, rows, cin, ldx, cout, groups, taps, w, b, res=None, act_in=0, act_out=0) -> Tensor:
        """inference: SiLU on the input (act_in) / output (act_out) fused, `res` added"""
        y = torch.empty(n, rows, cout, dtype=self.td, device=self.dev)
        self.lib.call("nbss_nb_conv_t", self.dt, n, rows, cin, ldx, cout, groups, taps, self.p(xin), self._f32(w), self._f32(b), self.p(y), self.p(res),
                      act_in, act_out, self.p(self.ws), self.st)
        return y

    def conv_train(self, xin, n, rows, cin, ldx, cout, groups, taps, w, b, res=None, y2=False):
        """training: -> y, or (y, SiLU(y)) with y2 (the producer writes what the consumer's backward needs)"""
        y = torch.empty(n, rows, cout, dtype=self.td, device=self.dev)
        ys = torch.empty_like(y) if y2 else None
        self.lib.call("nbss_nb_conv_t_train", self.dt, n, rows, cin, ldx, cout, groups, taps, self.p(xin), self._f32(w), self._f32(b), self.p(y), self.p(ys),
                      self.p(res), self.p(self.ws), self.st)
        return (y, ys) if y2 else y

    def conv_bwd(self, xin, n, rows, cin, ldx, cout, groups, taps, w, dy, x_pre=None, need_dx=True, bias=True):
        """-> (dx or None, dw flat, db or None); x_pre: xin = SiLU(x_pre), dx comes back multiplied by SiLU'(x_pre)"""
        dx = torch.empty(n, rows, ldx, dtype=self.td, device=self.dev) if need_dx else None
        dw = self.zeros(cout * (cin // groups) * taps)
        db = self.zeros(cout) if bias else None
        self.lib.call("nbss_nb_conv_t_bwd", self.dt, n, rows, cin, ldx, cout, groups, taps, self.p(xin), self._f32(w), self.p(dy), self.p(x_pre), self.p(dx),
                      self.p(dw), self.p(db), self.p(self.ws), self.st)
        return dx, dw, db

    # ---- norms -----------------------------------------------------------------------------------------------------------------------------------------
    def layernorm(self, h, mod, stats=None):
        """over the last axis of h -> (y, stats [rows][2])"""
        H = h.shape[-1]
        rows = h.numel() // H
        u = torch.empty_like(h)
        if stats is None:
            stats = torch.empty(rows, 2, dtype=torch.float32, device=self.dev)
        self.lib.call("nbss_nb_layernorm", self.dt, rows, H, self.p(h), self._f32(mod.weight), self._f32(mod.bias), self.p(u), self.p(stats), self.st)
        return u, stats

    def layernorm_bwd(self, xin, stats, mod, dy, dres):
        """-> (dx = LayerNorm'(dy) + dres, dweight, dbias)"""
        H = xin.shape[-1]
        dx, dg, db = torch.empty_like(xin), self.zeros(H), self.zeros(H)
        self.lib.call("nbss_nb_layernorm_bwd", self.dt, xin.numel() // H, H, self.p(xin), self.p(stats), self._f32(mod.weight), self.p(dy), self.p(dres),
                      self.p(dx), self.p(dg), self.p(db), self.st)
        return dx, dg, db

    def gbn(self, xin, mod, B, F, T, act):
        """GroupBatchNorm over (the F sequences of an utterance) x channels per frame, SiLU behind it with act"""
        y = torch.empty_like(xin)
        w, b = (mod.weight.reshape(-1), mod.bias.reshape(-1)) if mod.affine else (None, None)
        self.lib.call("nbss_nb_group_batch_norm", self.dt, B, F, T, xin.shape[-1], self.p(xin), self._f32(w), self._f32(b), C.c_float(mod.eps), act, self.p(y),
                      self.st)
        return y

    def gbn_bwd(self, xin, mod, B, F, T, act, dy):
        c = xin.shape[-1]
        dx, dg, db = torch.empty_like(xin), self.zeros(c), self.zeros(c)
        self.lib.call("nbss_nb_group_batch_norm_bwd", self.dt, B, F, T, c, self.p(xin), self._f32(mod.weight.reshape(-1)), self._f32(mod.bias.reshape(-1)),
                      C.c_float(mod.eps), act, self.p(dy), self.p(dx), self.p(dg), self.p(db), self.st)
        return dx, dg, db

    def group_norm(self, x, gn, act):
        """nn.GroupNorm of x [n][rows][c] per sequence over (rows x the group's channels), SiLU behind it with act"""
        n, rows, c = x.shape
        y = torch.empty_like(x)
        self.lib.call("nbss_nb_group_norm", self.dt, n, rows, c, gn.num_groups, self.p(x), self._f32(gn.weight), self._f32(gn.bias), act, self.p(y), self.st)
        return y

    def group_norm_train(self, x, gn, act):
        """-> (y, statistics [n * groups][2] for the backward)"""
        n, rows, c = x.shape
        y, gst = torch.empty_like(x), torch.empty(n * gn.num_groups, 2, dtype=torch.float32, device=self.dev)
        self.lib.call("nbss_nb_group_norm_train", self.dt, n, rows, c, gn.num_groups, self.p(x), self._f32(gn.weight), self._f32(gn.bias), act, self.p(y),
                      self.p(gst), self.st)
        return y, gst

    def group_norm_bwd(self, x, gst, gn, dy):
        """backward of group_norm_train(x, gn, 1), in place: dy becomes dx -> (dweight, dbias)"""
        n, rows, c = x.shape
        dg, db = self.zeros(c), self.zeros(c)
        self.lib.call("nbss_nb_group_norm_bwd", self.dt, n, rows, c, gn.num_groups, self.p(x), self.p(gst), self._f32(gn.weight), self._f32(gn.bias), self.p(dy),
                      self.p(dg), self.p(db), self.st)
        return dg, db


class TrainFn(torch.autograd.Function):
    """out = net(x) with the gradients of every parameter from the HIP building blocks.  inputs: (runner, x, *parameters in runner.param_list order).
    Each runner applies an empty subclass of its own (`train_fn`): the class name is the name of the node in the autograd graph (`_NBC2TrainFnBackward`, ...),
    which tells a reader of `y.grad_fn` — and the device tests — which native path produced a tensor."""

    @staticmethod
    def forward(ctx, runner, x, *params):
        out, saved = runner._forward_train(x)
        ops.graph_guard_save(ctx, runner, saved, params)
        return out

    @staticmethod
    def backward(ctx, dout):
        ops.graph_guard_check(ctx, f"{ctx.runner.label} native training")
        grads = ctx.runner._backward_train(ctx.saved, dout.contiguous())
        ctx.saved = None
        return (None, None, *grads)


class NativeRunner:
    """one torch.nn module run through the HIP building blocks; parameters are read from the module at every call (no copies).  Subclasses set `label`,
    `train_fn`, `supported`, `param_list` (and `train_supported`) and define `forward`, `_forward_train`, `_backward_train`."""
    label, kind = "", "native forward"
    train_supported = staticmethod(lambda net: None)

    def __init__(self, net, lib: Lib):
        why = self.supported(net)
        if why is not None:
            raise NbssError(f"{self.label} {self.kind}: {why}")
        # (a weak reference: models/arch/base/native.py caches the runner in a WeakKeyDictionary keyed by the module — a strong reference from the value
        #  would keep every module that ever ran on the device, and its parameters, alive for the life of the process)
        self._net, self.lib = weakref.ref(net), lib

    @property
    def net(self):
        net = self._net()
        if net is None:
            raise NbssError("the module this native runner was built for has been freed")
        return net

    def _p(self, t: Optional[Tensor]):
        return ops._ptr(self.lib, t)

    def forward_train(self, x: Tensor) -> Tensor:
        """training-mode forward with autograd: x [B,F,T,dim_input] -> [B,F,T,dim_output]; parameter gradients come from the HIP backward blocks"""
        why = self.train_supported(self.net)
        if why is not None:
            raise NbssError(f"{self.label} native training: {why}")
        return self.train_fn.apply(self, x, *self.param_list(self.net))
