"""Native training path of the OnlineSpatialNet's causal T-ConvFFN (csrc/online_train.hip: nbss_online_tconvffn_train_fwd / _bwd): LayerNorm -> 1x1 ->
SiLU -> causal grouped conv -> SiLU -> causal grouped conv -> GroupNorm of each frame over (24 channels x all frequencies) -> SiLU -> causal grouped conv
-> SiLU -> 1x1 -> + x, on the whole [B,F,T,96] stream in fp32 or bf16, with every parameter gradient from the HIP backward.

`models.arch.OnlineSpatialNet.SpatialNetLayer._tconvffn` takes it when NBSS_ONLINE_NATIVE_TRAIN=1 (off by default), the tensor is on a HIP device, the call
is not a streaming one, `supported(layer)` is None and the stream is fp32 (or autocast to bf16); attention and the cross-band blocks keep their torch.nn
modules in training."""
from __future__ import annotations

import contextlib
import os
from typing import List, Optional

import torch
from torch import Tensor

from . import ops
from ._lib import Lib, hip

# (module index in layer.tconvffn, attribute) in the order of the C ABI's parameter list
PARAM_SLOTS = ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias"), (3, "weight"), (3, "bias"), (5, "weight"), (5, "bias"), (6, "weight"), (6, "bias"),
               (8, "weight"), (8, "bias"), (10, "weight"), (10, "bias"))

_LIB_OVERRIDE: Optional[Lib] = None


def enabled() -> bool:
    """the switch, read at call time (like NBSS_NBC2_NATIVE); off unless it is exactly '1'"""
    return os.environ.get("NBSS_ONLINE_NATIVE_TRAIN", "0") == "1"


@contextlib.contextmanager
def use_lib(lib: Lib):
    """tests only: run the block through `lib` — the host-emulator build takes CPU tensors, so the module path can be exercised without a device"""
    global _LIB_OVERRIDE
    prev, _LIB_OVERRIDE = _LIB_OVERRIDE, lib
    try:
        yield
    finally:
        _LIB_OVERRIDE = prev


def active_lib(x: Tensor) -> Optional[Lib]:
    """the library a call on `x` would run through: the override for a tensor on its device, else the HIP library for a tensor on a HIP device, else None"""
    if _LIB_OVERRIDE is not None:
        return _LIB_OVERRIDE if (x.device.type == "cpu") == ops._is_emu(_LIB_OVERRIDE) else None
    return hip() if x.is_cuda else None


def tconvffn_params(layer) -> List[Tensor]:
    """the block's 14 parameters (the module's live tensors) in the order of the C ABI"""
    return [getattr(layer.tconvffn[i], a) for i, a in PARAM_SLOTS]


def supported(layer) -> Optional[str]:
    """None when the layer's T-ConvFFN is the geometry the kernels are built for (the checks of nbss_amd/online.py::supported that concern this block),
    else the reason"""
    from models.arch.OnlineSpatialNet import CausalConv1d
    tc = layer.tconvffn
    kinds = [type(m).__name__ for m in tc]
    if kinds != ["LayerNorm", "Conv1d", "SiLU", "CausalConv1d", "SiLU", "CausalConv1d", "GroupNorm", "SiLU", "CausalConv1d", "SiLU", "Conv1d"]:
        return f"the T-ConvFFN must be LN, 1x1, SiLU, conv, SiLU, conv, GN, SiLU, conv, SiLU, 1x1 (got {kinds})"
    if tuple(tc[0].normalized_shape) != (96,) or tc[1].in_channels != 96 or tc[10].out_channels != 96:
        return f"dim_hidden must be 96 (got {tc[1].in_channels})"
    if tc[1].out_channels != 192 or tc[10].in_channels != 192:
        return f"dim_ffn must be 192 (got {tc[1].out_channels})"
    if tc[1].kernel_size[0] != 1 or tc[10].kernel_size[0] != 1:
        return "the two linear maps must be 1x1 convolutions"
    for i in (3, 5, 8):
        c = tc[i]
        if not isinstance(c, CausalConv1d) or c.kernel_size[0] != 3:
            return f"the T-conv kernel size must be 3 (got {c.kernel_size[0]})"
        if c.groups != 8:
            return f"the T-convs must have 8 groups (got {c.groups})"
        if c.look_ahead != 0 or c.dilation[0] != 1 or c.stride[0] != 1:
            return "the T-convs must be causal (no look-ahead), without dilation or stride"
    if tc[6].num_groups != 8:
        return f"the GroupNorm must have 8 groups (got {tc[6].num_groups})"
    if tc[0].eps != 1e-5 or tc[6].eps != 1e-5:
        return "norm eps must be 1e-5"
    if any(getattr(tc[i], a) is None for i, a in PARAM_SLOTS):
        return "every norm and convolution of the block must have weight and bias"
    if layer.dropout_tconvffn.p > 0:
        return "dropout must be 0"
    return None


def _kernel_params(params) -> List[Tensor]:
    """fp32, contiguous, the 1x1 weights as matrices (views where the module's tensors already are all that)"""
    return [(p.detach()[:, :, 0] if (i in (2, 12)) else p.detach()).float().contiguous() for i, p in enumerate(params)]


class OnlineTConvFFNFn(torch.autograd.Function):
    """y = x + T-ConvFFN(x) through the HIP kernels; inputs (lib, x, *the 14 parameters): the parameters are inputs of the node, so p.grad is populated the
    usual way.  One backward per forward: the saved activations are freed by it (retain_graph and double backward are refused)."""

    @staticmethod
    def forward(ctx, lib, x, *params):
        xk = x.contiguous()
        p32 = _kernel_params(params)
        y, save = ops.online_tconvffn_train_fwd(lib, p32, xk, keep=True)
        ctx.lib, ctx.saved, ctx.params = lib, (xk, save, p32), params
        ctx.versions = [p._version for p in params]
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        ops.graph_guard_check(ctx, "OnlineSpatialNet native T-ConvFFN")
        xk, save, p32 = ctx.saved
        dx, grads = ops.online_tconvffn_train_bwd(ctx.lib, p32, xk, save, dy.contiguous())
        ctx.saved = None
        out = [g.reshape(p.shape).to(p.dtype) if ctx.needs_input_grad[2 + i] else None for i, (g, p) in enumerate(zip(grads, ctx.params))]
        return (None, dx if ctx.needs_input_grad[1] else None, *out)


def eligible(layer, x: Tensor, state) -> Optional[str]:
    """None when this call takes the native block; else why not.  A reason that starts with '!' is worth a warning (the switch is on, the tensor is on the
    library's device, and the layer or dtype does not fit); the others are the ordinary torch.nn cases."""
    if not enabled():
        return "NBSS_ONLINE_NATIVE_TRAIN is not 1"
    if state is not None:
        return "streaming call"
    if _LIB_OVERRIDE is None and not x.is_cuda:
        return "not on a HIP device"
    why = supported(layer)
    if why is not None:
        return "!" + why
    if x.dim() != 4 or x.shape[-1] != 96:
        return f"!input must be [B,F,T,96], got {tuple(x.shape)}"
    if x.dtype != torch.float32 and _stream_dtype(x) is None:
        return f"!the stream must be fp32, or bf16 under autocast (got {x.dtype})"
    if not 1 <= x.shape[2] <= 4096 or x.shape[1] > 272:
        return f"!1 <= T <= 4096 and F <= 272 (got T = {x.shape[2]}, F = {x.shape[1]})"
    return None


def _stream_dtype(x: Tensor) -> Optional[torch.dtype]:
    dev = "cuda" if x.is_cuda else "cpu"
    if torch.is_autocast_enabled(dev):
        return torch.bfloat16 if torch.get_autocast_dtype(dev) == torch.bfloat16 else None
    return torch.float32 if x.dtype == torch.float32 else None


def tconvffn_residual(layer, x: Tensor) -> Tensor:
    """x + T-ConvFFN(x) for a call `eligible` accepted; in the dtype of x.  Without autograd (no_grad, or nothing requires a gradient) the forward runs alone
    and keeps nothing."""
    lib = active_lib(x)
    if lib is None:
        raise ops.NbssError("OnlineSpatialNet native T-ConvFFN: no library for a tensor on " + str(x.device))
    params = tconvffn_params(layer)
    xs = x.to(_stream_dtype(x))
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        y = OnlineTConvFFNFn.apply(lib, xs, *params)
    else:
        y = ops.online_tconvffn_train_fwd(lib, _kernel_params(params), xs.contiguous(), keep=False)[0]
    return y.to(x.dtype)
