"""Native training path of the OnlineSpatialNet's causal T-ConvFFN (csrc/online_train.hip: nbss_online_tconvffn_train_fwd / _bwd): LayerNorm -> 1x1 ->
SiLU -> causal grouped conv -> SiLU -> causal grouped conv -> GroupNorm of each frame over (24 channels x all frequencies) -> SiLU -> causal grouped conv
-> SiLU -> 1x1 -> + x, on the whole [B,F,T,96] stream in fp32 or bf16, with every parameter gradient from the HIP backward.

`models.arch.OnlineSpatialNet.SpatialNetLayer._tconvffn` takes it when NBSS_ONLINE_NATIVE_TRAIN=1 (off by default), the tensor is on a HIP device, the call
is not a streaming one, `supported(layer)` is None and the stream is fp32 (or autocast to bf16); attention and the cross-band blocks have switches of
their own (below).

The chunkwise retention core (csrc/online_ret_train.hip: nbss_online_ret_train_fwd / _bwd) has a switch of its own, NBSS_ONLINE_NATIVE_RET=1 (off by default,
independent of the one above): `SpatialNetLayer._tsa` then runs the module's four projections and out_proj as its own nn.Linear's around
`OnlineRetentionFn`, which replaces MultiScaleRetention.chunk_recurrent_forward, the per-head RMSNorm and the SiLU gate (`ret_eligible` says when).

The cross-band trio (csrc/online_xband_train.hip: nbss_online_xband_train_fwd / _bwd) has the third switch, NBSS_ONLINE_NATIVE_XBAND=1 (off by default, independent
of the other two): `SpatialNetLayer._xband` then evaluates x + fconv1, + full-band, + fconv2 as one `OnlineXBandFn` node on SpatialNet-small's F-conv and full-band
kernels (`xband_eligible` says when).  With all three on, what stays torch.nn in a training layer is the LayerNorm and the linear projections around retention."""
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


# ---- the retention core (NBSS_ONLINE_NATIVE_RET) ---------------------------------------------------------------------------------------------------------
RET_CHUNK, RET_T_MAX = 64, 4096


def ret_enabled() -> bool:
    """the retention switch, read at call time; off unless it is exactly '1'"""
    return os.environ.get("NBSS_ONLINE_NATIVE_RET", "0") == "1"


def ret_supported(mhsa) -> Optional[str]:
    """None when the module is the retention the kernels are built for, else the reason"""
    if type(mhsa).__name__ != "MultiScaleRetention":
        return f"the attention must be retention (got {type(mhsa).__name__})"
    if mhsa.embed_dim != 96 or mhsa.value_dim != 192:
        return f"embed_dim must be 96 and value_dim 192 (got {mhsa.embed_dim}, {mhsa.value_dim})"
    if mhsa.num_heads != 4:
        return f"num_heads must be 4 (got {mhsa.num_heads})"
    if mhsa.look_ahead != 0:
        return f"look_ahead must be 0 (got {mhsa.look_ahead})"
    if mhsa.gate_fn is not torch.nn.functional.silu:
        return "the gate must be swish"
    if mhsa.group_norm.weight is not None or mhsa.group_norm.eps != 1e-6:
        return "the head norm must be RMSNorm(eps=1e-6) without affine"
    return None


def ret_eligible(layer, u: Tensor, rel_pos, chunkwise_recurrent: bool, rope, state, inference: bool) -> Optional[str]:
    """None when this call of `_tsa` takes the native retention core; else why not, with the conventions of `eligible` (a leading '!': worth a warning)"""
    if not ret_enabled():
        return "NBSS_ONLINE_NATIVE_RET is not 1"
    if state is not None or inference:
        return "streaming or recurrent call"
    if _LIB_OVERRIDE is None and not u.is_cuda:
        return "not on a HIP device"
    if active_lib(u) is None:
        return "no library for the tensor's device"
    why = ret_supported(layer.mhsa)
    if why is not None:
        return "!" + why
    inner = rel_pos[1] if isinstance(rel_pos, tuple) and len(rel_pos) == 2 else None
    if not chunkwise_recurrent or not (isinstance(inner, tuple) and inner[0] == "chunk"):
        return "!only the chunkwise form runs natively"
    if inner[1] != RET_CHUNK:
        return f"!the chunk size must be {RET_CHUNK} (got {inner[1]})"
    if rope is not False:
        return f"!rope must be False (got {rope!r})"
    if u.dim() != 3 or u.shape[-1] != 96:
        return f"!input must be [B F,T,96], got {tuple(u.shape)}"
    if u.dtype != torch.float32 and _stream_dtype(u) is None:
        return f"!the stream must be fp32, or bf16 under autocast (got {u.dtype})"
    if not 1 <= u.shape[1] <= RET_T_MAX:
        return f"!1 <= T <= {RET_T_MAX} (got T = {u.shape[1]})"
    return None


class OnlineRetentionFn(torch.autograd.Function):
    """out = SiLU(g) * RMSNorm_head(chunkwise retention(q, k_scale k, v)) through the HIP kernels; inputs (lib, q, k or None, v, g, k_scale, decay).  One
    backward per forward: the saved state is freed by it (retain_graph and double backward are refused)."""

    @staticmethod
    def forward(ctx, lib, q, k, v, g, k_scale, decay):
        q, v, g = q.contiguous(), v.contiguous(), g.contiguous()
        k = None if k is None else k.contiguous()
        out, save = ops.online_ret_train_fwd(lib, q, k, v, g, k_scale, decay, keep=True)
        ctx.lib, ctx.k_scale, ctx.saved, ctx.params, ctx.versions = lib, k_scale, (q, k, v, g, decay, save), (), []
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        ops.graph_guard_check(ctx, "OnlineSpatialNet native retention")
        q, k, v, g, decay, save = ctx.saved
        dq, dk, dv, dg = ops.online_ret_train_bwd(ctx.lib, q, k, v, g, ctx.k_scale, decay, save, d_out.contiguous())
        ctx.saved = None
        return None, dq, dk, dv, dg, None, None


def retention_forward(mhsa, u: Tensor, rel_pos) -> Tensor:
    """MultiScaleRetention.forward(u, rel_pos, chunkwise_recurrent=True, rope=False) for a call `ret_eligible` accepted: the projections and out_proj are the
    module's own nn.Linear's (torch GEMMs, autocast like any other), the core between them is native.  Without autograd the forward runs alone and keeps nothing."""
    lib = active_lib(u)
    if lib is None:
        raise ops.NbssError("OnlineSpatialNet native retention: no library for a tensor on " + str(u.device))
    dt = _stream_dtype(u)
    q = mhsa.q_proj(u).to(dt)
    k = None if mhsa.share_qk else mhsa.k_proj(u).to(dt)
    v, g = mhsa.v_proj(u).to(dt), mhsa.g_proj(u).to(dt)
    decay = rel_pos[1][2].detach().to(device=u.device, dtype=torch.float32).contiguous()
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k, v, g)):
        out = OnlineRetentionFn.apply(lib, q, k, v, g, float(mhsa.scaling), decay)
    else:
        out = ops.online_ret_train_fwd(lib, q.contiguous(), None if k is None else k.contiguous(), v.contiguous(), g.contiguous(), float(mhsa.scaling), decay,
                                       keep=False)[0]
    return mhsa.out_proj(out)


# ---- the cross-band trio (NBSS_ONLINE_NATIVE_XBAND) --------------------------------------------------------------------------------------------------------
XBAND_F_MAX, XBAND_T_MAX, XBAND_T_TRAIN_MAX, XBAND_F_TRAIN_MAX_FP32 = 272, 4096, 256, 160
# (attribute path, tensor) in the order of the C ABI's parameter list = state_dict order
XBAND_SLOTS = (("fconv1", 0, "weight"), ("fconv1", 0, "bias"), ("fconv1", 1, "weight"), ("fconv1", 1, "bias"), ("fconv1", 2, "weight"),
               ("norm_full", None, "weight"), ("norm_full", None, "bias"), ("squeeze", 0, "weight"), ("squeeze", 0, "bias"), ("full", None, "weight"),
               ("full", None, "bias"), ("unsqueeze", 0, "weight"), ("unsqueeze", 0, "bias"),
               ("fconv2", 0, "weight"), ("fconv2", 0, "bias"), ("fconv2", 1, "weight"), ("fconv2", 1, "bias"), ("fconv2", 2, "weight"))


def xband_enabled() -> bool:
    """the cross-band switch, read at call time; off unless it is exactly '1'"""
    return os.environ.get("NBSS_ONLINE_NATIVE_XBAND", "0") == "1"


def xband_params(layer) -> List[Tensor]:
    """the trio's 18 parameters (the module's live tensors; a LinearGroup shared across layers is the same tensor in each) in the order of the C ABI"""
    out = []
    for name, i, a in XBAND_SLOTS:
        m = getattr(layer, name)
        out.append(getattr(m if i is None else m[i], a, None))
    return out


def xband_supported(layer) -> Optional[str]:
    """None when the layer's fconv1 / full-band block / fconv2 are the geometry the kernels are built for (SpatialNet-small's cross-band blocks), else the reason"""
    for name, norm in (("norms[3]", layer.fconv1[0]), ("norms[4]", layer.fconv2[0]), ("norms[5]", layer.norm_full)):
        if type(norm).__name__ != "LayerNorm":
            return f"{name} must be LN (got {type(norm).__name__})"
        if tuple(norm.normalized_shape) != (96,):
            return f"dim_hidden must be 96 (got {norm.normalized_shape[0]})"
        if norm.eps != 1e-5 or norm.weight is None or norm.bias is None:
            return f"{name} must be LayerNorm(eps=1e-5) with weight and bias"
    if layer.dropout_full is not None:
        return "dropout[2] (dropout_full) must be 0"
    sq, usq = layer.squeeze[0], layer.unsqueeze[0]
    if sq.in_channels != 96 or usq.out_channels != 96:
        return f"dim_hidden must be 96 (got {sq.in_channels})"
    if sq.out_channels != 8 or usq.in_channels != 8 or layer.full.num_groups != 8:
        return f"dim_squeeze must be 8 (got {sq.out_channels})"
    if sq.kernel_size[0] != 1 or usq.kernel_size[0] != 1 or sq.bias is None or usq.bias is None:
        return "squeeze and unsqueeze must be 1x1 convolutions with bias"
    if type(layer.squeeze[1]).__name__ != "SiLU" or type(layer.unsqueeze[1]).__name__ != "SiLU":
        return "squeeze and unsqueeze must end in SiLU"
    if layer.full.bias is None:
        return "the LinearGroup must have a bias"
    if layer.full.in_features != layer.full.out_features:
        return "the LinearGroup must be square"
    for ml in (layer.fconv1, layer.fconv2):
        conv, act = ml[1], ml[2]
        if conv.in_channels != 96 or conv.out_channels != 96:
            return f"dim_hidden must be 96 (got {conv.in_channels})"
        if conv.groups != 8:
            return f"the F-convs must have 8 groups (got {conv.groups})"
        if conv.kernel_size[0] != 5 or conv.dilation[0] != 1 or conv.stride[0] != 1:
            return f"the F-conv kernel size must be 5 (got {conv.kernel_size[0]}), without dilation or stride"
        if conv.padding_mode != "zeros" or conv.padding != "same":
            return f"padding must be 'zeros' (got {conv.padding_mode!r})"
        if conv.bias is None:
            return "the F-convs must have a bias"
        if type(act).__name__ != "PReLU" or act.weight.numel() != 96:
            return "the F-conv activation must be a per-channel PReLU"
    return None


def xband_eligible(layer, x: Tensor, state) -> Optional[str]:
    """None when this call of `SpatialNetLayer.forward` takes the native cross-band trio; else why not, with the conventions of `eligible` (a leading '!':
    worth a warning)"""
    if not xband_enabled():
        return "NBSS_ONLINE_NATIVE_XBAND is not 1"
    if state is not None:
        return "streaming call"
    if _LIB_OVERRIDE is None and not x.is_cuda:
        return "not on a HIP device"
    if active_lib(x) is None:
        return "no library for the tensor's device"
    why = xband_supported(layer)
    if why is not None:
        return "!" + why
    if x.dim() != 4 or x.shape[-1] != 96:
        return f"!input must be [B,F,T,96], got {tuple(x.shape)}"
    dt = _stream_dtype(x)
    if dt is None:
        return f"!the stream must be fp32, or bf16 under autocast (got {x.dtype})"
    B, Fq, T = x.shape[:3]
    if Fq != layer.full.in_features:
        return f"!the input has {Fq} frequencies, the LinearGroup {layer.full.in_features}"
    if B < 1 or not 1 <= T <= XBAND_T_MAX or not 1 <= Fq <= XBAND_F_MAX or B * Fq * T * 288 >= 2 ** 31:
        return f"!1 <= T <= {XBAND_T_MAX}, F <= {XBAND_F_MAX} and B F T < 2^31 / 288 (got B = {B}, F = {Fq}, T = {T})"
    if _xband_needs_grad(layer, x) and (T > XBAND_T_TRAIN_MAX or (dt == torch.float32 and Fq > XBAND_F_TRAIN_MAX_FP32)):
        return f"!with gradients T <= {XBAND_T_TRAIN_MAX}, and F <= {XBAND_F_TRAIN_MAX_FP32} in fp32 (got T = {T}, F = {Fq})"
    return None


def _xband_needs_grad(layer, x: Tensor) -> bool:
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in xband_params(layer)))


def _xband_kernel_params(params) -> List[Tensor]:
    """fp32 and contiguous (views where the module's tensors already are: the 1x1 weights [O][I][1] are their matrices as they lie)"""
    return [p.detach().float().contiguous() for p in params]


class OnlineXBandFn(torch.autograd.Function):
    """y = the cross-band trio through the HIP kernels; inputs (lib, x, *the 18 parameters): the parameters are inputs of the node, so p.grad is populated
    the usual way (a LinearGroup shared by several layers is an input of several nodes: autograd sums).  Saved: x and the two block inputs the forward keeps.
    One backward per forward: the saved state is freed by it (retain_graph and double backward are refused)."""

    @staticmethod
    def forward(ctx, lib, x, *params):
        xk = x.contiguous()
        p32 = _xband_kernel_params(params)
        y, save = ops.online_xband_train_fwd(lib, p32, xk, keep=True)
        ctx.lib, ctx.saved, ctx.params = lib, (xk, save, p32), params
        ctx.versions = [p._version for p in params]
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        ops.graph_guard_check(ctx, "OnlineSpatialNet native cross-band blocks")
        xk, save, p32 = ctx.saved
        dx, grads = ops.online_xband_train_bwd(ctx.lib, p32, xk, save, dy.contiguous())
        ctx.saved = None
        out = [g.reshape(p.shape).to(p.dtype) if ctx.needs_input_grad[2 + i] else None for i, (g, p) in enumerate(zip(grads, ctx.params))]
        return (None, dx if ctx.needs_input_grad[1] else None, *out)


def xband_residual(layer, x: Tensor) -> Tensor:
    """x + fconv1, + full, + fconv2 for a call `xband_eligible` accepted; in the dtype of x.  Without autograd (no_grad, or nothing requires a gradient) the
    forward runs alone and keeps nothing."""
    lib = active_lib(x)
    if lib is None:
        raise ops.NbssError("OnlineSpatialNet native cross-band blocks: no library for a tensor on " + str(x.device))
    params = xband_params(layer)
    xs = x.to(_stream_dtype(x))
    if _xband_needs_grad(layer, x):
        y = OnlineXBandFn.apply(lib, xs, *params)
    else:
        with torch.no_grad():
            y = ops.online_xband_train_fwd(lib, _xband_kernel_params(params), xs.contiguous(), keep=False)[0]
    return y.to(x.dtype)
