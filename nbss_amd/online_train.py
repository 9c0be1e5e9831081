"""Native training paths of the OnlineSpatialNet's blocks, each behind an opt-in switch of its own (off unless exactly '1', read at call time,
independent of the others):

    TCONVFFN   NBSS_ONLINE_NATIVE_TRAIN   csrc/online_train.hip        x + causal T-ConvFFN(x) on the [B,F,T,96] stream        OnlineTConvFFNFn
    RETENTION  NBSS_ONLINE_NATIVE_RET     csrc/online_ret_train.hip    the chunkwise retention core between the projections    OnlineRetentionFn
    XBAND      NBSS_ONLINE_NATIVE_XBAND   csrc/online_xband_train.hip  x + fconv1, + full-band, + fconv2 as one node           OnlineXBandFn
    TSA        NBSS_ONLINE_NATIVE_TSA     csrc/online_tsa_train.hip    x + the whole retention block (LayerNorm, the four      OnlineTSAFn
                                                                       projections, the core, out_proj) as one node
    MAMBA      NBSS_ONLINE_NATIVE_MAMBA   csrc/online_mamba_train.hip  the core of a Mamba block between in_proj and out_proj  OnlineMambaFn
                                                                       (conv, SiLU, x_proj, dt_proj + softplus, the selective
                                                                       scan, the D skip, the gate) as one node

A block is one `Block` record: its switch, its label, its `supported` and the checks of the call.  Everything else is written once.  `take` is what
`models.arch.OnlineSpatialNet.SpatialNetLayer` asks per call: the common gate (`_gate`: switch, streaming call, device, library, geometry, stream dtype — fp32,
or bf16 under autocast), then the block's checks, then one warning when the switch is on and the layer or call does not fit (a reason that starts with '!');
every other refusal is an ordinary torch.nn case.  The three blocks of the form y = x + block(x) with N parameter inputs share one autograd Function body
(`_residual_fn`) and one driver (`_residual`); the retention core alone (RETENTION) has inputs of its own (q, k, v, g) and keeps its Function, with the
module's nn.Linear projections around it; where both TSA and RETENTION accept a call, TSA takes it.  MAMBA (the 'mamba(16,4)' variant, which itself is
behind NBSS_ONLINE_MAMBA=1 at construction: models/arch/OnlineSpatialNet.py) is asked per Mamba module, not per layer: its node has the inputs (xz, the seven
parameters of the core) and the module's in_proj / out_proj stay torch GEMMs around it (`mamba_forward`); the backward recomputes the states from checkpoints
every MAMBA_CKPT frames.  `_residual` and `mamba_forward` both stand on `_node`: the autograd node, or without autograd (no_grad, or nothing requires a
gradient) the forward entry alone under no_grad, which keeps nothing.  With TCONVFFN, TSA and XBAND on, a 'ret(2)' training layer is three native nodes and no torch op."""
from __future__ import annotations

import contextlib
import functools
import os
from dataclasses import dataclass
from typing import Callable, List, Optional

import torch
from torch import Tensor

from . import ops
from ._lib import Lib, hip

TCONVFFN_T_MAX, TCONVFFN_F_MAX = 4096, 272
RET_CHUNK, RET_T_MAX = 64, 4096
MAMBA_CKPT, MAMBA_T_MAX, MAMBA_GRID_CAP = 8, 4096, 512  # (csrc/online_mamba_train.hip: MB_CKPT, NBSS_T_MAX, MB_GRID_CAP)
XBAND_F_MAX, XBAND_T_MAX, XBAND_T_TRAIN_MAX, XBAND_F_TRAIN_MAX_FP32 = 272, 4096, 256, 160
# (module index in layer.tconvffn, attribute) in the order of the C ABI's parameter list
PARAM_SLOTS = ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias"), (3, "weight"), (3, "bias"), (5, "weight"), (5, "bias"), (6, "weight"), (6, "bias"),
               (8, "weight"), (8, "bias"), (10, "weight"), (10, "bias"))
# (attribute path, tensor) in the order of the C ABI's parameter list = state_dict order
XBAND_SLOTS = (("fconv1", 0, "weight"), ("fconv1", 0, "bias"), ("fconv1", 1, "weight"), ("fconv1", 1, "bias"), ("fconv1", 2, "weight"),
               ("norm_full", None, "weight"), ("norm_full", None, "bias"), ("squeeze", 0, "weight"), ("squeeze", 0, "bias"), ("full", None, "weight"),
               ("full", None, "bias"), ("unsqueeze", 0, "weight"), ("unsqueeze", 0, "bias"),
               ("fconv2", 0, "weight"), ("fconv2", 0, "bias"), ("fconv2", 1, "weight"), ("fconv2", 1, "bias"), ("fconv2", 2, "weight"))

_LIB_OVERRIDE: Optional[Lib] = None


@contextlib.contextmanager
def use_lib(lib: Lib):
    """tests only: run the blocks through `lib` — the host-emulator build takes CPU tensors, so the module path can be exercised without a device"""
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


# ---- what the kernels are built for ------------------------------------------------------------------------------------------------------------------------
def supported(layer) -> Optional[str]:
    """None when the layer's T-ConvFFN is the geometry the kernels are built for (the checks of nbss_amd/online.py::supported that concern this block),
    else the reason"""
    from models.arch.OnlineSpatialNet import CausalConv1d
    tc = layer.tconvffn
    if not isinstance(tc, torch.nn.ModuleList):
        return f"the T-ConvFFN must be the ModuleList of the mhsa / ret variants (got {type(tc).__name__})"
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


def tsa_supported(layer) -> Optional[str]:
    """None when the layer's norm_mhsa, retention and dropout are what the whole-block kernels are built for, else the reason"""
    why = ret_supported(layer.mhsa)
    if why is not None:
        return why
    norm, mhsa = layer.norm_mhsa, layer.mhsa
    if type(norm).__name__ != "LayerNorm" or tuple(norm.normalized_shape) != (96,) or norm.eps != 1e-5 or norm.weight is None or norm.bias is None:
        return "norms[0] (norm_mhsa) must be LayerNorm(96, eps=1e-5) with weight and bias"
    if any(lin is not None and lin.bias is not None for lin in (mhsa.q_proj, mhsa.k_proj, mhsa.v_proj, mhsa.g_proj, mhsa.out_proj)):
        return "the projections must have no bias"
    if (mhsa.k_proj is None) != bool(mhsa.share_qk):
        return "k_proj must be absent exactly with share_qk"
    if layer.dropout_mhsa.p > 0:
        return "dropout[0] (dropout_mhsa) must be 0"
    return None


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


def mamba_supported(mamba) -> Optional[str]:
    """None when the module is the Mamba the kernels are built for (OnlineSpatialNet's 'mamba(16,4)' at width 96), else the reason"""
    if type(mamba).__name__ != "Mamba":
        return f"the block must be Mamba (got {type(mamba).__name__})"
    if mamba.d_model != 96 or mamba.d_inner != 192:
        return f"d_model must be 96 and expand 2 (got {mamba.d_model}, {mamba.expand})"
    if mamba.d_state != 16:
        return f"d_state must be 16 (got {mamba.d_state})"
    if mamba.d_conv != 4:
        return f"d_conv must be 4 (got {mamba.d_conv})"
    if mamba.dt_rank != 6:
        return f"dt_rank must be 6 (got {mamba.dt_rank})"
    if mamba.in_proj.bias is not None or mamba.x_proj.bias is not None or mamba.out_proj.bias is not None:
        return "in_proj, x_proj and out_proj must have no bias"
    if mamba.conv1d.bias is None or mamba.dt_proj.bias is None:
        return "conv1d and dt_proj must have a bias"
    return None


def mamba_params(mamba, *_) -> List[Tensor]:
    """the seven parameters of the core (the module's live tensors) in the order of the C ABI"""
    return [mamba.conv1d.weight, mamba.conv1d.bias, mamba.x_proj.weight, mamba.dt_proj.weight, mamba.dt_proj.bias, mamba.A_log, mamba.D]


def tconvffn_params(layer) -> List[Tensor]:
    """the block's 14 parameters (the module's live tensors) in the order of the C ABI"""
    return [getattr(layer.tconvffn[i], a) for i, a in PARAM_SLOTS]


def xband_params(layer) -> List[Tensor]:
    """the trio's 18 parameters (the module's live tensors; a LinearGroup shared across layers is the same tensor in each) in the order of the C ABI"""
    out = []
    for name, i, a in XBAND_SLOTS:
        m = getattr(layer, name)
        out.append(getattr(m if i is None else m[i], a, None))
    return out


def tsa_params(layer, rel_pos, *_) -> List[Optional[Tensor]]:
    """the retention block's seven parameters (the module's live tensors; None at k_proj with share_qk) in the order of the C ABI, then the per-head decay
    of this call's `rel_pos` (fp32 on the parameters' device; a constant)"""
    m = layer.mhsa
    decay = rel_pos[1][2].detach().to(device=m.q_proj.weight.device, dtype=torch.float32).contiguous()
    return [layer.norm_mhsa.weight, layer.norm_mhsa.bias, m.q_proj.weight, None if m.k_proj is None else m.k_proj.weight, m.v_proj.weight, m.g_proj.weight,
            m.out_proj.weight, decay]


# ---- the checks of one call, after the common gate (a reason starts with '!': the switch is on and the call does not fit) ---------------------------------
def _tconvffn_call(layer, x: Tensor) -> Optional[str]:
    if x.dim() != 4 or x.shape[-1] != 96:
        return f"!input must be [B,F,T,96], got {tuple(x.shape)}"
    if not 1 <= x.shape[2] <= TCONVFFN_T_MAX or x.shape[1] > TCONVFFN_F_MAX:
        return f"!1 <= T <= {TCONVFFN_T_MAX} and F <= {TCONVFFN_F_MAX} (got T = {x.shape[2]}, F = {x.shape[1]})"
    return None


def _ret_call(layer, u: Tensor, rel_pos, chunkwise_recurrent: bool, rope) -> Optional[str]:
    inner = rel_pos[1] if isinstance(rel_pos, tuple) and len(rel_pos) == 2 else None
    if not chunkwise_recurrent or not (isinstance(inner, tuple) and inner[0] == "chunk"):
        return "!only the chunkwise form runs natively"
    if inner[1] != RET_CHUNK:
        return f"!the chunk size must be {RET_CHUNK} (got {inner[1]})"
    if rope is not False:
        return f"!rope must be False (got {rope!r})"
    if u.dim() != 3 or u.shape[-1] != 96:
        return f"!input must be [B F,T,96], got {tuple(u.shape)}"
    if not 1 <= u.shape[1] <= RET_T_MAX:
        return f"!1 <= T <= {RET_T_MAX} (got T = {u.shape[1]})"
    return None


def _tsa_call(layer, x: Tensor, rel_pos, chunkwise_recurrent: bool, rope) -> Optional[str]:
    if x.dim() != 4 or x.shape[0] < 1:
        return f"!input must be [B,F,T,96], got {tuple(x.shape)}"
    return _ret_call(layer, x[0], rel_pos, chunkwise_recurrent, rope)  # (a view [F,T,96]: the checks read T and the width)


def _xband_call(layer, x: Tensor) -> Optional[str]:
    if x.dim() != 4 or x.shape[-1] != 96:
        return f"!input must be [B,F,T,96], got {tuple(x.shape)}"
    B, Fq, T = x.shape[:3]
    if Fq != layer.full.in_features:
        return f"!the input has {Fq} frequencies, the LinearGroup {layer.full.in_features}"
    if B < 1 or not 1 <= T <= XBAND_T_MAX or not 1 <= Fq <= XBAND_F_MAX or B * Fq * T * 288 >= 2 ** 31:
        return f"!1 <= T <= {XBAND_T_MAX}, F <= {XBAND_F_MAX} and B F T < 2^31 / 288 (got B = {B}, F = {Fq}, T = {T})"
    if _needs_grad(x, xband_params(layer)) and (T > XBAND_T_TRAIN_MAX or (_stream_dtype(x) == torch.float32 and Fq > XBAND_F_TRAIN_MAX_FP32)):
        return f"!with gradients T <= {XBAND_T_TRAIN_MAX}, and F <= {XBAND_F_TRAIN_MAX_FP32} in fp32 (got T = {T}, F = {Fq})"
    return None


def _mamba_call(mamba, u: Tensor) -> Optional[str]:
    if u.dim() != 3 or u.shape[-1] != 96:
        return f"!input must be [B F,T,96], got {tuple(u.shape)}"
    if u.shape[0] < 1 or not 1 <= u.shape[1] <= MAMBA_T_MAX:
        return f"!1 <= T <= {MAMBA_T_MAX} (got T = {u.shape[1]})"
    return None


@dataclass(frozen=True)
class Block:
    """one natively trainable block of a SpatialNetLayer (MAMBA: `layer` is the Mamba module itself, a layer has up to two)"""
    switch: str  # the environment variable that turns it on
    what: str  # in warnings "OnlineSpatialNet <what>", in errors "OnlineSpatialNet native <what>"
    supported: Callable  # (layer) -> None, or why the layer is not what the kernels are built for
    call: Callable  # (layer, x, *what the call adds) -> None, or '!' and why this call does not fit
    streaming: str = "streaming call"  # the reason given to a call that carries a state
    # the y = x + block(x) form only:
    params: Optional[Callable] = None  # (layer, *what the call adds) -> the parameter inputs in the order of the C ABI (None: an absent one)
    entry: Optional[str] = None  # ops.<entry>_fwd / ops.<entry>_bwd (looked up at call time)

    @property
    def native(self) -> str:
        return "OnlineSpatialNet native " + self.what


TCONVFFN = Block("NBSS_ONLINE_NATIVE_TRAIN", "T-ConvFFN", supported, _tconvffn_call, params=tconvffn_params, entry="online_tconvffn_train")
RETENTION = Block("NBSS_ONLINE_NATIVE_RET", "retention", lambda layer: ret_supported(layer.mhsa), _ret_call, streaming="streaming or recurrent call")
XBAND = Block("NBSS_ONLINE_NATIVE_XBAND", "cross-band blocks", xband_supported, _xband_call, params=xband_params, entry="online_xband_train")
TSA = Block("NBSS_ONLINE_NATIVE_TSA", "retention block", tsa_supported, _tsa_call, streaming="streaming or recurrent call", params=tsa_params,
            entry="online_tsa_train")
MAMBA = Block("NBSS_ONLINE_NATIVE_MAMBA", "Mamba core", mamba_supported, _mamba_call, streaming="streaming or inference call", params=mamba_params,
              entry="online_mamba_train")


# ---- the scaffold: written once for the five blocks -------------------------------------------------------------------------------------------------------
def _on(block: Block) -> bool:
    return os.environ.get(block.switch, "0") == "1"


# the switches, read at call time (like NBSS_NBC2_NATIVE); each off unless it is exactly '1'
enabled, ret_enabled, xband_enabled, tsa_enabled, mamba_enabled = (functools.partial(_on, b) for b in (TCONVFFN, RETENTION, XBAND, TSA, MAMBA))


def _stream_dtype(x: Tensor) -> Optional[torch.dtype]:
    dev = "cuda" if x.is_cuda else "cpu"
    if torch.is_autocast_enabled(dev):
        return torch.bfloat16 if torch.get_autocast_dtype(dev) == torch.bfloat16 else None
    return torch.float32 if x.dtype == torch.float32 else None


def _needs_grad(x, params=()) -> bool:
    """whether autograd will ask for a gradient of the tensor (or tensors, None allowed) `x` or of a parameter"""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ((x,) if isinstance(x, Tensor) else tuple(x)) + tuple(params))


def _gate(block: Block, layer, x: Tensor, streaming: bool, *call) -> Optional[str]:
    """None when this call takes the native block; else why not.  A reason that starts with '!' is worth a warning (the switch is on, the tensor is on the
    library's device, and the layer, dtype or call does not fit); the others are the ordinary torch.nn cases."""
    if not _on(block):
        return f"{block.switch} is not 1"
    if streaming:
        return block.streaming
    if _LIB_OVERRIDE is None and not x.is_cuda:
        return "not on a HIP device"
    if active_lib(x) is None:
        return "no library for the tensor's device"
    why = block.supported(layer)
    if why is not None:
        return "!" + why
    if _stream_dtype(x) is None:
        return f"!the stream must be fp32, or bf16 under autocast (got {x.dtype})"
    return block.call(layer, x, *call)


def eligible(layer, x: Tensor, state) -> Optional[str]:
    """`_gate` for the T-ConvFFN of a call of `SpatialNetLayer._tconvffn`"""
    return _gate(TCONVFFN, layer, x, state is not None)


def ret_eligible(layer, u: Tensor, rel_pos, chunkwise_recurrent: bool, rope, state, inference: bool) -> Optional[str]:
    """`_gate` for the retention core of a call of `SpatialNetLayer._tsa`"""
    return _gate(RETENTION, layer, u, state is not None or inference, rel_pos, chunkwise_recurrent, rope)


def tsa_eligible(layer, x: Tensor, rel_pos, chunkwise_recurrent: bool, rope, state, inference: bool) -> Optional[str]:
    """`_gate` for the whole retention block of a call of `SpatialNetLayer.forward`"""
    return _gate(TSA, layer, x, state is not None or inference, rel_pos, chunkwise_recurrent, rope)


def mamba_eligible(mamba, u: Tensor, state, inference: bool) -> Optional[str]:
    """`_gate` for the core of one Mamba of a call of `SpatialNetLayer._mamba`"""
    return _gate(MAMBA, mamba, u, state is not None or inference)


def xband_eligible(layer, x: Tensor, state) -> Optional[str]:
    """`_gate` for the cross-band trio of a call of `SpatialNetLayer._xband`"""
    return _gate(XBAND, layer, x, state is not None)


def take(block: Block, layer, x: Tensor, streaming: bool, *call) -> bool:
    """whether this call of a SpatialNetLayer method takes the native block; with the switch on and a layer or call that does not fit, one warning per layer
    and reason, which points at the caller of that method"""
    why = _gate(block, layer, x, streaming, *call)
    if why is not None and why.startswith("!"):
        from models.arch.base.native import torch_path_note
        torch_path_note(layer, "OnlineSpatialNet " + block.what, why[1:], stacklevel=4)
    return why is None


def _lib_for(block: Block, x: Tensor) -> Lib:
    lib = active_lib(x)
    if lib is None:
        raise ops.NbssError(f"{block.native}: no library for a tensor on {x.device}")
    return lib


def _kernel_params(params) -> List[Optional[Tensor]]:
    """fp32 and contiguous (views where the module's tensors already are: the 1x1 weights [O][I][1] are their matrices as they lie); None stays None"""
    return [None if p is None else p.detach().float().contiguous() for p in params]


_xband_kernel_params = _kernel_params  # (the name tests/test_online_xband_train.py calls it by)


def _residual_fn(name: str, block: Block, doc: str):
    """the autograd Function `name` of y = x + block(x) through the HIP kernels; inputs (lib, x, *the block's parameters): the parameters are inputs of the
    node, so p.grad is populated the usual way.  One backward per forward: the saved state is freed by it (retain_graph and double backward are refused)."""

    def forward(ctx, lib, x, *params):
        xk = x.contiguous()
        p32 = _kernel_params(params)
        y, save = getattr(ops, block.entry + "_fwd")(lib, p32, xk, keep=True)
        ctx.lib, ctx.saved, ctx.inputs = lib, (xk, save, p32), params
        ctx.params = [p for p in params if p is not None]  # (what ops.graph_guard_check watches)
        ctx.versions = [p._version for p in ctx.params]
        return y

    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        ops.graph_guard_check(ctx, block.native)
        xk, save, p32 = ctx.saved
        dx, grads = getattr(ops, block.entry + "_bwd")(ctx.lib, p32, xk, save, dy.contiguous())
        ctx.saved = None
        out = [g.reshape(p.shape).to(p.dtype) if ctx.needs_input_grad[2 + i] else None for i, (g, p) in enumerate(zip(grads, ctx.inputs))]
        return (None, dx if ctx.needs_input_grad[1] else None, *out)

    return type(name, (torch.autograd.Function,), {"forward": staticmethod(forward), "backward": staticmethod(backward), "__doc__": doc,
                                                   "__module__": __name__})


OnlineTConvFFNFn = _residual_fn("OnlineTConvFFNFn", TCONVFFN, "y = x + T-ConvFFN(x); inputs (lib, x, *the 14 parameters).  Saved: x and the kernels' activations.")
OnlineXBandFn = _residual_fn("OnlineXBandFn", XBAND, "y = the cross-band trio; inputs (lib, x, *the 18 parameters) (a LinearGroup shared by several layers is an "
                             "input of several nodes: autograd sums).  Saved: x and the two block inputs the forward keeps.")
OnlineTSAFn = _residual_fn("OnlineTSAFn", TSA, "y = x + out_proj(SiLU(g) * RMSNorm_head(chunk_retention(q, k, v))) on LayerNorm(x); inputs (lib, x, ln.weight, "
                           "ln.bias, q_proj, k_proj or None, v_proj, g_proj, out_proj, decay).  Saved: x, q, k, v, g, the gated core output, the row statistics "
                           "and the core's chunk states.")


# (not a residual form, but the same shape of node: inputs (lib, xz, *parameters), one saved blob, every gradient from one backward entry)
OnlineMambaFn = _residual_fn("OnlineMambaFn", MAMBA, "out = y * SiLU(z) of a Mamba block on xz = in_proj(u); inputs (lib, xz, conv1d.weight, conv1d.bias, "
                             "x_proj.weight, dt_proj.weight, dt_proj.bias, A_log, D).  Saved: xz, the x_proj rows (dt_r, B, C) and the state h every "
                             "MAMBA_CKPT frames; the backward recomputes the states of an interval from its checkpoint.")


def _node(block: Block, fn, x: Tensor, params) -> Tensor:
    """the block's node `fn` on x (in the stream dtype already); without autograd (no_grad, or nothing requires a gradient) the forward entry alone,
    which keeps nothing"""
    lib = _lib_for(block, x)
    if _needs_grad(x, params):
        return fn.apply(lib, x, *params)
    with torch.no_grad():
        return getattr(ops, block.entry + "_fwd")(lib, _kernel_params(params), x.contiguous(), keep=False)[0]


def _residual(block: Block, fn, layer, x: Tensor, *call) -> Tensor:
    """x + block(x) for a call the gate accepted (`call`: what the call adds, as `take` got it); in the dtype of x.  Without autograd (no_grad, or nothing
    requires a gradient) the forward runs alone and keeps nothing."""
    return _node(block, fn, x.to(_stream_dtype(x)), block.params(layer, *call)).to(x.dtype)


# x + T-ConvFFN(x) for a call `eligible` accepted, and x + fconv1, + full, + fconv2 for a call `xband_eligible` accepted: (layer, x) -> y;
# x + the retention block for a call `tsa_eligible` accepted: (layer, x, rel_pos) -> y
tconvffn_residual = functools.partial(_residual, TCONVFFN, OnlineTConvFFNFn)
xband_residual = functools.partial(_residual, XBAND, OnlineXBandFn)
tsa_residual = functools.partial(_residual, TSA, OnlineTSAFn)


def mamba_forward(mamba, u: Tensor) -> Tensor:
    """Mamba.forward(u) for a call `mamba_eligible` accepted: in_proj and out_proj are the module's own nn.Linear's (torch GEMMs, autocast like any other),
    the core between them is native.  Without autograd the forward runs alone and keeps nothing."""
    return mamba.out_proj(_node(MAMBA, OnlineMambaFn, mamba.in_proj(u).to(_stream_dtype(u)), mamba_params(mamba)))


class OnlineRetentionFn(torch.autograd.Function):
    """out = SiLU(g) * RMSNorm_head(chunkwise retention(q, k_scale k, v)) through the HIP kernels; inputs (lib, q, k or None, v, g, k_scale, decay).  One
    backward per forward: the saved state is freed by it (retain_graph and double backward are refused)."""

    @staticmethod
    def forward(ctx, lib, q, k, v, g, k_scale, decay):
        q, v, g = q.contiguous(), v.contiguous(), g.contiguous()
        k = None if k is None else k.contiguous()
        out, save = ops.online_ret_train_fwd(lib, q, k, v, g, k_scale, decay, keep=True)
        ctx.lib, ctx.k_scale, ctx.saved = lib, k_scale, (q, k, v, g, decay, save)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        ops.graph_guard_check(ctx, RETENTION.native)
        q, k, v, g, decay, save = ctx.saved
        dq, dk, dv, dg = ops.online_ret_train_bwd(ctx.lib, q, k, v, g, ctx.k_scale, decay, save, d_out.contiguous())
        ctx.saved = None
        return None, dq, dk, dv, dg, None, None


def retention_forward(mhsa, u: Tensor, rel_pos) -> Tensor:
    """MultiScaleRetention.forward(u, rel_pos, chunkwise_recurrent=True, rope=False) for a call `ret_eligible` accepted: the projections and out_proj are the
    module's own nn.Linear's (torch GEMMs, autocast like any other), the core between them is native.  Without autograd the forward runs alone and keeps nothing."""
    lib = _lib_for(RETENTION, u)
    dt = _stream_dtype(u)
    q = mhsa.q_proj(u).to(dt)
    k = None if mhsa.share_qk else mhsa.k_proj(u).to(dt)
    v, g = mhsa.v_proj(u).to(dt), mhsa.g_proj(u).to(dt)
    decay = rel_pos[1][2].detach().to(device=u.device, dtype=torch.float32).contiguous()
    if _needs_grad((q, k, v, g)):
        out = OnlineRetentionFn.apply(lib, q, k, v, g, float(mhsa.scaling), decay)
    else:
        with torch.no_grad():
            out = ops.online_ret_train_fwd(lib, q.contiguous(), None if k is None else k.contiguous(), v.contiguous(), g.contiguous(), float(mhsa.scaling),
                                           decay, keep=False)[0]
    return mhsa.out_proj(out)
