"""Native streaming step of an OnlineSpatialNet (BASELINE config 5): the HIP kernels of csrc/online.hip for the
narrow-band halves (causal encoder, recurrent multi-scale retention, causal T-ConvFFN with its per-frame cross-frequency GroupNorm) and the
existing cross-band kernels (nbss_fconv_fwd / nbss_full_fwd) and decoder, on a chunk of C frames with all state in pre-allocated device
buffers — a fixed launch sequence that is captured once into a HIP graph and replayed per chunk.

`NativeOnlineStreamer(net, batch, chunk)` has the interface of models.arch.OnlineSpatialNet.OnlineStreamer (step / reset / graph) and serves
the geometry the kernels are built for: attention 'ret(F, share_qk | not_share_qk)' with value factor 2 and no rotary positions, or causal windowed
attention 'mhsa(N)' over a K / V ring, or — opt-in, NBSS_ONLINE_NATIVE_MAMBA_STEP=1, read by `supported` on every call, else refused with a reason that
names the switch — 'mamba(16,4)' / 'mamba(16,4,not_replace_ffn)': one nbss_online_mamba_step (csrc/online_mamba_step.hip) per Mamba block; dim_hidden 96,
dim_ffn 192, dim_squeeze 8, 4 heads, kernel sizes (5, 3), conv groups (8, 8), encoder kernel 5, norms LN/LN/GN/LN/LN/LN; everything else
raises NotImplementedError (callers fall back to OnlineStreamer, the torch.nn step).

A layer's two narrow-band steps are a pair of `Step` records, `layer_kinds(layer)` = (RET | MHSA | MAMBA, TCONVFFN | MAMBA): one record per C entry point
holds its argument list (leading integers, weights, then constants / state / scratch, all in ABI order), the buffers it owns and its part of `supported`;
the streamer walks the pair and knows no variant by name.  A further step kind is one more record."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import torch
from torch import Tensor

from models.arch.OnlineSpatialNet import GraphedStep

from . import ops
from ._lib import NBSS_F32, Lib, hip, make_cfg


MAMBA_STEP_SWITCH = "NBSS_ONLINE_NATIVE_MAMBA_STEP"
SLOTS = (("mhsa", "norm_mhsa"), ("tconvffn", "norm_tconvffn"))  # a layer's two steps: the module, and the norm in front of it (a T-ConvFFN holds its own)


def _zeros(s, *shape, dtype=torch.float32) -> Tensor:
    return torch.zeros(*shape, dtype=dtype, device=s.dev)


def _is_mamba(m) -> bool:
    return type(m).__name__ == "Mamba"


@dataclass(frozen=True)
class Step:
    """one narrow-band step kind = one C entry point `entry(*ints, *weights, *tail, h, stream)`; `s` is the streamer, `q` / `ln` a slot's two names"""
    entry: str
    ints: Callable  # (s) -> the leading integers
    weights: Callable  # (fp32 state_dict, 'layers.<l>.<q>.', 'layers.<l>.<ln>.') -> the weight arguments (None: a null pointer)
    state: Callable  # (s) -> {name: zeros}: the state one layer owns
    tail: Tuple[str, ...]  # what follows the weights: names of `state` and `shared`
    check: Callable = lambda net, layer, q: None  # (net, layer, q) -> why not, asked first and of every layer
    shared: Callable = lambda s: {}  # (s) -> {name: tensor}: what all layers pass (constants, scratch, and state when named in `rewound`)
    rewound: Tuple[str, ...] = ()  # the names of `shared` that are state: reset() and the capture's rewind cover them
    geometry: Callable = lambda l0: None  # (layers[0]) -> why not, asked after the gate's own geometry
    norms: Callable = lambda l0, ln: [getattr(l0, ln)]  # (layers[0], ln) -> its norm modules ...
    norm_kinds: Tuple[str, ...] = ("LayerNorm",)  # ... and what they must be
    after: Optional[Callable] = None  # (s, ptr, stream): a launch after the last layer


def _ret_check(net, layer, q) -> Optional[str]:
    from models.arch.base.retention import MultiScaleRetention, RetNetRelPos
    r = net.layers[0].mhsa
    if not isinstance(getattr(net, "pos", None), RetNetRelPos) or net.rope is not False:
        return "attention must be 'mhsa(N)' or retention without rotary positions ('ret(2)' with rope: false)"
    if not isinstance(r, MultiScaleRetention) or (r.embed_dim, r.value_dim, r.num_heads, r.look_ahead) != (96, 192, 4, 0):
        return "retention geometry must be embed 96, value 192 (factor 2), 4 heads, no look-ahead"
    return None


def _mhsa_check(net, layer, q) -> Optional[str]:
    import math
    r = net.layers[0].mhsa
    if net.rope is not False or getattr(net, "attn_scope", math.inf) is math.inf or net.attn_scope > 4096:
        return "windowed attention needs a finite window 'mhsa(N)' (N <= 4096) and no ALiBi / rotary positions"
    if (r.embed_dim, r.num_heads) != (96, 4) or r.in_proj_bias is None:
        return "attention geometry must be embed 96, 4 heads, with biases"
    return None


def _mamba_check(net, layer, q) -> Optional[str]:
    if os.environ.get(MAMBA_STEP_SWITCH, "0") != "1":  # read per call; off unless exactly '1'
        return (f"the 'mamba(..)' variant streams natively only with {MAMBA_STEP_SWITCH}=1 (opt-in like every native Mamba path: the project's Mamba stands in "
                "for mamba_ssm, parity not pinned); without it OnlineStreamer walks the module's step form")
    from .online_train import mamba_supported
    if _is_mamba(layer.tconvffn) != _is_mamba(net.layers[0].tconvffn):
        return "every layer must replace its T-ConvFFN by a Mamba, or none"
    why = mamba_supported(getattr(layer, q))
    return None if why is None else "mamba: " + why


def _tconvffn_geometry(l0) -> Optional[str]:
    if l0.tconvffn[1].out_channels != 192:
        return "geometry must be encoder kernel 5, dim_squeeze 8, dim_ffn 192"
    if l0.tconvffn[3].kernel_size[0] != 3 or l0.tconvffn[3].groups != 8:
        return "kernel sizes (5, 3) and conv groups (8, 8)"
    return None


def _ring(s) -> int:
    return int(s.net.attn_scope) - 1 + s.C  # the last scope - 1 frames and the chunk's


RET = Step(
    entry="nbss_online_ret_step", ints=lambda s: (s.B * s.F, s.C),
    weights=lambda sd, q, ln: [sd[ln + "weight"], sd[ln + "bias"], sd[q + "q_proj.weight"].t(), sd[q + "k_proj.weight"].t() if q + "k_proj.weight" in sd else None,
                               sd[q + "v_proj.weight"].t(), sd[q + "g_proj.weight"].t(), sd[q + "out_proj.weight"].t()],
    state=lambda s: {"kv": _zeros(s, s.B * s.F, 4, 24, 48), "scale": _zeros(s, s.B * s.F, 4)}, tail=("decay", "kv", "scale"), check=_ret_check,
    shared=lambda s: {"decay": s.net.pos.decay.detach().float().exp().contiguous().to(s.dev)})
MHSA = Step(  # K / V rings per layer, one device-side frame counter for the stream: advanced once per step, after the layers
    entry="nbss_online_mhsa_step", ints=lambda s: (s.B * s.F, s.C, int(s.net.attn_scope), _ring(s)),
    weights=lambda sd, q, ln: [sd[ln + "weight"], sd[ln + "bias"], sd[q + "in_proj_weight"].t(), sd[q + "in_proj_bias"], sd[q + "out_proj.weight"].t(), sd[q + "out_proj.bias"]],
    state=lambda s: {"kring": _zeros(s, s.B * s.F, _ring(s), 96), "vring": _zeros(s, s.B * s.F, _ring(s), 96)}, tail=("kring", "vring", "pos"), check=_mhsa_check,
    shared=lambda s: {"pos": _zeros(s, 1, dtype=torch.int32)}, rewound=("pos",),
    after=lambda s, ptr, st: s.lib.call("nbss_online_advance", ptr(s.shared["pos"]), s.C, st))
MAMBA = Step(  # in either slot; state: the convolution's last three inputs [BF][3][192] and h [BF][16][192] (Mamba.init_state's tensors, transposed)
    entry="nbss_online_mamba_step", ints=lambda s: (s.B * s.F, s.C),
    weights=lambda sd, q, ln: [sd[ln + "weight"], sd[ln + "bias"], sd[q + "in_proj.weight"].t(), sd[q + "conv1d.weight"][:, 0], sd[q + "conv1d.bias"], sd[q + "x_proj.weight"].t(),
                               sd[q + "dt_proj.weight"], sd[q + "dt_proj.bias"], sd[q + "A_log"], sd[q + "D"], sd[q + "out_proj.weight"].t()],
    state=lambda s: {"conv": _zeros(s, s.B * s.F, 3, 192), "ssm": _zeros(s, s.B * s.F, 16, 192)}, tail=("conv", "ssm"), check=_mamba_check)
TCONVFFN = Step(  # scratch: a3, and the GroupNorm sums [B] + per-frequency partials [B*F] (fixed-order fold)
    entry="nbss_online_tconvffn_step", ints=lambda s: (s.B, s.F, s.C),
    weights=lambda sd, q, ln: [sd[q + "0.weight"], sd[q + "0.bias"], sd[q + "1.weight"][:, :, 0].t(), sd[q + "1.bias"], sd[q + "3.weight"], sd[q + "3.bias"], sd[q + "5.weight"],
                               sd[q + "5.bias"], sd[q + "6.weight"], sd[q + "6.bias"], sd[q + "8.weight"], sd[q + "8.bias"], sd[q + "10.weight"][:, :, 0].t(), sd[q + "10.bias"]],
    state=lambda s: {n: _zeros(s, s.B * s.F, 2, 192) for n in ("s1", "s2", "s3")}, tail=("s1", "s2", "s3", "a3", "gn_sums"),
    shared=lambda s: {"a3": _zeros(s, s.B * s.F, s.C, 192), "gn_sums": _zeros(s, s.B + s.B * s.F, s.C, 8, 2)},
    geometry=_tconvffn_geometry, norms=lambda l0, ln: [l0.tconvffn[0], l0.tconvffn[6]], norm_kinds=("LayerNorm", "GroupNorm"))


def layer_kinds(layer) -> Tuple[Step, Step]:
    """(the attention's step kind, the FFN's); a Mamba in the T-ConvFFN's place asks for one in the attention's"""
    ffn = MAMBA if _is_mamba(layer.tconvffn) else TCONVFFN
    return (MAMBA if _is_mamba(layer.mhsa) or ffn is MAMBA else MHSA if isinstance(layer.mhsa, torch.nn.MultiheadAttention) else RET), ffn


def supported(net) -> Optional[str]:
    """None when `net` fits the native step, else the reason: each step kind's checks, around what is common to all"""
    l0 = net.layers[0]
    slots = list(zip(layer_kinds(l0), SLOTS))
    for layer in net.layers:
        for kind, (q, _) in slots:
            why = kind.check(net, layer, q)
            if why is not None:
                return why
    if net.encoder.kernel_size[0] != 5 or net.encoder.in_channels > 32 or l0.squeeze[0].out_channels != 8:
        return "geometry must be encoder kernel 5, dim_squeeze 8, dim_ffn 192"
    for kind, _ in slots:
        why = kind.geometry(l0)
        if why is not None:
            return why
    if l0.fconv1[1].kernel_size[0] != 5 or l0.fconv1[1].groups != 8:
        return "kernel sizes (5, 3) and conv groups (8, 8)"
    kinds = [type(m).__name__ for m in (*(m for kind, (_, ln) in slots for m in kind.norms(l0, ln)), l0.fconv1[0], l0.fconv2[0], l0.norm_full)]
    if kinds != [k for kind, _ in slots for k in kind.norm_kinds] + ["LayerNorm"] * 3:
        return f"norms must be LN, LN, GN, LN, LN, LN (got {kinds})"
    if any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in net.modules()):
        return "dropout must be 0"
    return None


class NativeOnlineStreamer(GraphedStep):
    def __init__(self, net, batch: int, chunk: int, device=None, use_graph: Optional[bool] = None, lib: Optional[Lib] = None):
        why = supported(net)
        if why is not None:
            raise NotImplementedError("native OnlineSpatialNet step: " + why)
        if not 0 < chunk <= 32:
            raise NotImplementedError("native OnlineSpatialNet step: 1..32 frames per chunk")
        self.net, self.B, self.C = net.eval(), batch, chunk
        self.dev = torch.device(device) if device is not None else net.decoder.weight.device
        self.lib = lib if lib is not None else hip()  # (tests pass the host emulator build)
        self.use_graph = self.dev.type == "cuda" if use_graph is None else use_graph
        self.F, self.din, self.dout, self.L = net.layers[0].full.in_features, net.encoder.in_channels, net.decoder.out_features, len(net.layers)
        sd = {k: v.detach().float() for k, v in net.state_dict().items()}
        # the cross-band kernels read SpatialNet's flat parameter buffer / packed fragments: same names for everything they touch;
        # the attention slots of that layout stay zero (the retention weights go to the native kernel directly)
        # (layers 0..full_share own a LinearGroup, the later ones share the last of them: OnlineSpatialNet.__init__)
        self.cfg = make_cfg(batch, self.F, chunk, self.din, self.dout, L=self.L, dtype=NBSS_F32, full_share=len({id(l.full) for l in net.layers}) - 1)
        p: Dict[str, Tensor] = {}
        from .params import param_specs
        for name, shape in param_specs(self.cfg):
            p[name] = sd[name] if (name in sd and ".mhsa." not in name) else torch.zeros(shape)
        self.flat = ops.flatten_params(self.lib, self.cfg, p, self.dev)
        self.packed = ops.pack_params(self.lib, self.cfg, self.flat)
        dv = lambda t: None if t is None else t.contiguous().to(self.dev)  # noqa: E731
        self.enc_w, self.enc_b = dv(sd["encoder.weight"]), dv(sd["encoder.bias"])
        self.kinds = layer_kinds(net.layers[0])
        slots = list(zip(self.kinds, SLOTS, ("", "ffn_")))
        # (allocated layer by layer and before the buffers, as the kernels have always found them: a layer's weights lie together)
        weights = [[[dv(w) for w in kind.weights(sd, f"layers.{l}.{q}.", f"layers.{l}.{ln}.")] for kind, (q, ln), _ in slots] for l in range(self.L)]
        self.x, self.y = _zeros(self, batch, self.F, chunk, self.din), _zeros(self, batch, self.F, chunk, self.dout)
        self.h = [_zeros(self, batch, self.F, chunk, 96), _zeros(self, batch, self.F, chunk, 96)]
        # state: 'enc', then per step kind name -> [per layer] (the FFN slot's under 'ffn_' + name) and its rewound shared tensors
        self.state = {"enc": _zeros(self, batch * self.F, 4, self.din)}
        self.shared = {n: t for kind in dict.fromkeys(self.kinds) for n, t in kind.shared(self).items()}
        self.steps = [[] for _ in range(self.L)]  # per layer [(kind, weights, tail)] x 2: the tensors of the call, in its order
        for i, (kind, _, pre) in enumerate(slots):
            for l, steps in enumerate(self.steps):
                own = kind.state(self)
                for n, t in own.items():
                    self.state.setdefault(pre + n, []).append(t)
                steps.append((kind, weights[l][i], [{**self.shared, **own}[n] for n in kind.tail]))
            self.state.update({n: self.shared[n] for n in kind.rewound})

    def _buffers(self):
        return [t for v in self.state.values() for t in (v if isinstance(v, list) else [v])]

    def _run(self) -> None:
        """one step: reads self.x, writes self.y, updates every state buffer in place (a fixed sequence of 5 L + 2 C-ABI calls: encoder, per layer
        fconv, full, fconv, the attention / retention / Mamba step, then the T-ConvFFN step or — 'mamba(16,4)' — a second Mamba step, and the decoder;
        + 1 for 'mhsa(N)': the frame counter's advance after the layers)"""
        lib, cfg, P = self.lib, C.byref(self.cfg), ops._ptr
        st = ops._stream(lib, self.x)
        f = lambda t: P(lib, t, torch.float32)  # noqa: E731
        ptr = lambda t: P(lib, t, None if t is None else t.dtype)  # noqa: E731  (each tensor's own dtype: the frame counter is int32)
        a, b = self.h
        lib.call("nbss_online_encoder_step", self.B * self.F, self.C, self.din, f(self.enc_w), f(self.enc_b), f(self.x), f(self.state["enc"]), f(a), st)
        for l, steps in enumerate(self.steps):
            lib.call("nbss_fconv_fwd", cfg, f(self.flat), P(lib, self.packed), l, 0, f(a), f(b), st)
            lib.call("nbss_full_fwd", cfg, f(self.flat), P(lib, self.packed), l, f(b), f(a), st)
            lib.call("nbss_fconv_fwd", cfg, f(self.flat), P(lib, self.packed), l, 1, f(a), f(b), st)
            for kind, w, tail in steps:
                lib.call(kind.entry, *kind.ints(self), *map(ptr, w), *map(ptr, tail), f(b), st)
            a, b = b, a
        for kind in self.kinds:
            if kind.after is not None:
                kind.after(self, ptr, st)
        lib.call("nbss_decoder_fwd", cfg, f(self.flat), P(lib, self.packed), f(a), f(self.y), st)

    @torch.no_grad()
    def step(self, x_chunk: Tensor) -> Tensor:
        self.x.copy_(x_chunk)
        self._replay()
        return self.y.clone()
