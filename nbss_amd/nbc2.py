"""Native forward of the narrow-band conformer NBC2 (reference: models/arch/NBC2.py:152-289) on the HIP device, sequenced from the
geometry-generic building blocks of the C ABI (`nbss_nb_*`, csrc/nb_blocks.hip): the encoder Conv1d along time, per block LayerNorm ->
in_proj -> softmax(q k^T / sqrt(dh)) v per (sequence, head) -> out_proj + residual, GroupBatchNorm -> Linear -> SiLU -> grouped conv ->
SiLU -> grouped conv -> GroupBatchNorm -> SiLU -> grouped conv -> SiLU -> Linear + residual, and the decoder.  Every GEMM-shaped step is
one MFMA tap-GEMM launch (weights re-laid on the fly from the module's own fp32 parameters); activations stay in the
[B*F, T, C] layout of the reference.  Inference (`torch.no_grad()`): `NativeNBC2.forward`.  Training (round 4): `NativeNBC2.forward_train` —
the autograd.Function of nb.py over the whole network (`_forward_train` / `_backward_train` here) whose backward walks the blocks with the `nbss_nb_*_bwd` entry points (transposed tap-GEMMs with
the SiLU' factor in their epilogue, the token-contraction weight gradients of csrc/wgrad.hip, LayerNorm / GroupBatchNorm / attention backward);
every parameter gradient comes from these kernels, torch contributes buffers and two residual adds per block.

`supported(net)` names what the kernels are built for: norms (LN, GBN, GBN) with per-frame GroupBatchNorm statistics, no dropout, head
width 24, 48 or 96 (96 = NBC2-large, dim_hidden 192 with 2 heads: the key-blocked attention of csrc/attn_kb.hip), channel counts that are multiples of 8 per conv group, sequences of at most 256 frames
— inference with NBSS_NB_LONG=1 (nb.long_enabled): at most 4096 frames, the attention of longer sequences through `nbss_nb_attention_long_fwd`."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from ._lib import NbssError
from .nb import T_LONG, T_WHOLE, Launcher, NativeRunner, TrainFn, long_enabled, pad8


def supported(net) -> Optional[str]:
    """None when `net` (models.arch.NBC2.NBC2) can run through the native forward, else the reason"""
    from models.arch.NBC2 import GroupBatchNorm, LayerNorm
    blocks = list(net.sa_layers)
    if not blocks:
        return "no layers"
    H, FFN = net.encoder.out_channels, blocks[0].linear1.out_features
    if net.encoder.kernel_size[0] % 2 == 0 or net.encoder.groups != 1:
        return "encoder must be an odd-kernel dense Conv1d"
    for b in blocks:
        if not isinstance(b.norm1, LayerNorm) or not isinstance(b.norm2, GroupBatchNorm) or not isinstance(b.conv[4], GroupBatchNorm):
            return "norms must be (LN, GBN, GBN)"
        if b.norm2.share_along_sequence_dim or b.conv[4].share_along_sequence_dim:
            return "GroupBatchNorm statistics must be per frame (share_along_sequence_dim = False)"
        if b.dropout1.p or b.dropout2.p or b.conv[8].p:
            return "dropout must be 0"
        if H // b.self_attn.num_heads not in (24, 48, 96) or not b.self_attn._qkv_same_embed_dim or b.self_attn.in_proj_bias is None:
            return "attention head width must be 24, 48 or 96 (packed in_proj with bias)"
        g = b.conv[1].groups
        if (FFN // g) % 8 or FFN % g or b.conv[1].kernel_size[0] % 2 == 0:
            return "conv groups must be multiples of 8 channels wide, odd kernel"
    if H % 8 or FFN % 8:
        return "dim_hidden / dim_ffn must be multiples of 8"
    return None


def _param_list(net):
    ps = [net.encoder.weight, net.encoder.bias]
    for b in net.sa_layers:
        ps += [b.norm1.weight, b.norm1.bias, b.self_attn.in_proj_weight, b.self_attn.in_proj_bias, b.self_attn.out_proj.weight, b.self_attn.out_proj.bias,
               b.norm2.weight, b.norm2.bias, b.linear1.weight, b.linear1.bias, b.conv[1].weight, b.conv[1].bias, b.conv[3].weight, b.conv[3].bias,
               b.conv[4].weight, b.conv[4].bias, b.conv[6].weight, b.conv[6].bias, b.linear2.weight, b.linear2.bias]
    return ps + [net.decoder.weight, net.decoder.bias]


def _train_supported(net) -> Optional[str]:
    why = supported(net)
    if why is not None:
        return why
    for b in net.sa_layers:
        if not (b.norm2.affine and b.conv[4].affine):
            return "training path expects affine GroupBatchNorm"
    return None


class _NBC2TrainFn(TrainFn):
    pass


class NativeNBC2(NativeRunner):
    """forward of one NBC2 module through the HIP building blocks; parameters are read from the module at every call (no copies)"""
    label, train_fn = "NBC2", _NBC2TrainFn
    supported, train_supported, param_list = staticmethod(supported), staticmethod(_train_supported), staticmethod(_param_list)

    def _geometry(self, x: Tensor, what: str):
        """checks the input against the kernels' limits -> (B, F, T, Cin, Cin8, Cout, Co8, H, FFN, heads, g, ks, ks_e) and the tap-GEMM shapes of the network"""
        net = self.net
        B, F, T, Cin = x.shape
        if what == "forward" and long_enabled():  # (inference alone: the backward blocks are whole-head kernels)
            if T > T_LONG:
                raise NbssError(f"NBC2 native {what}: {T} frames; the key-blocked attention takes <= {T_LONG} frames")
        elif T > T_WHOLE:
            kern = "kernels keep" if what == "training" else "kernel keeps"
            raise NbssError(f"NBC2 native {what}: {T} frames; the attention {kern} a sequence's K / V in LDS (<= 256 frames)")
        gs = net.sa_layers[0].norm2.group_size
        if F != gs:  # (the torch.nn module groups `group_size` consecutive sequences whatever F is; the kernel's groups are the utterances)
            raise NbssError(f"NBC2 native {what}: {F} frequencies per utterance, GroupBatchNorm group_size {gs}")
        b0 = net.sa_layers[0]
        H, FFN, heads, Cout = net.encoder.out_channels, b0.linear1.out_features, b0.self_attn.num_heads, net.decoder.out_features
        ks_e, g, ks = net.encoder.kernel_size[0], b0.conv[1].groups, b0.conv[1].kernel_size[0]
        Cin8, Co8 = pad8(Cin), pad8(Cout)
        shapes = ((H, Cin8, 1, ks_e), (3 * H, H, 1, 1), (H, H, 1, 1), (FFN, H, 1, 1), (FFN, FFN, g, ks), (H, FFN, 1, 1), (Co8, H, 1, 1))
        return (B, F, T, Cin, Cin8, Cout, Co8, H, FFN, heads, g, ks, ks_e), shapes

    def forward(self, x: Tensor) -> Tensor:
        """x [B,F,T,dim_input] (fp32 or bf16, HIP device) -> [B,F,T,dim_output] of the same dtype"""
        net = self.net
        (B, F, T, Cin, Cin8, Cout, Co8, H, FFN, heads, g, ks, ks_e), shapes = self._geometry(x, "forward")
        L = Launcher(self.lib, x)
        nseq = B * F
        L.alloc_ws(shapes)  # scratch for the re-laid weights of one launch (the largest of the network)
        stats = torch.empty(nseq * T, 2, dtype=torch.float32, device=L.dev)  # LayerNorm statistics (unused here: one buffer for all blocks)
        attention = "nbss_nb_attention_long_fwd" if T > T_WHOLE else "nbss_nb_attention_fwd"  # (beyond a head's K / V in LDS: walked in blocks of 64 keys)
        # SiLU is fused into the consumer (act_in) or behind the norm
        h = L.conv(L.pad_cols(x, nseq, T, Cin), nseq, T, Cin, Cin8, H, 1, ks_e, net.encoder.weight, net.encoder.bias)
        for b in net.sa_layers:
            u, _ = L.layernorm(h, b.norm1, stats)
            qkv = L.conv(u, nseq, T, H, H, 3 * H, 1, 1, b.self_attn.in_proj_weight, b.self_attn.in_proj_bias)
            o = torch.empty_like(h)
            L.lib.call(attention, L.dt, nseq, T, H, heads, L.p(qkv), L.p(o), L.st)
            h = L.conv(o, nseq, T, H, H, H, 1, 1, b.self_attn.out_proj.weight, b.self_attn.out_proj.bias, res=h)
            v = L.gbn(h, b.norm2, B, F, T, 0)
            a = L.conv(v, nseq, T, H, H, FFN, 1, 1, b.linear1.weight, b.linear1.bias)
            c1 = L.conv(a, nseq, T, FFN, FFN, FFN, g, ks, b.conv[1].weight, b.conv[1].bias, act_in=1)
            c2 = L.conv(c1, nseq, T, FFN, FFN, FFN, g, ks, b.conv[3].weight, b.conv[3].bias, act_in=1)
            n3 = L.gbn(c2, b.conv[4], B, F, T, 1)
            c3 = L.conv(n3, nseq, T, FFN, FFN, FFN, g, ks, b.conv[6].weight, b.conv[6].bias)
            h = L.conv(c3, nseq, T, FFN, FFN, H, 1, 1, b.linear2.weight, b.linear2.bias, res=h, act_in=1)
        # decoder: output columns padded to a multiple of 8 (zero weight rows), sliced afterwards
        wd, bd = L.padded(L.f32(net.decoder.weight), Co8, H), L.padded(L.f32(net.decoder.bias), Co8)
        return L.unpad(L.conv(h, nseq, T, H, H, Co8, 1, 1, wd, bd), B, F, T, Cout, x.dtype)

    def _forward_train(self, x: Tensor):
        net = self.net
        geo, shapes = self._geometry(x, "training")
        B, F, T, Cin, Cin8, Cout, Co8, H, FFN, heads, g, ks, ks_e = geo
        L = Launcher(self.lib, x)
        nseq = B * F
        ws = L.alloc_ws(shapes, bwd=True)
        # the producer writes SiLU(y) as a second output (y2) where the backward needs both
        xin = L.pad_cols(x, nseq, T, Cin)
        h = L.conv_train(xin, nseq, T, Cin, Cin8, H, 1, ks_e, net.encoder.weight, net.encoder.bias)
        per = []
        for b in net.sa_layers:
            u, stats = L.layernorm(h, b.norm1)
            qkv = L.conv_train(u, nseq, T, H, H, 3 * H, 1, 1, b.self_attn.in_proj_weight, b.self_attn.in_proj_bias)
            o = torch.empty_like(h)
            L.lib.call("nbss_nb_attention_fwd", L.dt, nseq, T, H, heads, L.p(qkv), L.p(o), L.st)
            h1 = L.conv_train(o, nseq, T, H, H, H, 1, 1, b.self_attn.out_proj.weight, b.self_attn.out_proj.bias, res=h)
            v = L.gbn(h1, b.norm2, B, F, T, 0)
            a, sa = L.conv_train(v, nseq, T, H, H, FFN, 1, 1, b.linear1.weight, b.linear1.bias, y2=True)
            c1, sc1 = L.conv_train(sa, nseq, T, FFN, FFN, FFN, g, ks, b.conv[1].weight, b.conv[1].bias, y2=True)
            c2 = L.conv_train(sc1, nseq, T, FFN, FFN, FFN, g, ks, b.conv[3].weight, b.conv[3].bias)
            n3 = L.gbn(c2, b.conv[4], B, F, T, 1)
            c3, sc3 = L.conv_train(n3, nseq, T, FFN, FFN, FFN, g, ks, b.conv[6].weight, b.conv[6].bias, y2=True)
            h2 = L.conv_train(sc3, nseq, T, FFN, FFN, H, 1, 1, b.linear2.weight, b.linear2.bias, res=h1)
            per.append(dict(h=h, u=u, stats=stats, qkv=qkv, o=o, h1=h1, v=v, a=a, sa=sa, c1=c1, sc1=sc1, c2=c2, n3=n3, c3=c3, sc3=sc3))
            h = h2
        wd, bd = L.padded(L.f32(net.decoder.weight), Co8, H), L.padded(L.f32(net.decoder.bias), Co8)
        out = L.conv_train(h, nseq, T, H, H, Co8, 1, 1, wd, bd)
        saved = dict(per=per, xin=xin, hL=h, wd=wd, geo=geo, ws=ws)
        return L.unpad(out, B, F, T, Cout, x.dtype), saved

    def _backward_train(self, sv, dout: Tensor):
        net = self.net
        B, F, T, Cin, Cin8, Cout, Co8, H, FFN, heads, g, ks, ks_e = sv["geo"]
        L = Launcher(self.lib, dout, ws=sv["ws"])
        nseq = B * F
        aws = torch.empty(L.lib._dll.nbss_nb_attention_bwd_ws_bytes(L.dt, nseq, T, H, heads), dtype=torch.uint8, device=L.dev)
        # decoder
        d8 = L.pad_cols(dout, nseq, T, Cout)
        dh, dwd, dbd = L.conv_bwd(sv["hL"], nseq, T, H, H, Co8, 1, 1, sv["wd"], d8)
        g_dec = [dwd.reshape(Co8, H)[:Cout], dbd[:Cout]]
        per_grads = []
        for b, s in zip(reversed(net.sa_layers), reversed(sv["per"])):
            # feed-forward branch: h2 = linear2(SiLU(c3)) + h1
            dc3, dw2, db2 = L.conv_bwd(s["sc3"], nseq, T, FFN, FFN, H, 1, 1, b.linear2.weight, dh, x_pre=s["c3"])
            dn3, dwc3, dbc3 = L.conv_bwd(s["n3"], nseq, T, FFN, FFN, FFN, g, ks, b.conv[6].weight, dc3)
            dc2, dgn3, dbn3 = L.gbn_bwd(s["c2"], b.conv[4], B, F, T, 1, dn3)
            dc1, dwc2, dbc2 = L.conv_bwd(s["sc1"], nseq, T, FFN, FFN, FFN, g, ks, b.conv[3].weight, dc2, x_pre=s["c1"])
            da, dwc1, dbc1 = L.conv_bwd(s["sa"], nseq, T, FFN, FFN, FFN, g, ks, b.conv[1].weight, dc1, x_pre=s["a"])
            dv, dw1, db1 = L.conv_bwd(s["v"], nseq, T, H, H, FFN, 1, 1, b.linear1.weight, da)
            dh1b, dgn2, dbn2 = L.gbn_bwd(s["h1"], b.norm2, B, F, T, 0, dv)
            dh1 = dh + dh1b  # residual: h2 = h1 + ffn(h1)
            # attention branch: h1 = out_proj(attn(in_proj(LN(h)))) + h
            do, dwo, dbo = L.conv_bwd(s["o"], nseq, T, H, H, H, 1, 1, b.self_attn.out_proj.weight, dh1)
            dqkv = torch.empty_like(s["qkv"])
            L.lib.call("nbss_nb_attention_bwd", L.dt, nseq, T, H, heads, L.p(s["qkv"]), L.p(do), L.p(dqkv), L.p(aws), L.st)
            du, dwi, dbi = L.conv_bwd(s["u"], nseq, T, H, H, 3 * H, 1, 1, b.self_attn.in_proj_weight, dqkv)
            dh, dg1, db1n = L.layernorm_bwd(s["h"], s["stats"], b.norm1, du, dh1)
            per_grads.append([dg1, db1n, dwi, dbi, dwo, dbo, dgn2, dbn2, dw1, db1, dwc1, dbc1, dwc2, dbc2, dgn3, dbn3, dwc3, dbc3, dw2, db2])
        # encoder (no input gradient)
        _, dwe, dbe = L.conv_bwd(sv["xin"], nseq, T, Cin, Cin8, H, 1, ks_e, net.encoder.weight, dh, need_dx=False)
        grads = [dwe, dbe]
        for gl in reversed(per_grads):
            grads += gl
        grads += g_dec
        return [gr.reshape(prm.shape).to(prm.dtype) for gr, prm in zip(grads, _param_list(net))]
