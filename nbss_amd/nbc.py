"""Native inference forward of the narrow-band conformer NBC (reference: models/arch/NBC.py:161-293: pre-norm blocks of Transformer-XL relative-position
attention and a convolutional feed-forward with GroupNorm) on the HIP device, sequenced from the `nbss_nb_*` building blocks of the C ABI (through the launcher
of nb.py; the relative-position attention launches, the encoder / decoder tap arithmetic, the q | k | v concatenation and the dropouts are here):

  encoder   Conv1d(k, no padding: T -> T - k + 1 frames)                = a zero-padded tap-GEMM, rows k/2 .. of its output
  block     LayerNorm -> q | k | v maps -> nbss_nb_attention_relpos_fwd (P = pos_proj of the sinusoid table, one small GEMM per block)
            -> out_proj + residual;  LayerNorm -> linear1 -> SiLU -> 3 x (grouped conv -> GroupNorm(8) -> SiLU) -> linear2 + residual
  decoder   ConvTranspose1d(k)                                          = a zero-padded tap-GEMM over the frames shifted by one, taps flipped

Inference beyond 256 frames (whole utterances) with NBSS_NB_LONG=1 (nb.long_enabled): `nbss_nb_attention_relpos_long_fwd`, up to 4096 frames and the sinusoid
table's 1001 frames behind the encoder.  Inference and training: `models.arch.NBC.NBC.forward` takes this path by default for every call on a HIP tensor the kernels support (NBSS_NBC_NATIVE=0
switches it off).  The reference trains NBC with dropout 0.1 inside the attention and the feed-forward (NBC.py:73-104,161-193): the attention dropout
goes through keep-bits both passes read (`_keep_bits`), the element-wise dropouts are device tensors.  `tests/test_nbc_native.py` runs both paths on the
emulator and on the device against the torch.nn module, `tests/test_nb_native_vs_reference.py` against numbers of the reference's own module."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from ._lib import NbssError
from .nb import T_LONG, T_WHOLE, Launcher, NativeRunner, TrainFn, long_enabled, pad8


def supported(net) -> Optional[str]:
    """None when `net` (models.arch.NBC.NBC) can run through the native forward, else the reason"""
    blocks = list(net.sa_layers)
    if not blocks:
        return "no layers"
    H = net.encoder.out_channels
    if net.encoder.groups != 1 or net.encoder.stride[0] != 1 or net.decoder.stride[0] != 1 or net.decoder.kernel_size != net.encoder.kernel_size:
        return "encoder / decoder must be dense stride-1 (transposed) convolutions of one kernel size"
    if net.encoder.kernel_size[0] != 4:
        return "encoder kernel size must be 4"
    for b in blocks:
        if not b.norm_first:
            return "norm_first = False"
        a = b.self_attn
        if H // a.num_heads not in (24, 48):
            return "attention head width must be 24 or 48"
        convs = [m for m in b.conv if isinstance(m, torch.nn.Conv1d)]
        gns = [m for m in b.conv if isinstance(m, torch.nn.GroupNorm)]
        if len(convs) != len(gns) or len(list(b.conv)) != 3 * len(convs):
            return "the feed-forward must be (conv, GroupNorm, SiLU) x n"
        for cv in convs:
            if cv.kernel_size[0] % 2 == 0 or (cv.in_channels // cv.groups) % 8 or cv.bias is None:
                return "grouped convs need an odd kernel, a bias and groups that are multiples of 8 channels wide"
            if cv.in_channels != b.linear1.out_features or cv.out_channels != b.linear1.out_features:
                return "the feed-forward convs must be ffn_size wide"
        for gn in gns:
            if abs(gn.eps - 1e-5) > 1e-12 or not gn.affine:
                return "GroupNorm must be affine with eps 1e-5"
    if H % 8 or blocks[0].linear1.out_features % 8:
        return "hidden_size / ffn_size must be multiples of 8"
    return None


# ---- training (round 5): the autograd.Function of nb.py; the backward walks the blocks in reverse over the nbss_nb_*_bwd building blocks, the relative-position
# attention through nbss_nb_attention_relpos_train / _bwd.  The reference's NBC trains with dropout 0.1 everywhere (NBC.py:83,168: not a constructor
# argument): the three element-wise dropouts of a block are torch ops on the device between the kernels (masks kept for backward), the attention dropout is
# a bit tensor [nseq][heads][T][ceil(T / 32)] drawn here with torch's generator and read by the forward AND the backward kernels. --------------------------------
def _param_list(net):
    ps = [net.encoder.weight, net.encoder.bias]
    for b in net.sa_layers:
        a = b.self_attn
        ps += [b.norm1.weight, b.norm1.bias, a.query_proj.weight, a.query_proj.bias, a.key_proj.weight, a.key_proj.bias, a.value_proj.weight, a.value_proj.bias,
               a.pos_proj.weight, a.u_bias, a.v_bias, a.out_proj.weight, a.out_proj.bias, b.norm2.weight, b.norm2.bias, b.linear1.weight, b.linear1.bias]
        for m in b.conv:
            if isinstance(m, (torch.nn.Conv1d, torch.nn.GroupNorm)):
                ps += [m.weight, m.bias]
        ps += [b.linear2.weight, b.linear2.bias]
    ps.append(net.decoder.weight)
    if net.decoder.bias is not None:
        ps.append(net.decoder.bias)
    return ps


def train_supported(net) -> Optional[str]:
    why = supported(net)
    if why is not None:
        return why
    if net.encoder.bias is None:
        return "encoder without bias"
    for b in net.sa_layers:
        a = b.self_attn
        if any(l.bias is None for l in (a.query_proj, a.key_proj, a.value_proj, a.out_proj, b.linear1, b.linear2)) or a.pos_proj.bias is not None:
            return "projections must have biases (pos_proj none)"
        for gn in (m for m in b.conv if isinstance(m, torch.nn.GroupNorm)):
            if (b.linear1.out_features // gn.num_groups) > 64:
                return "GroupNorm groups wider than 64 channels"
    if len(set(id(p) for p in _param_list(net))) != len(list(net.parameters())):
        return "parameters outside the native path"
    return None


def _keep_bits(shape, p: float, dev) -> Tensor:
    """attention-dropout keep-bits for [nseq, heads, T, T] probabilities: int32 words [nseq, heads, T, ceil(T / 32)], bit (j & 31) of word j >> 5 = (i, j) kept"""
    nseq, heads, T, _ = shape
    MW = (T + 31) // 32
    out = torch.empty(nseq, heads, T, MW, dtype=torch.int32, device=dev)
    wt = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
    # one head at a time, bytes not int64 words: the transient is one float32 + one byte per probability of a head (the first version drew all heads at
    # once and packed through two int64 copies: ~10 GB of transients per layer at B 4 x F 257 x 248 frames x 8 heads)
    for h in range(heads):
        keep = (torch.rand(nseq, T, MW, 4, 8, device=dev) >= p).to(torch.uint8)
        out[:, h] = (keep * wt).sum(-1, dtype=torch.uint8).view(torch.int32).squeeze(-1)  # (little-endian: byte k of a word = bits 8k .. 8k + 7)
    return out


class _NBCTrainFn(TrainFn):
    pass


class NativeNBC(NativeRunner):
    """one NBC module through the HIP building blocks; parameters are read from the module at every call (no copies)"""
    label, train_fn = "NBC", _NBCTrainFn
    supported, train_supported, param_list = staticmethod(supported), staticmethod(train_supported), staticmethod(_param_list)

    def _geometry(self, x: Tensor, what: str):
        """checks the frame count -> (B, F, T, Ti, K, K1, Cin, Cin8, Cout, Co8, H, FFN, heads) and the tap-GEMM shapes of the network"""
        net = self.net
        B, F, T, Cin = x.shape
        K = net.encoder.kernel_size[0]
        Ti = T - K + 1  # frames inside the network
        if what == "forward" and long_enabled() and Ti >= 1:  # (inference alone: the backward blocks are whole-head kernels)
            max_len = net.sa_layers[0].self_attn.rel_pos.max_len
            if T > T_LONG:
                raise NbssError(f"NBC native {what}: {T} frames; the key-blocked attention takes <= {T_LONG} frames")
            if Ti > max_len + 1:
                raise NbssError(f"NBC native {what}: {T} frames; the sinusoid table holds the offsets of {max_len + 1} frames behind the encoder (kernel {K})")
        elif Ti < 1 or T > T_WHOLE:
            lds = "kernels keep a sequence and its" if what == "training" else "kernel keeps a sequence's K / V /"
            raise NbssError(f"NBC native {what}: {T} frames (kernel {K}; the attention {lds} offsets table in LDS: <= 256)")
        b0 = net.sa_layers[0]
        H, FFN, heads, Cout = net.encoder.out_channels, b0.linear1.out_features, b0.self_attn.num_heads, net.decoder.out_channels
        Cin8, Co8 = pad8(Cin), pad8(Cout)
        K1 = K + 1  # (the building block takes odd kernels: one more tap with zero weights, same centre K/2)
        cv0 = [m for m in b0.conv if isinstance(m, torch.nn.Conv1d)][0]
        shapes = ((H, Cin8, 1, K1), (3 * H, H, 1, 1), (H, H, 1, 1), (FFN, H, 1, 1), (FFN, FFN, cv0.groups, cv0.kernel_size[0]), (H, FFN, 1, 1), (Co8, H, 1, K1))
        return (B, F, T, Ti, K, K1, Cin, Cin8, Cout, Co8, H, FFN, heads), shapes

    @staticmethod
    def _qkv(L: Launcher, a, what: str) -> Tensor:
        """the "weight" / "bias" of the three projections as those of one [3H][H] map"""
        return torch.cat([L.f32(getattr(m, what)) for m in (a.query_proj, a.key_proj, a.value_proj)], 0)

    @staticmethod
    def _pos_table(L: Launcher, a, Ti: int) -> Tensor:
        """sinusoid rows for the offsets -(Ti - 1) .. Ti - 1: pos_proj maps them to P, one [2 Ti - 1][H] x [H][H] map (a single "sequence") per block"""
        return a.rel_pos.pe[0, a.rel_pos.zero_index - (Ti - 1): a.rel_pos.zero_index + Ti].to(device=L.dev, dtype=L.td).contiguous()[None]

    @staticmethod
    def _decoder_weights(L: Launcher, net, Co8: int, H: int, K1: int):
        """ConvTranspose1d, y[t] = sum_k h[t - k] w[:, :, k] over T = Ti + K - 1 frames = the "same" conv (centre K/2) of z, z[j] = h[j - (K/2 - 1)], with the
        taps flipped: offset d = tap - K/2 reads z[t + d] = h[t - k] for k = K/2 - 1 - d (K = 4: k = 3 - tap); its weight is [in][out][k]"""
        bias = net.decoder.bias
        return L.padded(L.f32(net.decoder.weight).permute(1, 0, 2).flip(-1), Co8, H, K1), L.padded(L.f32(bias) if bias is not None else None, Co8)

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        """x [B,F,T,dim_input] (fp32 or bf16) -> [B,F,T,dim_output] of the same dtype (dropout inactive: eval semantics)"""
        net = self.net
        (B, F, T, Ti, K, K1, Cin, Cin8, Cout, Co8, H, FFN, heads), shapes = self._geometry(x, "forward")
        L = Launcher(self.lib, x)
        nseq = B * F
        L.alloc_ws(shapes)
        # (beyond a head's K / V / offsets table in LDS: keys and table rows walked in blocks; T, not Ti, decides — the launch sequence up to 256 frames is one)
        attention = "nbss_nb_attention_relpos_long_fwd" if T > T_WHOLE else "nbss_nb_attention_relpos_fwd"
        # encoder: y[t'] = sum_k x[t' + k] w[k] (t' < T - K + 1) = rows K/2 .. of the zero-padded ("same", centre K/2) conv over the T frames
        xin = L.pad_cols(x, nseq, T, Cin)
        wenc = L.padded(L.f32(net.encoder.weight), H, Cin8, K1)
        h = L.conv(xin, nseq, T, Cin8, Cin8, H, 1, K1, wenc, net.encoder.bias)[:, K // 2: K // 2 + Ti].contiguous()
        for b in net.sa_layers:
            a = b.self_attn
            u, _ = L.layernorm(h, b.norm1)
            qkv = L.conv(u, nseq, Ti, H, H, 3 * H, 1, 1, self._qkv(L, a, "weight"), self._qkv(L, a, "bias"))
            pos = L.conv(self._pos_table(L, a, Ti), 1, 2 * Ti - 1, H, H, H, 1, 1, a.pos_proj.weight, None)
            o = torch.empty_like(h)
            L.lib.call(attention, L.dt, nseq, Ti, H, heads, L.p(qkv), L.p(pos), L.p(L.f32(a.u_bias)), L.p(L.f32(a.v_bias)), 1.0 / a.sqrt_dim, L.p(o), L.st)
            h = L.conv(o, nseq, Ti, H, H, H, 1, 1, a.out_proj.weight, a.out_proj.bias, res=h)
            v, _ = L.layernorm(h, b.norm2)
            c = L.conv(v, nseq, Ti, H, H, FFN, 1, 1, b.linear1.weight, b.linear1.bias, act_out=1)
            mods = list(b.conv)
            for i in range(0, len(mods), 3):
                cv, gn = mods[i], mods[i + 1]
                c = L.group_norm(L.conv(c, nseq, Ti, FFN, FFN, FFN, cv.groups, cv.kernel_size[0], cv.weight, cv.bias), gn, 1)
            h = L.conv(c, nseq, Ti, FFN, FFN, H, 1, 1, b.linear2.weight, b.linear2.bias, res=h)
        z = torch.zeros(nseq, T, H, dtype=L.td, device=L.dev)
        z[:, K // 2 - 1: K // 2 - 1 + Ti] = h
        wdec, bdec = self._decoder_weights(L, net, Co8, H, K1)
        return L.unpad(L.conv(z, nseq, T, H, H, Co8, 1, K1, wdec, bdec), B, F, T, Cout, x.dtype)

    def _forward_train(self, x: Tensor):
        net = self.net
        geo, shapes = self._geometry(x, "training")
        B, F, T, Ti, K, K1, Cin, Cin8, Cout, Co8, H, FFN, heads = geo
        L = Launcher(self.lib, x)
        nseq, training = B * F, net.training
        ws = L.alloc_ws(shapes, bwd=True)

        def dropout(t, mod):
            """-> (dropped tensor, mask scaled by 1 / (1 - p) in the stream dtype, or None)"""
            if not training or mod.p == 0.0:
                return t, None
            m = (torch.rand_like(t, dtype=torch.float32) >= mod.p).to(L.td) * (1.0 / (1.0 - mod.p))
            return t * m, m

        xin = L.pad_cols(x, nseq, T, Cin)
        wenc = L.padded(L.f32(net.encoder.weight), H, Cin8, K1)
        h = L.conv_train(xin, nseq, T, Cin8, Cin8, H, 1, K1, wenc, net.encoder.bias)[:, K // 2: K // 2 + Ti].contiguous()
        per = []
        for b in net.sa_layers:
            a = b.self_attn
            u, st1 = L.layernorm(h, b.norm1)
            qkv = L.conv_train(u, nseq, Ti, H, H, 3 * H, 1, 1, self._qkv(L, a, "weight"), self._qkv(L, a, "bias"))
            pe = self._pos_table(L, a, Ti)
            pos = L.conv_train(pe, 1, 2 * Ti - 1, H, H, H, 1, 1, a.pos_proj.weight, None)
            pa = a.dropout.p if training else 0.0
            bits = _keep_bits((nseq, heads, Ti, Ti), pa, L.dev) if pa > 0 else None
            o = torch.empty_like(h)
            L.lib.call("nbss_nb_attention_relpos_train", L.dt, nseq, Ti, H, heads, L.p(qkv), L.p(pos), L.p(L.f32(a.u_bias)), L.p(L.f32(a.v_bias)), 1.0 / a.sqrt_dim,
                       L.p(bits), 1.0 / (1.0 - pa), L.p(o), L.st)
            att, m1 = dropout(L.conv_train(o, nseq, Ti, H, H, H, 1, 1, a.out_proj.weight, a.out_proj.bias), b.dropout1)
            h1 = h + att
            v, st2 = L.layernorm(h1, b.norm2)
            a1, c = L.conv_train(v, nseq, Ti, H, H, FFN, 1, 1, b.linear1.weight, b.linear1.bias, y2=True)
            mods = list(b.conv)
            chain = []  # per conv step: (input c_prev, pre-norm z, GroupNorm stats)
            for i in range(0, len(mods), 3):
                cv, gn = mods[i], mods[i + 1]
                z = L.conv_train(c, nseq, Ti, FFN, FFN, FFN, cv.groups, cv.kernel_size[0], cv.weight, cv.bias)
                y, gst = L.group_norm_train(z, gn, 1)
                chain.append((c, z, gst))
                c = y
            cd, md = dropout(c, b.dropout)
            f, m2 = dropout(L.conv_train(cd, nseq, Ti, FFN, FFN, H, 1, 1, b.linear2.weight, b.linear2.bias), b.dropout2)
            h2 = h1 + f
            per.append(dict(h=h, u=u, st1=st1, qkv=qkv, pe=pe, pos=pos, bits=bits, pa=pa, o=o, m1=m1, h1=h1, v=v, st2=st2, a1=a1, chain=chain, cd=cd, md=md, m2=m2))
            h = h2
        z = torch.zeros(nseq, T, H, dtype=L.td, device=L.dev)
        z[:, K // 2 - 1: K // 2 - 1 + Ti] = h
        wdec, bdec = self._decoder_weights(L, net, Co8, H, K1)
        out = L.conv_train(z, nseq, T, H, H, Co8, 1, K1, wdec, bdec)
        saved = dict(per=per, xin=xin, z=z, wenc=wenc, wdec=wdec, geo=geo, ws=ws)
        return L.unpad(out, B, F, T, Cout, x.dtype), saved

    def _backward_train(self, sv, dout: Tensor):
        net = self.net
        B, F, T, Ti, K, K1, Cin, Cin8, Cout, Co8, H, FFN, heads = sv["geo"]
        L = Launcher(self.lib, dout, ws=sv["ws"])
        nseq = B * F
        aws = torch.empty(L.lib._dll.nbss_nb_attention_relpos_bwd_ws_bytes(nseq, Ti, H, heads), dtype=torch.uint8, device=L.dev)
        # decoder (a transposed conv = the "same" conv of the zero-extended sequence with the taps flipped)
        d8 = L.pad_cols(dout, nseq, T, Cout)
        dz, dwd, dbd = L.conv_bwd(sv["z"], nseq, T, H, H, Co8, 1, K1, sv["wdec"], d8)
        dh = dz[:, K // 2 - 1: K // 2 - 1 + Ti].contiguous()
        g_dec = [dwd.view(Co8, H, K1)[:Cout, :, :K].flip(-1).permute(1, 0, 2).contiguous()]
        if net.decoder.bias is not None:
            g_dec.append(dbd[:Cout])
        per_grads = []
        for b, s in zip(reversed(net.sa_layers), reversed(sv["per"])):
            a = b.self_attn
            # feed-forward branch: h2 = h1 + dropout2(linear2(dropout(chain(SiLU(linear1(LN2(h1)))))))
            df = dh * s["m2"] if s["m2"] is not None else dh
            dcd, dw2, db2 = L.conv_bwd(s["cd"], nseq, Ti, FFN, FFN, H, 1, 1, b.linear2.weight, df.contiguous())
            dc = dcd * s["md"] if s["md"] is not None else dcd
            mods = list(b.conv)
            chain_grads = []
            steps = [(mods[i], mods[i + 1]) for i in range(0, len(mods), 3)]
            for idx in range(len(steps) - 1, -1, -1):
                cv, gn = steps[idx]
                c_prev, z, gst = s["chain"][idx]
                dzz = dc.contiguous()  # (ours alone: a conv_bwd output or the product with the dropout mask; the kernel works in place)
                dg, dbt = L.group_norm_bwd(z, gst, gn, dzz)
                # c_prev = SiLU(a1) for the first conv (x_pre: the gradient comes back multiplied by SiLU'(a1)), the previous step's output otherwise
                dc, dwc, dbc = L.conv_bwd(c_prev, nseq, Ti, FFN, FFN, FFN, cv.groups, cv.kernel_size[0], cv.weight, dzz, x_pre=s["a1"] if idx == 0 else None)
                chain_grads.append([dwc, dbc, dg, dbt])
            dv, dw1, db1 = L.conv_bwd(s["v"], nseq, Ti, H, H, FFN, 1, 1, b.linear1.weight, dc)
            dh1, dg2, db2n = L.layernorm_bwd(s["h1"], s["st2"], b.norm2, dv, dh)
            # attention branch: h1 = h + dropout1(out_proj(attention(...)))
            da = dh1 * s["m1"] if s["m1"] is not None else dh1
            do, dwo, dbo = L.conv_bwd(s["o"], nseq, Ti, H, H, H, 1, 1, a.out_proj.weight, da.contiguous())
            dqkv = torch.empty_like(s["qkv"])
            dpos, dub, dvb = L.zeros(2 * Ti - 1, H), L.zeros(H), L.zeros(H)
            L.lib.call("nbss_nb_attention_relpos_bwd", L.dt, nseq, Ti, H, heads, L.p(s["qkv"]), L.p(s["pos"]), L.p(L.f32(a.u_bias)), L.p(L.f32(a.v_bias)),
                       1.0 / a.sqrt_dim, L.p(s["bits"]), 1.0 / (1.0 - s["pa"]), L.p(do), L.p(dqkv), L.p(dpos), L.p(dub), L.p(dvb), L.p(aws), L.st)
            _, dwp, _ = L.conv_bwd(s["pe"], 1, 2 * Ti - 1, H, H, H, 1, 1, a.pos_proj.weight, dpos.to(L.td)[None].contiguous(), need_dx=False, bias=False)
            du, dwi, dbi = L.conv_bwd(s["u"], nseq, Ti, H, H, 3 * H, 1, 1, self._qkv(L, a, "weight"), dqkv)
            dh, dg1, db1n = L.layernorm_bwd(s["h"], s["st1"], b.norm1, du, dh1)
            dwi = dwi.view(3, H, H)
            gl = [dg1, db1n, dwi[0], dbi[:H], dwi[1], dbi[H:2 * H], dwi[2], dbi[2 * H:], dwp, dub, dvb, dwo, dbo, dg2, db2n, dw1, db1]
            for cg in reversed(chain_grads):
                gl += cg
            gl += [dw2, db2]
            per_grads.append(gl)
        # encoder (no input gradient): the "valid" conv = rows K/2 .. of the zero-padded odd-kernel conv
        dfull = torch.zeros(nseq, T, H, dtype=L.td, device=L.dev)
        dfull[:, K // 2: K // 2 + Ti] = dh
        _, dwe, dbe = L.conv_bwd(sv["xin"], nseq, T, Cin8, Cin8, H, 1, K1, sv["wenc"], dfull, need_dx=False)
        grads = [dwe.view(H, Cin8, K1)[:, :Cin, :K].contiguous(), dbe]
        for gl in reversed(per_grads):
            grads += gl
        grads += g_dec
        return [gr.reshape(prm.shape).to(prm.dtype) for gr, prm in zip(grads, _param_list(net))]
