"""NB-BLSTM (models/arch/blstm2_fc1.py; reference blstm2_fc1.py:45-68) on the HIP building blocks: per bidirectional layer ONE dense map for the input part of the
gates (nbss_nb_conv_t), ONE persistent launch for the recurrences of both directions over all frames (nbss_nb_blstm_fwd: gates GEMM on MFMA, h in LDS, c in
registers), and in training the reverse walk (nbss_nb_blstm_bwd) followed by dense contractions for the weight / bias / input gradients (nbss_nb_conv_t_bwd).
The module keeps its nn.LSTM parameters (state_dict keys unchanged); they are read at every call.  The dense maps go through the launcher of nb.py, the
runner base and the training autograd.Function are nb.py's; the recurrence launches and the W_hh contraction are here."""
from typing import Optional

import torch
from torch import Tensor

from .nb import Launcher, NativeRunner, TrainFn, pad8


def supported(net) -> Optional[str]:
    """None when `net` (models.arch.blstm2_fc1.BLSTM2_FC1) can run through the native path, else the reason"""
    for rnn in (net.blstm1, net.blstm2):
        if rnn.hidden_size not in (128, 256):
            return f"hidden size {rnn.hidden_size} (the recurrence kernels are built for 128 and 256)"
        if rnn.num_layers != 1 or not rnn.bidirectional or not rnn.batch_first or not rnn.bias or rnn.proj_size != 0:
            return "LSTM layers must be single bidirectional batch-first layers with biases"
    if net.dropout:
        return "dropout between the layers"
    if net.activation_func is not None:
        return "output activation"
    return None


def _param_list(net):
    ps = []
    for rnn in (net.blstm1, net.blstm2):
        for sfx in ("", "_reverse"):
            ps += [getattr(rnn, f"weight_ih_l0{sfx}"), getattr(rnn, f"weight_hh_l0{sfx}"), getattr(rnn, f"bias_ih_l0{sfx}"), getattr(rnn, f"bias_hh_l0{sfx}")]
    return ps + [net.linear.weight, net.linear.bias]


class _BLSTMTrainFn(TrainFn):
    pass


class NativeBLSTM(NativeRunner):
    label, kind, train_fn = "NB-BLSTM", "native path", _BLSTMTrainFn
    supported, param_list = staticmethod(supported), staticmethod(_param_list)

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        return self._run(x, train=False)[0]

    def _forward_train(self, x: Tensor):
        return self._run(x, train=True)

    def _run(self, x: Tensor, train: bool):
        net = self.net
        B, F, T, Cin = x.shape
        L = Launcher(self.lib, x)
        n = B * F
        h = x.reshape(n, T, Cin).to(L.td)
        layers = []
        for rnn in (net.blstm1, net.blstm2):
            HD, I = rnn.hidden_size, h.shape[-1]
            I8 = pad8(I)
            h = (L.pad_cols(h, n, T, I) if I8 != I else h).contiguous()
            # the input maps of both directions as one [8 HD][I8] map, the two bias vectors of each direction summed
            wih = L.zeros(8 * HD, I8)
            wih[:4 * HD, :I] = L.f32(rnn.weight_ih_l0)
            wih[4 * HD:, :I] = L.f32(rnn.weight_ih_l0_reverse)
            bias = torch.cat([L.f32(rnn.bias_ih_l0) + L.f32(rnn.bias_hh_l0), L.f32(rnn.bias_ih_l0_reverse) + L.f32(rnn.bias_hh_l0_reverse)])
            L.alloc_ws([(8 * HD, I8, 1, 1)], bwd=True, at_least=L.lib._dll.nbss_nb_blstm_ws_bytes(L.dt, HD))
            gx = L.conv_train(h, n, T, I8, I8, 8 * HD, 1, 1, wih, bias)
            y = torch.empty(n, T, 2 * HD, dtype=L.td, device=L.dev)
            save = torch.empty(2, n, T, 5 * HD, dtype=L.td, device=L.dev) if train else None
            L.lib.call("nbss_nb_blstm_fwd", L.dt, n, T, HD, 8 * HD, L.p(gx), L.p(L.f32(rnn.weight_hh_l0)), L.p(L.f32(rnn.weight_hh_l0_reverse)), L.p(y), L.p(save),
                       L.p(L.ws), L.st)
            layers.append(dict(x=h, I=I, I8=I8, HD=HD, wih=wih, y=y, save=save))
            h = y
        Cout = net.linear.out_features
        Co8, K2 = pad8(Cout), h.shape[-1]
        wl, bl = L.padded(L.f32(net.linear.weight), Co8, K2), L.padded(L.f32(net.linear.bias), Co8)
        L.alloc_ws([(Co8, K2, 1, 1)], bwd=True)
        out = L.conv_train(h, n, T, K2, K2, Co8, 1, 1, wl, bl)
        saved = dict(layers=layers, wl=wl, geo=(B, F, T, n, Cout, Co8)) if train else None
        return L.unpad(out, B, F, T, Cout, x.dtype), saved

    def _backward_train(self, sv, dout: Tensor):
        net = self.net
        B, F, T, n, Cout, Co8 = sv["geo"]
        L = Launcher(self.lib, dout)

        def dense_bwd(xin, cin, cout, w, dy, need_dx=True):
            """gradients of y = x w^T + b over all (sequence, frame) rows -> (dx or None, dw [cout][cin], db [cout])"""
            L.alloc_ws([(cout, cin, 1, 1)], bwd=True)
            dx, dw, db = L.conv_bwd(xin, n, T, cin, cin, cout, 1, 1, w, dy, need_dx=need_dx)
            return dx, dw.view(cout, cin), db

        L1, L2 = sv["layers"]
        d8 = L.pad_cols(dout, n, T, Cout)
        dy, dwl, dbl = dense_bwd(L2["y"], L2["y"].shape[-1], Co8, sv["wl"], d8)
        grads_rev = [[dwl[:Cout], dbl[:Cout]]]
        for S, rnn, need_dx in ((L2, net.blstm2, True), (L1, net.blstm1, False)):
            HD, I, I8 = S["HD"], S["I"], S["I8"]
            ws = torch.empty(L.lib._dll.nbss_nb_blstm_ws_bytes(L.dt, HD), dtype=torch.uint8, device=L.dev)
            dg = torch.empty(n, T, 8 * HD, dtype=L.td, device=L.dev)
            whh = L.f32(rnn.weight_hh_l0), L.f32(rnn.weight_hh_l0_reverse)
            dyc = dy.contiguous()  # (named: a temporary would be returned to the allocator before the call that reads it is made)
            L.lib.call("nbss_nb_blstm_bwd", L.dt, n, T, HD, L.p(dyc), L.p(S["save"]), L.p(whh[0]), L.p(whh[1]), L.p(dg), L.p(ws), L.st)
            dx, dwih, dbih = dense_bwd(S["x"], I8, 8 * HD, S["wih"], dg, need_dx=need_dx)
            # recurrent weights: dW_hh = sum over (sequence, frame) of dG_t^T h_{t-1}; h_{t-1} = the direction's output one frame earlier in ITS order
            y = S["y"]
            gl = []
            for d in range(2):
                hp = torch.zeros(n, T, HD, dtype=L.td, device=L.dev)
                if d == 0:
                    hp[:, 1:] = y[:, :-1, :HD]
                else:
                    hp[:, :-1] = y[:, 1:, HD:]
                _, dwhh, _ = dense_bwd(hp, HD, 4 * HD, whh[d], dg[..., 4 * HD * d: 4 * HD * (d + 1)].contiguous(), need_dx=False)
                b = dbih[4 * HD * d: 4 * HD * (d + 1)]
                gl += [dwih[4 * HD * d: 4 * HD * (d + 1), :I], dwhh, b, b.clone()]
            grads_rev.append(gl)
            dy = dx[..., :I] if need_dx else None
        grads = grads_rev[2] + grads_rev[1] + grads_rev[0]
        return [g.reshape(prm.shape).to(prm.dtype) for g, prm in zip(grads, _param_list(net))]
