"""Mamba — the selective state-space block (Gu & Dao, "Mamba: Linear-Time Sequence Modeling with Selective State Spaces", 2023) in plain torch, written
from the published equations with the constructor arguments and state_dict keys of `mamba_ssm.Mamba`, so that a checkpoint trained with that package
loads here.  It stands in for mamba_ssm (a CUDA-only wheel: nothing of it runs on an MI355X), parity with that package is NOT pinned: it is not installed
where this project is tested.

    E = expand d_model, R = ceil(d_model / 16), N = d_state, K = d_conv
    x, z   = split(in_proj(u))                                        [.., E] each
    x      = SiLU(causal depthwise conv_K(x) + conv1d.bias)           K - 1 zeros on the left
    dt_r, B, C = split(x_proj(x))                                     R, N, N
    dt     = softplus(dt_proj.weight dt_r + dt_proj.bias)
    A      = -exp(A_log)
    h_t[e,n] = exp(dt_t[e] A[e,n]) h_{t-1}[e,n] + dt_t[e] B_t[n] x_t[e]      h_{-1} = 0
    y_t[e] = sum_n C_t[n] h_t[e,n] + D[e] x_t[e]
    out    = out_proj(y * SiLU(z))

`core(xz)` is everything between in_proj and out_proj: what the HIP kernels of nbss_amd/csrc/online_mamba_train.hip compute for the width-96 block
(nbss_amd/online_train.py: MAMBA) and what their tests differentiate in fp64.  `step` is the same recurrence for one frame on an explicit state
(`init_state`: the last K - 1 inputs of the convolution and h)."""
import math
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor


class Mamba(nn.Module):
    def __init__(self, d_model: int, d_state: int = 16, d_conv: int = 4, expand: int = 2, dt_rank="auto", dt_min: float = 0.001, dt_max: float = 0.1,
                 dt_init_floor: float = 1e-4, layer_idx: Optional[int] = None, device=None, dtype=None) -> None:
        super().__init__()
        kw = {"device": device, "dtype": dtype}
        self.d_model, self.d_state, self.d_conv, self.expand = d_model, d_state, d_conv, expand
        self.d_inner = expand * d_model
        self.dt_rank = math.ceil(d_model / 16) if dt_rank == "auto" else dt_rank
        self.layer_idx = layer_idx  # (accepted for mamba_ssm's signature; unused)
        E, R, N = self.d_inner, self.dt_rank, d_state
        self.in_proj = nn.Linear(d_model, 2 * E, bias=False, **kw)
        self.conv1d = nn.Conv1d(E, E, kernel_size=d_conv, groups=E, padding=d_conv - 1, bias=True, **kw)
        self.x_proj = nn.Linear(E, R + 2 * N, bias=False, **kw)
        self.dt_proj = nn.Linear(R, E, bias=True, **kw)
        nn.init.uniform_(self.dt_proj.weight, -R ** -0.5, R ** -0.5)
        dt = torch.exp(torch.rand(E, **kw) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min)).clamp(min=dt_init_floor)
        with torch.no_grad():
            self.dt_proj.bias.copy_(dt + torch.log(-torch.expm1(-dt)))  # softplus^-1(dt)
        self.A_log = nn.Parameter(torch.log(torch.arange(1, N + 1, dtype=torch.float32, device=device)).repeat(E, 1).to(dtype or torch.float32))
        self.D = nn.Parameter(torch.ones(E, **kw))
        self.out_proj = nn.Linear(E, d_model, bias=False, **kw)

    # ---- whole sequences -------------------------------------------------------------------------------------------------------------------------------
    def core(self, xz: Tensor) -> Tensor:
        """xz [BF,T,2E] (the output of in_proj) -> y * SiLU(z) [BF,T,E] (the input of out_proj)"""
        E, R, N, K = self.d_inner, self.dt_rank, self.d_state, self.d_conv
        T = xz.shape[1]
        x, z = xz[..., :E], xz[..., E:]
        x = F.silu(F.conv1d(F.pad(x.transpose(1, 2), (K - 1, 0)), self.conv1d.weight, self.conv1d.bias, groups=E).transpose(1, 2))
        dt_r, Bm, Cm = torch.split(F.linear(x, self.x_proj.weight), [R, N, N], dim=-1)
        dt = F.softplus(F.linear(dt_r, self.dt_proj.weight, self.dt_proj.bias))
        # the recurrence in fp32 at least (under autocast the linear maps above come back in bf16; the state must not be rounded to it)
        st = torch.promote_types(self.A_log.dtype, torch.float32)
        x, dt, Bm, Cm = x.to(st), dt.to(st), Bm.to(st), Cm.to(st)
        A = -torch.exp(self.A_log.to(st))
        decay = torch.exp(dt.unsqueeze(-1) * A)  # [BF,T,E,N]
        drive = (dt * x).unsqueeze(-1) * Bm.unsqueeze(2)
        h = torch.zeros(xz.shape[0], E, N, dtype=st, device=xz.device)
        ys = []
        for t in range(T):
            h = decay[:, t] * h + drive[:, t]
            ys.append((h * Cm[:, t].unsqueeze(1)).sum(-1))
        y = torch.stack(ys, dim=1) + self.D.to(st) * x
        return y * F.silu(z.to(st))

    def forward(self, u: Tensor, inference_params=None) -> Tensor:
        """u [BF,T,d_model] -> [BF,T,d_model]"""
        assert inference_params is None, "stream with `step` on an explicit state"
        return self.out_proj(self.core(self.in_proj(u)).to(u.dtype))

    # ---- one frame on an explicit state ----------------------------------------------------------------------------------------------------------------
    def init_state(self, batch: int, device=None, dtype=None) -> Dict[str, Tensor]:
        """{"conv": the last K - 1 inputs of the convolution [batch,E,K-1], "ssm": h [batch,E,N]}, zeros: no frame seen yet"""
        dev, dt = device if device is not None else self.D.device, dtype if dtype is not None else self.D.dtype
        return {"conv": torch.zeros(batch, self.d_inner, self.d_conv - 1, device=dev, dtype=dt),
                "ssm": torch.zeros(batch, self.d_inner, self.d_state, device=dev, dtype=dt)}

    def step(self, u: Tensor, state: Dict[str, Tensor]) -> Tensor:
        """u [BF,1,d_model] (or [BF,d_model]): the next frame -> the frame of forward(); `state` gets the new tensors (not written in place)"""
        E, R, N = self.d_inner, self.dt_rank, self.d_state
        squeeze = u.dim() == 2
        xz = self.in_proj(u.reshape(u.shape[0], -1))
        x, z = xz[:, :E], xz[:, E:]
        win = torch.cat([state["conv"], x.unsqueeze(-1)], dim=-1)  # [BF,E,K]
        state["conv"] = win[..., 1:]
        x = F.silu((win * self.conv1d.weight[:, 0]).sum(-1) + self.conv1d.bias)
        dt_r, Bm, Cm = torch.split(F.linear(x, self.x_proj.weight), [R, N, N], dim=-1)
        dt = F.softplus(F.linear(dt_r, self.dt_proj.weight, self.dt_proj.bias))
        A = -torch.exp(self.A_log)
        h = torch.exp(dt.unsqueeze(-1) * A) * state["ssm"] + (dt * x).unsqueeze(-1) * Bm.unsqueeze(1)
        state["ssm"] = h
        y = (h * Cm.unsqueeze(1)).sum(-1) + self.D * x
        out = self.out_proj(y * F.silu(z))
        return out if squeeze else out.unsqueeze(1)
