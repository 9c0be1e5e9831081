"""Loss — drop-in for the reference's models/io/loss.py: the callables the YAMLs name (`neg_si_sdr`, configs/SpatialNet.yaml:38; `neg_snr`, the
reference's configs/onlineSpatialNet.yaml; `neg_sa_sdr`, `cc_mse`) and `Loss(loss_func, pit, loss_func_kwargs).forward(yr_hat, yr, reorder,
reduce_batch, **loss_paras) -> (loss, perms, yr_hat)`, `to_CC`.  For tensors on a HIP device every supported loss, with or without PIT, runs on the MI355X
kernels (nbss_amd/csrc/loss_optim.hip, which restate torchmetrics' si_sdr / snr / sa_sdr / pit): neg_si_sdr through nbss_pit_neg_sisdr, the others through
nbss_pit_loss.  Host tensors (`trainer.accelerator=cpu`) go through the same closed forms in torch.
Supported: neg_si_sdr, neg_snr, neg_sa_sdr (scale_invariant False | True), cc_mse.  Not supported: cirm_mse — it needs the mask pair of the reference's
models/io/cirm.py (build_complex_ideal_ratio_mask / decompress_cIRM), which is not ported; it raises NotImplementedError."""
import itertools
from typing import Any, Callable, Dict, Tuple

import torch
from torch import Tensor, nn


def _identity_pairing(p: Tensor, t: Tensor, need_grad: bool):
    """no PIT: speaker s of the estimate is paired with speaker s of the target = the PIT kernel on one speaker at a time
    (S launches, not B*S); returns (mean loss [1], per-item loss [B], d loss / d p or None)"""
    from nbss_amd import ops
    from nbss_amd._lib import hip
    S = p.shape[1]
    parts = [ops.pit_neg_sisdr(hip(), p[:, s:s + 1].contiguous(), t[:, s:s + 1].contiguous(), need_grad=need_grad, return_items=True) for s in range(S)]
    loss = sum(x[0] for x in parts) / S
    items = sum(x[3] for x in parts) / S
    dp = torch.cat([x[2] for x in parts], 1) / S if need_grad else None
    return loss, items, dp


class _PitSiSdrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, target, pit: bool):
        from nbss_amd import ops
        from nbss_amd._lib import hip
        B, S, N = preds.shape
        p, t = preds.float().contiguous(), target.float().contiguous()
        if pit:
            loss, perm, dp, items = ops.pit_neg_sisdr(hip(), p, t, need_grad=True, return_items=True)
        else:
            loss, items, dp = _identity_pairing(p, t, True)
            perm = torch.arange(S, device=p.device, dtype=torch.int32).expand(B, S).contiguous()
        ctx.save_for_backward(dp)
        ctx.mark_non_differentiable(perm, items)
        return loss.reshape(()), perm, items

    @staticmethod
    def backward(ctx, dloss, _p, _i):
        (dp,) = ctx.saved_tensors
        return dp * dloss, None, None


def _host_pair_sisdr(p: Tensor, t: Tensor) -> Tensor:
    """[B,S,N] x [B,S,N] -> SI-SDR of every (estimate i, target j) pair [B,S,S] (zero_mean=False; eps = float32 machine epsilon)"""
    eps = torch.finfo(p.dtype).eps
    pt = torch.einsum("bin,bjn->bij", p, t)
    tt, pp = (t * t).sum(-1)[:, None, :], (p * p).sum(-1)[:, :, None]
    alpha = (pt + eps) / (tt + eps)
    num = alpha * alpha * tt
    return 10 * torch.log10((num + eps) / (num - 2 * alpha * pt + pp + eps))


def _host_pit(p: Tensor, t: Tensor, pit: bool):
    """host (torch, differentiable) uPIT neg-SI-SDR: per-item loss [B] and the pairing perm [B,S] (perm[s] = estimate paired with target s)"""
    B, S, _ = p.shape
    sd = _host_pair_sisdr(p.float(), t.float())
    perms = list(itertools.permutations(range(S))) if pit else [tuple(range(S))]
    vals = torch.stack([-sum(sd[:, pm[s], s] for s in range(S)) / S for pm in perms], 1)  # [B, S!] in itertools order (torchmetrics' order)
    best, idx = vals.min(1)
    return best, torch.tensor(perms, dtype=torch.long, device=p.device)[idx]


def neg_si_sdr(preds: Tensor, target: Tensor) -> Tensor:
    """-mean over speakers of SI-SDR, shape [batch] (loss.py:21-29)"""
    if not preds.is_cuda:
        return _host_pit(preds, target, False)[0]
    return _identity_pairing(preds.float().contiguous(), target.float().contiguous(), False)[1]


class _PitLossFn(torch.autograd.Function):
    """one nbss_pit_loss call: mean loss, pairing, per-item losses; the gradient is the kernel's d loss / d preds"""

    @staticmethod
    def forward(ctx, preds, target, kind: str, pit: bool, scale_invariant: bool):
        from nbss_amd import ops
        from nbss_amd._lib import hip
        p, t = preds.float().contiguous(), target.float().contiguous()
        loss, perm, dp, items = ops.pit_loss(hip(), kind, p, t, pit=pit, scale_invariant=scale_invariant, need_grad=True, return_items=True)
        ctx.save_for_backward(dp)
        ctx.mark_non_differentiable(perm, items)
        return loss.reshape(()), perm, items

    @staticmethod
    def backward(ctx, dloss, _p, _i):
        (dp,) = ctx.saved_tensors
        return dp * dloss, None, None, None, None


def _host_family(kind: str, p: Tensor, t: Tensor, scale_invariant: bool = False) -> Tensor:
    """host (torch, differentiable) closed forms of torchmetrics' snr / sa_sdr and of _mse (loss.py:15-18,32-53): p, t [B,S,...] -> loss [B]"""
    B, S = p.shape[:2]
    p, t = p.float().reshape(B, S, -1), t.float().reshape(B, S, -1)
    eps = torch.finfo(torch.float32).eps
    if kind == "neg_snr":
        return -(10 * torch.log10(((t * t).sum(-1) + eps) / (((t - p) ** 2).sum(-1) + eps))).mean(1)
    if kind == "neg_sa_sdr":
        if scale_invariant:
            alpha = ((p * t).sum((1, 2), keepdim=True) + eps) / ((t * t).sum((1, 2), keepdim=True) + eps)
            t = alpha * t
        return -10 * torch.log10(((t * t).sum((1, 2)) + eps) / (((t - p) ** 2).sum((1, 2)) + eps))
    assert kind == "cc_mse", kind
    return ((p - t) ** 2).mean((1, 2))


def _host_pit_family(kind: str, p: Tensor, t: Tensor, pit: bool, scale_invariant: bool = False):
    """host uPIT of the family: the loss of (p[:, perm], t) for every perm in itertools order, the smallest per item (the first wins a tie)"""
    S = p.shape[1]
    perms = list(itertools.permutations(range(S))) if pit else [tuple(range(S))]
    vals = torch.stack([_host_family(kind, p[:, list(pm)], t, scale_invariant) for pm in perms], 1)
    best, idx = vals[:, 0], torch.zeros(p.shape[0], dtype=torch.long, device=p.device)
    for k in range(1, len(perms)):
        better = vals[:, k] < best
        best, idx = torch.where(better, vals[:, k], best), torch.where(better, torch.full_like(idx, k), idx)
    return best, torch.tensor(perms, dtype=torch.long, device=p.device)[idx]


def _family_items(kind: str, preds: Tensor, target: Tensor, scale_invariant: bool = False) -> Tensor:
    if preds.dim() < 3:  # [B,N]: one source per item
        preds, target = preds[:, None], target[:, None]
    if not preds.is_cuda:
        return _host_family(kind, preds, target, scale_invariant)
    from nbss_amd import ops
    from nbss_amd._lib import hip
    return ops.pit_loss(hip(), kind, preds.float().contiguous(), target.float().contiguous(), pit=False, scale_invariant=scale_invariant,
                        need_grad=False, return_items=True)[3]


def neg_snr(preds: Tensor, target: Tensor) -> Tensor:
    """-mean over speakers of torchmetrics' signal_noise_ratio, shape [batch] (loss.py:32-40)"""
    return _family_items("neg_snr", preds, target)


def neg_sa_sdr(preds: Tensor, target: Tensor, scale_invariant: bool = False) -> Tensor:
    """-source-aggregated SDR over the speaker axis, shape [batch] (loss.py:15-18; the reference's default is scale_invariant=False)"""
    return _family_items("neg_sa_sdr", preds, target, scale_invariant)


def cc_mse(preds: Tensor, target: Tensor) -> Tensor:
    """mean squared error of a batch of STFT coefficients (real view), shape [batch] (loss.py:43-53,65-71)"""
    return _family_items("cc_mse", preds, target)


def cirm_mse(preds: Tensor, target: Tensor) -> Tensor:
    raise NotImplementedError("cirm_mse needs the cIRM mask pair of the reference's models/io/cirm.py (build_complex_ideal_ratio_mask / decompress_cIRM), "
                              "which is not ported; neg_si_sdr, neg_snr, neg_sa_sdr and cc_mse are supported")


class Loss(nn.Module):
    is_scale_invariant_loss: bool
    name: str
    mask: str

    def __init__(self, loss_func: Callable, pit: bool, loss_func_kwargs: Dict[str, Any] = dict()):
        super().__init__()
        if isinstance(loss_func, str):  # YAML callable path
            import importlib
            mod, _, fn = loss_func.rpartition(".")
            loss_func = getattr(importlib.import_module(mod), fn)
        if loss_func is cirm_mse:
            cirm_mse(None, None)  # raises, with the reason
        table = {  # loss.py:85-91
            neg_sa_sdr: bool(loss_func_kwargs.get("scale_invariant", False) == True),  # noqa: E712 (the reference's comparison)
            neg_si_sdr: True,
            neg_snr: False,
            cc_mse: False,
        }
        if loss_func not in table:
            raise NotImplementedError(f"Loss({getattr(loss_func, '__name__', loss_func)}): the MI355X kernels implement neg_si_sdr, neg_snr, neg_sa_sdr and cc_mse")
        unknown = sorted(set(loss_func_kwargs) - ({"scale_invariant"} if loss_func is neg_sa_sdr else set()))
        if unknown:
            raise TypeError(f"{loss_func.__name__}() got unexpected keyword arguments {unknown}")
        self.loss_func, self.pit, self.loss_func_kwargs = loss_func, pit, loss_func_kwargs
        self.is_scale_invariant_loss = table[loss_func]
        self.name = loss_func.__name__
        self.mask = None

    def forward(self, yr_hat: Tensor, yr: Tensor, reorder: bool = None, reduce_batch: bool = True, **kwargs) -> Tuple[Tensor, Tensor, Tensor]:
        if self.loss_func is neg_si_sdr:
            if not yr_hat.is_cuda:  # host path
                items, perm = _host_pit(yr_hat, yr, self.pit)
                loss = items.mean()
            else:
                loss, perm, items = _PitSiSdrFn.apply(yr_hat, yr, self.pit)
        else:
            if self.loss_func is cc_mse:  # STFT-domain loss on the normalised coefficients (loss.py:101-105)
                for k in ("out", "XrMM", "stft"):
                    if kwargs.get(k) is None:
                        raise ValueError(f"Loss(cc_mse).forward needs the keyword argument '{k}' (TrainModule passes its loss_paras: out, XrMM, stft)")
                Yr, _ = kwargs["stft"].stft(yr)
                preds, target = torch.view_as_real(kwargs["out"]), torch.view_as_real(Yr / kwargs["XrMM"])
            else:
                preds, target = yr_hat, yr
            si = bool(self.loss_func_kwargs.get("scale_invariant", False))
            if not preds.is_cuda:
                items, perm = _host_pit_family(self.name, preds, target, self.pit, si)
                loss = items.mean()
            else:
                loss, perm, items = _PitLossFn.apply(preds, target, self.name, self.pit, si)
        if not reduce_batch:  # the reference's test step: one loss per utterance (loss.py:111-118), no gradient
            loss = items
        perms = perm.long() if self.pit else None
        if reorder and perms is not None:
            yr_hat = torch.gather(yr_hat, 1, perms[..., None].expand_as(yr_hat))  # torchmetrics pit_permutate
        return loss, perms, yr_hat

    def to_CC(self, out: Tensor, Xr: Tensor, stft, XrMM: Tensor):
        return out, {"out": out, "Xr": Xr, "stft": stft, "XrMM": XrMM}

    def extra_repr(self) -> str:
        kwargs = "".join(f"{k}={v}," for k, v in self.loss_func_kwargs.items())
        return f"loss_func={self.loss_func.__name__}({kwargs}), pit={self.pit}, mask={self.mask}"
