"""Tensor-level wrappers of the C ABI (include/nbss_hip.h): torch is used for device memory
and streams only.  Every function takes the library handle explicitly (`lib`); the product
passes `nbss_amd._lib.hip()`; tests may pass the host-emulator build to run the same kernel
sources on CPU tensors.  There is no other code path.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import torch
from torch import Tensor

from ._lib import (NBSS_BF16, NBSS_F32, NBSS_LOSS_MSE, NBSS_LOSS_PIT, NBSS_LOSS_SA_SDR, NBSS_LOSS_SCALE_INVARIANT, NBSS_LOSS_SI_SDR, NBSS_LOSS_SNR,
                   NBSS_SCALE_NORM_IF_EXCEED_1, NBSS_SCALE_TOGETHER, NBSS_SDR_ZERO_MEAN, NBSS_STOI_EXTENDED, _ERR, Cfg, Lib, NbssError)
from .params import param_table


def _is_emu(lib: Lib) -> bool:
    if not hasattr(lib, "_is_emu"):
        lib._is_emu = "emulator" in lib.build_info()
    return lib._is_emu


def stream_dtype(cfg: Cfg) -> torch.dtype:
    return torch.bfloat16 if cfg.dtype == NBSS_BF16 else torch.float32


def _ptr(lib: Lib, t: Optional[Tensor], dtype=None) -> Optional[int]:
    if t is None:
        return None
    if not t.is_contiguous():
        raise NbssError("nbss_amd ops need contiguous tensors")
    if dtype is not None and t.dtype != dtype:
        raise NbssError(f"expected {dtype}, got {t.dtype}")
    if _is_emu(lib):
        if t.device.type != "cpu":
            raise NbssError("the emulator library only takes CPU tensors")
    elif t.device.type != "cuda":
        raise NbssError("libnbss_hip.so needs tensors on a HIP device (no CPU fallback exists)")
    return t.data_ptr()


def _stream(lib: Lib, t: Tensor) -> Optional[int]:
    if _is_emu(lib):
        return None
    return torch.cuda.current_stream(t.device).cuda_stream


def random_params(lib: Lib, cfg: Cfg, device, seed: int = 0) -> Tensor:
    """flat fp32 parameter buffer with plausible random values (tools / micro-benchmarks: weights ~ N(0, fan_in^-1/2), norm
    weights 1, biases small) — no state_dict needed"""
    n = lib.nbss_param_count(C.byref(cfg))
    if n <= 0:
        raise NbssError("unsupported configuration")
    g = torch.Generator().manual_seed(seed)
    flat = torch.zeros(n, dtype=torch.float32)
    for name, (off, shape) in param_table(lib, cfg).items():
        k = 1
        for d in shape:
            k *= d
        if len(shape) == 1:
            is_norm_w = name.endswith("weight") and ("norm" in name or name.split(".")[-2] in ("0", "6"))
            v = torch.ones(k) if is_norm_w else (torch.full((k,), 0.25) if len(shape) == 1 and name.endswith(".2.weight") else 0.02 * torch.randn(k, generator=g))
        else:
            fan_in = k // shape[0]
            v = torch.randn(k, generator=g) / fan_in ** 0.5
        flat[off:off + k] = v
    return flat.to(device)


def flatten_params(lib: Lib, cfg: Cfg, p: Dict[str, Tensor], device) -> Tensor:
    """state_dict-style dict -> flat fp32 buffer in nbss_param_table order."""
    n = lib.nbss_param_count(C.byref(cfg))
    if n <= 0:
        raise NbssError("unsupported configuration")
    flat = torch.zeros(n, dtype=torch.float32)
    for name, (off, shape) in param_table(lib, cfg).items():
        t = p[name]
        if tuple(t.shape) != tuple(shape):
            raise NbssError(f"{name}: shape {tuple(t.shape)} != {shape}")
        flat[off:off + t.numel()] = t.detach().reshape(-1).to(torch.float32).cpu()
    return flat.to(device)


def pack_params(lib: Lib, cfg: Cfg, flat: Tensor, out: Optional[Tensor] = None) -> Tensor:
    nbytes = lib.nbss_packed_bytes(C.byref(cfg))
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=flat.device)
    lib.call("nbss_pack_params", C.byref(cfg), _ptr(lib, flat, torch.float32), _ptr(lib, out), _stream(lib, flat))
    return out


def encoder_fwd(lib, cfg, flat, packed, xin):
    y = torch.empty(cfg.B, cfg.F, cfg.T, cfg.H, dtype=stream_dtype(cfg), device=xin.device)
    lib.call("nbss_encoder_fwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, packed), _ptr(lib, xin, stream_dtype(cfg)), _ptr(lib, y), _stream(lib, xin))
    return y


def decoder_fwd(lib, cfg, flat, packed, x):
    out = torch.empty(cfg.B, cfg.F, cfg.T, cfg.C_out, dtype=torch.float32, device=x.device)
    lib.call("nbss_decoder_fwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, packed), _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, out), _stream(lib, x))
    return out


def fconv_fwd(lib, cfg, flat, packed, layer, which, x):
    y = torch.empty_like(x)
    lib.call("nbss_fconv_fwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, packed), layer, which, _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, y), _stream(lib, x))
    return y


def full_fwd(lib, cfg, flat, packed, layer, x):
    y = torch.empty_like(x)
    lib.call("nbss_full_fwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, packed), layer, _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, y), _stream(lib, x))
    return y


def scratch(nbytes: int, device) -> Tensor:
    """caller-owned scratch for the library (workspaces, saved activations).  NBSS_POISON_SCRATCH=1 (set by tests/conftest.py)
    fills it with 0xFF bytes — NaN in bf16 and fp32 — so that a kernel that reads scratch it has not written shows up as NaN in
    the checked outputs instead of passing on freshly mapped, zeroed pages."""
    t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    if os.environ.get("NBSS_POISON_SCRATCH") == "1":
        t.fill_(0xFF)
    return t


def mhsa_save(lib, cfg, device) -> Tensor:
    """buffer for what mhsa_bwd needs from the forward pass (attention output before out_proj + log-sum-exp rows)"""
    return scratch(lib.nbss_mhsa_save_bytes(C.byref(cfg)), device)


def mhsa_fwd(lib, cfg, flat, packed, layer, x, o_save=None):
    y = torch.empty_like(x)
    lib.call("nbss_mhsa_fwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, packed), layer, _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, y),
             _ptr(lib, o_save, torch.uint8 if o_save is not None else None), _stream(lib, x))
    return y


def mhsa_bwd(lib, cfg, flat, grads, packed, layer, x, dy, o_save, ws):
    dx = torch.empty_like(x)
    lib.call("nbss_mhsa_bwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, grads, torch.float32), _ptr(lib, packed), layer,
             _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, dy, stream_dtype(cfg)), _ptr(lib, o_save, torch.uint8), _ptr(lib, dx), _ptr(lib, ws),
             _stream(lib, x))
    return dx


def tconvffn_save(lib, cfg, device) -> Optional[Tensor]:
    """buffer for what a training-mode T-ConvFFN forward keeps for backward (None: this geometry / stream type recomputes instead)"""
    n = lib.nbss_tconvffn_save_bytes(C.byref(cfg))
    return scratch(n, device) if n > 0 else None


def tconvffn_fwd(lib, cfg, flat, packed, layer, x, t_save=None):
    y = torch.empty_like(x)
    lib.call("nbss_tconvffn_fwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, packed), layer, _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, y),
             _ptr(lib, t_save, torch.uint8) if t_save is not None else None, _stream(lib, x))
    return y


def workspace(lib, cfg, device) -> Tensor:
    return scratch(lib.nbss_workspace_bytes(C.byref(cfg)), device)


def tconvffn_bwd(lib, cfg, flat, grads, packed, layer, x, dy, ws, t_save=None):
    dx = torch.empty_like(x)
    lib.call("nbss_tconvffn_bwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, grads, torch.float32), _ptr(lib, packed), layer,
             _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, dy, stream_dtype(cfg)), _ptr(lib, t_save, torch.uint8) if t_save is not None else None,
             _ptr(lib, dx), _ptr(lib, ws), _stream(lib, x))
    return dx


def fconv_bwd(lib, cfg, flat, grads, packed, layer, which, x, dy, ws):
    dx = torch.empty_like(x)
    lib.call("nbss_fconv_bwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, grads, torch.float32), _ptr(lib, packed), layer, which,
             _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, dy, stream_dtype(cfg)), _ptr(lib, dx), _ptr(lib, ws), _stream(lib, x))
    return dx


def full_bwd(lib, cfg, flat, grads, packed, layer, x, dy, ws):
    dx = torch.empty_like(x)
    lib.call("nbss_full_bwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, grads, torch.float32), _ptr(lib, packed), layer,
             _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, dy, stream_dtype(cfg)), _ptr(lib, dx), _ptr(lib, ws), _stream(lib, x))
    return dx


def decoder_bwd(lib, cfg, flat, grads, packed, x, dout, ws):
    dx = torch.empty_like(x)
    lib.call("nbss_decoder_bwd", C.byref(cfg), _ptr(lib, flat), _ptr(lib, grads, torch.float32), _ptr(lib, packed),
             _ptr(lib, x, stream_dtype(cfg)), _ptr(lib, dout, torch.float32), _ptr(lib, dx), _ptr(lib, ws), _stream(lib, x))
    return dx


def encoder_bwd(lib, cfg, grads, xin, dy):
    lib.call("nbss_encoder_bwd", C.byref(cfg), _ptr(lib, grads, torch.float32), _ptr(lib, xin, stream_dtype(cfg)),
             _ptr(lib, dy, stream_dtype(cfg)), _stream(lib, xin))


def stft_tables(lib, n_fft: int, window: int, device) -> Tensor:
    nb = lib.nbss_stft_tables_bytes(n_fft)
    if nb <= 0:
        raise NbssError(f"n_fft={n_fft} is not supported (256 or 512)")
    tab = torch.empty(nb // 4, dtype=torch.float32, device=device)
    lib.call("nbss_stft_tables", n_fft, window, _ptr(lib, tab), _stream(lib, tab))
    return tab


def stft_norm_fwd(lib, n_fft, dtype, tables, x, ref_channel):
    """x [B,C,N] fp32 -> (X [B,F,T,2C] stream dtype, xrmm [B,F,T] fp32)"""
    B, Cc, N = x.shape
    F, T = n_fft // 2 + 1, N // (n_fft // 2) + 1
    X = torch.empty(B, F, T, 2 * Cc, dtype=torch.bfloat16 if dtype == NBSS_BF16 else torch.float32, device=x.device)
    xrmm = torch.empty(B, F, T, dtype=torch.float32, device=x.device)
    lib.call("nbss_stft_norm_fwd", n_fft, dtype, B, Cc, N, ref_channel, _ptr(lib, tables), _ptr(lib, x, torch.float32), _ptr(lib, X), _ptr(lib, xrmm),
             _stream(lib, x))
    return X, xrmm


def inorm_istft_fwd(lib, n_fft, tables, out, xrmm, N):
    """out [B,F,T,2S] fp32 -> y [B,S,N] fp32"""
    B, F, T, S2 = out.shape
    S = S2 // 2
    ws = torch.empty(lib.nbss_istft_ws_bytes(n_fft, B, S, N) // 4, dtype=torch.float32, device=out.device)
    y = torch.empty(B, S, N, dtype=torch.float32, device=out.device)
    lib.call("nbss_inorm_istft_fwd", n_fft, B, S, N, _ptr(lib, tables), _ptr(lib, out, torch.float32), _ptr(lib, xrmm, torch.float32), _ptr(lib, ws),
             _ptr(lib, y), _stream(lib, out))
    return y


def inorm_istft_bwd(lib, n_fft, tables, dy, xrmm):
    B, S, N = dy.shape
    F, T = xrmm.shape[1], xrmm.shape[2]
    dout = torch.empty(B, F, T, 2 * S, dtype=torch.float32, device=dy.device)
    lib.call("nbss_inorm_istft_bwd", n_fft, B, S, N, _ptr(lib, tables), _ptr(lib, dy, torch.float32), _ptr(lib, xrmm, torch.float32), _ptr(lib, dout),
             _stream(lib, dy))
    return dout


def pit_neg_sisdr(lib, preds, target, need_grad=True, return_items=False):
    """-> (loss [1], perm [B,S] int32, dpreds or None[, per-item losses [B]])"""
    B, S, N = preds.shape
    dev = preds.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    perm = torch.empty(B, S, dtype=torch.int32, device=dev)
    dp = torch.empty_like(preds) if need_grad else None
    ws = torch.empty(lib.nbss_pit_ws_bytes(B, S) // 4, dtype=torch.float32, device=dev)
    lib.call("nbss_pit_neg_sisdr", B, S, N, _ptr(lib, preds, torch.float32), _ptr(lib, target, torch.float32), _ptr(lib, loss), _ptr(lib, perm),
             _ptr(lib, dp), _ptr(lib, ws), _stream(lib, preds))
    if return_items:  # workspace tail (include/nbss_hip.h): ... | per-item loss [B] | pairing coefficients [3 B S]
        return loss, perm, dp, ws[ws.numel() - B - 3 * B * S: ws.numel() - 3 * B * S].clone()
    return loss, perm, dp


LOSS_KINDS = {"neg_si_sdr": NBSS_LOSS_SI_SDR, "neg_snr": NBSS_LOSS_SNR, "neg_sa_sdr": NBSS_LOSS_SA_SDR, "cc_mse": NBSS_LOSS_MSE}


def pit_loss(lib, kind, preds, target, pit=True, scale_invariant=False, need_grad=True, return_items=False):
    """the loss family of nbss_pit_loss: kind = NBSS_LOSS_* or the reference's function name (LOSS_KINDS); preds / target [B,S,...] (trailing
    dimensions are flattened: cc_mse hands in [B,S,F,T,2]); pit=False pairs estimate s with target s in the same single call
    -> (loss [1], perm [B,S] int32, dpreds (shaped as preds) or None[, per-item losses [B]])"""
    kind = LOSS_KINDS[kind] if isinstance(kind, str) else int(kind)
    B, S = preds.shape[:2]
    if target.shape != preds.shape or preds.dim() < 3:
        raise NbssError(f"pit_loss: preds {tuple(preds.shape)} and target {tuple(target.shape)} must be the same [B,S,...]")
    N = preds[0, 0].numel()
    dev = preds.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    perm = torch.empty(B, S, dtype=torch.int32, device=dev)
    dp = torch.empty_like(preds) if need_grad else None
    nws = lib.nbss_pit_loss_ws_bytes(kind, B, S)
    if nws <= 0:
        raise NbssError(f"nbss_pit_loss_ws_bytes(kind={kind}, B={B}, S={S}): no such loss kind or empty batch")
    ws = torch.empty(nws // 4, dtype=torch.float32, device=dev)
    flags = (NBSS_LOSS_PIT if pit else 0) | (NBSS_LOSS_SCALE_INVARIANT if scale_invariant else 0)
    lib.call("nbss_pit_loss", kind, flags, B, S, N, _ptr(lib, preds, torch.float32), _ptr(lib, target, torch.float32), _ptr(lib, loss), _ptr(lib, perm),
             _ptr(lib, dp), _ptr(lib, ws), _stream(lib, preds))
    if return_items:  # workspace tail (include/nbss_hip.h): ... | per-item loss [B] | pairing coefficients [3 B S]
        return loss, perm, dp, ws[ws.numel() - B - 3 * B * S: ws.numel() - 3 * B * S].clone()
    return loss, perm, dp


def _metric_pair(what, preds, target):
    if preds.dim() != 3 or target.shape != preds.shape:
        raise NbssError(f"{what}: preds {tuple(preds.shape)} and target {tuple(target.shape)} must be the same [B,S,N]")
    return preds.shape


def signal_ratios(lib, preds, target, ws=None):
    """preds / target [B,S,N] fp32, estimate s paired with target s -> [B,S,3] fp32: SNR, SI-SDR, SI-SNR in dB (nbss_signal_ratios)"""
    B, S, N = _metric_pair("signal_ratios", preds, target)
    if ws is None:
        nws = lib.nbss_signal_ratios_ws_bytes(B, S)
        if nws <= 0:
            raise NbssError(f"nbss_signal_ratios_ws_bytes(B={B}, S={S}): empty batch")
        ws = scratch(nws, preds.device)
    out = torch.empty(B, S, 3, dtype=torch.float32, device=preds.device)
    lib.call("nbss_signal_ratios", B, S, N, _ptr(lib, preds, torch.float32), _ptr(lib, target, torch.float32), _ptr(lib, out), _ptr(lib, ws, torch.uint8),
             _stream(lib, preds))
    return out


def sdr(lib, preds, target, filter_length: int = 512, zero_mean: bool = False, ws=None):
    """torchmetrics' signal_distortion_ratio of every (estimate s, target s): preds / target [B,S,N] fp32 -> [B,S] fp32 in dB (nbss_sdr)"""
    B, S, N = _metric_pair("sdr", preds, target)
    if ws is None:
        nws = lib.nbss_sdr_ws_bytes(B, S, N, int(filter_length))
        if nws <= 0:
            raise NbssError(f"nbss_sdr_ws_bytes(B={B}, S={S}, N={N}, filter_length={filter_length}): every size must be positive")
        ws = scratch(nws, preds.device)
    out = torch.empty(B, S, dtype=torch.float32, device=preds.device)
    lib.call("nbss_sdr", B, S, N, int(filter_length), NBSS_SDR_ZERO_MEAN if zero_mean else 0, _ptr(lib, preds, torch.float32), _ptr(lib, target, torch.float32),
             _ptr(lib, out), _ptr(lib, ws, torch.uint8), _stream(lib, preds))
    return out


def stoi(lib, preds, target, fs: int, extended: bool = False, ws=None):
    """STOI (extended: eSTOI) of every (estimate s, target s) as include/nbss_hip.h defines it: preds / target [B,S,N] fp32 at fs Hz -> [B,S] fp32"""
    B, S, N = _metric_pair("stoi", preds, target)
    if ws is None:
        nws = lib.nbss_stoi_ws_bytes(B, S, N, int(fs))
        if nws <= 0:
            raise NbssError(f"nbss_stoi_ws_bytes(B={B}, S={S}, N={N}, fs={fs}): {_ERR.get(int(nws), nws)} (fs in 8000 | 10000 | 16000, S <= 4, B <= 1024, "
                            "at least 257 samples at 10 kHz)")
        ws = scratch(nws, preds.device)
    out = torch.empty(B, S, dtype=torch.float32, device=preds.device)
    lib.call("nbss_stoi", B, S, N, int(fs), NBSS_STOI_EXTENDED if extended else 0, _ptr(lib, preds, torch.float32), _ptr(lib, target, torch.float32),
             _ptr(lib, out), _ptr(lib, ws, torch.uint8), _stream(lib, preds))
    return out


def recover_scale(lib, preds, mixture, scale_src_together: bool, norm_if_exceed_1: bool = True, ws=None):
    """preds [B,S,N], mixture [B,N] fp32 -> preds times the least-squares scales that explain the mixture (nbss_recover_scale)"""
    if preds.dim() != 3 or mixture.shape != (preds.shape[0], preds.shape[2]):
        raise NbssError(f"recover_scale: preds {tuple(preds.shape)} must be [B,S,N] and mixture {tuple(mixture.shape)} [B,N]")
    B, S, N = preds.shape
    if ws is None:
        nws = lib.nbss_recover_scale_ws_bytes(B, S)
        if nws <= 0:
            raise NbssError(f"nbss_recover_scale_ws_bytes(B={B}, S={S}): empty batch")
        ws = scratch(nws, preds.device)
    out = torch.empty_like(preds)
    flags = (NBSS_SCALE_TOGETHER if scale_src_together else 0) | (NBSS_SCALE_NORM_IF_EXCEED_1 if norm_if_exceed_1 else 0)
    lib.call("nbss_recover_scale", B, S, N, flags, _ptr(lib, preds, torch.float32), _ptr(lib, mixture, torch.float32), _ptr(lib, out),
             _ptr(lib, ws, torch.uint8), _stream(lib, preds))
    return out


def rir_tail_start(t_diff: float, fs: float) -> int:
    """k_d = ceil(t_diff fs): the first sample of the diffuse tail (include/nbss_hip.h: nbss_rir_tail)"""
    return int(math.ceil(float(t_diff) * float(fs) - 1e-9))


class RirTailError(ValueError):
    """a diffuse tail that would start at sample `k_d`, outside round(tw fs) <= k_d < n_samples, in room `room` (None for one t_diff for the batch)"""

    def __init__(self, msg: str, room: Optional[int], k_d: int):
        super().__init__(msg)
        self.room, self.k_d = room, k_d


def rir_tail_starts(t_diff, fs: float, B: int, n_samples: int, tw: float, what: str = "rir_ism") -> List[int]:
    """k_d[b] = rir_tail_start(t_diff[b], fs) of a per-room t_diff (a sequence or a [B] tensor of positive seconds), each checked against the
    kernels' limits round(tw fs) <= k_d[b] < n_samples; ValueError (RirTailError for the limits) names the room.  None, NaN or a value <= 0 is
    no entry: a batch without a tail is t_diff=None.  One number for the batch is checked once and gives B equal entries."""
    rooms = _per_room(t_diff)
    vals = [t_diff] if not rooms else t_diff.detach().reshape(-1).tolist() if torch.is_tensor(t_diff) else list(t_diff)
    if rooms and len(vals) != B:
        raise ValueError(f"{what}: a per-room t_diff needs one value per room, B = {B}, got {len(vals)}")
    K, out = int(round(float(tw) * float(fs))), []
    for b, v in enumerate(vals):
        if rooms and (v is None or not float(v) > 0.0 or math.isinf(float(v))):
            raise ValueError(f"{what}: t_diff[{b}] = {v!r} of room {b} must be a positive number of seconds (t_diff=None switches the tail off for every room)")
        k_d = rir_tail_start(v, fs)
        if not K <= k_d < int(n_samples):
            raise RirTailError(f"{what}: the diffuse tail must start at a sample k_d with {K} <= k_d < {int(n_samples)}, got {k_d}"
                               f"{f' for room {b}' if rooms else ''}", b if rooms else None, k_d)
        out.append(k_d)
    return out if rooms else out * B


def _per_room(t_diff) -> bool:
    """a t_diff with one value per room (a sequence, an array or a tensor with a dimension), not one number for the batch"""
    return isinstance(t_diff, (list, tuple)) or getattr(t_diff, "ndim", 0) > 0


def rir_ism(lib, room_sz, beta, pos_src, pos_rcv, nb_img, n_samples: int, fs: float, c: float = 343.0, tw: float = 8e-3, t_diff=None,
            rt60=None, seed: int = 0, ws=None, out=None):
    """image-source room impulse responses of a batch of rooms (nbss_rir_ism, with t_diff also nbss_rir_tail): room_sz [B,3], beta [B,6],
    pos_src [B,S,3], pos_rcv [B,M,3] (any float dtype: the kernel takes fp64), nb_img (Nx, Ny, Nz) shared or [B,3] per room (host integers)
    -> h [B,S,M,n_samples] fp32.  t_diff (seconds, with rt60 [B] or a number) switches to the diffuse tail from sample ceil(t_diff fs) on; a
    sequence or a [B] tensor of t_diff switches per room (nbss_rir_ism_rooms, nbss_rir_tail_rooms)."""
    dev = room_sz.device
    f64 = lambda t: t.detach().to(device=dev, dtype=torch.float64).contiguous()
    room_sz, beta, pos_src, pos_rcv = f64(room_sz), f64(beta), f64(pos_src), f64(pos_rcv)
    if room_sz.dim() != 2 or room_sz.shape[1] != 3 or pos_src.dim() != 3 or pos_rcv.dim() != 3 or pos_src.shape[2] != 3 or pos_rcv.shape[2] != 3:
        raise NbssError(f"rir_ism: room_sz {tuple(room_sz.shape)} must be [B,3], pos_src {tuple(pos_src.shape)} [B,S,3], pos_rcv {tuple(pos_rcv.shape)} [B,M,3]")
    B, S, M = room_sz.shape[0], pos_src.shape[1], pos_rcv.shape[1]
    if beta.shape != (B, 6) or pos_src.shape[0] != B or pos_rcv.shape[0] != B:
        raise NbssError(f"rir_ism: beta {tuple(beta.shape)} must be [B,6] and every tensor must hold B = {B} rooms")
    nb = torch.as_tensor(nb_img, device="cpu").to(torch.int32).reshape(-1, 3)
    nb = (nb.expand(B, 3) if nb.shape[0] == 1 else nb).contiguous()
    if nb.shape[0] != B:
        raise NbssError(f"rir_ism: nb_img must be (Nx, Ny, Nz) or [B,3], got {tuple(nb.shape)}")
    nws = lib.nbss_rir_ism_ws_bytes(B, nb.data_ptr())
    if nws < 0:
        raise NbssError(f"nbss_rir_ism_ws_bytes failed: {_ERR.get(nws, nws)}")
    if ws is None:
        ws = scratch(nws, dev)
    rooms = _per_room(t_diff)
    if rooms:
        k_ds = torch.tensor(rir_tail_starts(t_diff, fs, B, n_samples, tw), dtype=torch.int32)  # host array, read before the calls return
    else:
        k_d = 0 if t_diff is None else rir_tail_start(t_diff, fs)
    h = torch.empty(B, S, M, int(n_samples), dtype=torch.float32, device=dev) if out is None else out
    if h.shape != (B, S, M, int(n_samples)):
        raise NbssError(f"rir_ism: out must be [B,S,M,n_samples] = {(B, S, M, int(n_samples))}, got {tuple(h.shape)}")
    lib.call("nbss_rir_ism_rooms" if rooms else "nbss_rir_ism", B, S, M, int(n_samples), float(fs), float(c), float(tw), k_ds.data_ptr() if rooms else k_d,
             _ptr(lib, room_sz), _ptr(lib, beta), _ptr(lib, pos_src), _ptr(lib, pos_rcv), nb.data_ptr(), _ptr(lib, h, torch.float32), _ptr(lib, ws, torch.uint8),
             ws.numel(), _stream(lib, h))
    if t_diff is not None:
        if rt60 is None:
            raise NbssError("rir_ism: the diffuse tail (t_diff) needs rt60")
        rt = torch.as_tensor(rt60, dtype=torch.float64).to(dev).reshape(-1)
        rt = (rt.expand(B) if rt.numel() == 1 else rt).contiguous()
        if rt.numel() != B:
            raise NbssError(f"rir_ism: rt60 must be a number or [B], got {tuple(rt.shape)}")
        lib.call("nbss_rir_tail_rooms" if rooms else "nbss_rir_tail", B, S, M, int(n_samples), float(fs), float(tw), k_ds.data_ptr() if rooms else k_d,
                 _ptr(lib, rt), int(seed), _ptr(lib, h), _stream(lib, h))
    return h


def rir_delay(lib, h, ref_channel: int = 0):
    """h [B,S,M,L] fp32 -> delay [B,S] int32: the index of the maximum of h[b,s,ref_channel,:], the lowest one on a tie (nbss_rir_delay)"""
    if h.dim() != 4:
        raise NbssError(f"rir_delay: h {tuple(h.shape)} must be [B,S,M,L]")
    B, S, M, L = h.shape
    delay = torch.empty(B, S, dtype=torch.int32, device=h.device)
    lib.call("nbss_rir_delay", B, S, M, L, int(ref_channel), _ptr(lib, h, torch.float32), _ptr(lib, delay), _stream(lib, h))
    return delay


def _conv_run(lib, fn: str, x, M: int, out, check: bool, call, why: str):
    """what fir_convolve and fir_convolve_traj share: the output [B,S,M,N] (`out`, checked, or a new tensor), the status word, the library call
    call(y pointer, status pointer) and, with `check`, the read-back: a status other than 0 raises NBSS_EINVAL with `why`"""
    B, S, N = x.shape
    y = torch.empty(B, S, M, N, dtype=torch.float32, device=x.device) if out is None else out
    if y.shape != (B, S, M, N):
        raise NbssError(f"{fn}: out must be [B,S,M,N] = {(B, S, M, N)}, got {tuple(y.shape)}")
    status = torch.zeros(1, dtype=torch.int32, device=x.device) if check else None
    call(_ptr(lib, y, torch.float32), _ptr(lib, status))
    if check and int(status.item()) != 0:
        raise NbssError(f"nbss_{fn} failed: {_ERR[-1]}: {why}")
    return y


def fir_convolve(lib, x, h, delay, check: bool = True, out=None):
    """x [B,S,N], h [B,S,M,L] fp32, delay [B,S] int32 on the same device -> y [B,S,M,N] fp32 with y[b,s,m,n] = sum_k h[b,s,m,k] x[b,s,n + delay[b,s] - k]
    (nbss_fir_convolve: the window of the linear convolution that starts at the delay).  The kernel validates the delays; with `check` the status word
    is read back (one synchronisation) and a delay outside [0, L) raises NBSS_EINVAL.  check=False is for delays that come from rir_delay."""
    if x.dim() != 3 or h.dim() != 4 or h.shape[:2] != x.shape[:2] or tuple(delay.shape) != tuple(x.shape[:2]):
        raise NbssError(f"fir_convolve: x {tuple(x.shape)} must be [B,S,N], h {tuple(h.shape)} [B,S,M,L] and delay {tuple(delay.shape)} [B,S]")
    B, S, N = x.shape
    M, L = h.shape[2], h.shape[3]
    call = lambda y, status: lib.call("nbss_fir_convolve", B, S, M, N, L, _ptr(lib, x, torch.float32), _ptr(lib, h, torch.float32),
                                      _ptr(lib, delay, torch.int32), y, status, _stream(lib, x))
    return _conv_run(lib, "fir_convolve", x, M, out, check, call, f"a delay lies outside [0, L = {L})")


TRAJ_MODES = {'switch': 0, 'trapezium': 1}


def fir_convolve_traj(lib, x, h, hop, delay, mode: str = 'trapezium', ramp: int = 20, check: bool = True, out=None):
    """x [B,S,N], h [B,S,P,M,L] fp32 (one RIR set per trajectory point), hop [B,S] and delay [B,S] int32 on the same device -> y [B,S,M,N] fp32: the
    source sample j is heard through RIR j // hop (mode 'switch') or cross-faded between RIRs j // hop and j // hop + 1 by a trapezium window with
    `ramp` samples per slope (mode 'trapezium'), and the result is the window of the full convolution that starts at the delay
    (nbss_fir_convolve_traj; include/nbss_hip.h has the closed form).  The kernel validates the items; with `check` the status word is read back (one
    synchronisation) and a hop < 1, a hop <= ramp or ramp < 2 when cross-fading, too few trajectory points or a delay outside [0, L) raise NBSS_EINVAL."""
    if mode not in TRAJ_MODES:
        raise NbssError(f"fir_convolve_traj: mode must be 'switch' or 'trapezium', got {mode!r}")
    if (x.dim() != 3 or h.dim() != 5 or h.shape[:2] != x.shape[:2] or tuple(hop.shape) != tuple(x.shape[:2])
            or tuple(delay.shape) != tuple(x.shape[:2])):
        raise NbssError(f"fir_convolve_traj: x {tuple(x.shape)} must be [B,S,N], h {tuple(h.shape)} [B,S,P,M,L], hop {tuple(hop.shape)} and "
                        f"delay {tuple(delay.shape)} [B,S]")
    B, S, N = x.shape
    P, M, L = h.shape[2:]
    call = lambda y, status: lib.call("nbss_fir_convolve_traj", B, S, P, M, N, L, TRAJ_MODES[mode], int(ramp), _ptr(lib, x, torch.float32),
                                      _ptr(lib, h, torch.float32), _ptr(lib, hop, torch.int32), _ptr(lib, delay, torch.int32), y, status, _stream(lib, x))
    return _conv_run(lib, "fir_convolve_traj", x, M, out, check, call,
                     f"a hop is < 1{' or <= ramp, ramp is < 2' if mode == 'trapezium' else ''}, P = {P} trajectory points are too few for a hop, or a "
                     f"delay lies outside [0, L = {L})")


def diffuse_noise(lib, white, Cs, nfft: int = 256, out=None):
    """white [B,M,N] fp32 (M mutually independent noises per item), Cs [F,M,M] complex64 (F = nfft // 2 + 1; the mixing matrices of
    diffuse_mixing_matrices, shared by the batch) on the same device -> noise [B,M,N] fp32: mean removal, STFT, X[n] = sum_m conj(Cs[f,m,n]) N[m],
    inverse STFT, in one kernel (nbss_diffuse_noise; include/nbss_hip.h has the definition).  Arguments that do not fit raise ValueError, a negative
    code of the library NbssError."""
    if white.dim() != 3 or white.dtype != torch.float32 or not white.is_contiguous():
        raise ValueError(f"diffuse_noise: white must be a contiguous fp32 [B,M,N] tensor, got {tuple(white.shape)} {white.dtype}"
                         f"{'' if white.is_contiguous() else ', not contiguous'}")
    B, M, N = white.shape
    if Cs.dtype != torch.complex64 or tuple(Cs.shape) != (nfft // 2 + 1, M, M) or Cs.device != white.device:
        raise ValueError(f"diffuse_noise: Cs must be complex64 [F,M,M] = {(nfft // 2 + 1, M, M)} on {white.device}, got {tuple(Cs.shape)} {Cs.dtype} on {Cs.device}")
    if white.device.type != ("cpu" if _is_emu(lib) else "cuda"):
        raise ValueError("diffuse_noise: the emulator library only takes CPU tensors" if _is_emu(lib) else
                         "diffuse_noise: libnbss_hip.so needs tensors on a HIP device (no CPU fallback exists)")
    y = torch.empty_like(white) if out is None else out
    if y.shape != white.shape or y.device != white.device:
        raise ValueError(f"diffuse_noise: out must be [B,M,N] = {(B, M, N)} on {white.device}, got {tuple(y.shape)} on {y.device}")
    nb = lib.nbss_diffuse_noise_ws_bytes(B, M)
    if nb < 0:
        raise NbssError(f"nbss_diffuse_noise_ws_bytes failed: {_ERR.get(nb, nb)}")
    ws = scratch(nb, white.device)
    lib.call("nbss_diffuse_noise", int(nfft), B, M, N, _ptr(lib, white, torch.float32), _ptr(lib, torch.view_as_real(Cs.contiguous()), torch.float32),
             _ptr(lib, ws), _ptr(lib, y, torch.float32), _stream(lib, white))
    return y


def clip_adam_step(lib, params, grads, exp_avg, exp_avg_sq, scratch, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                   max_norm=5.0, grad_scale=1.0, zero_grad=True, decoupled_weight_decay=False):
    lib.call("nbss_clip_adam_step", params.numel(), _ptr(lib, params, torch.float32), _ptr(lib, grads, torch.float32), _ptr(lib, exp_avg, torch.float32),
             _ptr(lib, exp_avg_sq, torch.float32), _ptr(lib, scratch, torch.float32), float(max_norm), float(grad_scale), float(lr), float(betas[0]),
             float(betas[1]), float(eps), float(weight_decay), int(step), int(bool(zero_grad)) | (2 if decoupled_weight_decay else 0), _stream(lib, params))


def clip_adam_step_dev(lib, params, grads, exp_avg, exp_avg_sq, scratch, hyper, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=5.0,
                       grad_scale=1.0, zero_grad=True, decoupled_weight_decay=False):
    """clip_adam_step with the per-step scalars read from the DEVICE buffer `hyper` = [lr, 1 - beta1^step, sqrt(1 - beta2^step)] (filled by
    nbss_adam_hyper on the host): the launch sequence has no per-step arguments and can be replayed from a HIP graph"""
    lib.call("nbss_clip_adam_step_dev", params.numel(), _ptr(lib, params, torch.float32), _ptr(lib, grads, torch.float32), _ptr(lib, exp_avg, torch.float32),
             _ptr(lib, exp_avg_sq, torch.float32), _ptr(lib, scratch, torch.float32), _ptr(lib, hyper, torch.float32), float(max_norm), float(grad_scale),
             float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(bool(zero_grad)) | (2 if decoupled_weight_decay else 0), _stream(lib, params))


def selftest_mma(lib, dtype: int, kperm: int, A: Tensor, B: Tensor) -> Tensor:
    D = torch.empty(16, 16, dtype=torch.float32, device=A.device)
    lib.call("nbss_selftest_mma", dtype, kperm, _ptr(lib, A, torch.float32), _ptr(lib, B, torch.float32), _ptr(lib, D), _stream(lib, A))
    return D


def graph_guard_save(ctx, runner, saved, params):
    """state of a native autograd.Function between forward and backward: the runner, its module (kept alive while the graph is), the saved device
    tensors and the version counters of the parameters backward will re-read from the live module"""
    ctx.runner, ctx.net, ctx.saved, ctx.params = runner, runner.net, saved, params
    ctx.versions = [p._version for p in params]


def graph_guard_check(ctx, what: str):
    """torch.nn raises when a tensor saved for backward was modified in place or the graph was already freed; the native paths re-read the module's
    parameters in backward, so they check the same two conditions themselves"""
    if ctx.saved is None:
        raise RuntimeError(f"{what}: trying to backward through the graph a second time: the native path frees its saved state after the first backward "
                           "(retain_graph is not supported)")
    for p, v in zip(getattr(ctx, "params", ()), getattr(ctx, "versions", ())):  # (a node that saved no parameters has none to check)
        if p._version != v:
            raise RuntimeError(f"{what}: a parameter needed for the gradient computation was modified in place between forward and backward "
                               f"(shape {tuple(p.shape)}, version {p._version}, expected {v})")


# ---- OnlineSpatialNet: the blocks for training (csrc/online_train.hip, online_ret_train.hip, online_tsa_train.hip, online_xband_train.hip, online_mamba_train.hip)
# The four blocks with parameters are one `OnlineBlock` record each and share one driver (`_online_fwd` / `_online_bwd`); the records state where the entry
# points differ.  The retention core alone (four tensor inputs, no parameters, four gradients) keeps its two functions on the shared `_online_dims`.
def _online_bytes(lib: Lib, name: str, *dims: int) -> int:
    n = getattr(lib, name)(*dims)
    if n < 0:
        raise NbssError(f"{name} failed: {_ERR.get(n, n)}")
    return n


def _online_dims(what: str, name: str, t: Tensor, width: int, ranks=(3,)):
    """`t` must be fp32 or bf16, `width` wide and of a rank in `ranks` -> (dtype, B, F, T) for ranks (4,), else (dtype, BF, T) with the leading sizes folded"""
    if t.dim() not in ranks or t.shape[-1] != width or t.dtype not in (torch.float32, torch.bfloat16):
        shapes = " or ".join(f"[BF,T,{width}]" if r == 3 else f"[B,F,T,{width}]" for r in ranks)
        raise NbssError(f"{what}: {name} must be {shapes} in fp32 or bf16, got {tuple(t.shape)} {t.dtype}")
    dt = NBSS_BF16 if t.dtype == torch.bfloat16 else NBSS_F32
    return (dt, *t.shape[:3]) if ranks == (4,) else (dt, math.prod(t.shape[:-2]), t.shape[-2])


@dataclass(frozen=True)
class OnlineBlock:
    """the C ABI of one block with parameters (include/nbss_hip.h).  Forward: (dtype, sizes..., inputs..., y, save, ws, stream); backward: (dtype, sizes...,
    inputs..., save, dy, dx, one gradient per parameter..., ws, stream); the two size functions: (dtype, sizes..., extras...)."""
    what: str  # the label in errors
    fwd: str  # the four C symbols
    bwd: str
    save_bytes: str
    ws_bytes: str
    x: str  # the input: its name in errors, its width, the ranks it may have (`_online_dims`) and the width of the output
    width: int
    out_width: int
    ranks: tuple
    sizes: Callable  # (F, or None without a frequency axis) -> the element count of every parameter slot
    want: str  # ... in words, for the refusal ({F}, {sizes} are filled in)
    grads_want: Optional[str] = None  # the refusal of a wrong `grads` where it has a wording of its own
    optional: tuple = ()  # the slots that may be None (TSA: wk, absent with shared keys)
    consts: int = 0  # trailing slots that are inputs without a gradient (TSA: decay)
    size_extra: Callable = lambda params: ()  # the extra integers the two size functions take (TSA: share_qk)
    x_first: bool = False  # the input stands before the parameters in the call (Mamba), not after them
    new_grad: Callable = torch.empty_like  # a gradient buffer when `grads` is not given: the backward WRITES it; torch.zeros_like: it ACCUMULATES (T-ConvFFN)
    cached_ws: bool = False  # the workspace is the shared cached one (`_online_ws`), not a fresh one per call


_T3 = 192 * 24 * 3  # a T-conv of the T-ConvFFN: 192 channels in 8 groups, 3 taps
ONLINE_TCONVFFN = OnlineBlock(
    what="online T-ConvFFN", fwd="nbss_online_tconvffn_train_fwd", bwd="nbss_online_tconvffn_train_bwd",
    save_bytes="nbss_online_tconvffn_train_save_bytes", ws_bytes="nbss_online_tconvffn_train_ws_bytes", x="x", width=96, out_width=96, ranks=(4,),
    sizes=lambda F: (96, 96, 192 * 96, 192, _T3, 192, _T3, 192, 192, 192, _T3, 192, 96 * 192, 96),
    want="the 14 tensors of LayerNorm, 1x1, T-conv, T-conv, GroupNorm, T-conv, 1x1 (weight, bias each) of {sizes} elements", new_grad=torch.zeros_like)
ONLINE_XBAND = OnlineBlock(
    what="online cross-band", fwd="nbss_online_xband_train_fwd", bwd="nbss_online_xband_train_bwd", save_bytes="nbss_online_xband_save_bytes",
    ws_bytes="nbss_online_xband_ws_bytes", x="x", width=96, out_width=96, ranks=(4,),
    sizes=lambda F: (96, 96, 96 * 12 * 5, 96, 96, 96, 96, 8 * 96, 8, 8 * F * F, 8 * F, 96 * 8, 96, 96, 96, 96 * 12 * 5, 96, 96),
    want="the 18 tensors of fconv1, norm_full, squeeze, full, unsqueeze, fconv2 for {F} frequencies", cached_ws=True)
# y = x + out_proj(SiLU(g) * RMSNorm_head(chunk_retention(q, k, v))) on LayerNorm(x)
ONLINE_TSA = OnlineBlock(
    what="online retention block", fwd="nbss_online_tsa_train_fwd", bwd="nbss_online_tsa_train_bwd", save_bytes="nbss_online_tsa_save_bytes",
    ws_bytes="nbss_online_tsa_ws_bytes", x="x", width=96, out_width=96, ranks=(3, 4),
    sizes=lambda F: (96, 96, 96 * 96, 96 * 96, 192 * 96, 192 * 96, 96 * 192, 4),
    want="(ln_w, ln_b, wq, wk or None, wv, wg, wo, decay) of 96, 96, 96x96, 96x96, 192x96, 192x96, 96x192 and 4 elements",
    grads_want="grads must match the seven parameters (None where the parameter is absent, and at decay)", optional=(3,), consts=1,
    size_extra=lambda params: (int(params[3] is None),), cached_ws=True)
# y * SiLU(z) from xz = in_proj(u)
ONLINE_MAMBA = OnlineBlock(
    what="online Mamba core", fwd="nbss_online_mamba_train_fwd", bwd="nbss_online_mamba_train_bwd", save_bytes="nbss_online_mamba_train_save_bytes",
    ws_bytes="nbss_online_mamba_train_ws_bytes", x="xz", width=384, out_width=192, ranks=(3,),
    sizes=lambda F: (192 * 4, 192, 38 * 192, 192 * 6, 192, 192 * 16, 192),
    want="(conv1d.weight, conv1d.bias, x_proj.weight, dt_proj.weight, dt_proj.bias, A_log, D) of {sizes} elements", x_first=True)


def _online_check(rec: OnlineBlock, which: str, tensors, F, none_at):
    """the entry points take bare pointers: `tensors` ('params' or 'grads') must have the sizes the kernels will read / write, and None exactly at `none_at`"""
    want = rec.sizes(F)
    expect, got = list(want), [None if t is None else t.numel() for t in tensors]
    for i in none_at:
        expect[i] = None
    if got != expect:
        if which == "grads" and rec.grads_want is not None:
            raise NbssError(f"{rec.what}: {rec.grads_want}")
        raise NbssError(f"{rec.what}: {which} must be {rec.want.format(F=F, sizes=want)} (got sizes {got})")


def _online_head(rec: OnlineBlock, params, x: Tensor):
    """the checks both directions share -> (dtype, sizes...), F or None, the size functions' extras"""
    dims = _online_dims(rec.what, rec.x, x, rec.width, rec.ranks)
    F = dims[2] if rec.ranks == (4,) else None
    _online_check(rec, "params", params, F, [i for i in rec.optional if i < len(params) and params[i] is None])
    return dims, F, rec.size_extra(params)


def _online_ws(rec: OnlineBlock, lib: Lib, dims, extra, device) -> Tensor:
    """the workspace of a call: fresh, or with rec.cached_ws ONE buffer per (library, device, dtype, extras), shared by every layer and both directions (the
    calls are in order on one stream and each writes what it reads).  A new shape frees the old buffer before the new one is allocated.  The slots live on the
    Lib object and go with it."""
    if not rec.cached_ws:
        return scratch(_online_bytes(lib, rec.ws_bytes, *dims, *extra), device)
    slots, slot = vars(lib).setdefault("_online_ws", {}), (rec.ws_bytes, device, dims[0], *extra)
    if slot not in slots or slots[slot][0] != dims[1:]:
        slots.pop(slot, None)
        slots[slot] = (dims[1:], scratch(_online_bytes(lib, rec.ws_bytes, *dims, *extra), device))
    return slots[slot][1]


def _online_ins(rec: OnlineBlock, lib: Lib, params, x: Tensor):
    """the pointers of the inputs in the order of the block's entry points"""
    ps, xs = [_ptr(lib, p, torch.float32) for p in params], [_ptr(lib, x)]
    return xs + ps if rec.x_first else ps + xs


def _online_fwd(rec: OnlineBlock, lib: Lib, params, x: Tensor, keep: bool = True, ws: Optional[Tensor] = None):
    """the forward of a block -> (y, save): `save` is what the backward needs (None with keep=False); `ws` overrides the workspace"""
    dims, _, extra = _online_head(rec, params, x)
    y = torch.empty_like(x) if rec.out_width == rec.width else x.new_empty((*x.shape[:-1], rec.out_width))
    save = scratch(_online_bytes(lib, rec.save_bytes, *dims, *extra), x.device) if keep else None
    if ws is None:
        ws = _online_ws(rec, lib, dims, extra, x.device)  # (held until the call returns)
    lib.call(rec.fwd, *dims, *_online_ins(rec, lib, params, x), _ptr(lib, y), _ptr(lib, save), _ptr(lib, ws), _stream(lib, x))
    return y, save


def _online_bwd(rec: OnlineBlock, lib: Lib, params, x: Tensor, save: Tensor, dy: Tensor, grads=None, ws: Optional[Tensor] = None):
    """the backward of the same -> (dx, grads): `grads` has the slots of `params` (None where a parameter is absent or a constant)"""
    dims, F, extra = _online_head(rec, params, x)
    if tuple(dy.shape) != (*x.shape[:-1], rec.out_width) or dy.dtype != x.dtype:
        like = f"x {tuple(x.shape)}" if rec.out_width == rec.width else f"[{dims[1]},{dims[2]},{rec.out_width}]"
        raise NbssError(f"{rec.what}: dy {tuple(dy.shape)} {dy.dtype} does not match {like} {x.dtype}")
    n = len(params) - rec.consts
    if grads is None:
        grads = [None if p is None else rec.new_grad(p) for p in params[:n]] + [None] * rec.consts
    else:
        _online_check(rec, "grads", grads, F, [i for i, p in enumerate(params) if p is None or i >= n])
    dx = torch.empty_like(x)
    if ws is None:
        ws = _online_ws(rec, lib, dims, extra, x.device)
    lib.call(rec.bwd, *dims, *_online_ins(rec, lib, params, x), _ptr(lib, save), _ptr(lib, dy), _ptr(lib, dx), *(_ptr(lib, g, torch.float32) for g in grads[:n]),
             _ptr(lib, ws), _stream(lib, x))
    return dx, grads


def _online_sizer(name: str):
    return lambda lib, dtype, B, F, T: _online_bytes(lib, name, dtype, B, F, T)


online_tconvffn_train_save_bytes, online_tconvffn_train_ws_bytes = _online_sizer(ONLINE_TCONVFFN.save_bytes), _online_sizer(ONLINE_TCONVFFN.ws_bytes)
online_xband_save_bytes, online_xband_ws_bytes = _online_sizer(ONLINE_XBAND.save_bytes), _online_sizer(ONLINE_XBAND.ws_bytes)


def online_tconvffn_train_fwd(lib: Lib, params: List[Tensor], x: Tensor, keep: bool = True):
    """y = x + T-ConvFFN(x) on x [B,F,T,96] (fp32 or bf16); params: the 14 fp32 tensors in the order of include/nbss_hip.h (state_dict layout).
    -> (y, save): `save` is what online_tconvffn_train_bwd needs (None with keep=False: inference)"""
    return _online_fwd(ONLINE_TCONVFFN, lib, params, x, keep)


def online_tconvffn_train_bwd(lib: Lib, params: List[Tensor], x: Tensor, save: Tensor, dy: Tensor, grads: Optional[List[Tensor]] = None):
    """-> (dx, grads): dx includes the residual path; the 14 fp32 parameter gradients are ACCUMULATED into `grads` (zeros of the parameters' shapes when
    not given)"""
    return _online_bwd(ONLINE_TCONVFFN, lib, params, x, save, dy, grads)


def online_xband_ws(lib: Lib, x: Tensor) -> Tensor:
    """the workspace of the cross-band entry points for the shape of x: ONE buffer per (library, device, dtype, shape), shared by every layer and by both
    directions (its largest part is the reused backward kernels' workspace, ~0.9 GB at batch 4 in fp32; the calls are in order on one stream and each
    writes what it reads).  A new shape on the same device and dtype replaces the old buffer."""
    return _online_ws(ONLINE_XBAND, lib, _online_dims(ONLINE_XBAND.what, "x", x, 96, (4,)), (), x.device)


def online_xband_train_fwd(lib: Lib, params: List[Tensor], x: Tensor, keep: bool = True, ws: Optional[Tensor] = None):
    """y = the cross-band trio (x + fconv1, + full, + fconv2) on x [B,F,T,96] (fp32 or bf16); params: the 18 fp32 tensors in state_dict order.
    -> (y, save): `save` (the inputs of the second and third block) is what online_xband_train_bwd needs (None with keep=False: inference)"""
    return _online_fwd(ONLINE_XBAND, lib, params, x, keep, ws)


def online_xband_train_bwd(lib: Lib, params: List[Tensor], x: Tensor, save: Tensor, dy: Tensor, grads: Optional[List[Tensor]] = None,
                           ws: Optional[Tensor] = None):
    """-> (dx, grads): dx includes the residual paths; the 18 fp32 parameter gradients are WRITTEN into `grads` (uninitialised buffers of the parameters'
    shapes when not given)"""
    return _online_bwd(ONLINE_XBAND, lib, params, x, save, dy, grads, ws)


def online_tsa_ws(lib: Lib, dt: int, BF: int, T: int, share: int, device) -> Tensor:
    """the workspace of the retention-block entry points: ONE buffer per (library, device, dtype, keys), shared by every layer and both directions (the calls
    are in order on one stream and each writes what it reads); a new shape replaces the old buffer"""
    return _online_ws(ONLINE_TSA, lib, (dt, BF, T), (share,), device)


def online_tsa_save_views(lib: Lib, save: Tensor, x: Tensor, share_qk: bool) -> Dict[str, Optional[Tensor]]:
    """q, k (None with shared keys), v, g, go (the gated core output) and stats as views of what online_tsa_train_fwd kept (include/nbss_hip.h: the layout)"""
    BF, T = x.numel() // (x.shape[-2] * 96), x.shape[-2]
    esz, out, o = x.element_size(), {}, 0
    flat = save.view(torch.uint8).reshape(-1)
    for name, width, dtype, size in (("q", 96, x.dtype, esz), ("k", 96, x.dtype, esz), ("v", 192, x.dtype, esz), ("g", 192, x.dtype, esz),
                                     ("go", 192, x.dtype, esz), ("stats", 2, torch.float32, 4)):
        if name == "k" and share_qk:
            out[name] = None
            continue
        n = BF * T * width * size
        out[name] = flat[o:o + n].view(dtype).reshape(BF, T, width)
        o += (n + 255) // 256 * 256
    return out


def online_tsa_train_fwd(lib: Lib, params: List[Optional[Tensor]], x: Tensor, keep: bool = True):
    """y = x + the retention block on x [BF,T,96] or [B,F,T,96] (fp32 or bf16); params: the fp32 tensors (ln_w, ln_b, wq, wk or None: shared keys, wv, wg, wo)
    in state_dict layout and decay [4], the per-head gamma.  -> (y, save): `save` is what online_tsa_train_bwd needs (None with keep=False: inference)"""
    return _online_fwd(ONLINE_TSA, lib, params, x, keep)


def online_tsa_train_bwd(lib: Lib, params: List[Optional[Tensor]], x: Tensor, save: Tensor, dy: Tensor, grads: Optional[List[Optional[Tensor]]] = None):
    """-> (dx, grads): dx includes the residual path; the fp32 gradients of the seven parameters are WRITTEN into `grads` (eight entries in the order of
    `params`: None at wk with shared keys and at decay; uninitialised buffers of the parameters' shapes when not given)"""
    return _online_bwd(ONLINE_TSA, lib, params, x, save, dy, grads)


def online_mamba_train_fwd(lib: Lib, params: List[Tensor], xz: Tensor, keep: bool = True):
    """out [BF,T,192] = y * SiLU(z) of Mamba(96, d_state 16, d_conv 4, expand 2) on xz [BF,T,384] (fp32 or bf16); params: the seven fp32 tensors in
    state_dict layout.  -> (out, save): `save` is what online_mamba_train_bwd needs (None with keep=False: inference)"""
    return _online_fwd(ONLINE_MAMBA, lib, params, xz, keep)


def online_mamba_train_bwd(lib: Lib, params: List[Tensor], xz: Tensor, save: Tensor, dy: Tensor, grads: Optional[List[Tensor]] = None):
    """-> (dxz, grads): the seven fp32 parameter gradients are WRITTEN into `grads` (uninitialised buffers of the parameters' shapes when not given)"""
    return _online_bwd(ONLINE_MAMBA, lib, params, xz, save, dy, grads)


# the chunkwise retention core
def _online_ret_inputs(q: Tensor, k: Optional[Tensor], v: Tensor, g: Tensor):
    dt, BF, T = _online_dims("online retention", "q", q, 96)
    for name, t, width in (("k", k, 96), ("v", v, 192), ("g", g, 192)):
        if t is not None and (tuple(t.shape) != (BF, T, width) or t.dtype != q.dtype):
            raise NbssError(f"online retention: {name} must be [{BF},{T},{width}] {q.dtype}, got {tuple(t.shape)} {t.dtype}")
    return dt, BF, T


def online_ret_train_fwd(lib: Lib, q: Tensor, k: Optional[Tensor], v: Tensor, g: Tensor, k_scale: float, decay: Tensor, keep: bool = True):
    """out [BF,T,192] = SiLU(g) * RMSNorm_head(chunkwise retention(q, k_scale k, v)); k = None shares the keys with q; decay [4] fp32: the per-head gamma.
    -> (out, save): `save` is what online_ret_train_bwd needs (None with keep=False: inference)"""
    dt, BF, T = _online_ret_inputs(q, k, v, g)
    out = torch.empty_like(v)
    save = scratch(_online_bytes(lib, "nbss_online_ret_train_save_bytes", dt, BF, T), q.device) if keep else None
    ws = scratch(_online_bytes(lib, "nbss_online_ret_train_ws_bytes", dt, BF, T), q.device)
    lib.call("nbss_online_ret_train_fwd", dt, BF, T, _ptr(lib, q), _ptr(lib, k), _ptr(lib, v), _ptr(lib, g), k_scale, _ptr(lib, decay, torch.float32),
             _ptr(lib, out), _ptr(lib, save), _ptr(lib, ws), _stream(lib, q))
    return out, save


def online_ret_train_bwd(lib: Lib, q: Tensor, k: Optional[Tensor], v: Tensor, g: Tensor, k_scale: float, decay: Tensor, save: Tensor, d_out: Tensor):
    """-> (dq, dk, dv, dg), written (not accumulated); dk includes k_scale and is None when k is (dq then holds both roles of q)"""
    dt, BF, T = _online_ret_inputs(q, k, v, g)
    if d_out.shape != v.shape or d_out.dtype != v.dtype:
        raise NbssError(f"online retention: d_out {tuple(d_out.shape)} {d_out.dtype} does not match v {tuple(v.shape)} {v.dtype}")
    dq, dk, dv, dg = torch.empty_like(q), None if k is None else torch.empty_like(q), torch.empty_like(v), torch.empty_like(v)
    ws = scratch(_online_bytes(lib, "nbss_online_ret_train_ws_bytes", dt, BF, T), q.device)
    lib.call("nbss_online_ret_train_bwd", dt, BF, T, _ptr(lib, q), _ptr(lib, k), _ptr(lib, v), _ptr(lib, g), k_scale, _ptr(lib, decay, torch.float32),
             _ptr(lib, save), _ptr(lib, d_out), _ptr(lib, dq), _ptr(lib, dk), _ptr(lib, dv), _ptr(lib, dg), _ptr(lib, ws), _stream(lib, q))
    return dq, dk, dv, dg

