"""On-GPU simulation of multichannel noisy-reverberant mixtures: the per-item numpy pipeline of the
reference's dataset modules, batched on the device so that the loader keeps up with the HIP training step (hundreds of utterances/s
per GPU; the reference's 10 CPU workers produce far fewer):
    dry sources  --RIR convolution (FFT, or convolve='native': csrc/conv1d.hip), aligned to the direct path of the reference channel-->  images / targets
    --relative scaling of speaker 2 to a sampled SIR-->  mixture  --spatially diffuse noise (torch.fft, or diffuse='native': csrc/diffuse.hip) at a sampled SNR-->
    peak scaling 0.9
following data_loaders/sms_wsj_plus.py:157-220, utils/mix.py:122-134 (convolve), :328-346 (energy ratio), utils/diffuse_noise.py:19-93
(spherically isotropic coherence sinc(w d / c), mixing matrices from its eigendecomposition, STFT-domain mixing of independent
noises).  Everything is torch (hipFFT / rocSOLVER through torch-ROCm) and device-agnostic: the CPU tests check it against
scipy and, when the reference tree is present, against the reference's own functions.
The corpora (WSJ0, measured/simulated RIR sets) are not available here: `SimulatedRoomDataModule` draws band-limited random
sources and, by default, synthetic exponentially decaying RIRs; with rir='ism' it draws shoebox rooms and computes their impulse
responses by the image-source method on the device (nbss_amd/rir.py: simulate_rir), and with moving=(vmin, vmax[, prob]) the speakers walk:
a trajectory of responses per speaker, cross-faded along the source (utils/mix.py:197-244; convolve_traj_aligned, csrc/conv_traj.hip).
With rir_att_diff (dB; the reference's generate_rirs.py uses 15) every room sums its images only to that much of its own decay and continues
with the diffuse tail of nbss_rir_tail (simulate_rir with one t_diff per room); None, the default, sums every image down to 60 dB.
`mix_batch` itself takes any sources / RIRs."""
import math
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from data_loaders.synthetic import rank_strided_indices
from nbss_amd import ops
from nbss_amd.ops import TRAJ_MODES
from nbss_amd.rir import TW, att2t, beta_sabine, rotate_z, simulate_rir, t2n


def fft_convolve(x: Tensor, h: Tensor) -> Tensor:
    """full linear convolution along the last axis (scipy.signal.fftconvolve(mode='full')); leading dims broadcast"""
    n = x.shape[-1] + h.shape[-1] - 1
    nfft = 1 << (n - 1).bit_length()
    return torch.fft.irfft(torch.fft.rfft(x, nfft) * torch.fft.rfft(h, nfft), nfft)[..., :n]


def convolve_aligned(wav: Tensor, rir: Tensor, rir_target: Optional[Tensor] = None, ref_channel: int = 0) -> Tuple[Tensor, Tensor]:
    """wav [B,S,N], rir [B,S,M,L] -> (reverberant image, target image) [B,S,M,N], both cut from the direct-path delay of the
    reference channel of `rir` (utils/mix.py:122-134, align=True)"""
    B, S, N = wav.shape
    full = fft_convolve(wav[:, :, None, :], rir)
    tgt = full if rir_target is None else fft_convolve(wav[:, :, None, :], rir_target)
    delay = rir[:, :, ref_channel].argmax(-1)  # [B,S]
    idx = delay[:, :, None, None] + torch.arange(N, device=wav.device)[None, None, None, :]
    idx = idx.expand(B, S, rir.shape[2], N)
    return full.gather(-1, idx), tgt.gather(-1, idx)


CONVOLVE_MODES = ('fft', 'native')


def _native_lib(lib, t: Tensor, what: str):
    """the library of a native path: `lib` when one is handed in (the tests' emulator build), else the product library, which takes device tensors only"""
    if lib is not None:
        return lib
    if not t.is_cuda:
        raise ValueError(f"{what}='native' runs the HIP kernels and needs tensors on the device; use {what}='fft' on the host")
    from nbss_amd._lib import hip
    return hip()


def convolve_aligned_native(wav: Tensor, rir: Tensor, rir_target: Optional[Tensor] = None, ref_channel: int = 0, lib=None) -> Tuple[Tensor, Tensor]:
    """convolve_aligned by the HIP kernels of csrc/conv1d.hip: the delay by nbss_rir_delay (the lowest index of the maximum), then one direct
    convolution per RIR set (nbss_fir_convolve) that forms only the N samples from the delay onward; without `rir_target` the same tensor is
    returned twice.  Device tensors only: a host tensor raises ValueError (`lib` lets the tests hand in the emulator build of the same kernels)."""
    lib = _native_lib(lib, wav, 'convolve')
    wav, rir = wav.float().contiguous(), rir.float().contiguous()
    delay = ops.rir_delay(lib, rir, ref_channel)
    full = ops.fir_convolve(lib, wav, rir, delay, check=False)  # the delays come from rir_delay: inside [0, L)
    if rir_target is None:
        return full, full
    if rir_target.shape[:3] != rir.shape[:3]:
        raise ValueError(f"rir_target {tuple(rir_target.shape)} must match rir {tuple(rir.shape)} in [B,S,M]")
    # a target response shorter than the delay would put it outside [0, L): checked by the kernel (one synchronisation) only in that case
    return full, ops.fir_convolve(lib, wav, rir_target.float().contiguous(), delay, check=rir_target.shape[-1] != rir.shape[-1])


def _check_convolve(convolve: str) -> None:
    if convolve not in CONVOLVE_MODES:
        raise ValueError(f"convolve must be 'fft' or 'native', got {convolve!r}")


def traj_rirs_needed(N: int, hop: int, mode: str = 'trapezium') -> int:
    """RIRs that N source samples need at `hop` samples per trajectory point: ceil(N / hop) when switched (mix.py:171-174), ceil((N + hop - 1) / hop)
    when cross-faded (mix.py:231, len(range(0, N + hop - 1, hop)))"""
    return -(-N // hop) if mode == 'switch' else -(-(N + hop - 1) // hop)


def _check_traj(N: int, hmin: int, P: Optional[int], mode: str, ramp: int) -> int:
    """the checks of a trajectory of P responses (None: as many as needed) for N samples at no fewer than hmin samples per point -> P"""
    if mode not in TRAJ_MODES:
        raise ValueError(f"traj mode must be 'switch' or 'trapezium', got {mode!r}")
    if hmin < 1 or (mode == 'trapezium' and (ramp < 2 or hmin <= ramp)):
        raise ValueError(f"every hop must be >= 1, and > ramp = {ramp} >= 2 for the trapezium window; the smallest hop is {hmin}")
    need = traj_rirs_needed(N, hmin, mode)
    if P is not None and P < need:
        raise ValueError(f"{P} trajectory points are too few for {N} samples at {hmin} samples per point in mode {mode!r}: {need} are needed")
    return need if P is None else P


def traj_weights(N: int, hop, mode: str = 'trapezium', ramp: int = 20, P: Optional[int] = None, dtype=torch.float32, device=None) -> Tensor:
    """w [..., P, N]: the weight with which RIR p of a trajectory hears the source sample j, for `hop` (an int, or an integer tensor [...]) samples
    per trajectory point.  With q = j // hop and r = j % hop, 'switch' (mix.py:151-194, convolve_traj) gives RIR q the weight 1; 'trapezium'
    (mix.py:197-244, convolve_traj_with_win(..., f'trapezium{ramp}')) gives RIR q the weight down(r) and RIR q + 1 the weight up(r): the two halves
    of the reference's window [zeros(z), arange(ramp) / (ramp - 1), ones(2 o), the ramp reversed, zeros(z)], z = (hop - ramp) // 2, o = hop - ramp - z.
    P defaults to what the smallest hop needs; a larger P gives zero rows."""
    hop = torch.as_tensor(hop, device=device).long()
    P = _check_traj(N, int(hop.min()), P, mode, ramp)
    return torch.stack([_traj_weight_row(N, hop, p, mode, ramp, dtype) for p in range(P)], -2)


def _traj_weight_row(N: int, hop: Tensor, p: int, mode: str, ramp: int, dtype) -> Tensor:
    """w_p [..., N] of traj_weights for one trajectory point (hop an integer tensor [...], already validated)"""
    H = hop[..., None]
    t = torch.arange(N, device=hop.device) - p * H          # the source sample relative to the point's own segment [p H, (p + 1) H)
    here = (t >= 0) & (t < H)
    if mode == 'switch':
        return here.to(dtype)
    z = (H - ramp) // 2
    o = H - ramp - z
    down = ((ramp - 1 - (t - o)).to(dtype) / (ramp - 1)).clamp(0, 1)   # heard through `down` inside the own segment ...
    up = ((t + H - z).to(dtype) / (ramp - 1)).clamp(0, 1)               # ... and through `up` inside the segment before it
    return here.to(dtype) * down + ((t >= -H) & (t < 0)).to(dtype) * up


def convolve_traj_aligned(wav: Tensor, rir: Tensor, hop: Tensor, rir_target: Optional[Tensor] = None, mode: str = 'trapezium', ramp: int = 20,
                          ref_channel: int = 0, convolve: str = 'fft', lib=None) -> Tuple[Tensor, Tensor]:
    """wav [B,S,N], rir [B,S,P,M,L] (one RIR set per trajectory point), hop [B,S] (source samples per trajectory point) -> (reverberant image, target
    image) [B,S,M,N] of MOVING sources: the time-varying convolution of traj_weights, both cut from the direct-path delay of the reference channel at
    the FIRST trajectory point of `rir_target` (of `rir` without one), as chime3_moving.py:202-204 does.
    convolve: 'fft' (the default, any device: one fft_convolve of the weighted source per trajectory point, accumulated) or 'native'
    (nbss_fir_convolve_traj, csrc/conv_traj.hip: device tensors only, `lib` as in convolve_aligned_native)."""
    _check_convolve(convolve)
    if wav.dim() != 3 or rir.dim() != 5 or rir.shape[:2] != wav.shape[:2] or tuple(hop.shape) != tuple(wav.shape[:2]):
        raise ValueError(f"wav {tuple(wav.shape)} must be [B,S,N], rir {tuple(rir.shape)} [B,S,P,M,L] and hop {tuple(hop.shape)} [B,S]")
    if rir_target is not None and rir_target.shape[:4] != rir.shape[:4]:
        raise ValueError(f"rir_target {tuple(rir_target.shape)} must match rir {tuple(rir.shape)} in [B,S,P,M]")
    B, S, N = wav.shape
    P, M = rir.shape[2], rir.shape[3]
    first = (rir if rir_target is None else rir_target)[:, :, 0]  # [B,S,M,L']: the delay is that of the first trajectory point
    if convolve == 'native':
        lib = _native_lib(lib, wav, 'convolve')
        wav, rir, hop32 = wav.float().contiguous(), rir.float().contiguous(), hop.to(torch.int32).contiguous()
        delay = ops.rir_delay(lib, first.float().contiguous(), ref_channel)
        # the mode is checked by ops, the hops and P by the kernel: one status read-back (a synchronisation) covers both calls; the delay comes from
        # the target and is inside its [0, L')
        try:
            full = ops.fir_convolve_traj(lib, wav, rir, hop32, delay, mode=mode, ramp=ramp, check=True)
        except ops.NbssError as e:
            raise ValueError(str(e)) from e
        if rir_target is None:
            return full, full
        return full, ops.fir_convolve_traj(lib, wav, rir_target.float().contiguous(), hop32, delay, mode=mode, ramp=ramp, check=False)
    hop = hop.to(wav.device).long()
    _check_traj(N, int(hop.min()), P, mode, ramp)
    delay = first[:, :, ref_channel].argmax(-1)
    idx = (delay[:, :, None, None] + torch.arange(N, device=wav.device)[None, None, None, :]).expand(B, S, M, N)

    def image(h: Tensor) -> Tensor:
        if h.shape[-1] <= int(delay.max()):
            raise ValueError(f"a delay of {int(delay.max())} lies outside the response of {h.shape[-1]} samples")
        full = None
        for p in range(P):  # the weight row of one point at a time: [B,S,N], never [B,S,P,N]
            part = fft_convolve((wav * _traj_weight_row(N, hop, p, mode, ramp, wav.dtype))[:, :, None, :], h[:, :, p])
            full = part if full is None else full + part
        return full.gather(-1, idx)

    full = image(rir)
    return full, (full if rir_target is None else image(rir_target))


def energy_ratio_coeff(a: Tensor, b: Tensor, target_db: Tensor) -> Tensor:
    """factor for `b` such that 10 log10(mean(a^2) / mean((coeff b)^2)) = target_db; a, b [B,...], target_db [B] (mix.py:328-346)"""
    ea = a.reshape(a.shape[0], -1).pow(2).mean(1)
    eb = b.reshape(b.shape[0], -1).pow(2).mean(1)
    return torch.sqrt(ea / eb * torch.pow(10.0, -target_db / 10))


def diffuse_mixing_matrices(pos_mics: Tensor, fs: int, nfft: int = 256, c: float = 343.0) -> Tuple[Tensor, Tensor]:
    """spherically isotropic noise field: coherence DSC[m,n,k] = sinc(w_k d_mn / c) and one mixing matrix per frequency with
    C^H C = DSC (eigendecomposition; frequency 0 is left empty like in diffuse_noise.py:40-59) -> (DSC [M,M,F], Cs [F,M,M] complex)"""
    M, Fq = pos_mics.shape[0], nfft // 2 + 1
    w = 2 * math.pi * fs * torch.arange(Fq, dtype=torch.float64, device=pos_mics.device) / nfft
    dist = (pos_mics[:, None, :] - pos_mics[None, :, :]).double().norm(dim=-1)
    dsc = torch.sinc(w[None, None, :] * dist[:, :, None] / (c * math.pi))  # torch.sinc(x) = sin(pi x) / (pi x), as numpy's
    ev, V = torch.linalg.eigh(dsc.permute(2, 0, 1))  # symmetric PSD: [F,M], [F,M,M]
    Cs = (V.transpose(1, 2) * ev.clamp(min=0).sqrt()[:, :, None]).to(torch.complex128)
    Cs[0] = 0
    return dsc, Cs


def _stft_scipy(x: Tensor, nfft: int) -> Tensor:
    """scipy.signal.stft(window='hann', nperseg=nfft, noverlap=0.75 nfft, boundary='zeros', padded=True): [..., L] -> [..., F, T]"""
    hop = nfft // 4
    x = torch.nn.functional.pad(x, (nfft // 2, nfft // 2))
    extra = (-(x.shape[-1] - nfft)) % hop
    x = torch.nn.functional.pad(x, (0, extra))
    win = torch.hann_window(nfft, periodic=True, dtype=x.dtype, device=x.device)
    fr = x.unfold(-1, nfft, hop) * win
    return torch.fft.rfft(fr, nfft).transpose(-1, -2) / win.sum()


def _istft_scipy(X: Tensor, nfft: int) -> Tensor:
    """inverse of _stft_scipy (overlap-add with the hann window, window-envelope normalisation, boundary trimmed)"""
    hop = nfft // 4
    win = torch.hann_window(nfft, periodic=True, dtype=X.real.dtype, device=X.device)
    fr = torch.fft.irfft(X.transpose(-1, -2) * win.sum(), nfft) * win  # [..., T, nfft]
    T = fr.shape[-2]
    n = nfft + hop * (T - 1)
    lead = fr.shape[:-2]
    out = torch.nn.functional.fold(fr.reshape(-1, T, nfft).transpose(1, 2), (1, n), (1, nfft), stride=(1, hop)).reshape(*lead, n)
    env = torch.nn.functional.fold((win * win).expand(1, T, nfft).transpose(1, 2), (1, n), (1, nfft), stride=(1, hop)).reshape(n)
    return (out / env.clamp(min=1e-10))[..., nfft // 2: n - nfft // 2]


def gen_diffuse_noise(noise: Tensor, L: int, Cs: Tensor, nfft: int = 256) -> Tensor:
    """M mutually independent noises [..., M, >= L] -> diffuse noise [..., M, L] with the coherence the matrices `Cs` encode
    (diffuse_noise.py:64-93: zero-mean, STFT, X[n] = sum_m conj(C[f,m,n]) N[m], inverse STFT)"""
    noise = noise[..., :L] - noise[..., :L].mean(-1, keepdim=True)
    N = _stft_scipy(noise, nfft)  # [..., M, F, T]
    X = torch.einsum("fmn,...mft->...nft", Cs.conj().to(N.dtype), N)
    return _istft_scipy(X, nfft)[..., :L]


DIFFUSE_MODES = ('fft', 'native')


def gen_diffuse_noise_native(white: Tensor, L: int, Cs: Tensor, nfft: int = 256, lib=None) -> Tensor:
    """gen_diffuse_noise by the fused HIP kernel of csrc/diffuse.hip (nbss_diffuse_noise): white [..., M, >= L] fp32 -> [..., M, L], Cs [F,M,M] complex.
    Device tensors only: a host tensor raises ValueError (`lib` lets the tests hand in the emulator build of the same kernel)."""
    lib = _native_lib(lib, white, 'diffuse')
    if white.dim() < 2 or white.dtype != torch.float32 or white.shape[-1] < L:
        raise ValueError(f"gen_diffuse_noise_native: white must be fp32 [..., M, >= {L}], got {tuple(white.shape)} {white.dtype}")
    lead, M = white.shape[:-2], white.shape[-2]
    w = white[..., :L].reshape(-1, M, L).contiguous()
    return ops.diffuse_noise(lib, w, Cs.to(device=white.device, dtype=torch.complex64), nfft).reshape(*lead, M, L)


def _check_diffuse(diffuse: str) -> None:
    if diffuse not in DIFFUSE_MODES:
        raise ValueError(f"diffuse must be 'fft' or 'native', got {diffuse!r}")


def mix_batch(cleans: Tensor, rir: Tensor, Cs: Tensor, sir_db: Optional[Tensor], snr_db: Tensor, gen: Optional[torch.Generator], rir_target: Optional[Tensor] = None,
              nfft: int = 256, white: Optional[Tensor] = None, convolve: str = 'fft', lib=None, traj_hop: Optional[Tensor] = None,
              traj_mode: str = 'trapezium', traj_ramp: int = 20, diffuse: str = 'fft') -> Tuple[Tensor, Tensor, Dict[str, Tensor]]:
    """cleans [B,S,N] dry sources, rir [B,S,M,L] -> (mix [B,M,N], targets [B,S,M,N], paras): steps 5-7 of SmsWsjPlusDataset.__getitem__
    (full overlap) for a whole batch on the device of `cleans`.  convolve: 'fft' (torch.fft, the default) or 'native' (convolve_aligned_native:
    the HIP kernels, device tensors only; `lib` as there).  Moving sources: rir [B,S,P,M,L] together with traj_hop [B,S] goes through
    convolve_traj_aligned (traj_mode, traj_ramp as there); everything after the convolution is the same.  diffuse: 'fft' (gen_diffuse_noise, the
    default) or 'native' (gen_diffuse_noise_native: the fused HIP kernel, fp32 device tensors only, the same `lib`); `white` is drawn the same way."""
    _check_convolve(convolve)
    _check_diffuse(diffuse)
    B, S, N = cleans.shape
    M = rir.shape[-2]
    if (rir.dim() == 5) != (traj_hop is not None):
        raise ValueError(f"a trajectory needs both rir [B,S,P,M,L] and traj_hop [B,S]; got rir {tuple(rir.shape)} and traj_hop "
                         f"{None if traj_hop is None else tuple(traj_hop.shape)}")
    if traj_hop is not None:
        rvbt, tgt = convolve_traj_aligned(cleans, rir, traj_hop, rir_target, mode=traj_mode, ramp=traj_ramp, convolve=convolve, lib=lib)
    else:
        rvbt, tgt = convolve_aligned_native(cleans, rir, rir_target, lib=lib) if convolve == 'native' else convolve_aligned(cleans, rir, rir_target)
    if sir_db is not None and S == 2:  # speaker 2 relative to speaker 1
        coeff = energy_ratio_coeff(rvbt[:, 0], rvbt[:, 1], sir_db)
        scale = torch.stack([torch.ones_like(coeff), coeff], 1)[:, :, None, None]
        rvbt, tgt = rvbt * scale, tgt * scale
    mix = rvbt.sum(1)
    if white is None:
        white = torch.randn(B, M, N, generator=gen, device=cleans.device, dtype=cleans.dtype)
    if diffuse == 'native':
        noise = gen_diffuse_noise_native(white, N, Cs, nfft, lib=lib)
    else:
        noise = gen_diffuse_noise(white, N, Cs.to(cleans.device), nfft)
    noise = noise * energy_ratio_coeff(mix, noise, snr_db)[:, None, None]
    snr_real = 10 * torch.log10(mix.pow(2).sum((1, 2)) / noise.pow(2).sum((1, 2)))
    mix = mix + noise
    peak = torch.maximum(mix.abs().amax((1, 2)), tgt.abs().amax((1, 2, 3)))
    s = 0.9 / peak
    return mix * s[:, None, None], tgt * s[:, None, None, None], {"snr": snr_real, "scale": s}


class SimulatedRoomDataModule:
    """The batch contract of the reference's data modules (x [B,C,N], ys [B,Spk,C,N], paras), produced ON THE TRAINING DEVICE:
    synthetic band-limited sources, synthetic RIRs (direct path + exponentially decaying diffuse tail, RT60 sampled per item, mic
    delays from a circular array geometry), SIR / SNR sampled like configs/datasets/sms_wsj_plus.yaml.  Items are addressed by
    (index, seed) and sharded rank-strided like MyDistributedSampler."""

    def __init__(self, batch_size: List[int] = (2, 2), num_samples: List[int] = (64, 8, 8), audio_time_len: List[float] = (4.0, 4.0, 4.0),
                 num_channels: int = 6, num_speakers: int = 2, sample_rate: int = 8000, sir: Tuple[float, float] = (-5.0, 5.0),
                 snr: Tuple[float, float] = (0.0, 20.0), rt60: Tuple[float, float] = (0.2, 0.6), array_radius: float = 0.1, seeds: List[int] = (0, 1, 2),
                 device: Optional[str] = None, rir: str = 'synthetic', room_size_lims: Tuple[Tuple[float, float], ...] = ((3.0, 8.0), (3.0, 8.0), (3.0, 4.0)),
                 mic_zlim: Tuple[float, float] = (1.0, 1.5), spk_zlim: Tuple[float, float] = (1.0, 1.8), convolve: str = 'fft', conv_lib=None,
                 moving: Optional[Tuple[float, ...]] = None, traj_dist: float = 0.05, diffuse: str = 'fft', rir_att_diff: Optional[float] = None):
        _check_convolve(convolve)
        _check_diffuse(diffuse)
        self.rir_att_diff = None
        if rir_att_diff is not None:  # dB of decay after which a room's images give way to the diffuse tail (the reference's att_diff = 15)
            if rir != 'ism':
                raise ValueError(f"rir_att_diff switches image-source responses to their diffuse tail: rir must be 'ism', got {rir!r}")
            if not 0.0 < float(rir_att_diff) < 60.0:
                raise ValueError(f"rir_att_diff must lie between 0 and the 60 dB the responses decay by, got {rir_att_diff!r}")
            self.rir_att_diff = float(rir_att_diff)
        self.moving, self.traj_dist = None, float(traj_dist)
        if moving is not None:  # (vmin, vmax) or (vmin, vmax, prob) in m/s, named after the reference's 'moving(0.12,0.4[,p])' datasets
            if rir != 'ism':
                raise ValueError(f"moving speakers need trajectories of image-source responses: rir must be 'ism', got {rir!r}")
            mv = tuple(float(v) for v in moving)
            if len(mv) not in (2, 3) or not 0.0 < mv[0] <= mv[1] or not 0.0 <= (mv[2] if len(mv) == 3 else 1.0) <= 1.0 or traj_dist <= 0:
                raise ValueError(f"moving must be (vmin, vmax) or (vmin, vmax, prob) with 0 < vmin <= vmax and 0 <= prob <= 1, traj_dist > 0; got {moving!r}, "
                                 f"{traj_dist!r}")
            self.moving = (mv[0], mv[1], mv[2] if len(mv) == 3 else 1.0)
        self.convolve, self.conv_lib = convolve, conv_lib  # conv_lib: the tests hand in the emulator library; None = the product library
        self.diffuse = diffuse
        if rir not in ('synthetic', 'ism'):
            raise ValueError(f"rir must be 'synthetic' or 'ism', got {rir!r}")
        self.rir, self.room_size_lims, self.mic_zlim, self.spk_zlim = rir, [tuple(l) for l in room_size_lims], tuple(mic_zlim), tuple(spk_zlim)
        self.batch_size, self.num_samples, self.audio_time_len = list(batch_size), list(num_samples), list(audio_time_len)
        self.C, self.S, self.sr, self.sir, self.snr, self.rt60, self.seeds = num_channels, num_speakers, sample_rate, sir, snr, rt60, list(seeds)
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        ang = torch.arange(num_channels) * (2 * math.pi / num_channels)
        self.pos_mics = torch.stack([array_radius * torch.cos(ang), array_radius * torch.sin(ang), torch.zeros(num_channels)], 1)
        if convolve == 'native' and self.device.type != 'cuda' and conv_lib is None:
            raise ValueError("convolve='native' runs the HIP kernels and needs a HIP device; use convolve='fft' (one of 'fft', 'native') on the host")
        if diffuse == 'native' and self.device.type != 'cuda' and conv_lib is None:
            raise ValueError("diffuse='native' runs the HIP kernel and needs a HIP device; use diffuse='fft' (one of 'fft', 'native') on the host")
        self.Cs = diffuse_mixing_matrices(self.pos_mics, sample_rate)[1].to(torch.complex64).to(self.device)

    def _rirs(self, B: int, gen: torch.Generator) -> Tensor:
        """[B,S,M,L]: unit direct path at a per-(speaker, mic) delay from a random far-field direction + decaying Gaussian tail"""
        dev, L = self.device, int(0.4 * self.sr)
        rt = self.rt60[0] + (self.rt60[1] - self.rt60[0]) * torch.rand(B, 1, 1, 1, generator=gen, device=dev)
        t = torch.arange(L, device=dev) / self.sr
        tail = torch.randn(B, self.S, self.C, L, generator=gen, device=dev) * torch.exp(-6.9 * t / rt) * 0.3
        az = 2 * math.pi * torch.rand(B, self.S, generator=gen, device=dev)
        direction = torch.stack([torch.cos(az), torch.sin(az), torch.zeros_like(az)], -1)  # [B,S,3]
        delay = (16 + (-(direction @ self.pos_mics.to(dev).T) / 343.0 * self.sr)).round().long().clamp(0, L - 1)  # [B,S,M]
        tail.masked_fill_(torch.arange(L, device=dev)[None, None, None, :] < delay[..., None], 0.0)
        return tail.scatter(-1, delay[..., None], 1.0)

    def _ism_scene(self, B: int, gen: torch.Generator) -> Dict[str, Tensor]:
        """B shoebox rooms drawn from `gen` (fp64, on the device): room size, RT60 (redrawn while Sabine's formula cannot reach it in that room:
        RT60 < 0.161 V / S), wall coefficients, the array (centre at least 0.5 m from the side walls, height in mic_zlim, rotated about z) and the
        speakers (at least 0.3 m from the side walls, height in spk_zlim), and what follows from them: image counts down to 60 dB of decay and the
        RIR length int((max RT60 + 0.1) fs)"""
        dev = self.device
        u = lambda *shape: torch.rand(*shape, generator=gen, device=dev, dtype=torch.float64)
        lims = torch.tensor(self.room_size_lims, dtype=torch.float64, device=dev)  # [3,2]
        room = lims[:, 0] + (lims[:, 1] - lims[:, 0]) * u(B, 3)
        floor = 0.161 * room.prod(-1) / (2.0 * (room[:, 0] * room[:, 1] + room[:, 0] * room[:, 2] + room[:, 1] * room[:, 2]))
        rt = self.rt60[0] + (self.rt60[1] - self.rt60[0]) * u(B)
        for _ in range(16):
            again = self.rt60[0] + (self.rt60[1] - self.rt60[0]) * u(B)  # drawn every time: the stream of draws does not depend on the rooms
            rt = torch.where(rt < floor, again, rt)
        rt = torch.maximum(rt, floor)  # a room whose floor lies above the whole RT60 range keeps its shortest reachable RT60
        beta = beta_sabine(room, rt)[0]
        xy = lambda margin, *shape: margin + (room[:, None, :2] - 2.0 * margin) * u(*shape)
        z = lambda lim, *shape: lim[0] + (lim[1] - lim[0]) * u(*shape)
        centre = torch.cat([xy(0.5, B, 1, 2), z(self.mic_zlim, B, 1, 1)], -1)  # [B,1,3]
        pos_rcv = centre + rotate_z(self.pos_mics.to(dev).double().expand(B, self.C, 3), 2.0 * math.pi * u(B))
        pos_src = torch.cat([xy(0.3, B, self.S, 2), z(self.spk_zlim, B, self.S, 1)], -1)
        return {"room_sz": room, "rt60": rt, "beta": beta, "pos_rcv": pos_rcv, "pos_src": pos_src,
                "nb_img": t2n(att2t(60.0, rt), room).cpu(), "n_samples": int((float(rt.max()) + 0.1) * self.sr)}

    def _ism_tail(self, sc: Dict[str, Tensor], gen: torch.Generator) -> Dict:
        """what the reverberant simulate_rir call takes besides the scene.  Without rir_att_diff: the scene's image counts down to 60 dB, and no
        draw from `gen`.  With it, per room b: t_diff[b] = att2t(rir_att_diff, rt60[b]), the image counts t2n(t_diff[b], room) that reach it, the
        diffuse tail governed by rt60[b] from there to the scene's n_samples, and the tail's seed: one integer drawn from `gen`, after every draw of
        the scene (items stay addressed by (index, seed))."""
        if self.rir_att_diff is None:
            return {"nb_img": sc["nb_img"]}
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen, device=self.device))
        t_diff = att2t(self.rir_att_diff, sc["rt60"])
        try:
            ops.rir_tail_starts(t_diff, self.sr, len(t_diff), sc["n_samples"], TW)
        except ops.RirTailError as e:  # said again in the data module's terms
            raise ValueError(f"rir_att_diff = {self.rir_att_diff:g} dB puts the diffuse tail of room {e.room} (RT60 {float(sc['rt60'][e.room]):.3f} s) at "
                             f"sample {e.k_d}, outside {int(round(TW * self.sr))} <= k_d < {sc['n_samples']}") from e
        return {"nb_img": t2n(t_diff, sc["room_sz"]).cpu(), "t_diff": t_diff, "rt60": sc["rt60"], "seed": seed}

    def _ism_pair(self, sc: Dict[str, Tensor], pos_src: Tensor, gen: torch.Generator) -> Tuple[Tensor, Tensor]:
        """(reverberant, direct-path) fp32 RIRs [B, sources, M, L] of the scene's rooms for the sources pos_src [B, sources, 3]: one simulate_rir call
        each; with rir_att_diff the reverberant one sums each room's images to that decay only and continues with the diffuse tail (_ism_tail)"""
        kw = dict(pos_src=pos_src, pos_rcv=sc["pos_rcv"], n_samples=sc["n_samples"], fs=self.sr)
        rir = simulate_rir(sc["room_sz"], sc["beta"], **self._ism_tail(sc, gen), **kw)
        rir_dp = simulate_rir(sc["room_sz"], torch.zeros_like(sc["beta"]), nb_img=(1, 1, 1), **kw)
        return rir.float(), rir_dp.float()

    def _ism_rirs(self, B: int, gen: torch.Generator) -> Tuple[Tensor, Tensor]:
        """(reverberant, direct-path) RIRs [B,S,M,L] of B rooms drawn from `gen` (_ism_pair)"""
        sc = self._ism_scene(B, gen)
        return self._ism_pair(sc, sc["pos_src"], gen)

    TRAJ_RAMP = 20         # the reference's 'trapezium20'
    TRAJ_WAVELENGTH = 2.0  # of the lateral wobble, in metres walked
    TRAJ_WOBBLE = 0.2      # its largest amplitude in metres: the slope stays below 0.2 * 2 pi / 2 = 0.63, adjacent points below 1.19 traj_dist

    def _trajectory(self, sc: Dict[str, Tensor], P: int, gen: torch.Generator) -> Tensor:
        """[B,S,P,3]: from each drawn speaker position, steps of traj_dist along a drawn horizontal direction with a sinusoidal lateral wobble
        (amplitude, phase drawn), reflected back into the speaker box (0.3 m from the side walls); the height stays.  After the idea of the
        reference's '4points+sin' trajectories (generate_rirs.py:389-446), not its draws."""
        dev, B = self.device, sc["pos_src"].shape[0]
        u = lambda *shape: torch.rand(*shape, generator=gen, device=dev, dtype=torch.float64)
        theta, amp, phase = 2.0 * math.pi * u(B, self.S), self.TRAJ_WOBBLE * u(B, self.S), 2.0 * math.pi * u(B, self.S)
        along = self.traj_dist * torch.arange(P, device=dev, dtype=torch.float64)                                   # [P]
        side = amp[..., None] * (torch.sin(2.0 * math.pi * along / self.TRAJ_WAVELENGTH + phase[..., None]) - torch.sin(phase)[..., None])  # [B,S,P], 0 at the start
        e = torch.stack([torch.cos(theta), torch.sin(theta)], -1)[:, :, None, :]                                    # [B,S,1,2]
        en = torch.stack([-torch.sin(theta), torch.cos(theta)], -1)[:, :, None, :]
        xy = sc["pos_src"][:, :, None, :2] + along[None, None, :, None] * e + side[..., None] * en                   # [B,S,P,2]
        lo, width = 0.3, (sc["room_sz"][:, None, None, :2] - 0.6)
        t = torch.remainder(xy - lo, 2.0 * width)                                                                   # reflect at both faces of the box
        xy = lo + torch.where(t > width, 2.0 * width - t, t)
        return torch.cat([xy, sc["pos_src"][:, :, None, 2:].expand(B, self.S, P, 1)], -1)

    def _traj_draws(self, B: int, N: int, gen: torch.Generator) -> Tuple[Dict[str, Tensor], Tensor, Tensor, Tensor]:
        """the scene, the samples per trajectory point hop [B,S] int32, the speeds [B,S] in m/s (0 for a speaker that stands) and the trajectory points
        [B,S,P,3] of B items of N samples.  Every speaker draws its own speed (the reference draws one and, through a truncating zip, moves only the
        first speaker); P is what the smallest hop of the batch needs; a standing speaker has one point P times."""
        sc = self._ism_scene(B, gen)
        u = lambda *shape: torch.rand(*shape, generator=gen, device=self.device, dtype=torch.float64)
        vmin, vmax, prob = self.moving
        speed = vmin + (vmax - vmin) * u(B, self.S)
        walks = u(B, self.S) < prob
        hop = torch.round(self.traj_dist / speed * self.sr).to(torch.int32)
        hmin = int(hop.min())
        if hmin <= self.TRAJ_RAMP:
            raise ValueError(f"traj_dist / vmax * sample_rate = {hmin} samples per trajectory point must exceed the window's ramp of {self.TRAJ_RAMP}")
        pts = self._trajectory(sc, traj_rirs_needed(N, hmin, 'trapezium'), gen)
        pts = torch.where(walks[:, :, None, None], pts, pts[:, :, :1].expand_as(pts))
        return sc, hop, torch.where(walks, speed, torch.zeros_like(speed)), pts

    def _ism_traj_rirs(self, B: int, N: int, gen: torch.Generator) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """(reverberant, direct-path) RIRs [B,S,P,M,L] along the trajectories of _traj_draws, with its hop and speeds: _ism_pair with the
        trajectory points as sources.  With rir_att_diff (_ism_tail) every trajectory point is a source of its own to the kernel and so
        gets its own tail noise xi(seed, b, s P + p, m, k): the tails of adjacent points are independent, not a continuation of one another."""
        sc, hop, speed, pts = self._traj_draws(B, N, gen)
        P = pts.shape[2]
        rir, rir_dp = self._ism_pair(sc, pts.reshape(B, self.S * P, 3), gen)
        shape = (B, self.S, P, self.C, sc["n_samples"])
        return rir.reshape(shape), rir_dp.reshape(shape), hop, speed

    def batches(self, stage: int, rank: int = 0, world: int = 1, epoch: int = 0):
        N = int(self.audio_time_len[stage] * self.sr)
        bs = self.batch_size[min(stage, len(self.batch_size) - 1)]
        items = rank_strided_indices(self.num_samples[stage], rank, world, epoch, self.seeds[stage], shuffle=stage == 0)
        k = torch.hann_window(33, device=self.device)
        for i in range(0, len(items) - bs + 1, bs):
            chunk = items[i:i + bs]
            gen = torch.Generator(device=self.device).manual_seed(int(chunk[0][1]) * 1000003 + int(chunk[0][0]))
            src = torch.randn(bs * self.S, 1, N, generator=gen, device=self.device)
            src = torch.nn.functional.conv1d(src, (k / k.sum())[None, None], padding=16).reshape(bs, self.S, N) * 3.0
            sir = self.sir[0] + (self.sir[1] - self.sir[0]) * torch.rand(bs, generator=gen, device=self.device)
            snr = self.snr[0] + (self.snr[1] - self.snr[0]) * torch.rand(bs, generator=gen, device=self.device)
            kw, speed = {}, None
            if self.moving is not None:  # moving speakers: trajectories of image-source responses, cross-faded along the source
                rir, rir_dp, hop, speed = self._ism_traj_rirs(bs, N, gen)
                kw = dict(rir_target=rir_dp, traj_hop=hop, traj_ramp=self.TRAJ_RAMP)
            elif self.rir == 'ism':  # the targets are the direct-path images
                rir, rir_dp = self._ism_rirs(bs, gen)
                kw = dict(rir_target=rir_dp)
            else:
                rir = self._rirs(bs, gen)
            mix, tgt, paras = mix_batch(src, rir, self.Cs, sir if self.S == 2 else None, snr, gen, convolve=self.convolve, diffuse=self.diffuse,
                                        lib=self.conv_lib, **kw)
            more = [{}] * bs if speed is None else [{"speed": v} for v in speed.tolist()]
            yield mix, tgt, [{"index": ix, "seed": sd, "sample_rate": self.sr, "snr": float(paras["snr"][j]), "sir": float(sir[j]), **more[j]}
                             for j, (ix, sd) in enumerate(chunk)]
