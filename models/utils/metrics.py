"""metrics — drop-in for the reference's models/utils/metrics.py: `cal_metrics_functional` (metrics.py:26-151) and `recover_scale` (metrics.py:192-218).
SDR, SI_SDR, SI_SNR and SNR — what the reference's device pass computes through torchmetrics — run on the MI355X kernels (nbss_amd/csrc/metrics.hip:
nbss_sdr, nbss_signal_ratios, nbss_recover_scale) for tensors on a HIP device and through the same closed forms in torch for host tensors (fp64 for SDR
and for the scales), as models/io/loss.py does for the CPU accelerator.  NB_PESQ, WB_PESQ, STOI, ESTOI, DNSMOS and pDNSMOS need the packages pesq, pystoi
and onnxruntime, which are not ported: the device pass (`device_only='gpu'`) skips them, every other pass raises NotImplementedError naming the package.

Opt-in: NBSS_NATIVE_STOI=1 (read on every call, on only for exactly '1') serves STOI and ESTOI natively, as include/nbss_hip.h defines them
(nbss_amd/csrc/stoi.hip: nbss_stoi on a HIP device, the same definition in fp64 numpy / scipy on the host), under the reference's keys, in the
None, 'gpu' and 'cpu' passes.  pystoi was never run against it: parity with pystoi is not pinned, which is why the switch is off by default."""
import math
import os
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

ALL_AUDIO_METRICS = ['SDR', 'SI_SDR', 'SI_SNR', 'SNR', 'NB_PESQ', 'WB_PESQ', 'STOI', 'DNSMOS', 'pDNSMOS']
NATIVE_METRICS = ('SDR', 'SI_SDR', 'SI_SNR', 'SNR')
_PACKAGE = {'NB_PESQ': 'pesq', 'WB_PESQ': 'pesq', 'STOI': 'pystoi', 'ESTOI': 'pystoi', 'DNSMOS': 'onnxruntime', 'PDNSMOS': 'onnxruntime'}
_RATIO_COLUMN = {'SNR': 0, 'SI_SDR': 1, 'SI_SNR': 2}  # nbss_signal_ratios: out[..., 3]
SDR_FILTER_LENGTH = 512  # torchmetrics' default
STOI_METRICS = ('STOI', 'ESTOI')
STOI_RATIO = {8000: (5, 4), 16000: (5, 8), 10000: (1, 1)}  # p / q to 10 kHz


def native_stoi_enabled() -> bool:
    return os.environ.get('NBSS_NATIVE_STOI') == '1'


def get_metric_list_on_device(device: Optional[str]):
    """the metrics a pass with `device_only=device` evaluates (metrics.py:17-23, without the ones that are not ported on the device pass)"""
    return {None: ['SDR', 'SI_SDR', 'SNR', 'SI_SNR', 'NB_PESQ', 'WB_PESQ', 'STOI', 'ESTOI', 'DNSMOS', 'PDNSMOS'],
            'cpu': ['NB_PESQ', 'WB_PESQ', 'STOI', 'ESTOI'],
            'gpu': ['SDR', 'SI_SDR', 'SNR', 'SI_SNR'] + (list(STOI_METRICS) if native_stoi_enabled() else [])}[device]


# ---- host closed forms (torchmetrics restated) ------------------------------------------------------------------------------------------------------
def _host_sisdr(p: Tensor, t: Tensor, zero_mean: bool) -> Tensor:
    eps = torch.finfo(torch.float32).eps
    if zero_mean:
        p, t = p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)
    alpha = ((p * t).sum(-1, keepdim=True) + eps) / ((t * t).sum(-1, keepdim=True) + eps)
    ts = alpha * t
    return 10 * torch.log10(((ts * ts).sum(-1) + eps) / (((ts - p) ** 2).sum(-1) + eps))


def _host_ratios(p: Tensor, t: Tensor) -> Tensor:
    """[..., N] fp64 -> [..., 3]: SNR, SI-SDR, SI-SNR"""
    eps = torch.finfo(torch.float32).eps
    snr = 10 * torch.log10(((t * t).sum(-1) + eps) / (((t - p) ** 2).sum(-1) + eps))
    return torch.stack([snr, _host_sisdr(p, t, False), _host_sisdr(p, t, True)], -1)


def _host_sdr(p: Tensor, t: Tensor, filter_length: int = SDR_FILTER_LENGTH, zero_mean: bool = False) -> Tensor:
    """torchmetrics signal_distortion_ratio in fp64: unit-norm signals, auto- and cross-correlation over `filter_length` lags (linear, through a
    zero-padded FFT), the symmetric Toeplitz system, the coherence"""
    p, t = p.double(), t.double()
    if zero_mean:
        p, t = p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)
    t = t / torch.clamp(torch.linalg.norm(t, dim=-1, keepdim=True), min=1e-6)
    p = p / torch.clamp(torch.linalg.norm(p, dim=-1, keepdim=True), min=1e-6)
    n = 2 ** math.ceil(math.log2(2 * p.shape[-1] - 1)) if p.shape[-1] > 1 else 1
    tf, pf = torch.fft.rfft(t, n=n), torch.fft.rfft(p, n=n)
    r = torch.fft.irfft(tf.real ** 2 + tf.imag ** 2, n=n)[..., :filter_length]
    b = torch.fft.irfft(tf.conj() * pf, n=n)[..., :filter_length]
    lag = (torch.arange(filter_length, device=p.device)[:, None] - torch.arange(filter_length, device=p.device)[None, :]).abs()
    # one LAPACK call per pair: a batched solve of matrices this large can stall inside torch's CPU thread pool once torch.set_num_threads has been called
    rf, bf = r.reshape(-1, filter_length), b.reshape(-1, filter_length)
    x = torch.stack([torch.linalg.solve(rf[i][lag], bf[i]) for i in range(rf.shape[0])]).reshape(b.shape) if rf.shape[0] else torch.zeros_like(b)
    coh = (b * x).sum(-1)
    return 10 * torch.log10(coh / (1 - coh))


def native_metrics(preds: Tensor, target: Tensor, names) -> Dict[str, Tensor]:
    """{NAME: fp32 tensor shaped like preds.shape[:-1]} for the names of NATIVE_METRICS: one nbss_sdr and / or one nbss_signal_ratios call on a HIP
    device, the closed forms on the host.  preds / target [..., N], estimate paired with target along every leading axis."""
    names = [n.upper() for n in names]
    assert all(n in NATIVE_METRICS for n in names), names
    if preds.shape != target.shape or preds.dim() < 1:
        raise ValueError(f"metrics: preds {tuple(preds.shape)} and target {tuple(target.shape)} must have the same shape [..., time]")
    lead, N = preds.shape[:-1], preds.shape[-1]
    if N < SDR_FILTER_LENGTH and 'SDR' in names:
        raise ValueError(f"SDR needs at least filter_length = {SDR_FILTER_LENGTH} samples, got {N}")
    p, t = preds.detach().reshape(-1, 1, N), target.detach().reshape(-1, 1, N)
    out: Dict[str, Tensor] = {}
    if p.is_cuda:
        from nbss_amd import ops
        from nbss_amd._lib import hip
        p, t = p.float().contiguous(), t.float().contiguous()
        rows = range(0, p.shape[0], 1024)  # the kernels take up to 1024 items a call
        if 'SDR' in names:
            out['SDR'] = torch.cat([ops.sdr(hip(), p[i:i + 1024], t[i:i + 1024], SDR_FILTER_LENGTH) for i in rows]).reshape(lead)
        if any(n in _RATIO_COLUMN for n in names):
            ratios = torch.cat([ops.signal_ratios(hip(), p[i:i + 1024], t[i:i + 1024]) for i in rows]).reshape(*lead, 3)
    else:
        if 'SDR' in names:
            out['SDR'] = _host_sdr(p[:, 0], t[:, 0]).float().reshape(lead)
        if any(n in _RATIO_COLUMN for n in names):
            ratios = _host_ratios(p[:, 0].double(), t[:, 0].double()).float().reshape(*lead, 3)
    for n in names:
        if n in _RATIO_COLUMN:
            out[n] = ratios[..., _RATIO_COLUMN[n]]
    return out


# ---- STOI / eSTOI: the definition of include/nbss_hip.h in fp64 (host) ------------------------------------------------------------------------------
def _stoi_taps(p: int, q: int):
    import numpy as np
    fc = 1.0 / (2 * max(p, q))
    L = int(math.ceil((60 - 8) / (28.714 * fc / 10)))
    h = np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7)) * 2 * p * fc * np.sinc(2 * fc * np.arange(-L, L + 1))
    return p * h / h.sum(), L


def _stoi_resample(x, p: int, q: int):
    """out[m] = sum_k h[m q - k p + L] x[k], m < ceil(N p / q): the zero-stuffed signal through h, every q-th sample from L on"""
    import numpy as np
    if p == q:
        return x
    h, L = _stoi_taps(p, q)
    up = np.zeros(len(x) * p + 2 * L)
    up[:len(x) * p:p] = x
    return np.convolve(up, h)[L + q * np.arange(-(-len(x) * p // q))]


def _stoi_frames(x):
    import numpy as np
    n = max(-(-(len(x) - 256) // 128), 0)  # starts 0, 128, ... < len - 256
    return x[128 * np.arange(n)[:, None] + np.arange(256)[None, :]]


def _host_stoi(x, y, fs: int, extended: bool) -> float:
    """one pair in fp64 numpy: clean x, estimate y"""
    import numpy as np
    eps = 2.0 ** -52
    p, q = STOI_RATIO[fs]
    x, y = _stoi_resample(np.asarray(x, np.float64), p, q), _stoi_resample(np.asarray(y, np.float64), p, q)
    if len(x) < 257:
        raise ValueError(f"STOI needs at least 257 samples at 10 kHz, got {len(x)}")
    w = np.hanning(258)[1:-1]
    xf, yf = _stoi_frames(x) * w, _stoi_frames(y) * w
    energy = 20 * np.log10(np.sqrt((xf * xf).sum(1)) + eps)
    keep = energy > energy.max() - 40
    xf, yf = xf[keep], yf[keep]
    K = len(xf)
    if K - 1 < 30:
        return 1e-5
    xs, ys = np.zeros(128 * (K + 1)), np.zeros(128 * (K + 1))
    for half in (0, 1):  # overlap-add at hop 128: the first halves of the frames, then the second halves one hop later
        xs[128 * half:128 * (K + half)] += xf[:, 128 * half:128 * (half + 1)].reshape(-1)
        ys[128 * half:128 * (K + half)] += yf[:, 128 * half:128 * (half + 1)].reshape(-1)
    f = np.arange(257) * (10000 / 512)
    sel = np.zeros((15, 257))
    for k in range(15):
        sel[k, np.argmin((f - 150 * 2 ** ((2 * k - 1) / 6)) ** 2):np.argmin((f - 150 * 2 ** ((2 * k + 1) / 6)) ** 2)] = 1
    X = np.sqrt(sel @ (np.abs(np.fft.rfft(_stoi_frames(xs) * w, 512, axis=1)) ** 2).T)
    Y = np.sqrt(sel @ (np.abs(np.fft.rfft(_stoi_frames(ys) * w, 512, axis=1)) ** 2).T)
    M = X.shape[1] - 29
    idx = np.arange(M)[:, None] + np.arange(30)[None, :]
    Xs, Ys = X[:, idx].transpose(1, 0, 2), Y[:, idx].transpose(1, 0, 2)  # [M, 15, 30]
    if extended:
        def normed(a):
            a = a - a.mean(2, keepdims=True)
            a = a / (np.sqrt((a * a).sum(2, keepdims=True)) + eps)
            a = a - a.mean(1, keepdims=True)
            return a / (np.sqrt((a * a).sum(1, keepdims=True)) + eps)
        return float((normed(Xs) * normed(Ys)).sum() / (30 * M))
    alpha = np.sqrt((Xs * Xs).sum(2, keepdims=True)) / (np.sqrt((Ys * Ys).sum(2, keepdims=True)) + eps)
    Yp = np.minimum(alpha * Ys, Xs * (1 + 10 ** (15 / 20)))
    xc, yc = Xs - Xs.mean(2, keepdims=True), Yp - Yp.mean(2, keepdims=True)
    return float(((xc * yc).sum(2) / ((np.sqrt((xc * xc).sum(2)) + eps) * (np.sqrt((yc * yc).sum(2)) + eps))).mean())


def native_stoi(preds: Tensor, target: Tensor, fs: int, extended: bool) -> Tensor:
    """STOI (extended: eSTOI) as include/nbss_hip.h defines it: preds / target [..., N] at fs Hz -> fp32 [...]: one nbss_stoi call per 1024 items on a
    HIP device, the fp64 closed form on the host.  Parity with pystoi is not pinned."""
    if preds.shape != target.shape or preds.dim() < 1:
        raise ValueError(f"metrics: preds {tuple(preds.shape)} and target {tuple(target.shape)} must have the same shape [..., time]")
    if int(fs) not in STOI_RATIO:
        raise ValueError(f"STOI: the sampling rate must be one of {sorted(STOI_RATIO)}, got {fs}")
    lead, N = preds.shape[:-1], preds.shape[-1]
    p, t = preds.detach().reshape(-1, 1, N), target.detach().reshape(-1, 1, N)
    if p.is_cuda:
        from nbss_amd import ops
        from nbss_amd._lib import hip
        p, t = p.float().contiguous(), t.float().contiguous()
        return torch.cat([ops.stoi(hip(), p[i:i + 1024], t[i:i + 1024], int(fs), extended) for i in range(0, p.shape[0], 1024)]).reshape(lead)
    pn, tn = p[:, 0].double().numpy(), t[:, 0].double().numpy()
    return torch.tensor([_host_stoi(tn[i], pn[i], int(fs), extended) for i in range(pn.shape[0])], dtype=torch.float32).reshape(lead)


def pit_reorder(yr_hat: Tensor, perm: Optional[Tensor]) -> Tensor:
    """the estimates in the order of the targets they were paired with (perm [B,S]: estimate paired with target s; torchmetrics pit_permutate)"""
    if perm is None:
        return yr_hat
    return torch.gather(yr_hat, 1, perm.long()[..., None].expand_as(yr_hat)).contiguous()


def val_metrics(yr_hat: Tensor, yr: Tensor) -> Tuple[float, float]:
    """(SDR, SI-SDR) of a validation batch, means over utterances and speakers (the reference's SharedTrainer.py:166-168)"""
    v = native_metrics(yr_hat, yr, ("SDR", "SI_SDR"))
    return float(v["SDR"].mean()), float(v["SI_SDR"].mean())


def cal_metrics_functional(metric_list: List[str], preds: Tensor, target: Tensor, original: Optional[Tensor], fs: int, device_only: Optional[str] = None,
                           chunk: Tuple[float, float] = None, suffix: str = "") -> Tuple[Dict[str, object], Dict[str, object], Dict[str, object]]:
    """metrics, input metrics (of `original` against `target`) and their improvements under the reference's key names: `sdr`, `sdr_all`,
    `input_sdr`, `input_sdr_all`, `sdr_i`, `sdr_all_i`, ... — the mean as a float, `_all` as nested lists shaped like preds.shape[:-1].
    chunk = (length, hop) in seconds adds the same keys per chunk with the suffix `_{start}s-{end}s` (metrics.py:37-50)."""
    if device_only not in (None, 'cpu', 'gpu'):
        raise ValueError(f"device_only must be None, 'cpu' or 'gpu', got {device_only!r}")
    metrics, input_metrics, imp_metrics = {}, {}, {}
    if chunk is not None:
        clen, chop = int(fs * chunk[0]), int(fs * chunk[1])
        for i in range(int((preds.shape[-1] / fs - chunk[0]) / chunk[1]) + 1):
            m_c, im_c, imp_c = cal_metrics_functional(metric_list, preds[..., i * chop:i * chop + clen], target[..., i * chop:i * chop + clen],
                                                      original[..., i * chop:i * chop + clen] if original is not None else None, fs, device_only,
                                                      chunk=None, suffix=f"_{i*chunk[1]+1}s-{i*chunk[1]+chunk[0]}s")
            metrics.update(m_c), input_metrics.update(im_c), imp_metrics.update(imp_c)

    served = []
    for m in metric_list:
        if m.upper() not in NATIVE_METRICS and m.upper() not in _PACKAGE:
            raise ValueError('Unkown audio metric ' + m)
        if m.upper() in STOI_METRICS and native_stoi_enabled():
            served.append(m)  # in every pass: the 'cpu' pass evaluates them on host tensors
            continue
        if m.upper() in _PACKAGE:
            if device_only == 'gpu':
                continue  # the device pass leaves them to the host pass, as the reference's does
            if m.upper() == 'WB_PESQ' and fs == 8000:
                continue  # there is narrow band (nb) mode only when the sampling rate is 8000 Hz
            raise NotImplementedError(f"{m} needs the package {_PACKAGE[m.upper()]}, which this port does not use: SDR, SI_SDR, SI_SNR and SNR are "
                                      "computed natively (device_only='gpu' skips the rest)"
                                      + ("; NBSS_NATIVE_STOI=1 serves STOI and ESTOI by this port's own definition (include/nbss_hip.h), whose parity with "
                                         "pystoi is not pinned" if m.upper() in STOI_METRICS else ""))
        if m.upper() not in get_metric_list_on_device(device_only):
            continue  # the host pass leaves the native ones to the device pass
        served.append(m)
    if not served:
        return metrics, input_metrics, imp_metrics
    def evaluate(p: Tensor) -> Dict[str, Tensor]:
        out = native_metrics(p, target, [m for m in served if m.upper() in NATIVE_METRICS])
        for m in served:
            if m.upper() in STOI_METRICS:
                on_host = device_only == 'cpu'
                out[m.upper()] = native_stoi(p.cpu() if on_host else p, target.cpu() if on_host else target, fs, m.upper() == 'ESTOI')
        return out

    vals = evaluate(preds)
    in_vals = evaluate(original) if original is not None else None
    for m in served:
        mname = m.lower() + suffix
        v = vals[m.upper()].double().cpu()
        metrics[mname] = v.mean().item()
        metrics[mname + '_all'] = v.tolist()  # _all means not averaged
        if in_vals is None:
            continue
        iv = in_vals[m.upper()].double().cpu()
        input_metrics['input_' + mname] = iv.mean().item()
        input_metrics['input_' + mname + '_all'] = iv.tolist()
        imp_metrics[mname + '_i'] = metrics[mname] - input_metrics['input_' + mname]  # _i means improvement
        imp_metrics[mname + '_all' + '_i'] = (v - iv).tolist()
    return metrics, input_metrics, imp_metrics


def recover_scale(preds: Tensor, mixture: Tensor, scale_src_together: bool, norm_if_exceed_1: bool = True) -> Tensor:
    """recover the scale a scale-invariant loss leaves open: preds [batch, n_src, time] times the least-squares solution a of
    min ||sum_s a_s preds_s - mixture|| (one a for the summed sources with scale_src_together); mixture [batch, time].  With norm_if_exceed_1 a
    source whose magnitude then exceeds 1 is divided by its maximum.  Defined for linearly independent estimates (a non-singular Gram matrix)."""
    if preds.dim() != 3 or mixture.shape != (preds.shape[0], preds.shape[2]):
        raise ValueError(f"recover_scale: preds {tuple(preds.shape)} must be [batch, n_src, time] and mixture {tuple(mixture.shape)} [batch, time]")
    if preds.is_cuda:
        from nbss_amd import ops
        from nbss_amd._lib import hip
        outs = [ops.recover_scale(hip(), preds[i:i + 1024].detach().float().contiguous(), mixture[i:i + 1024].detach().float().contiguous(),
                                  scale_src_together, norm_if_exceed_1) for i in range(0, preds.shape[0], 1024)]
        return torch.cat(outs).to(preds.dtype)
    p, x = preds.detach().double(), mixture.detach().double()
    if scale_src_together:
        s = p.sum(1)
        a = ((s * x).sum(-1) / (s * s).sum(-1))[:, None, None].expand(-1, p.shape[1], 1)
    else:
        a = torch.linalg.solve(p @ p.transpose(-1, -2), p @ x[..., None])  # the normal equations: Gram matrix [S,S], right-hand side [S,1]
    out = p * a
    if norm_if_exceed_1:
        mx = out.abs().amax(-1, keepdim=True)
        out = out / torch.where(mx > 1, mx, torch.ones_like(mx))
    return out.to(preds.dtype)
