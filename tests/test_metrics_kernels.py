"""The metric kernels (nbss_amd/csrc/metrics.hip: nbss_sdr, nbss_signal_ratios, nbss_recover_scale) against an fp64 restatement of torchmetrics'
definitions, on the emulator and, under -m gpu, on the device.

The restatement of signal_distortion_ratio below is torchmetrics' own sequence (unit-norm signals, FFT auto- and cross-correlation with
n = 2^ceil(log2(2N - 1)), symmetric Toeplitz matrix, torch.linalg.solve, coherence) in fp64; it is first checked against the values torchmetrics
publishes in its docstrings, then used as the reference.

Bars.  SDR against the restatement: 1e-4 dB.  The fp64 error in coh is about cond(R) * 512 * 2^-53 <= 1e4 * 512 * 1.1e-16 = 6e-10, relative to
1 - coh >= 1e-3 (SDR <= 30 dB) 6e-7, i.e. 2.6e-6 dB; the fp32 output adds half an ulp at 30 dB, 1e-6 dB.  The test asserts cond(R) <= 1e4 and
SDR <= 30 dB on its inputs at N = 4001, where the sample autocorrelation is close to the process's.  At N = 512 ... 1000 with 512 lags the sample
autocorrelation matrix of the same AR(2) signals is worse conditioned (up to 2.1e5) and the 512-tap filter fits up to 31 dB, so there the test
asserts what those two numbers stand for: the same error estimate, evaluated on the case's own cond(R) and coh, stays below the bar (the worst
case of the grid gives 6.6e-5 dB).  The bar is 1e-4 dB for every case.  Near-perfect estimate (60 dB, 1 - coh = 1e-6): 1e-2 dB (the same estimate gives 2.6e-3 dB); fp32 correlation sums
(6e-8 relative to 1e-6) could not meet it.  Published values: 2e-4 dB = their printed precision plus fp32 input rounding."""
import functools
import math

import pytest
import torch

from nbss_amd import ops
from nbss_amd._lib import NbssError

EPS = torch.finfo(torch.float32).eps


def ref_sdr(preds, target, filter_length=512, zero_mean=False, return_r=False):
    p, t = preds.double(), target.double()
    if zero_mean:
        p, t = p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)
    t = t / torch.clamp(torch.linalg.norm(t, dim=-1, keepdim=True), min=1e-6)
    p = p / torch.clamp(torch.linalg.norm(p, dim=-1, keepdim=True), min=1e-6)
    n = 2 ** math.ceil(math.log2(2 * p.shape[-1] - 1))
    tf, pf = torch.fft.rfft(t, n=n), torch.fft.rfft(p, n=n)
    r = torch.fft.irfft(tf.real ** 2 + tf.imag ** 2, n=n)[..., :filter_length]
    b = torch.fft.irfft(tf.conj() * pf, n=n)[..., :filter_length]
    lag = (torch.arange(filter_length)[:, None] - torch.arange(filter_length)[None, :]).abs()
    R = r[..., lag]
    Rf, bf = R.reshape(-1, filter_length, filter_length), b.reshape(-1, filter_length)
    x = torch.stack([torch.linalg.solve(Rf[i], bf[i]) for i in range(bf.shape[0])]).reshape(b.shape)  # one call per matrix: see models/utils/metrics.py
    coh = (b * x).sum(-1)
    val = 10 * torch.log10(coh / (1 - coh))
    return (val, R) if return_r else val


def ref_ratios(preds, target):
    """fp64 closed forms of torchmetrics' snr, si_sdr, si_snr (element-wise distortions) -> [..., 3]"""
    p, t = preds.double(), target.double()

    def sisdr(p, t):
        alpha = ((p * t).sum(-1, keepdim=True) + EPS) / ((t * t).sum(-1, keepdim=True) + EPS)
        ts = alpha * t
        return 10 * torch.log10(((ts * ts).sum(-1) + EPS) / (((ts - p) ** 2).sum(-1) + EPS))

    snr = 10 * torch.log10(((t * t).sum(-1) + EPS) / (((t - p) ** 2).sum(-1) + EPS))
    return torch.stack([snr, sisdr(p, t), sisdr(p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True))], -1)


@functools.lru_cache(maxsize=None)
def ar2_pair(B, S, N, dc=0.0, noise=0.05, filtered=True):
    """targets: AR(2) noise s[n] = 1.6 s[n-1] - 0.8 s[n-2] + e[n]; estimates: the target through [0.1, 0.9, 0.2, -0.05] plus `noise` (relative to the
    target's RMS) white noise, or (filtered=False) the target itself plus the noise.  fp32 [B,S,N]; dc is added to both."""
    g = torch.Generator().manual_seed(1000 * B + 100 * S + N)
    burn = 64
    e = torch.randn(B, S, N + burn, generator=g, dtype=torch.float64)
    s = torch.zeros_like(e)
    for n in range(2, N + burn):
        s[..., n] = 1.6 * s[..., n - 1] - 0.8 * s[..., n - 2] + e[..., n]
    s = s[..., burn:]
    if filtered:
        h = torch.tensor([0.1, 0.9, 0.2, -0.05], dtype=torch.float64)
        est = torch.nn.functional.conv1d(torch.nn.functional.pad(s.reshape(B * S, 1, N), (3, 0)), h.flip(0)[None, None]).reshape(B, S, N)
    else:
        est = s.clone()
    est = est + noise * s.pow(2).mean(-1, keepdim=True).sqrt() * torch.randn(B, S, N, generator=g, dtype=torch.float64)
    return (s + dc).float().contiguous(), (est + dc).float().contiguous()


def to(backend, *ts):
    return [t.to(backend.device).contiguous() for t in ts]


# ---------------- published values ----------------
def test_restatement_reproduces_the_published_values():
    torch.manual_seed(1)
    preds, target = torch.randn(8000), torch.randn(8000)
    assert abs(float(ref_sdr(preds, target)) - (-12.0589)) <= 2e-4
    target, preds = torch.tensor([3.0, -0.5, 2.0, 7.0]), torch.tensor([2.5, 0.0, 2.0, 8.0])
    got = ref_ratios(preds, target)
    for v, want in zip(got.tolist(), (16.1805, 18.4030, 15.0918)):
        assert abs(v - want) <= 2e-4, (got, want)


def test_published_sdr(backend):
    torch.manual_seed(1)
    preds, target = torch.randn(8000), torch.randn(8000)
    p, t = to(backend, preds[None, None], target[None, None])
    got = float(ops.sdr(backend.lib, p, t))
    print("sdr", got, "restatement", float(ref_sdr(preds, target)))
    assert abs(got - (-12.0589)) <= 2e-4


def test_published_ratios_and_filter_length_1(backend):
    target, preds = torch.tensor([3.0, -0.5, 2.0, 7.0]), torch.tensor([2.5, 0.0, 2.0, 8.0])
    p, t = to(backend, preds[None, None], target[None, None])
    got = ops.signal_ratios(backend.lib, p, t)[0, 0].tolist()
    print("snr, si_sdr, si_snr", got)
    for v, want in zip(got, (16.1805, 18.4030, 15.0918)):
        assert abs(v - want) <= 2e-4, (got, want)
    sdr1 = float(ops.sdr(backend.lib, p, t, filter_length=1))
    assert abs(sdr1 - float(ref_sdr(preds, target, 1))) <= 1e-4


# ---------------- SDR against the restatement ----------------
@pytest.mark.parametrize("zero_mean", [False, True], ids=["raw", "zero_mean"])
@pytest.mark.parametrize("B,S", [(1, 1), (3, 3), (5, 2)])
@pytest.mark.parametrize("L", [512, 16, 1])
@pytest.mark.parametrize("N", [512, 513, 1000, 4001])
def test_sdr_matches_restatement(backend, N, L, B, S, zero_mean):
    target, preds = ar2_pair(B, S, N, dc=0.3 if zero_mean else 0.0)
    want, R = ref_sdr(preds, target, L, zero_mean, return_r=True)
    cond = float(torch.linalg.cond(R).max())
    predicted = cond * 512 * 2.0 ** -53 * (10 / math.log(10)) * (1 + 10 ** (float(want.max()) / 10))  # 1 / (1 - coh) = 1 + 10^(SDR / 10)
    assert predicted <= 1e-4, (cond, want, predicted)
    if N == 4001:
        assert cond <= 1e4 and float(want.max()) <= 30.0, (cond, want)
    p, t = to(backend, preds, target)
    got = ops.sdr(backend.lib, p, t, filter_length=L, zero_mean=zero_mean).cpu().double()
    err = float((got - want).abs().max())
    print(f"N={N} L={L} B={B} S={S} zero_mean={zero_mean}: cond {cond:.3g} sdr {float(want.min()):.3f}..{float(want.max()):.3f} dB, max |err| {err:.3g} dB")
    assert err <= 1e-4


def test_sdr_near_perfect_estimate(backend):
    target, preds = ar2_pair(2, 2, 4001, noise=1e-3, filtered=False)
    want = ref_sdr(preds, target)
    assert float(want.min()) > 55.0
    p, t = to(backend, preds, target)
    got = ops.sdr(backend.lib, p, t).cpu().double()
    print("near-perfect", want.tolist(), got.tolist())
    assert float((got - want).abs().max()) <= 1e-2


# ---------------- repeatability, workspace, refusals ----------------
def _guarded(nbytes, device):
    buf = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=device)
    return buf, buf[:nbytes]


def test_two_calls_are_bitwise_equal_and_ws_is_exact(backend):
    lib, dev = backend.lib, backend.device
    target, preds = ar2_pair(3, 3, 1000)
    p, t = to(backend, preds, target)
    mix = p.sum(1).contiguous()
    calls = {
        "sdr": (lib.nbss_sdr_ws_bytes(3, 3, 1000, 512), lambda ws: ops.sdr(lib, p, t, ws=ws)),
        "ratios": (lib.nbss_signal_ratios_ws_bytes(3, 3), lambda ws: ops.signal_ratios(lib, p, t, ws=ws)),
        "scale": (lib.nbss_recover_scale_ws_bytes(3, 3), lambda ws: ops.recover_scale(lib, p, mix + 0.1 * t[:, 0], False, True, ws=ws)),
    }
    for name, (nbytes, fn) in calls.items():
        assert nbytes > 0, name
        buf, ws = _guarded(nbytes, dev)
        a = fn(ws)
        assert bool((buf[nbytes:] == 0xA5).all()), f"{name} wrote behind its workspace"
        b = fn(None)  # fresh (poisoned) workspace
        assert torch.isfinite(a).all() and torch.equal(a, b), name


def test_refusals(backend):
    lib, dev = backend.lib, backend.device
    x = torch.zeros(1025 * 512, dtype=torch.float32, device=dev)
    o = torch.zeros(1025 * 5, dtype=torch.float32, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    xp, op, wp = x.data_ptr(), o.data_ptr(), ws.data_ptr()
    st = None if backend.name == "emu" else torch.cuda.current_stream(dev).cuda_stream
    EUNSUPPORTED = -2
    assert lib.nbss_sdr(1, 1, 1000, 0, 0, xp, xp, op, wp, st) == EUNSUPPORTED     # filter_length 0
    assert lib.nbss_sdr(1, 1, 1000, 513, 0, xp, xp, op, wp, st) == EUNSUPPORTED   # filter_length 513
    assert lib.nbss_sdr(1, 1, 511, 512, 0, xp, xp, op, wp, st) == EUNSUPPORTED    # N < filter_length
    assert lib.nbss_sdr(1, 5, 512, 512, 0, xp, xp, op, wp, st) == EUNSUPPORTED    # S = 5
    assert lib.nbss_sdr(1025, 1, 512, 512, 0, xp, xp, op, wp, st) == EUNSUPPORTED  # B = 1025
    assert lib.nbss_signal_ratios(1, 5, 512, xp, xp, op, wp, st) == EUNSUPPORTED
    assert lib.nbss_signal_ratios(1025, 1, 512, xp, xp, op, wp, st) == EUNSUPPORTED
    assert lib.nbss_recover_scale(1, 5, 512, 0, xp, xp, op, wp, st) == EUNSUPPORTED
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.sdr(lib, x[:2 * 600].view(1, 2, 600), x[:2 * 600].view(1, 2, 600), filter_length=601)


# ---------------- SNR, SI-SDR, SI-SNR ----------------
@pytest.mark.parametrize("B,S,N", [(1, 1, 1), (3, 3, 37), (2, 2, 4001)])
def test_signal_ratios_match_closed_forms(backend, B, S, N):
    g = torch.Generator().manual_seed(N)
    target = torch.randn(B, S, N, generator=g) + 0.4  # a mean: SI-SNR removes it, the other two do not
    preds = 0.8 * target + 0.3 * torch.randn(B, S, N, generator=g) + 0.2
    want = ref_ratios(preds, target)
    p, t = to(backend, preds, target)
    got = ops.signal_ratios(backend.lib, p, t).cpu().double()
    print(f"B={B} S={S} N={N}: max |err| {float((got - want).abs().max()):.3g} dB; first pair {got[0, 0].tolist()}")
    assert float((got - want).abs().max()) <= 1e-4


# ---------------- recover_scale ----------------
@pytest.mark.parametrize("norm", [False, True], ids=["keep_max", "norm_if_exceed_1"])
@pytest.mark.parametrize("together", [False, True], ids=["per_source", "together"])
@pytest.mark.parametrize("B,S,N", [(3, 2, 1000), (2, 3, 513)])
def test_recover_scale_matches_lstsq(backend, B, S, N, together, norm):
    g = torch.Generator().manual_seed(7 * N + S)
    preds = torch.randn(B, S, N, generator=g)  # independent noise: a well conditioned Gram matrix
    gains = 0.5 + 2.0 * torch.rand(B, S, 1, generator=g)
    mixture = (gains * preds).sum(1) + 0.1 * torch.randn(B, N, generator=g)
    pd, xd = preds.double(), mixture.double()
    assert float(torch.linalg.cond(pd @ pd.transpose(-1, -2)).max()) <= 100
    A = (pd.sum(1, keepdim=True) if together else pd).transpose(-1, -2)
    want = pd * torch.linalg.lstsq(A, xd[..., None]).solution
    if norm:
        mx = want.abs().amax(-1, keepdim=True)
        assert bool((mx > 1).any())
        want = want / torch.where(mx > 1, mx, torch.ones_like(mx))
    p, x = to(backend, preds, mixture)
    got = ops.recover_scale(backend.lib, p, x, together, norm).cpu().double()
    rel = float((got - want).abs().max() / want.abs().max())
    print(f"B={B} S={S} N={N} together={together} norm={norm}: relative error {rel:.3g}")
    assert rel <= 1e-5
