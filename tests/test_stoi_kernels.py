"""nbss_stoi (nbss_amd/csrc/stoi.hip) against an fp64 restatement of the definition in include/nbss_hip.h, on the emulator and, under -m gpu, on the
device.  The restatement below is written from that comment alone (numpy / scipy; the resampler is scipy.signal.resample_poly with the stated
taps), independently of models/utils/metrics.py.  pystoi itself is not installed: parity with it is not pinned anywhere.

Bar.  Not fixed in advance: the yardstick is the same restatement evaluated in fp32 throughout (fp32 taps, resampler, window, FFT, band sums and
segment statistics) against the fp64 one, the worst difference over the grid of `test_matches_restatement` (4 shapes x 2 flags x 4 pairs at 0 .. 20 dB).
The kernel may err by at most 4 x that (the margin is for another summation order in the MFMA DFT and the FIR).
Measured: fp32 restatement 1.05e-07 worst (STOI and eSTOI alike, per case 4.9e-08 .. 1.05e-07), so the bar is 4.21e-07; the kernel 4.61e-08 worst on
the emulator and 4.61e-08 on an MI355X (per case 2.1e-08 .. 4.6e-08: it resamples and takes its statistics in fp64, only the spectra are fp32, and
half an ulp of the fp32 result below 1 is already 3e-08).

The keep-or-drop decision of the silent-frame removal is a threshold: every test that compares values first asserts that no fp64 frame energy of its
inputs lies within 0.05 dB of max - 40 (the seeds are chosen so that this holds)."""
import functools

import numpy as np
import pytest
import scipy.fft
import scipy.signal
import torch

from nbss_amd import ops
from nbss_amd._lib import NbssError

EPS = 2.0 ** -52
RATIO = {8000: (5, 4), 16000: (5, 8), 10000: (1, 1)}
GRID = [(4001, 8000), (8000, 8000), (8000, 10000), (8000, 16000)]


# ---------------- the restatement ----------------
def ref_taps(p, q):
    fc = 1.0 / (2 * max(p, q))
    L = int(np.ceil((60 - 8) / (28.714 * fc / 10)))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7)) * 2 * p * fc * np.sinc(2 * fc * t)
    return p * h / h.sum()


def ref_frames(x, dt):
    """frames of 256 at hop 128, starts < len - 256 -> [frames, 256]"""
    starts = np.arange(0, len(x) - 256, 128)
    return np.stack([x[s:s + 256] for s in starts]).astype(dt) if len(starts) else np.zeros((0, 256), dt)


def ref_stoi(x, y, fs, extended, dt=np.float64, details=None):
    """one pair: clean x, estimate y (1-D arrays) -> the value, every step in `dt`"""
    x, y = np.asarray(x).astype(dt), np.asarray(y).astype(dt)
    p, q = RATIO[fs]
    if p != q:
        win = (ref_taps(p, q) / p).astype(dt)
        x, y = (scipy.signal.resample_poly(v, p, q, window=win).astype(dt) for v in (x, y))
    w = np.hanning(258)[1:-1].astype(dt)
    xf, yf = ref_frames(x, dt) * w, ref_frames(y, dt) * w
    E = 20 * np.log10(np.linalg.norm(xf, axis=1) + dt(EPS))
    mask = E > E.max() - 40
    if details is not None:
        details.update(energy=E.astype(np.float64), kept=int(mask.sum()), frames=len(E), resampled=len(x))
    xf, yf = xf[mask], yf[mask]
    K = len(xf)
    xs, ys = np.zeros(128 * (K - 1) + 256, dt), np.zeros(128 * (K - 1) + 256, dt)
    for i in range(K):
        xs[128 * i:128 * i + 256] += xf[i]
        ys[128 * i:128 * i + 256] += yf[i]
    f = np.arange(257) * (10000 / 512)
    k = np.arange(15)
    lo, hi = 150 * 2.0 ** ((2 * k - 1) / 6), 150 * 2.0 ** ((2 * k + 1) / 6)
    obm = np.zeros((15, 257), dt)
    for b in range(15):
        obm[b, np.argmin((f - lo[b]) ** 2):np.argmin((f - hi[b]) ** 2)] = 1

    def bands(s):
        fr = ref_frames(s, dt) * w
        if not len(fr):
            return np.zeros((15, 0), dt)
        spec = scipy.fft.rfft(fr, n=512, axis=1)
        return np.sqrt(obm @ (spec.real ** 2 + spec.imag ** 2).T.astype(dt))

    X, Y = bands(xs), bands(ys)
    if X.shape[1] < 30:
        return 1e-5
    M = X.shape[1] - 29
    Xs = np.stack([X[:, m:m + 30] for m in range(M)])
    Ys = np.stack([Y[:, m:m + 30] for m in range(M)])
    eps = dt(EPS)
    if extended:
        def rowcol(a):
            a = a - a.mean(2, keepdims=True)
            a = a / (np.linalg.norm(a, axis=2, keepdims=True) + eps)
            a = a - a.mean(1, keepdims=True)
            return a / (np.linalg.norm(a, axis=1, keepdims=True) + eps)
        return float((rowcol(Xs) * rowcol(Ys)).sum() / dt(30 * M))
    alpha = np.linalg.norm(Xs, axis=2, keepdims=True) / (np.linalg.norm(Ys, axis=2, keepdims=True) + eps)
    Yp = np.minimum(alpha * Ys, Xs * dt(1 + 10 ** (15 / 20)))
    xc, yc = Xs - Xs.mean(2, keepdims=True), Yp - Yp.mean(2, keepdims=True)
    d = (xc * yc).sum(2) / ((np.linalg.norm(xc, axis=2) + eps) * (np.linalg.norm(yc, axis=2) + eps))
    return float(d.mean())


def ref_batch(preds, target, fs, extended, dt=np.float64, margin=True):
    """[B,S,N] tensors -> [B,S] float64; asserts the threshold margin of every pair"""
    p, t = preds.numpy(), target.numpy()
    out = np.zeros(p.shape[:2])
    for b in range(p.shape[0]):
        for s in range(p.shape[1]):
            det = {}
            out[b, s] = ref_stoi(t[b, s], p[b, s], fs, extended, dt, det)
            if margin and dt is np.float64:
                gap = np.abs(det["energy"] - (det["energy"].max() - 40)).min()
                assert gap > 0.05, f"a frame energy lies {gap:.3g} dB from the threshold: pick another seed"
    return out


# ---------------- inputs ----------------
@functools.lru_cache(maxsize=None)
def ar2_pair(B, S, N, seed=0, lo_db=0.0, hi_db=20.0):
    """targets: AR(2) noise s[n] = 1.6 s[n-1] - 0.8 s[n-2] + e[n] (as test_metrics_kernels.ar2_pair); estimates: the target plus white noise at
    lo_db .. hi_db SNR, spread evenly over the B S pairs.  fp32 [B,S,N] -> (target, preds)"""
    g = torch.Generator().manual_seed(1000 * B + 100 * S + N + 7919 * seed)
    burn = 64
    e = torch.randn(B, S, N + burn, generator=g, dtype=torch.float64)
    s = torch.zeros_like(e)
    for n in range(2, N + burn):
        s[..., n] = 1.6 * s[..., n - 1] - 0.8 * s[..., n - 2] + e[..., n]
    s = s[..., burn:]
    s = 0.1 * s / s.pow(2).mean(-1, keepdim=True).sqrt()
    snr = torch.linspace(lo_db, hi_db, B * S, dtype=torch.float64).reshape(B, S, 1) if B * S > 1 else torch.full((1, 1, 1), 0.5 * (lo_db + hi_db))
    est = s + 0.1 * 10 ** (-snr / 20) * torch.randn(B, S, N, generator=g, dtype=torch.float64)
    return s.float().contiguous(), est.float().contiguous()


def to(backend, *ts):
    return [t.to(backend.device).contiguous() for t in ts]


@functools.lru_cache(maxsize=None)
def grid_refs():
    """{(N, fs, extended): (fp64 values, fp32 values)} of the grid, computed once"""
    out = {}
    for N, fs in GRID:
        target, preds = ar2_pair(2, 2, N)
        for ext in (False, True):
            out[N, fs, ext] = (ref_batch(preds, target, fs, ext), ref_batch(preds, target, fs, ext, np.float32))
    return out


@functools.lru_cache(maxsize=None)
def bar():
    refs = grid_refs()
    fp32 = max(float(np.abs(a - b).max()) for a, b in refs.values())
    assert fp32 > 0
    return 4 * fp32


def run(backend, preds, target, fs, ext, **kw):
    p, t = to(backend, preds, target)
    return ops.stoi(backend.lib, p, t, fs, ext, **kw).cpu().double().numpy()


# ---------------- the resampler's taps ----------------
def test_tap_counts_and_sum():
    for (p, q), n in (((5, 4), 365), ((5, 8), 581)):
        h = ref_taps(p, q)
        assert len(h) == n and abs(h.sum() - p) < 1e-12


@pytest.mark.parametrize("fs,n,p", [(8000, 365, 5), (16000, 581, 5), (10000, 1, 1)])
def test_kernel_taps(backend, fs, n, p):
    """the head of the workspace holds the taps after a call: their count, sum and values"""
    lib, N = backend.lib, 2400
    target, preds = ar2_pair(1, 1, N)
    nbytes = lib.nbss_stoi_ws_bytes(1, 1, N, fs)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=backend.device)
    pp, tt = to(backend, preds, target)
    ops.stoi(lib, pp, tt, fs, False, ws=ws)
    taps = ws[:592 * 8].cpu().view(torch.float64).numpy()
    assert np.count_nonzero(taps) == n and not taps[n:].any()
    assert abs(taps.sum() - p) < 1e-12
    want = ref_taps(*RATIO[fs]) if n > 1 else np.ones(1)
    assert np.abs(taps[:n] - want).max() < 1e-13


# ---------------- against the restatement ----------------
@pytest.mark.parametrize("ext", [False, True], ids=["stoi", "estoi"])
@pytest.mark.parametrize("N,fs", GRID)
def test_matches_restatement(backend, N, fs, ext):
    target, preds = ar2_pair(2, 2, N)
    want, want32 = grid_refs()[N, fs, ext]
    got = run(backend, preds, target, fs, ext)
    err = float(np.abs(got - want).max())
    print(f"N={N} fs={fs} ext={ext}: values {want.ravel().round(4).tolist()}, fp32 restatement {float(np.abs(want32 - want).max()):.3g}, "
          f"kernel {err:.3g}, bar {bar():.3g}")
    assert err <= bar()


def test_first_case_has_38_frames():
    det = {}
    target, preds = ar2_pair(2, 2, 4001)
    ref_stoi(target[0, 0].numpy(), preds[0, 0].numpy(), 8000, False, details=det)
    assert det["resampled"] == 5002 and det["frames"] == 38


@pytest.mark.parametrize("ext", [False, True], ids=["stoi", "estoi"])
def test_identity_and_scale(backend, ext):
    target, preds = ar2_pair(2, 2, 4001)
    ref_batch(preds, target, 8000, ext)  # the margin of these inputs
    one = run(backend, target, target, 8000, ext)
    print("stoi(x, x) - 1:", (one - 1).ravel().tolist())
    assert np.abs(one - 1).max() <= bar()
    base = run(backend, preds, target, 8000, ext)
    scaled_est = run(backend, 3.7 * preds, target, 8000, ext)
    scaled_both = run(backend, 0.31 * preds, 0.31 * target, 8000, ext)
    print("scale:", np.abs(scaled_est - base).max(), np.abs(scaled_both - base).max())
    assert np.abs(scaled_est - base).max() <= bar() and np.abs(scaled_both - base).max() <= bar()


@pytest.mark.parametrize("ext", [False, True], ids=["stoi", "estoi"])
def test_silent_middle_drops_frames(backend, ext):
    N, fs = 12000, 8000
    target, preds = ar2_pair(1, 2, N, seed=1)
    gain = torch.ones(N)
    gain[4000:8000] = 1e-3  # the middle 0.5 s is 60 dB down
    target, preds = (target * gain).contiguous(), (preds * gain).contiguous()
    det = {}
    ref_stoi(target[0, 0].numpy(), preds[0, 0].numpy(), fs, ext, details=det)
    assert det["kept"] < det["frames"] - 20 and det["kept"] > 31, det
    want = ref_batch(preds, target, fs, ext)
    got = run(backend, preds, target, fs, ext)
    print(f"kept {det['kept']} of {det['frames']} frames; err {np.abs(got - want).max():.3g}")
    assert np.abs(got - want).max() <= bar()


def test_fewer_than_30_frames(backend):
    target, preds = ar2_pair(1, 2, 2400)
    for ext in (False, True):
        got = ops.stoi(backend.lib, *to(backend, preds, target), 8000, ext).cpu()
        assert torch.equal(got, torch.full((1, 2), 1e-5, dtype=torch.float32))


def test_more_pairs_than_one_grid_pass_and_batch_invariance(backend):
    """65 pairs (the per-pair kernels walk 64 per grid pass), 33 frames each: every item equals the same item computed alone, bit for bit"""
    N = 3500
    target, preds = ar2_pair(65, 1, N, lo_db=5.0, hi_db=15.0)
    for ext in (False, True):
        want = ref_batch(preds[[0, 64]], target[[0, 64]], 8000, ext)
        p, t = to(backend, preds, target)
        got = ops.stoi(backend.lib, p, t, 8000, ext)
        assert np.abs(got[[0, 64]].cpu().double().numpy() - want).max() <= bar()
        for i in (0, 33, 64):
            alone = ops.stoi(backend.lib, p[i:i + 1].contiguous(), t[i:i + 1].contiguous(), 8000, ext)
            assert torch.equal(alone[0], got[i]), (i, ext)
        if ext:
            pair = ops.stoi(backend.lib, p[63:65].reshape(1, 2, N).contiguous(), t[63:65].reshape(1, 2, N).contiguous(), 8000, ext)
            assert torch.equal(pair.reshape(-1), got[63:65].reshape(-1))


@pytest.mark.parametrize("off", [1, 2])
def test_unaligned_rows(backend, off):
    """rows of preds 4 and 8 bytes off a 16-byte boundary (N odd, and the tensor itself offset)"""
    N = 4001
    target, preds = ar2_pair(2, 2, N)
    want = grid_refs()[N, 8000, True][0]
    buf = torch.zeros(off + preds.numel() + 4, dtype=torch.float32, device=backend.device)
    p = buf[off:off + preds.numel()].view(2, 2, N)
    p.copy_(preds)
    assert p.data_ptr() % 16 == 4 * off
    t, = to(backend, target)
    got = ops.stoi(backend.lib, p, t, 8000, True).cpu().double().numpy()
    assert np.abs(got - want).max() <= bar()


def test_two_calls_are_bitwise_equal_and_ws_is_exact(backend):
    lib, dev = backend.lib, backend.device
    target, preds = ar2_pair(2, 2, 4001)
    p, t = to(backend, preds, target)
    nbytes = lib.nbss_stoi_ws_bytes(2, 2, 4001, 8000)
    assert nbytes > 0
    for ext in (False, True):
        buf = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
        a = ops.stoi(lib, p, t, 8000, ext, ws=buf[:nbytes])
        assert bool((buf[nbytes:] == 0xA5).all()), "nbss_stoi wrote behind its workspace"
        b = ops.stoi(lib, p, t, 8000, ext)  # fresh (poisoned) workspace
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_refusals(backend):
    lib, dev = backend.lib, backend.device
    x = torch.zeros(4096, dtype=torch.float32, device=dev)
    o = torch.zeros(8192, dtype=torch.float32, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    xp, op, wp = x.data_ptr(), o.data_ptr(), ws.data_ptr()
    st = None if backend.name == "emu" else torch.cuda.current_stream(dev).cuda_stream
    EUNSUPPORTED = -2
    assert lib.nbss_stoi(1, 1, 4000, 44100, 0, xp, xp, op, wp, st) == EUNSUPPORTED   # fs
    assert lib.nbss_stoi(1, 5, 800, 8000, 0, xp, xp, op, wp, st) == EUNSUPPORTED     # S = 5
    assert lib.nbss_stoi(1025, 1, 800, 8000, 0, xp, xp, op, wp, st) == EUNSUPPORTED  # B = 1025
    assert lib.nbss_stoi(1, 1, 204, 8000, 0, xp, xp, op, wp, st) == EUNSUPPORTED     # 255 resampled samples (N = 205 gives 257)
    assert lib.nbss_stoi(1, 1, 256, 10000, 0, xp, xp, op, wp, st) == EUNSUPPORTED
    assert lib.nbss_stoi(1, 1, 409, 16000, 0, xp, xp, op, wp, st) == EUNSUPPORTED    # ceil(409 * 5 / 8) = 256 (N = 410 gives 257)
    assert lib.nbss_stoi(1, 1, 800, 8000, 2, xp, xp, op, wp, st) == -1               # an unknown flag
    for args in ((1, 1, 4000, 44100), (1, 5, 800, 8000), (1025, 1, 800, 8000), (1, 1, 204, 8000)):
        assert lib.nbss_stoi_ws_bytes(*args) == EUNSUPPORTED
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.stoi(lib, x[:800].view(1, 1, 800), x[:800].view(1, 1, 800), 44100)
