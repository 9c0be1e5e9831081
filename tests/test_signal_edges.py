"""The signal front and back end (nbss_amd/csrc/signal.hip) at its edges, against torch.stft / torch.istft in fp64 with the window handed over
explicitly (oracle/io_ref.py: hann_window(n_fft), or its square root for window=1).  tests/test_signal_loss_optim.py holds the round sizes; here:

  * sample counts that are no multiple of 4 (rows of x off the 16-byte boundary: the sample-by-sample instantiation of stft_norm_kernel), of the
    hop or of 16 frames, the shortest signal (N = n_fft), the last sample one short of a hop (N % hop == hop - 1, where the hann envelope is at its
    smallest), every reference channel, both windows, both stream dtypes;
  * inorm + iSTFT and its adjoint at the same lengths with 1 - 4 speakers, and at every wave split of a (b, speaker, 16-frame strip) task
    (istft_parts 8 / 4 / 2 / 1) including the grid-stride pass of istft_finalize_kernel;
  * models.io.stft.STFT on the device at [2, 3, 1201] (every leading dimension folded into the batch with one channel: rows 1201 samples apart);
  * one STFT launch beyond the 4096-workgroup cap of the grid.

The bars are those of tests/test_signal_loss_optim.py.  Not covered: the grid cap of the iSTFT kernels (more than 16 384 wave tasks there needs
hundreds of MB of fp64 reference)."""
import functools
import types

import pytest
import torch

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32, NbssError
from oracle import io_ref
from util import rel_l2

WIN = {0: "hann_window", 1: "sqrt_hann_window"}

# (B, C, N, n_fft): 1201 / 1203 / 1027 / 257 / 383 / 2302 are no multiple of 4 (2302: rows alternately 8 and 16 bytes aligned), 300 and 256 are but
# are shorter than three hops; 256 = n_fft is the shortest signal the entry point takes (T = 3); 383 = 3 hops - 1
STFT_CASES = [(2, 2, 1201, 256), (2, 3, 1203, 256), (3, 1, 1027, 512), (1, 2, 300, 256), (1, 1, 256, 256), (2, 1, 257, 256), (1, 1, 383, 256),
              (2, 2, 2302, 256)]


def case_id(c):
    return "x".join(map(str, c))


@functools.lru_cache(maxsize=None)
def stft_reference(B, C, N, n_fft, window):
    """seeded x [B,C,N] and torch.stft of it in fp64 -> (x, complex [B,C,F,T]); computed once per case, never modified"""
    g = torch.Generator().manual_seed(1000 * window + N + 7 * B + C)
    x = torch.randn(B, C, N, generator=g)
    return x, io_ref.stft(x.double(), n_fft, n_fft // 2, WIN[window])


def check_stft_norm(backend, B, C, N, n_fft, window):
    x, Xc = stft_reference(B, C, N, n_fft, window)
    want = io_ref.to_real_layout(Xc)
    tab = ops.stft_tables(backend.lib, n_fft, window, backend.device)
    xd = x.to(backend.device)
    worst = {}

    def bar(what, err, tol):
        worst[what] = max(worst.get(what, 0.0), err)
        assert err <= tol, (what, err, tol)

    for ref in range(C):
        Xn, mm = io_ref.norm_frequency_online(Xc, ref)
        wantn = io_ref.to_real_layout(Xn)
        X, xrmm = ops.stft_norm_fwd(backend.lib, n_fft, NBSS_F32, tab, xd, ref_channel=ref)
        assert X.shape == want.shape and xrmm.shape == mm[:, 0].shape
        bar("xrmm", rel_l2(xrmm, mm[:, 0]), 2e-5)
        # un-normalised spectrum (fp32 DFT accuracy), with the reference's magnitudes as tests/test_signal_loss_optim.py does and with the kernel's
        # own as STFT.stft does; the normalised one divides by |X_ref|, which can be ~1e-3: single bins amplify the rounding of the magnitude
        bar("f32 X*mm_ref", rel_l2(X.double().cpu() * mm[:, 0][..., None], want), 2e-5)
        bar("f32 X*xrmm", rel_l2(X.double().cpu() * xrmm.double().cpu()[..., None], want), 2e-5)
        bar("f32 X", rel_l2(X, wantn), 1e-3)
        Xb, xrmm_b = ops.stft_norm_fwd(backend.lib, n_fft, NBSS_BF16, tab, xd, ref_channel=ref)
        assert Xb.dtype == torch.bfloat16
        bar("xrmm", rel_l2(xrmm_b, mm[:, 0]), 2e-5)
        bar("bf16 X*xrmm", rel_l2(Xb.double().cpu() * xrmm.double().cpu()[..., None], want), 5e-3)
        bar("bf16 X", rel_l2(Xb.float(), wantn), 5e-3)
    print(f"stft_norm [{backend.name}] {(B, C, N, n_fft)} window {window}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("case", STFT_CASES, ids=case_id)
def test_stft_norm_edges(backend, case, window):
    check_stft_norm(backend, *case, window)


def test_stft_norm_refuses_short_signals(backend):
    for n_fft in (256, 512):
        x = torch.zeros(1, 1, n_fft - 1, device=backend.device)
        tab = ops.stft_tables(backend.lib, n_fft, 0, backend.device)
        with pytest.raises(NbssError, match="EINVAL"):
            ops.stft_norm_fwd(backend.lib, n_fft, NBSS_F32, tab, x, ref_channel=0)


@pytest.mark.gpu
def test_stft_norm_beyond_the_grid_cap(hip_lib):
    """B cdiv(T,16) MTq = 32 * 16 * 33 = 16 896 wave tasks > 4096 workgroups of 4 waves: the task loop of stft_norm_kernel takes a second pass"""
    B, C, N, n_fft = 32, 1, 62721, 512
    assert B * -(-(N // (n_fft // 2) + 1) // 16) * -(-(n_fft + 2) // 16) > 16384
    check_stft_norm(types.SimpleNamespace(name="hip", lib=hip_lib, device=torch.device("cuda:0")), B, C, N, n_fft, 0)


# ---- inorm + iSTFT, forward and adjoint ----
def check_istft(backend, B, S, N, n_fft, window):
    g = torch.Generator().manual_seed(N + 31 * S + 1000 * window + B)
    F, T = n_fft // 2 + 1, N // (n_fft // 2) + 1
    out = torch.randn(B, F, T, 2 * S, generator=g)
    xrmm = torch.rand(B, F, T, generator=g) + 0.5
    dy = torch.randn(B, S, N, generator=g)
    tab = ops.stft_tables(backend.lib, n_fft, window, backend.device)
    y = ops.inorm_istft_fwd(backend.lib, n_fft, tab, out.to(backend.device), xrmm.to(backend.device), N)
    o64 = out.double().requires_grad_(True)
    want = io_ref.istft(io_ref.from_real_layout(o64) * xrmm.double()[:, None], N, n_fft, n_fft // 2, WIN[window])
    e_fwd = rel_l2(y, want)
    (want * dy.double()).sum().backward()
    dout = ops.inorm_istft_bwd(backend.lib, n_fft, tab, dy.to(backend.device), xrmm.to(backend.device))
    e_bwd = rel_l2(dout, o64.grad)
    print(f"inorm_istft [{backend.name}] {(B, S, N, n_fft)} window {window}: fwd {e_fwd:.2e} bwd {e_bwd:.2e}")
    assert y.shape == (B, S, N) and e_fwd <= 2e-5, e_fwd
    assert dout.shape == out.shape and e_bwd <= 2e-5, e_bwd
    return e_fwd, e_bwd


@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("case", STFT_CASES, ids=case_id)
def test_inorm_istft_edges(backend, case, window):
    B, _, N, n_fft = case
    for S in (1, 2, 3, 4):
        check_istft(backend, B, S, N, n_fft, window)


# The iSTFT kernels deal a (b, speaker, 16-frame strip) task to istft_parts(ntask) waves, ntask = B S cdiv(T, 16): np doubles from 1 while np < 8 and
# ntask np < 1024.  n_fft 256: N = 1200 has T = 10 (one strip), N = 2300 has T = 18 (two strips).
#   (1, 1, 1200)    ntask    1 -> 8 waves
#   (32, 4, 1200)   ntask  128 -> 8 waves (128 * 4 = 512 is still below 1024)
#   (64, 4, 1200)   ntask  256 -> 4 waves
#   (128, 4, 1200)  ntask  512 -> 2 waves; B S N = 614 400 > 2048 * 256: istft_finalize_kernel takes a second grid-stride pass
#   (64, 4, 2300)   ntask  512 -> 2 waves, two strips
#   (128, 4, 2300)  ntask 1024 -> 1 wave, two strips (the only value that needs ntask >= 1024); the finalize kernel strides here too
WAVE_SPLIT_CASES = [(1, 1, 1200, 8), (32, 4, 1200, 8), (64, 4, 1200, 4), (128, 4, 1200, 2), (64, 4, 2300, 2), (128, 4, 2300, 1)]


def istft_parts(ntask):
    """restated from signal.hip"""
    n = 1
    while n < 8 and ntask * n < 1024:
        n *= 2
    return n


@pytest.mark.parametrize("B,S,N,parts", WAVE_SPLIT_CASES, ids=lambda v: str(v))
def test_inorm_istft_wave_splits(backend, B, S, N, parts):
    n_fft = 256
    assert istft_parts(B * S * -(-(N // (n_fft // 2) + 1) // 16)) == parts
    check_istft(backend, B, S, N, n_fft, 0)


def test_wave_split_cases_reach_every_split_and_the_finalize_stride():
    assert {c[3] for c in WAVE_SPLIT_CASES} == {1, 2, 4, 8}
    assert any(B * S * N > 2048 * 256 for (B, S, N, _) in WAVE_SPLIT_CASES)


def test_inorm_istft_noncontiguous_out_is_refused(backend):
    """`out` as a strided view (the speaker pairs of a wider tensor): ops._ptr refuses it before anything is launched, it is not read with the wrong
    strides; its contiguous copy gives the parity of the other tests"""
    B, S, N, n_fft = 2, 2, 1201, 256
    F, T = n_fft // 2 + 1, N // (n_fft // 2) + 1
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(B, F, T, 4 * S, generator=g).to(backend.device)
    out = wide[..., :2 * S]
    assert not out.is_contiguous()
    xrmm = (torch.rand(B, F, T, generator=g) + 0.5).to(backend.device)
    tab = ops.stft_tables(backend.lib, n_fft, 0, backend.device)
    with pytest.raises(NbssError, match="contiguous"):
        ops.inorm_istft_fwd(backend.lib, n_fft, tab, out, xrmm, N)
    y = ops.inorm_istft_fwd(backend.lib, n_fft, tab, out.contiguous(), xrmm, N)
    want = io_ref.istft(io_ref.from_real_layout(out.cpu().double()) * xrmm.cpu().double()[:, None], N, n_fft, n_fft // 2)
    assert rel_l2(y, want) <= 2e-5


# ---- the module: models/io/stft.py on the device ----
def check_stft_module(stft_cls, device, n_fft, win):
    mod = stft_cls(n_fft, n_fft // 2, win=win)
    N = 1201
    g = torch.Generator().manual_seed(n_fft)
    x = torch.randn(2, 3, N, generator=g)
    X, length = mod.stft(x.to(device))
    want = io_ref.stft(x.double(), n_fft, n_fft // 2, win)
    assert length == N and X.shape == want.shape and X.dtype == torch.complex64
    e_stft = rel_l2(X, want)
    y = mod.istft(X, N)
    assert y.shape == x.shape
    e_round = rel_l2(y, x)
    # gradient of .istft (through _IstftFn) against autograd of torch.istft, at a random spectrum
    Xr = torch.view_as_complex(torch.randn(2, 3, n_fft // 2 + 1, X.shape[-1], 2, generator=g))
    dy = torch.randn(2, 3, N, generator=g)
    leaf = Xr.clone().to(device).requires_grad_(True)
    (mod.istft(leaf, N) * dy.to(device)).sum().backward()
    leaf64 = Xr.to(torch.complex128).requires_grad_(True)
    (io_ref.istft(leaf64, N, n_fft, n_fft // 2, win) * dy.double()).sum().backward()
    e_grad = rel_l2(leaf.grad, leaf64.grad)
    print(f"STFT({n_fft}, {n_fft // 2}, win={win}) on {device}: stft {e_stft:.2e} round trip {e_round:.2e} istft gradient {e_grad:.2e}")
    assert e_stft <= 2e-5, e_stft
    assert e_round <= 1e-5, e_round
    assert e_grad <= 2e-5, e_grad


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,win", [(256, "hann_window"), (512, "sqrt_hann_window")])
def test_stft_module_on_the_device(hip_lib, n_fft, win):
    from models.io.stft import STFT
    check_stft_module(STFT, torch.device("cuda:0"), n_fft, win)
