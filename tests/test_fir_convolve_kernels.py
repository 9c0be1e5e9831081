"""The RIR convolution kernels (nbss_amd/csrc/conv1d.hip: nbss_fir_convolve, nbss_rir_delay) against an fp64 restatement of the definition in
include/nbss_hip.h, on the emulator and, under -m gpu, on the device.

Comparator: `ref_window`, numpy.convolve in fp64 cut at the delay; `test_comparator_against_scipy` checks it against scipy.signal.fftconvolve.

Bar, rel-L2 against the comparator: the larger of
  * twice the error of the shipped path (data_loaders.gpu_simulation.fft_convolve in fp32, cut at the same delay) on the same inputs, measured here, and
  * eps_fp32 sqrt(L), the random-walk bound of an L-term fp32 sum.
Every case prints both errors and the bar.

Sizes at which the kernel takes another path: 16 (a tap block, a tile row), 256 (an MFMA tile), 2048 (outputs of a workgroup, taps of a chunk),
N % 4 or L % 4 != 0 (element-wise staging), M in {1, 2 | 4, others} (1, 2 or 3 microphones per workgroup), more than 2048 (b, s) pairs (grid walk)."""
import functools

import numpy as np
import pytest
import torch

from data_loaders.gpu_simulation import fft_convolve
from nbss_amd import ops
from nbss_amd._lib import NbssError

EPS = float(np.finfo(np.float32).eps)
ITEMS_PER_PASS = 2048  # CONV_MAX_ITEMS in conv1d.hip


def ref_window(x, h, delay):
    """x [B,S,N], h [B,S,M,L], delay [B,S] -> y [B,S,M,N] in fp64: the full convolution, N samples from the delay onward"""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    (B, S, N), (M, L) = x.shape, h.shape[2:]
    y = np.zeros((B, S, M, N))
    for b in range(B):
        for s in range(S):
            for m in range(M):
                full = np.concatenate([np.convolve(x[b, s], h[b, s, m]), np.zeros(L)])  # N + 2 L - 1 samples: delay + N never runs out
                y[b, s, m] = full[delay[b, s]: delay[b, s] + N]
    return y


def rel_l2(y, ref):
    return float(np.linalg.norm(np.asarray(y, dtype=np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


@functools.lru_cache(maxsize=None)
def inputs(B, S, M, N, L, seed=0):
    g = torch.Generator().manual_seed(1000 * N + L + 7 * M + seed)
    return torch.randn(B, S, N, generator=g), torch.randn(B, S, M, L, generator=g)


def fft_window(x, h, delay, device):
    """the shipped path: fp32 FFT convolution on the backend's device, cut like convolve_aligned does"""
    full = fft_convolve(x.to(device)[:, :, None, :], h.to(device))
    idx = delay.to(device).long()[:, :, None, None] + torch.arange(x.shape[-1], device=device)
    return full.gather(-1, idx.expand(*h.shape[:3], x.shape[-1])).cpu()


def native(backend, x, h, delay, **kw):
    return ops.fir_convolve(backend.lib, x.to(backend.device), h.to(backend.device), delay.to(backend.device), **kw).cpu()


def check_bar(backend, x, h, delay, what):
    ref = ref_window(x.numpy(), h.numpy(), delay.numpy())
    e_nat = rel_l2(native(backend, x, h, delay).numpy(), ref)
    e_fft = rel_l2(fft_window(x, h, delay, backend.device).numpy(), ref)
    bar = max(2.0 * e_fft, EPS * h.shape[-1] ** 0.5)
    print(f"{backend.name} {what}: native {e_nat:.3e} fft {e_fft:.3e} bar {bar:.3e}")
    assert e_nat <= bar, (what, e_nat, e_fft, bar)


def delays_of(L):
    return sorted({0, L - 1, L // 2})


def test_comparator_against_scipy():
    from scipy.signal import fftconvolve
    x, h = inputs(2, 2, 3, 257, 100)
    x, h = x.double().numpy(), h.double().numpy()
    full = fftconvolve(x[:, :, None, :], h, mode="full", axes=-1)
    delay = np.array([[0, 99], [50, 7]])
    want = np.stack([np.stack([full[b, s, :, delay[b, s]: delay[b, s] + 257] for s in range(2)]) for b in range(2)])
    got = ref_window(x, h, delay)
    assert got.shape == want.shape and rel_l2(got, want) < 1e-14


@pytest.mark.parametrize("L", [1, 15, 16, 17, 31, 33, 100])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 255, 257])
def test_shapes(backend, N, L):
    """tap-block and output-tile edges, N < L, aligned and unaligned rows, every delay of {0, L - 1, mid}"""
    x, h = inputs(1, 1, 6, N, L)
    for d in delays_of(L):
        check_bar(backend, x, h, torch.tensor([[d]], dtype=torch.int32), f"N {N} L {L} delay {d}")


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("M", [1, 6, 7])
def test_microphones_sources_batches(backend, M, S, B):
    N, L = 257, 33
    x, h = inputs(B, S, M, N, L)
    delay = torch.tensor(delays_of(L) * 2, dtype=torch.int32)[:B * S].reshape(B, S)
    check_bar(backend, x, h, delay, f"B {B} S {S} M {M}")


@pytest.mark.parametrize("M,N,L", [(2, 2100, 2100), (4, 2048, 2048), (3, 4100, 40)], ids=lambda v: str(v))
def test_beyond_one_workgroup_and_one_chunk(backend, M, N, L):
    """more than 2048 outputs (a second workgroup along n) and more than 2048 taps (a second chunk through the LDS image)"""
    x, h = inputs(1, 1, M, N, L)
    check_bar(backend, x, h, torch.tensor([[L // 3]], dtype=torch.int32), f"M {M} N {N} L {L}")


def test_unaligned_base_pointer(backend):
    """aligned sizes on rows that do not start on a 16-byte boundary take the element-wise staging: the same bits"""
    x, h = inputs(1, 2, 2, 64, 32)
    delay = torch.tensor([[3, 17]], dtype=torch.int32)
    want = native(backend, x, h, delay)
    dev = backend.device
    xb, hb = torch.zeros(x.numel() + 1, device=dev), torch.zeros(h.numel() + 1, device=dev)
    xo, ho = xb[1:].view(x.shape), hb[1:].view(h.shape)
    xo.copy_(x), ho.copy_(h)
    assert xo.data_ptr() % 16 != 0 and ho.data_ptr() % 16 != 0 and xo.is_contiguous()
    got = ops.fir_convolve(backend.lib, xo, ho, delay.to(dev)).cpu()
    assert torch.equal(got, want)
    check_bar(backend, x, h, delay, "unaligned base")


def test_more_items_than_one_grid_pass(backend):
    """B S above the 2048 (b, s) pairs of one grid pass, at a tiny N: every item is computed, each with its own delay"""
    B, S, M, N, L = 683, 3, 1, 3, 2
    assert B * S > ITEMS_PER_PASS
    x, h = inputs(B, S, M, N, L)
    delay = (torch.arange(B * S, dtype=torch.int32) % L).reshape(B, S)
    y = native(backend, x, h, delay)
    xp = torch.nn.functional.pad(x.double(), (L, L))  # y[n] = sum_k h[k] x[n + d - k], written out
    n = torch.arange(N)
    want = sum(h[:, :, :, k:k + 1].double() * xp[:, :, None, :].expand(B, S, M, -1).gather(-1, (n + L + delay.long()[:, :, None, None] - k).expand(B, S, M, N))
               for k in range(L))
    assert rel_l2(y.numpy(), want.numpy()) <= EPS * L ** 0.5
    assert rel_l2(y[-1].numpy(), want[-1].numpy()) <= EPS * L ** 0.5 and float(y[-1].abs().max()) > 0  # the last item, reached in the second pass


def test_bitwise_repeatable_and_batch_invariant(backend):
    x, h = inputs(2, 3, 6, 257, 100)
    delay = torch.tensor([[0, 99, 50], [7, 31, 64]], dtype=torch.int32)
    y1, y2 = native(backend, x, h, delay), native(backend, x, h, delay)
    assert torch.equal(y1, y2)
    alone = native(backend, x[:1].contiguous(), h[:1].contiguous(), delay[:1].contiguous())
    assert torch.equal(alone[0], y1[0])


@pytest.mark.parametrize("N,L", [(257, 100), (16, 16), (2100, 2100)])
def test_unit_impulse_at_the_delay_reproduces_x(backend, N, L):
    x, _ = inputs(1, 2, 3, N, L)
    delay = torch.tensor([[L - 1, L // 2]], dtype=torch.int32)
    h = torch.zeros(1, 2, 3, L)
    h.scatter_(-1, delay.long()[:, :, None, None].expand(1, 2, 3, 1), 1.0)
    y = native(backend, x, h, delay)
    assert torch.equal(y, x[:, :, None, :].expand(1, 2, 3, N))


def test_refusals(backend):
    dev, lib = backend.device, backend.lib
    z = lambda *shape: torch.zeros(*shape, device=dev)
    d = lambda v, B=1, S=1: torch.full((B, S), v, dtype=torch.int32, device=dev)
    with pytest.raises(NbssError, match="EINVAL"):  # N < 1
        ops.fir_convolve(lib, z(1, 1, 0), z(1, 1, 2, 8), d(0))
    with pytest.raises(NbssError, match="EINVAL"):  # L < 1
        ops.fir_convolve(lib, z(1, 1, 8), z(1, 1, 2, 0), d(0))
    rc = lib.nbss_fir_convolve(1, 1, 2, 0, 8, z(4).data_ptr(), z(16).data_ptr(), d(0).data_ptr(), z(4).data_ptr(), None, None)
    assert rc == -1
    rc = lib.nbss_fir_convolve(1, 1, 2, 8, 0, z(8).data_ptr(), z(16).data_ptr(), d(0).data_ptr(), z(16).data_ptr(), None, None)
    assert rc == -1
    for bad in (-1, 8, 1 << 20):  # a delay outside [0, L): validated on the device
        with pytest.raises(NbssError, match="EINVAL"):
            ops.fir_convolve(lib, z(1, 1, 8), z(1, 1, 2, 8), d(bad))
    ops.fir_convolve(lib, z(1, 1, 8), z(1, 1, 2, 8), d(7))  # the last valid one
    # the caps of the header: L <= 65536, M <= 4096, B S M <= 2^22, N <= 2^24
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.fir_convolve(lib, z(1, 1, 8), z(1, 1, 1, 65537), d(0))
    ops.fir_convolve(lib, z(1, 1, 8), z(1, 1, 1, 65536), d(65535))
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.fir_convolve(lib, z(1, 1, 1), z(1, 1, 4097, 1), d(0))
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.fir_convolve(lib, z(2049, 2049, 1), z(2049, 2049, 1, 1), d(0, 2049, 2049))
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.fir_convolve(lib, z(1, 1, (1 << 24) + 1), z(1, 1, 1, 1), d(0))
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.rir_delay(lib, z(1, 1, 1, 65537), 0)
    for ref in (-1, 2):
        with pytest.raises(NbssError, match="EINVAL"):
            ops.rir_delay(lib, z(1, 1, 2, 8), ref)
    with pytest.raises(NbssError):  # shapes that do not belong together
        ops.fir_convolve(lib, z(1, 2, 8), z(1, 1, 2, 8), d(0))


# ---------------------------------------------------------------- nbss_rir_delay
def host_delay(h, ref):
    """the definition: the lowest index of the maximum, an fp64 loop"""
    h = np.asarray(h, dtype=np.float64)
    out = np.zeros(h.shape[:2], dtype=np.int64)
    for b in range(h.shape[0]):
        for s in range(h.shape[1]):
            best, at = -np.inf, 0
            for k, v in enumerate(h[b, s, ref]):
                if v > best:
                    best, at = v, k
            out[b, s] = at
    return out


@pytest.mark.parametrize("L", [1, 100, 257, 1000])
@pytest.mark.parametrize("ref", [0, 2])
def test_rir_delay_unique_maximum(backend, L, ref):
    _, h = inputs(2, 3, 4, 16, L, seed=3)
    if L > 1:
        assert all(len(np.unique(r)) == L for r in h[:, :, ref].reshape(-1, L).numpy())  # unique values: torch.argmax is defined
    got = ops.rir_delay(backend.lib, h.to(backend.device), ref).cpu()
    assert got.dtype == torch.int32 and got.shape == (2, 3)
    assert torch.equal(got.long(), h.to(backend.device)[:, :, ref].argmax(-1).cpu())
    assert np.array_equal(got.numpy(), host_delay(h.numpy(), ref))


def test_rir_delay_tie_takes_the_lowest_index(backend):
    L = 1000
    h = torch.rand(2, 2, 3, L, generator=torch.Generator().manual_seed(5)) - 2.0  # all below the planted maxima
    ties = {(0, 0): [300, 44, 700], (0, 1): [999, 998], (1, 0): [556, 300, 812], (1, 1): [0, 511]}  # 300 = 44 + 256: one thread; 556 = 300 + 256
    for (b, s), ks in ties.items():
        h[b, s, 1, ks] = 0.5
        h[b, s, 0, 10] = 3.0  # another channel's maximum must not matter
    got = ops.rir_delay(backend.lib, h.to(backend.device), 1).cpu()
    assert np.array_equal(got.numpy(), host_delay(h.numpy(), 1))
    assert got.tolist() == [[44, 998], [300, 0]]
    flat = torch.full((1, 1, 1, 700), -1.0)  # every sample equal: index 0
    assert ops.rir_delay(backend.lib, flat.to(backend.device), 0).item() == 0


def test_rir_delay_more_items_than_one_grid_pass(backend):
    B, S, L = 683, 3, 5
    h = torch.zeros(B, S, 1, L)
    want = (torch.arange(B * S) % L).reshape(B, S)
    h.scatter_(-1, want[:, :, None, None], 1.0)
    assert torch.equal(ops.rir_delay(backend.lib, h.to(backend.device), 0).cpu().long(), want)
