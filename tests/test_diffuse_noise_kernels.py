"""The diffuse-noise kernel (nbss_amd/csrc/diffuse.hip: nbss_diffuse_noise) against the definition in include/nbss_hip.h, on the emulator and, under
-m gpu, on the device.

Comparator: data_loaders.gpu_simulation.gen_diffuse_noise on fp64 copies of the inputs; `test_comparator_against_golden_pin` re-checks it against the
reference's own generator as stored in tests/golden/oracle_pins.npz (the noise drawn exactly as tests/test_gpu_simulation.py draws it).

Bar, rel-L2 against the comparator: the larger of
  * twice the error of the shipped path (gen_diffuse_noise in fp32 on the backend's device) on the same inputs, measured here, and
  * eps_fp32 sqrt(2 nfft + M), the random-walk bound of the three chained fp32 sums (forward transform, mix, inverse transform).
Every case prints both errors and the bar.

Cs is RANDOM complex unless a case says otherwise: not symmetric, bin 0 not empty, imaginary parts at bins 0 and nfft / 2: a swapped index, a missing
conjugate or a mishandled edge bin does not pass.

Sizes at which the kernel takes another path: 64 (a hop: the number of frames changes), 128 / 256 (the padding, a whole frame), STRIP = 832 output samples
of one workgroup (a second strip along n), M = 1 .. 16 (one instantiation each; above 7 channels the LDS image passes 64 KB), more than ITEMS_PER_PASS
items (grid walk)."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import data_loaders.gpu_simulation as gs
from nbss_amd import ops
from nbss_amd._lib import NbssError

EPS = float(np.finfo(np.float32).eps)
NFFT = 256
F = NFFT // 2 + 1
STRIP = 832           # DiffuseGeom<256>::STRIP in diffuse.hip: 13 hops of 64 output samples per workgroup
ITEMS_PER_PASS = 128  # DN_MAX_ITEMS in diffuse.hip


def rel_l2(y, ref):
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(y - ref) / max(np.linalg.norm(ref), 1e-300))


@functools.lru_cache(maxsize=None)
def random_cs(M, seed=0):
    g = torch.Generator().manual_seed(977 * M + seed)
    return torch.complex(torch.randn(F, M, M, generator=g), torch.randn(F, M, M, generator=g))


@functools.lru_cache(maxsize=None)
def inputs(B, M, N, seed=0, offset=0.0):
    return offset + torch.randn(B, M, N, generator=torch.Generator().manual_seed(1000 * N + 7 * M + B + seed))


def comparator(white, Cs):
    return gs.gen_diffuse_noise(white.double(), white.shape[-1], Cs.to(torch.complex128)).numpy()


def native(backend, white, Cs, **kw):
    return ops.diffuse_noise(backend.lib, white.to(backend.device), Cs.to(backend.device), **kw).cpu()


def check_bar(backend, white, Cs, what, ref=None):
    M, N = white.shape[-2:]
    ref = comparator(white, Cs) if ref is None else ref
    y = native(backend, white, Cs)
    assert y.shape == white.shape and y.dtype == torch.float32 and torch.isfinite(y).all()
    e_nat = rel_l2(y.numpy(), ref)
    e_fft = rel_l2(gs.gen_diffuse_noise(white.to(backend.device), N, Cs.to(backend.device)).cpu().numpy(), ref)
    bar = max(2.0 * e_fft, EPS * (2 * NFFT + M) ** 0.5)
    print(f"{backend.name} {what}: native {e_nat:.3e} torch {e_fft:.3e} bar {bar:.3e}")
    assert e_nat <= bar, (what, e_nat, e_fft, bar)
    return y


@functools.lru_cache(maxsize=None)
def golden():
    """(noise [3, 4000] fp64, Cs complex128, the reference's output) of tests/test_gpu_simulation.py::test_diffuse_noise_coherence_and_reference"""
    pos = torch.tensor([[0.0, 0, 0], [0.05, 0, 0], [0.2, 0, 0]])
    Cs = gs.diffuse_mixing_matrices(pos, 8000)[1]
    g = torch.Generator().manual_seed(2)
    torch.randn(3, 160000, generator=g, dtype=torch.float64)  # the existing test's first draw from the same generator
    noise = torch.randn(3 * 4000, generator=g, dtype=torch.float64).reshape(3, 4000)
    return noise, Cs, np.load(Path(__file__).resolve().parent / "golden" / "oracle_pins.npz")["diffuse/noise"]


def test_comparator_against_golden_pin():
    noise, Cs, want = golden()
    got = gs.gen_diffuse_noise(noise, 4000, Cs)
    assert np.abs(got.numpy() - want).max() < 1e-8 * max(1.0, np.abs(want).max())


def test_golden_pin_through_the_kernel(backend):
    """N = 4000, M = 3: five strips, the last one partial; the reference's own output is the target"""
    noise, Cs, want = golden()
    white, Cs32 = noise.float()[None], Cs.to(torch.complex64)
    y = check_bar(backend, white, Cs32, "golden N 4000 M 3")
    e_pin, bar = rel_l2(y[0].numpy(), want), EPS * (2 * NFFT + 3) ** 0.5
    print(f"{backend.name} against the pin: {e_pin:.3e} bar {bar:.3e}")
    assert e_pin <= bar


@pytest.mark.parametrize("N", [2, 63, 64, 65, 127, 129, 255, 256, 257, 1000, STRIP - 1, STRIP, STRIP + 1])
def test_lengths(backend, N):
    """hop, padding, frame and strip edges; rows that do not start on 16-byte boundaries"""
    check_bar(backend, inputs(2, 3, N), random_cs(3), f"N {N}")


def test_one_sample_gives_exactly_zero(backend):
    y = native(backend, inputs(2, 3, 1), random_cs(3))
    assert y.shape == (2, 3, 1) and torch.equal(y, torch.zeros(2, 3, 1))


@pytest.mark.parametrize("M", [1, 2, 3, 6, 8, 16])
def test_channels(backend, M):
    check_bar(backend, inputs(1, M, 257), random_cs(M), f"M {M}")


def test_circular_array_mixing_matrices(backend):
    """the matrices the data module uses: six microphones on a circle of 10 cm, bin 0 empty"""
    ang = torch.arange(6) * (2 * np.pi / 6)
    pos = torch.stack([0.1 * torch.cos(ang), 0.1 * torch.sin(ang), torch.zeros(6)], 1)
    Cs = gs.diffuse_mixing_matrices(pos, 8000)[1].to(torch.complex64)
    check_bar(backend, inputs(2, 6, 1000), Cs, "circular array M 6 N 1000")


def test_more_items_than_one_grid_pass(backend):
    B = ITEMS_PER_PASS + 3
    white, Cs = inputs(B, 1, 65), random_cs(1)
    ref = comparator(white, Cs)
    y = check_bar(backend, white, Cs, f"B {B} M 1 N 65", ref)
    bar = EPS * (2 * NFFT + 1) ** 0.5
    assert rel_l2(y[-1].numpy(), ref[-1]) <= bar and float(y[-1].abs().max()) > 0  # the last item, reached in the second pass


def test_large_offset_exercises_the_mean_removal(backend):
    white = inputs(2, 3, 1000, offset=100.0)
    assert abs(float(white.mean()) - 100.0) < 0.2 and abs(float(white.std()) - 1.0) < 0.1
    check_bar(backend, white, random_cs(3), "mean 100")


def test_bitwise_repeatable_and_batch_invariant(backend):
    white, Cs = inputs(5, 6, 1000), random_cs(6)
    y1, y2 = native(backend, white, Cs), native(backend, white, Cs)
    assert torch.equal(y1, y2)
    for b in range(5):
        assert torch.equal(native(backend, white[b:b + 1].contiguous(), Cs)[0], y1[b]), b


def test_refusals(backend):
    dev, lib = backend.device, backend.lib
    z = lambda *shape: torch.zeros(*shape, device=dev)
    cs = lambda M, Fq=F: torch.zeros(Fq, M, M, dtype=torch.complex64, device=dev)
    with pytest.raises(NbssError, match="EUNSUPPORTED"):  # the only transform size is 256
        ops.diffuse_noise(lib, z(1, 2, 600), cs(2, 257), nfft=512)
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.diffuse_noise(lib, z(1, 17, 8), cs(17))
    ops.diffuse_noise(lib, z(1, 16, 8), cs(16))  # the last valid one
    with pytest.raises(NbssError, match="EINVAL"):
        ops.diffuse_noise(lib, z(1, 2, 0), cs(2))
    w = z(1, 2, 64)
    with pytest.raises(NbssError, match="EINVAL"):  # the output may not alias the input
        ops.diffuse_noise(lib, w, cs(2), out=w)
    with pytest.raises(NbssError, match="EUNSUPPORTED"):  # N <= 2^24, B M <= 2^22
        ops.diffuse_noise(lib, z(1, 1, (1 << 24) + 1), cs(1))
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.diffuse_noise(lib, z((1 << 18) + 1, 16, 1), cs(16))
    # the C entry point itself: no workspace, no items
    p = z(64).data_ptr()
    assert lib.nbss_diffuse_noise(256, 1, 1, 8, p, cs(1).data_ptr(), None, z(64).data_ptr(), None) == -1
    assert lib.nbss_diffuse_noise_ws_bytes(0, 1) < 0 and lib.nbss_diffuse_noise_ws_bytes(1, 0) < 0 and lib.nbss_diffuse_noise_ws_bytes(1, 1) > 0
    # arguments that do not fit: ValueError before anything is launched
    with pytest.raises(ValueError, match="Cs"):
        ops.diffuse_noise(lib, z(1, 2, 64), cs(3))
    with pytest.raises(ValueError, match="Cs"):
        ops.diffuse_noise(lib, z(1, 2, 64), cs(2, 128))
    with pytest.raises(ValueError, match="Cs"):
        ops.diffuse_noise(lib, z(1, 2, 64), torch.zeros(F, 2, 2, 2, device=dev))  # real pairs, not complex
    with pytest.raises(ValueError, match="contiguous"):
        ops.diffuse_noise(lib, z(1, 2, 128)[:, :, ::2], cs(2))
    with pytest.raises(ValueError, match="fp32"):
        ops.diffuse_noise(lib, z(1, 2, 64).double(), cs(2))
    with pytest.raises(ValueError, match="out"):
        ops.diffuse_noise(lib, z(1, 2, 64), cs(2), out=z(1, 2, 65))
    other = "cuda:0" if backend.name == "emu" else "cpu"  # a tensor on the device the library cannot read
    if other == "cpu" or torch.cuda.is_available():
        with pytest.raises(ValueError, match="CPU tensors" if backend.name == "emu" else "HIP device"):
            ops.diffuse_noise(lib, torch.zeros(1, 2, 64, device=other), torch.zeros(F, 2, 2, dtype=torch.complex64, device=other))


def test_host_tensor_on_the_product_library_is_refused():
    """no CPU fallback: loading libnbss_hip.so needs the HIP runtime but no GPU, and a host tensor is refused before any launch"""
    from nbss_amd._lib import hip
    from nbss_amd.build import build_hip
    build_hip()
    with pytest.raises(ValueError, match="HIP device"):
        ops.diffuse_noise(hip(), torch.zeros(1, 2, 64), torch.zeros(F, 2, 2, dtype=torch.complex64))
