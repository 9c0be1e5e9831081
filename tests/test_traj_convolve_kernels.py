"""The trajectory convolution kernel (nbss_amd/csrc/conv_traj.hip: nbss_fir_convolve_traj) against an fp64 restatement of the definition in
include/nbss_hip.h, on the emulator and, under -m gpu, on the device.

Comparator: `ref_traj`, the closed form in fp64 numpy (weights from `ref_weights`, one numpy.convolve per trajectory point that carries weight).
`test_comparator_against_the_reference` pins it to the reference's own convolve_traj_with_win(..., 'trapezium20') and convolve_traj (utils/mix.py) through
tests/golden/traj_convolve.npz (tests/golden/make_golden_traj.py), absolute error <= 1e-5 (the reference accumulates in float32: 1.8e-6 was measured at
output magnitudes up to 34 on randn inputs; the margin covers another BLAS / FFT build), and against the live functions where the reference tree exists.

Bar for the kernel, rel-L2 against the comparator: the larger of
  * twice the error of the fp32 torch path (data_loaders.gpu_simulation: traj_weights + fft_convolve per trajectory point) on the same inputs, and
  * eps_fp32 sqrt(2 L), the random-walk bound of a sum of 2 L fp32 terms (every tap meets at most two trajectory points).
Every case prints both errors and the bar.

Sizes at which the kernel takes another path: 16 (a tap block), 256 (the output tile of a workgroup), 2048 (taps of a chunk), hops around the tile
(255, 256, 257), hops just above the ramp (21, 22 at ramp 20; 6 at ramps 2 and 5), N in {H, H + 1, 2 H - 1, 3 H + 7} (one point, the first cross-fade, the
last point cut short), N % 4 or L % 4 != 0 (element-wise staging), M in {1, 2, 6} (1, 2 or 3 microphones per workgroup), more than 2048 (b, s) pairs."""
import functools
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from data_loaders.gpu_simulation import fft_convolve, traj_rirs_needed, traj_weights
from nbss_amd import ops
from nbss_amd._lib import NbssError

EPS = float(np.finfo(np.float32).eps)
ITEMS_PER_PASS = 2048  # CONV_MAX_ITEMS in conv_common.h
TILE, CHUNK = 256, 2048  # TRAJ_NT, TRAJ_KT in conv_traj.hip
GOLDEN = Path(__file__).parent / "golden" / "traj_convolve.npz"
REF = Path("/root/reference")
MODES = ("trapezium", "switch")


def ref_weights(N, H, mode, ramp, P):
    """w [P, N] in fp64: the definition of include/nbss_hip.h written out sample by sample"""
    w = np.zeros((P, N))
    z = (H - ramp) // 2
    o = H - ramp - z
    for j in range(N):
        q, r = divmod(j, H)
        if mode == "switch":
            w[q, j] = 1.0
            continue
        up = 0.0 if r < z else (r - z) / (ramp - 1) if r < z + ramp else 1.0
        down = 1.0 if r < o else (ramp - 1 - (r - o)) / (ramp - 1) if r < o + ramp else 0.0
        w[q, j] = down
        if up != 0.0:
            w[q + 1, j] = up  # an IndexError here means P is too small
    return w


def ref_full(x, h, H, mode, ramp):
    """x [N], h [P, M, L] -> the full time-varying convolution [M, N + L - 1] in fp64; RIRs without weight are not read"""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    (N,), (P, M, L) = x.shape, h.shape
    w = ref_weights(N, H, mode, ramp, P)
    full = np.zeros((M, N + L - 1))
    for p in range(P):
        if w[p].any():
            for m in range(M):
                full[m] += np.convolve(x * w[p], h[p, m])
    return full


def ref_traj(x, h, hop, delay, mode, ramp=20):
    """x [B,S,N], h [B,S,P,M,L], hop, delay [B,S] -> y [B,S,M,N] in fp64: N samples of the full convolution from the delay onward"""
    x, h = np.asarray(x), np.asarray(h)
    (B, S, N), (M, L) = x.shape, h.shape[3:]
    y = np.zeros((B, S, M, N))
    for b in range(B):
        for s in range(S):
            full = np.concatenate([ref_full(x[b, s], h[b, s], int(hop[b, s]), mode, ramp), np.zeros((M, L))], -1)
            y[b, s] = full[:, delay[b, s]: delay[b, s] + N]
    return y


def rel_l2(y, ref):
    return float(np.linalg.norm(np.asarray(y, dtype=np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


@functools.lru_cache(maxsize=None)
def inputs(B, S, P, M, N, L, seed=0):
    g = torch.Generator().manual_seed(1000 * N + L + 7 * M + 31 * P + seed)
    return torch.randn(B, S, N, generator=g), torch.randn(B, S, P, M, L, generator=g)


def i32(v):
    return torch.tensor(v, dtype=torch.int32)


def fft_window(x, h, hop, delay, mode, ramp, device):
    """the fp32 torch path on the backend's device: the weighted source through fft_convolve, once per trajectory point, cut at the given delay"""
    x, h = x.to(device), h.to(device)
    w = traj_weights(x.shape[-1], hop.to(device), mode, ramp, P=h.shape[2], device=device)
    full = sum(fft_convolve((x * w[:, :, p])[:, :, None, :], h[:, :, p]) for p in range(h.shape[2]))
    full = torch.nn.functional.pad(full, (0, h.shape[-1]))
    idx = delay.to(device).long()[:, :, None, None] + torch.arange(x.shape[-1], device=device)
    return full.gather(-1, idx.expand(*h.shape[:2], h.shape[3], x.shape[-1])).cpu()


def native(backend, x, h, hop, delay, mode="trapezium", ramp=20, **kw):
    dev = backend.device
    return ops.fir_convolve_traj(backend.lib, x.to(dev), h.to(dev), hop.to(dev), delay.to(dev), mode=mode, ramp=ramp, **kw).cpu()


def check_bar(backend, x, h, hop, delay, mode, ramp, what):
    ref = ref_traj(x.numpy(), h.numpy(), hop.numpy(), delay.numpy(), mode, ramp)
    e_nat = rel_l2(native(backend, x, h, hop, delay, mode, ramp).numpy(), ref)
    e_fft = rel_l2(fft_window(x, h, hop, delay, mode, ramp, backend.device).numpy(), ref)
    bar = max(2.0 * e_fft, EPS * (2 * h.shape[-1]) ** 0.5)
    print(f"{backend.name} {mode} {what}: native {e_nat:.3e} fft {e_fft:.3e} bar {bar:.3e}")
    assert e_nat <= bar, (mode, what, e_nat, e_fft, bar)


def delays_of(L):
    return sorted({0, L - 1, L // 2})


def one_item(backend, M, N, L, H, ramp, mode, delays=None, spare=0):
    P = traj_rirs_needed(N, H, mode) + spare
    x, h = inputs(1, 1, P, M, N, L)
    for d in delays_of(L) if delays is None else delays:
        check_bar(backend, x, h, i32([[H]]), i32([[d]]), mode, ramp, f"M {M} N {N} L {L} H {H} ramp {ramp} delay {d}")


# ---------------------------------------------------------------- the comparator
def test_comparator_against_the_reference():
    g = np.load(GOLDEN)
    live = None
    if REF.exists():
        spec = importlib.util.spec_from_file_location("reference_mix", REF / "data_loaders" / "utils" / "mix.py")
        live = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(live)
    assert g["cases"].tolist() == [[1000, 100, 37], [1003, 100, 64], [950, 100, 5], [260, 21, 33], [999, 333, 70], [1000, 1000, 16], [64, 23, 300]]
    for i, (N, H, L) in enumerate(g["cases"].tolist()):
        x, h = g[f"x16_{i}"] / 16.0, g[f"h16_{i}"] / 16.0
        assert x.shape == (N,) and h.shape == (traj_rirs_needed(N, H, "trapezium"), 2, L)
        P0 = traj_rirs_needed(N, H, "switch")
        got = {"win": ref_full(x, h, H, "trapezium", 20), "switch": ref_full(x, h[:P0], H, "switch", 20)}
        for key, mine in got.items():
            err = float(np.abs(mine - g[f"{key}_{i}"]).max())
            print(f"case {i} (N {N} hop {H} L {L}) {key}: max |comparator - fixture| {err:.2e} at max |y| {np.abs(mine).max():.1f}")
            assert g[f"{key}_{i}"].shape == mine.shape and err <= 1e-5
        if live is not None:
            assert np.abs(got["win"] - live.convolve_traj_with_win(x, h, H, wintype="trapezium20")).max() <= 1e-5
            assert np.abs(got["switch"] - live.convolve_traj(x, h[:P0], h[:P0], H, align=False)[0]).max() <= 1e-5


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H", [21, 22, 100, 255, 256, 257])
def test_hops_and_lengths(backend, H, mode):
    """hops just above the ramp and around the output tile; N = one point, the first sample of the second, just short of two, three and a cut one"""
    for N in (H, H + 1, 2 * H - 1, 3 * H + 7):
        one_item(backend, 2, N, 17, H, 20, mode)


@pytest.mark.parametrize("ramp", [2, 5])
def test_short_ramps(backend, ramp):
    for N in (6, 7, 11, 25):
        one_item(backend, 2, N, 17, 6, ramp, "trapezium")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [1, 16, 17, 100])
def test_response_lengths(backend, L, mode):
    """N = 300: 16-byte staging with L in {16, 100}, element-wise with the others"""
    one_item(backend, 2, 300, L, 100, 20, mode)
    one_item(backend, 2, 307, L, 100, 20, mode, delays=[L // 2])


@pytest.mark.parametrize("mode", MODES)
def test_more_taps_than_one_chunk(backend, mode):
    """a point whose taps do not fit one chunk of 2048: its support of H + ramp = 2120 samples is heard from a tile of 256 outputs through 2375 taps"""
    H, L = 2100, CHUNK + 352
    assert TILE + H + 20 - 1 > CHUNK and L > CHUNK
    one_item(backend, 1, 2200, L, H, 20, mode, delays=[L // 2])
    one_item(backend, 2, 2201, L + 1, H, 20, mode, delays=[L])  # delay L = (L + 1) - 1, unaligned rows


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("taps", [CHUNK, CHUNK + 1])
def test_the_chunk_edge(backend, taps, mode):
    """a point heard through exactly 2048 taps (one full chunk) and through 2049 (a second chunk of one tap block).  The first tile of an item with
    delay d hears the first point's support [0, s) through the taps 0 .. min(255, N - 1) + d, which the first chunk starts at 0: d = taps - 256
    (s = H + (ramp - 1 when cross-faded) > taps, so the support does not cut the range short)"""
    H, L = 2100, CHUNK + 40
    assert H > taps
    one_item(backend, 2, 2 * TILE + 3, L, H, 20, mode, delays=[taps - TILE])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", [1, 2, 6])
def test_microphones(backend, M, mode):
    one_item(backend, M, 73, 16, 22, 20, mode)


@pytest.mark.parametrize("mode", MODES)
def test_a_hop_per_item(backend, mode):
    """different H per (b, s) inside one call, P set by the smallest; the others never read their surplus"""
    hop = i32([[21, 50], [100, 37]])
    N, L, M = 207, 33, 3
    x, h = inputs(2, 2, traj_rirs_needed(N, 21, mode), M, N, L)
    check_bar(backend, x, h, hop, i32([[0, 32], [16, 5]]), mode, 20, "hops 21 50 100 37")


@pytest.mark.parametrize("mode", MODES)
def test_surplus_rirs_are_never_read(backend, mode):
    """more RIRs than required, the surplus filled with NaN: the output is finite and bitwise that of the exact-P call.  At N = 3 H + 1 the last sample
    has r = 0: in mode 1 it points at index q + 1 = P with up(0) = 0, and that index, here a NaN response, must not be read"""
    L, M, H = 17, 2, 100
    for N in (3 * H + 7, 3 * H + 1, 3 * H):
        P = traj_rirs_needed(N, H, mode)
        x, h = inputs(1, 2, P, M, N, L)
        hop, delay = i32([[H, H + 1]]), i32([[3, 16]])
        want = native(backend, x, h, hop, delay, mode)
        more = torch.cat([h, torch.full((1, 2, 2, M, L), float("nan"))], 2).contiguous()
        got = native(backend, x, more, hop, delay, mode)
        assert torch.isfinite(got).all() and torch.equal(got, want), N


@pytest.mark.parametrize("mode", MODES)
def test_more_items_than_one_grid_pass(backend, mode):
    """B S above the 2048 (b, s) pairs of one grid pass, at N = 32, L = 4: every item is computed, each with its own hop and delay"""
    B, S, M, N, L = 683, 3, 1, 32, 4
    assert B * S > ITEMS_PER_PASS
    hop = (21 + torch.arange(B * S, dtype=torch.int32) % 12).reshape(B, S)
    delay = (torch.arange(B * S, dtype=torch.int32) % L).reshape(B, S)
    x, h = inputs(B, S, traj_rirs_needed(N, 21, mode), M, N, L)
    y = native(backend, x, h, hop, delay, mode).numpy()
    want = ref_traj(x.numpy(), h.numpy(), hop.numpy(), delay.numpy(), mode)
    bar = EPS * (2 * L) ** 0.5
    assert rel_l2(y, want) <= bar
    assert rel_l2(y[-1], want[-1]) <= bar and float(np.abs(y[-1]).max()) > 0  # the last item, reached in the second pass


@pytest.mark.parametrize("mode", MODES)
def test_bitwise_repeatable_and_batch_invariant(backend, mode):
    N, L, M = 557, 100, 6
    hop = i32([[100], [21], [257]])
    delay = i32([[50], [0], [99]])
    x, h = inputs(3, 1, traj_rirs_needed(N, 21, mode), M, N, L)
    y1, y2 = native(backend, x, h, hop, delay, mode), native(backend, x, h, hop, delay, mode)
    assert torch.equal(y1, y2)
    alone = native(backend, x[:1].contiguous(), h[:1].contiguous(), hop[:1].contiguous(), delay[:1].contiguous(), mode)
    assert torch.equal(alone[0], y1[0])


def test_unaligned_base_pointer(backend):
    """aligned sizes on rows that do not start on a 16-byte boundary take the element-wise staging: the same bits"""
    N, L, H = 64, 32, 24
    x, h = inputs(1, 2, traj_rirs_needed(N, H), 2, N, L)
    hop, delay = i32([[H, H + 3]]), i32([[3, 17]])
    want = native(backend, x, h, hop, delay)
    dev = backend.device
    xb, hb = torch.zeros(x.numel() + 1, device=dev), torch.zeros(h.numel() + 1, device=dev)
    xo, ho = xb[1:].view(x.shape), hb[1:].view(h.shape)
    xo.copy_(x), ho.copy_(h)
    assert xo.data_ptr() % 16 != 0 and ho.data_ptr() % 16 != 0 and xo.is_contiguous()
    assert torch.equal(ops.fir_convolve_traj(backend.lib, xo, ho, hop.to(dev), delay.to(dev)).cpu(), want)


def test_constant_trajectory_is_the_static_convolution(backend):
    """all P responses equal and H - ramp even (z = o: the two weights sum to 1 everywhere): nbss_fir_convolve within fp32 round-off"""
    N, L, M, H = 300, 33, 3, 100
    x, h = inputs(1, 1, 1, M, N, L)
    dev = backend.device
    hp = h.expand(1, 1, traj_rirs_needed(N, H), M, L).contiguous()
    for mode in MODES:
        got = native(backend, x, hp, i32([[H]]), i32([[7]]), mode)
        want = ops.fir_convolve(backend.lib, x.to(dev), h[:, :, 0].contiguous().to(dev), i32([[7]]).to(dev)).cpu()
        assert rel_l2(got.numpy(), want.double().numpy()) <= EPS * (2 * L) ** 0.5


# ---------------------------------------------------------------- validation on the device, refusals on the host
STATUS_CASES = {  # name -> (mode, hop of the middle item, responses short of what that hop needs, delay of the middle item)
    "hop 0": ("switch", 0, 0, 5),
    "hop 0, cross-faded": ("trapezium", 0, 0, 5),
    "hop <= ramp": ("trapezium", 20, 0, 5),
    "P one too small": ("trapezium", 30, 1, 5),
    "P one too small, switched": ("switch", 30, 1, 5),
    "delay = L": ("trapezium", 50, 0, 16),
    "delay < 0": ("switch", 50, 0, -3),
}


@pytest.mark.parametrize("case", list(STATUS_CASES))
def test_status(backend, case):
    """the middle item of three is invalid: it gets zeros (or the clamped delay), its neighbours are bitwise what they are in a valid batch, and
    ops raises with check=True"""
    mode, hbad, short, dbad = STATUS_CASES[case]
    N, L, M = 100, 16, 2
    hop_ok, delay_ok = i32([[50], [50], [64]]), i32([[0], [5], [15]])
    P = traj_rirs_needed(N, 30 if short else 50, mode) - short  # short: enough for the hops 50 and 64, one too few for 30
    assert P >= traj_rirs_needed(N, 50, mode)
    x, h = inputs(3, 1, P, M, N, L)
    good = native(backend, x, h, hop_ok, delay_ok, mode)
    hop, delay = hop_ok.clone(), delay_ok.clone()
    hop[1, 0], delay[1, 0] = hbad, dbad
    with pytest.raises(NbssError, match="EINVAL"):
        native(backend, x, h, hop, delay, mode)
    dev = backend.device
    y = torch.full((3, 1, M, N), 7.0, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    xd, hd, hopd, delayd = x.to(dev), h.to(dev), hop.to(dev), delay.to(dev)
    rc = backend.lib.nbss_fir_convolve_traj(3, 1, P, M, N, L, ops.TRAJ_MODES[mode], 20, xd.data_ptr(), hd.data_ptr(), hopd.data_ptr(), delayd.data_ptr(),
                                            y.data_ptr(), status.data_ptr(), None)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert rc == 0 and int(status.item()) == 1
    y = y.cpu()
    assert torch.equal(y[0], good[0]) and torch.equal(y[2], good[2])
    if 0 <= dbad < L:
        assert torch.equal(y[1], torch.zeros(1, M, N))
    else:  # clamped into [0, L)
        delay[1, 0] = min(max(dbad, 0), L - 1)
        assert torch.equal(y[1], native(backend, x, h, hop, delay, mode)[1]) and float(y[1].abs().max()) > 0


def test_ramp_below_two_is_an_invalid_item(backend):
    x, h = inputs(1, 1, 4, 2, 64, 16)
    with pytest.raises(NbssError, match="EINVAL"):
        native(backend, x, h, i32([[32]]), i32([[0]]), "trapezium", ramp=1)
    assert torch.equal(native(backend, x, h, i32([[32]]), i32([[0]]), "trapezium", ramp=1, check=False), torch.zeros(1, 1, 2, 64))
    native(backend, x, h, i32([[32]]), i32([[0]]), "switch", ramp=1)  # the switch has no ramp


def test_refusals(backend):
    dev, lib = backend.device, backend.lib
    z = lambda *shape: torch.zeros(*shape, device=dev)
    d = lambda v, B=1, S=1: torch.full((B, S), v, dtype=torch.int32, device=dev)
    with pytest.raises(NbssError, match="EINVAL"):  # N < 1
        ops.fir_convolve_traj(lib, z(1, 1, 0), z(1, 1, 1, 2, 8), d(30), d(0))
    with pytest.raises(NbssError, match="EINVAL"):  # L < 1
        ops.fir_convolve_traj(lib, z(1, 1, 8), z(1, 1, 1, 2, 0), d(30), d(0))
    with pytest.raises(NbssError, match="EINVAL"):  # P < 1
        ops.fir_convolve_traj(lib, z(1, 1, 8), z(1, 1, 0, 2, 8), d(30), d(0))
    with pytest.raises(NbssError, match="mode"):
        ops.fir_convolve_traj(lib, z(1, 1, 8), z(1, 1, 1, 2, 8), d(30), d(0), mode="hann")
    keep = (z(8), z(32), d(30), d(0), z(16))  # x [1,1,8], h [1,1,2,2,8], hop, delay, y [1,1,2,8]: alive for the calls below
    args = (*(t.data_ptr() for t in keep), None, None)
    assert lib.nbss_fir_convolve_traj(1, 1, 2, 2, 8, 8, 0, 20, *args) == 0
    for mode in (-1, 2):
        assert lib.nbss_fir_convolve_traj(1, 1, 2, 2, 8, 8, mode, 20, *args) == -1
    assert lib.nbss_fir_convolve_traj(1, 1, 2, 2, 0, 8, 0, 20, *args) == -1
    assert lib.nbss_fir_convolve_traj(1, 1, 2, 2, 8, 0, 0, 20, *args) == -1
    assert lib.nbss_fir_convolve_traj(1, 1, 0, 2, 8, 8, 0, 20, *args) == -1
    assert lib.nbss_fir_convolve_traj(1, 1, 2, 2, 8, 8, 0, 20, None, *args[1:]) == -1  # a null pointer
    # the caps of the header: L <= 65536, M <= 4096, B S P M <= 2^22, N <= 2^24
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.fir_convolve_traj(lib, z(1, 1, 8), z(1, 1, 1, 1, 65537), d(30), d(0))
    ops.fir_convolve_traj(lib, z(1, 1, 8), z(1, 1, 2, 1, 65536), d(30), d(65535))
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.fir_convolve_traj(lib, z(1, 1, 1), z(1, 1, 1, 4097, 1), d(30), d(0))
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.fir_convolve_traj(lib, z(1025, 1, 1), z(1025, 1, 4096, 1, 1), d(30, 1025), d(0, 1025))
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        ops.fir_convolve_traj(lib, z(1, 1, (1 << 24) + 1), z(1, 1, 1, 1, 1), d(1 << 25), d(0))
    with pytest.raises(NbssError):  # shapes that do not belong together
        ops.fir_convolve_traj(lib, z(1, 2, 8), z(1, 1, 1, 2, 8), d(30), d(0))
    with pytest.raises(NbssError):
        ops.fir_convolve_traj(lib, z(1, 1, 8), z(1, 1, 2, 8), d(30), d(0))
