"""STFT+norm, inorm+iSTFT (fwd/bwd), uPIT neg-SI-SDR (fwd/bwd) and clip+Adam against the oracle (torch.stft /
torch.istft / restated torchmetrics / torch.optim.Adam) on the same seeded inputs.  fp32 arithmetic everywhere:
<= 2e-5 rel-L2 (direct-DFT on the exact-f32 MFMA path vs pocketfft)."""
import functools
import itertools

import pytest
import torch

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32, NbssError
from oracle import io_ref
from test_loss_family import KINDS, check_against_comparator, ref_pit  # the fp64 comparator of the loss family (pinned to torchmetrics' published values there)
from util import rel_l2

CASES = [(1, 2, 1200, 256), (2, 6, 4000, 256), (1, 3, 2300, 512)]


def cases_for(backend):
    return CASES + ([(2, 6, 32000, 256)] if backend.name == "hip" else [])


def test_stft_norm(backend):
    for (B, C, N, n_fft) in cases_for(backend):
        g = torch.Generator().manual_seed(N)
        x = torch.randn(B, C, N, generator=g)
        tab = ops.stft_tables(backend.lib, n_fft, 0, backend.device)
        X, xrmm = ops.stft_norm_fwd(backend.lib, n_fft, NBSS_F32, tab, x.to(backend.device), ref_channel=C - 1)
        Xc = io_ref.stft(x.double(), n_fft, n_fft // 2)
        Xn, mm = io_ref.norm_frequency_online(Xc, C - 1)
        assert rel_l2(xrmm, mm[:, 0]) < 2e-5
        # un-normalised spectrum: fp32 DFT accuracy; the normalised one divides by |X_ref| which can be ~1e-3, so
        # individual bins amplify the fp32 rounding of the magnitude (the fp32 reference has the same sensitivity)
        mm_l = mm[:, 0].permute(0, 1, 2)[..., None]
        assert rel_l2(X.double().cpu() * mm_l, io_ref.to_real_layout(Xc)) < 2e-5
        assert rel_l2(X, io_ref.to_real_layout(Xn)) < 1e-3
        Xb, _ = ops.stft_norm_fwd(backend.lib, n_fft, NBSS_BF16, tab, x.to(backend.device), ref_channel=C - 1)
        assert rel_l2(Xb.float(), io_ref.to_real_layout(Xn)) < 5e-3


def test_inorm_istft_fwd_bwd(backend):
    for (B, S, N, n_fft) in cases_for(backend):
        S = min(S, 3)
        g = torch.Generator().manual_seed(N + 1)
        F, T = n_fft // 2 + 1, N // (n_fft // 2) + 1
        out = torch.randn(B, F, T, 2 * S, generator=g)
        xrmm = torch.rand(B, F, T, generator=g) + 0.5
        dy = torch.randn(B, S, N, generator=g)
        tab = ops.stft_tables(backend.lib, n_fft, 0, backend.device)
        y = ops.inorm_istft_fwd(backend.lib, n_fft, tab, out.to(backend.device), xrmm.to(backend.device), N)
        o64 = out.double().requires_grad_(True)
        want = io_ref.istft(io_ref.from_real_layout(o64) * xrmm.double()[:, None], N, n_fft, n_fft // 2)
        assert rel_l2(y, want) < 2e-5
        (want * dy.double()).sum().backward()
        dout = ops.inorm_istft_bwd(backend.lib, n_fft, tab, dy.to(backend.device), xrmm.to(backend.device))
        assert rel_l2(dout, o64.grad) < 2e-5


def test_stft_istft_roundtrip(backend):
    """the reference's own smoke check (models/io/stft.py:106-112), tightened from rtol=1e-1"""
    n_fft, N = 256, 4000
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 1, N, generator=g)
    tab = ops.stft_tables(backend.lib, n_fft, 0, backend.device)
    X, xrmm = ops.stft_norm_fwd(backend.lib, n_fft, NBSS_F32, tab, x.to(backend.device), ref_channel=0)
    y = ops.inorm_istft_fwd(backend.lib, n_fft, tab, X, xrmm, N)  # (X / |X|) * |X| -> istft
    assert rel_l2(y[:, 0], x[:, 0]) < 1e-5


@pytest.mark.parametrize("S", [1, 2, 3])
def test_pit_neg_sisdr(backend, S):
    B, N = 3, 5000
    g = torch.Generator().manual_seed(S)
    t = torch.randn(B, S, N, generator=g)
    p = 0.7 * t[:, torch.randperm(S, generator=g)] + 0.5 * torch.randn(B, S, N, generator=g)
    loss, perm, dp = ops.pit_neg_sisdr(backend.lib, p.to(backend.device), t.to(backend.device))
    p64 = p.double().requires_grad_(True)
    want, _, wperm = io_ref.pit_neg_si_sdr(p64, t.double())
    want.backward()
    assert abs(float(loss) - float(want)) < 2e-5 * max(1.0, abs(float(want)))
    assert torch.equal(perm.cpu().long(), wperm)
    assert rel_l2(dp, p64.grad) < 2e-5


def test_sisdr_known_answers():
    """closed-form pins of the restated torchmetrics definitions (oracle self-check, fp64)"""
    g = torch.Generator().manual_seed(0)
    t = torch.randn(2, 1, 1000, generator=g, dtype=torch.float64)
    assert float(io_ref.si_sdr(3.0 * t, t).min()) > 100.0          # scale invariance, p = a t -> "infinite" (eps-limited)
    n = torch.randn(2, 1, 1000, generator=g, dtype=torch.float64)
    n = n - (n * t).sum(-1, keepdim=True) / (t * t).sum(-1, keepdim=True) * t   # orthogonal noise
    snr = 10 * torch.log10((t * t).sum(-1) / (n * n).sum(-1))
    assert torch.allclose(io_ref.si_sdr(t + n, t), snr, atol=1e-9)  # orthogonal noise -> plain SNR
    assert torch.allclose(io_ref.si_sdr(-t + n, t), io_ref.si_sdr(t + n, t), atol=1e-9)  # the projection makes it sign invariant
    # uPIT picks the permutation with the smaller mean neg-SI-SDR: swapped estimates are un-swapped
    tt = torch.randn(3, 2, 800, generator=g, dtype=torch.float64)
    est = tt.flip(1) + 0.01 * torch.randn(3, 2, 800, generator=g, dtype=torch.float64)
    loss, per_item, perm = io_ref.pit_neg_si_sdr(est, tt)
    assert perm.tolist() == [[1, 0]] * 3 and float(loss) < -35.0 and per_item.shape == (3,)


def test_clip_adam(backend):
    n = 10007
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=g)
    ref_p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref_p], lr=1e-3)
    p = p0.clone().to(backend.device)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    scratch = torch.zeros(300, device=backend.device)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g) * (3.0 if step == 2 else 0.01)  # step 2 is clipped, the others are not
        ref_p.grad = grad.clone()
        norm = torch.nn.utils.clip_grad_norm_([ref_p], 5.0)
        opt.step()
        gdev = grad.clone().to(backend.device)
        ops.clip_adam_step(backend.lib, p, gdev, m, v, scratch, step, lr=1e-3, max_norm=5.0)
        assert abs(float(scratch[0]) - float(norm)) < 1e-4 * float(norm)
        assert float(gdev.abs().max()) == 0.0  # gradient buffer re-zeroed
        assert rel_l2(p, ref_p.detach()) < 1e-6


@pytest.mark.parametrize("decoupled", [False, True])
def test_clip_adam_weight_decay(backend, decoupled):
    """weight decay: torch.optim.Adam adds wd * p to the gradient, torch.optim.AdamW shrinks p by lr * wd (configs of the online
    models use AdamW): the kernel's flag bit 1 selects the decoupled form"""
    n = 4099
    g = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=g)
    ref_p = p0.clone().requires_grad_(True)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([ref_p], lr=1e-2, weight_decay=0.05)
    p = p0.clone().to(backend.device)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    scratch = torch.zeros(300, device=backend.device)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g) * 0.01
        ref_p.grad = grad.clone()
        opt.step()
        ops.clip_adam_step(backend.lib, p, grad.clone().to(backend.device), m, v, scratch, step, lr=1e-2, weight_decay=0.05, max_norm=0.0,
                           decoupled_weight_decay=decoupled)
        assert rel_l2(p, ref_p.detach()) < 1e-6


# ---- the losses at their edges: more items than one wave of finalize threads (one thread per item: 64 lanes), the batch limit of 1024, fewer samples
# than the 64 chunks of the dots kernels (N = 37, 41: most chunks are empty), a gradient beyond one pass of sisdr_grad_kernel's grid, unaligned rows ----
EDGE_SHAPES = [(130, 4, 37), (65, 3, 41), (1024, 1, 512)]
LOSSES = ["shipped_si_sdr"] + list(KINDS)  # ops.pit_neg_sisdr, then the four kinds of ops.pit_loss and the scale-invariant SA-SDR


@functools.lru_cache(maxsize=None)
def edge_inputs(B, S, N):
    """the recipe of test_loss_family.parity_inputs, p = 0.8 t[pi_b] + 0.3 noise with a permutation per item, at batch B: 2 B items are drawn and the
    first B whose best and second-best pairing are more than 1 dB (MSE: 10 %) apart in fp64 under EVERY loss are kept (at N = 37 a few are not)
    -> (p, t, items of the pool that miss the margin, pool size); computed once per shape, never modified"""
    pool = 2 * B if S > 1 else B
    g = torch.Generator().manual_seed(B * 100 + S * 10 + N % 7)
    t = torch.randn(pool, S, N, generator=g)
    allp = torch.tensor(list(itertools.permutations(range(S))))
    pis = allp[(torch.arange(pool) + 1) % len(allp)]
    p = 0.8 * t[torch.arange(pool)[:, None], pis] + 0.3 * torch.randn(pool, S, N, generator=g)
    keep = torch.ones(pool, dtype=torch.bool)
    if S > 1:
        for name in KINDS:
            srt = ref_pit(name, p.double(), t.double(), True)[2].sort(1).values
            keep &= (srt[:, 1] - srt[:, 0]) > (0.1 * srt[:, 0].abs() if name == "mse" else 1.0)
    idx = keep.nonzero()[:B, 0]
    return p[idx].contiguous(), t[idx].contiguous(), int((~keep).sum()), pool


def test_edge_pools_suffice():
    """no item is dropped silently: the pool holds B items with the margin at every shape, and the count of those without is printed"""
    for (B, S, N) in EDGE_SHAPES:
        p, t, missed, pool = edge_inputs(B, S, N)
        print(f"(B, S, N) = {(B, S, N)}: {missed} of {pool} drawn items miss the margin")
        assert p.shape == (B, S, N) and t.shape == (B, S, N)


def check_shipped_si_sdr(backend, p, t):
    """ops.pit_neg_sisdr against the fp64 comparator at the bars of test_pit_neg_sisdr, per-item losses included"""
    B, S, N = p.shape
    p64 = p.double().requires_grad_(True)
    witems, wperm, vals = ref_pit("si_sdr", p64, t.double(), True)
    if S > 1:
        srt = vals.detach().sort(1).values
        assert ((srt[:, 1] - srt[:, 0]) > 1.0).all()
    witems.mean().backward()
    witems = witems.detach()
    want = float(witems.mean())
    loss, perm, dp, items = ops.pit_neg_sisdr(backend.lib, p.to(backend.device), t.to(backend.device), return_items=True)
    e_items = float(((items.cpu().double() - witems).abs() / witems.abs().clamp(min=1.0)).max())
    print(f"pit_neg_sisdr [{backend.name}] {(B, S, N)}: loss {float(loss):.7f} want {want:.7f} items_err/bar {e_items:.3e} grad_rel_l2 {rel_l2(dp, p64.grad):.3e}")
    assert abs(float(loss) - want) < 2e-5 * max(1.0, abs(want))
    assert torch.equal(perm.cpu().long(), wperm)
    assert e_items < 2e-5
    assert rel_l2(dp, p64.grad) < 2e-5


def check_loss(backend, loss, p, t):
    if loss == "shipped_si_sdr":
        check_shipped_si_sdr(backend, p, t)
    else:
        check_against_comparator(backend, loss, p, t, True)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pit_losses_at_the_batch_edges(backend, shape, loss):
    p, t, _, _ = edge_inputs(*shape)
    check_loss(backend, loss, p, t)


def test_pit_losses_refuse_more_than_1024_items(backend):
    z = torch.zeros(1025, 1, 64, device=backend.device)
    with pytest.raises(NbssError, match="UNSUPPORTED"):
        ops.pit_neg_sisdr(backend.lib, z, z)
    for name, (kind, si) in KINDS.items():
        with pytest.raises(NbssError, match="UNSUPPORTED"):
            ops.pit_loss(backend.lib, kind, z, z, pit=True, scale_invariant=si)


@pytest.mark.parametrize("loss", LOSSES)
def test_pit_loss_gradient_beyond_one_grid_pass(backend, loss):
    """B S N = 1 280 000 > 4096 * 256: sisdr_grad_kernel (shared by every loss) takes a second grid-stride pass"""
    B, S, N = 8, 4, 40000
    assert B * S * N > 4096 * 256
    p, t, missed, _ = edge_inputs(B, S, N)
    assert missed == 0
    check_loss(backend, loss, p, t)


@pytest.mark.parametrize("name", list(KINDS))
def test_pit_loss_unaligned_rows(backend, name):
    """preds / target as views that start 4 and 8 bytes off a 16-byte boundary (N = 4096 would allow 16-byte loads): nbss_pit_loss must fall back to
    V = 1 and V = 2 floats per load; the results meet the bars against fp64 and against the aligned call"""
    kind, si = KINDS[name]
    B, S, N = 4, 2, 4096
    p, t, missed, _ = edge_inputs(B, S, N)
    assert missed == 0
    p64 = p.double().requires_grad_(True)
    witems, wperm, _ = ref_pit(name, p64, t.double(), True)
    witems.mean().backward()
    witems = witems.detach()
    want = float(witems.mean())
    got = {}
    for off in (0, 1, 2):  # floats
        bufs = [torch.zeros(B * S * N + 4, device=backend.device) for _ in range(2)]
        views = []
        for buf, src in zip(bufs, (p, t)):
            assert buf.data_ptr() % 16 == 0
            v = buf[off:off + B * S * N].view(B, S, N)
            v.copy_(src)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
            views.append(v)
        loss, perm, dp, items = ops.pit_loss(backend.lib, kind, views[0], views[1], pit=True, scale_invariant=si, return_items=True)
        got[off] = (loss, perm, dp, items)
        e_items = float(((items.cpu().double() - witems).abs() / witems.abs().clamp(min=1.0)).max())
        print(f"{name} [{backend.name}] offset {4 * off} bytes: loss {float(loss):.7f} want {want:.7f} items_err/bar {e_items:.3e} "
              f"grad_rel_l2 {rel_l2(dp, p64.grad):.3e}")
        assert abs(float(loss) - want) < 2e-5 * max(1.0, abs(want))
        assert torch.equal(perm.cpu().long(), wperm)
        assert e_items < 2e-5
        assert rel_l2(dp, p64.grad) < 2e-5
    for off in (1, 2):
        assert abs(float(got[off][0]) - float(got[0][0])) < 2e-5 * max(1.0, abs(float(got[0][0])))
        assert torch.equal(got[off][1], got[0][1]) and rel_l2(got[off][2], got[0][2]) < 2e-5


# ---- clip + Adam beyond one pass of either grid (sumsq_kernel: 256 * 256 threads, adam_kernel: 1024 * 256), at one element and at one block + 1, with
# the gradient scale of a data-parallel world of 4 and with the gradient buffer kept ----
def adam_grads(n, g):
    """three gradients whose scaled norm 0.25 |grad| is 1, 12 and 0.5: with max_norm 5 the second step is clipped and the others are not"""
    out = []
    for norm in (1.0, 12.0, 0.5):
        z = torch.randn(n, generator=g)
        out.append(z / z.norm() * (norm / 0.25))
    return out


def hyper_of(lib, step, lr, betas, device):
    hh = torch.empty(3, dtype=torch.float32)  # host memory
    lib.call("nbss_adam_hyper", int(step), float(lr), float(betas[0]), float(betas[1]), hh.data_ptr())
    return hh.to(device)


@pytest.mark.parametrize("zero_grad", [False, True], ids=["keep_grad", "zero_grad"])
@pytest.mark.parametrize("n", [1, 257, 300001])
def test_clip_adam_edges(backend, n, zero_grad):
    lr, betas, scale = 1e-3, (0.9, 0.999), 0.25
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    ref_p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref_p], lr=lr, betas=betas)
    dev = backend.device
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pd, md, vd = p.clone(), m.clone(), v.clone()  # the same steps through clip_adam_step_dev + adam_hyper
    scratch, scratch_d = torch.zeros(300, device=dev), torch.zeros(300, device=dev)
    for step, grad in enumerate(adam_grads(n, g), start=1):
        ref_p.grad = scale * grad
        norm = float(torch.nn.utils.clip_grad_norm_([ref_p], 5.0))
        assert (norm > 5.0) == (step == 2)
        opt.step()
        gdev = grad.clone().to(dev)
        ops.clip_adam_step(backend.lib, p, gdev, m, v, scratch, step, lr=lr, betas=betas, max_norm=5.0, grad_scale=scale, zero_grad=zero_grad)
        e_norm, e_p = abs(float(scratch[0]) - norm) / norm, rel_l2(p, ref_p.detach())
        print(f"clip_adam [{backend.name}] n {n} step {step}: norm {float(scratch[0]):.6f} want {norm:.6f} (rel {e_norm:.2e}), params rel_l2 {e_p:.2e}")
        assert e_norm < 1e-4
        if zero_grad:
            assert float(gdev.abs().max()) == 0.0 and float(gdev[n - 1]) == 0.0  # all of it, the last element included
        else:
            assert torch.equal(gdev.cpu(), grad)  # untouched
        assert e_p < 1e-6
        # the device-scalar variant: bitwise the eager call (include/nbss_hip.h)
        gdev_d = grad.clone().to(dev)
        ops.clip_adam_step_dev(backend.lib, pd, gdev_d, md, vd, scratch_d, hyper_of(backend.lib, step, lr, betas, dev), betas=betas, max_norm=5.0,
                               grad_scale=scale, zero_grad=zero_grad)
        assert torch.equal(pd, p) and torch.equal(md, m) and torch.equal(vd, v) and torch.equal(gdev_d, gdev)
        assert torch.equal(scratch_d[:2], scratch[:2])
