"""The loss family beside neg-SI-SDR — neg_snr, neg_sa_sdr (scale-invariant or not), cc_mse, each with PIT or identity pairing — through
ops.pit_loss (nbss_pit_loss) and through the drop-in surface models/io/loss.py, against an fp64 restatement of torchmetrics' definitions that
is written here (never imported from the code under test) and is itself pinned to the values torchmetrics publishes in its docstrings."""
import itertools

import pytest
import torch

from nbss_amd import ops
from nbss_amd._lib import NBSS_LOSS_MSE, NBSS_LOSS_SA_SDR, NBSS_LOSS_SI_SDR, NBSS_LOSS_SNR
from util import rel_l2

EPS = float(torch.finfo(torch.float32).eps)

# (id, kind of ops.pit_loss, scale_invariant)
KINDS = {"si_sdr": (NBSS_LOSS_SI_SDR, False), "snr": (NBSS_LOSS_SNR, False), "sa_sdr": (NBSS_LOSS_SA_SDR, False),
         "sa_sdr_si": (NBSS_LOSS_SA_SDR, True), "mse": (NBSS_LOSS_MSE, False)}


# ---- the comparator: torchmetrics' closed forms (zero_mean=False, eps = float32 epsilon, sums over the last axis), in the dtype handed in ----
def ref_si_sdr(p, t):
    alpha = ((p * t).sum(-1, keepdim=True) + EPS) / ((t * t).sum(-1, keepdim=True) + EPS)
    ts = alpha * t
    return 10 * torch.log10(((ts * ts).sum(-1) + EPS) / (((ts - p) ** 2).sum(-1) + EPS))


def ref_snr(p, t):
    return 10 * torch.log10(((t * t).sum(-1) + EPS) / (((t - p) ** 2).sum(-1) + EPS))


def ref_sa_sdr(p, t, scale_invariant):
    """[..., S, N] -> [...]"""
    if scale_invariant:
        alpha = ((p * t).sum((-1, -2), keepdim=True) + EPS) / ((t * t).sum((-1, -2), keepdim=True) + EPS)
        t = alpha * t
    return 10 * torch.log10(((t * t).sum((-1, -2)) + EPS) / (((t - p) ** 2).sum((-1, -2)) + EPS))


def ref_items(name, p, t):
    """the reference's loss functions (neg_si_sdr, neg_snr, neg_sa_sdr, _mse): [B,S,N] -> [B]"""
    if name == "si_sdr":
        return -ref_si_sdr(p, t).mean(1)
    if name == "snr":
        return -ref_snr(p, t).mean(1)
    if name in ("sa_sdr", "sa_sdr_si"):
        return -ref_sa_sdr(p, t, name == "sa_sdr_si")
    return ((p - t) ** 2).reshape(p.shape[0], -1).mean(1)


def ref_pit(name, p, t, pit):
    """permutation-wise / min: every permutation in itertools order on (p[:, perm], t), first minimum wins -> (items [B], perm [B,S], all [B,S!])"""
    S = p.shape[1]
    perms = list(itertools.permutations(range(S))) if pit else [tuple(range(S))]
    vals = torch.stack([ref_items(name, p[:, list(pm)], t) for pm in perms], 1)
    best, idx = vals[:, 0], torch.zeros(p.shape[0], dtype=torch.long)
    for k in range(1, len(perms)):
        better = vals[:, k] < best
        best, idx = torch.where(better, vals[:, k], best), torch.where(better, torch.full_like(idx, k), idx)
    return best, torch.tensor(perms, dtype=torch.long)[idx], vals


def published():
    """torchmetrics' docstring examples: (preds, target) of the three published values"""
    snr_pt = torch.tensor([2.5, 0.0, 2.0, 8.0]), torch.tensor([3.0, -0.5, 2.0, 7.0])
    torch.manual_seed(1)
    sa_p, sa_t = torch.randn(2, 8000), torch.randn(2, 8000)
    pit_p, pit_t = torch.randn(4, 2, 8000), torch.randn(4, 2, 8000)
    return snr_pt, (sa_p, sa_t), (pit_p, pit_t)


PUB_SNR, PUB_SA_SDR = 16.1805, -41.6579
PUB_PIT, PUB_PERM = [-37.9511, -41.9124, -42.7369, -42.5155], [[1, 0], [1, 0], [0, 1], [1, 0]]
PUB_TOL = 5e-5  # the four printed decimals


def test_comparator_reproduces_the_published_values():
    (sp, st), (ap, at), (pp, pt) = published()
    assert abs(float(ref_snr(sp.double(), st.double())) - PUB_SNR) < PUB_TOL
    assert abs(float(ref_sa_sdr(ap.double(), at.double(), True)) - PUB_SA_SDR) < PUB_TOL
    items, perm, _ = ref_pit("sa_sdr_si", pp.double(), pt.double(), True)  # eval_func max on the metric = min on its negative
    assert (-items - torch.tensor(PUB_PIT, dtype=torch.float64)).abs().max() < PUB_TOL and perm.tolist() == PUB_PERM


def test_published_vectors_through_the_kernel(backend):
    """1. the three published values via ops.pit_loss"""
    (sp, st), (ap, at), (pp, pt) = published()
    dev = backend.device
    loss, perm, _ = ops.pit_loss(backend.lib, NBSS_LOSS_SNR, sp[None, None].to(dev), st[None, None].to(dev), pit=False, need_grad=False)
    assert abs(float(loss) + PUB_SNR) < PUB_TOL and perm.tolist() == [[0]]
    loss, perm, _ = ops.pit_loss(backend.lib, NBSS_LOSS_SA_SDR, ap[None].contiguous().to(dev), at[None].contiguous().to(dev), pit=False,
                                 scale_invariant=True, need_grad=False)
    assert abs(float(loss) + PUB_SA_SDR) < PUB_TOL and perm.tolist() == [[0, 1]]
    loss, perm, _, items = ops.pit_loss(backend.lib, NBSS_LOSS_SA_SDR, pp.to(dev), pt.to(dev), pit=True, scale_invariant=True, need_grad=False,
                                        return_items=True)
    assert (items.cpu().double() + torch.tensor(PUB_PIT, dtype=torch.float64)).abs().max() < PUB_TOL
    assert perm.cpu().tolist() == PUB_PERM
    assert abs(float(loss) + sum(PUB_PIT) / 4) < PUB_TOL


# 5000: a multiple of 4 but not of 256 * 64; 4999: odd (scalar loads); 129 * 251 * 2: the cc_mse shape (pairs)
PARITY_N = (5000, 4999, 129 * 251 * 2)


def parity_inputs(S, N, seed):
    """p = t[:, pi_b] * g + sigma * noise with a different pi_b per item: the winning permutation leads by a wide margin"""
    B = 4
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, S, N, generator=g)
    allp = list(itertools.permutations(range(S)))
    pis = [allp[(b + 1) % len(allp)] for b in range(B)]
    p = torch.stack([t[b, list(pis[b])] for b in range(B)]) * 0.8 + 0.3 * torch.randn(B, S, N, generator=g)
    return p, t


def check_against_comparator(backend, name, p, t, pit, margin=True):
    kind, si = KINDS[name]
    B, S, N = p.shape
    p64 = p.double().requires_grad_(True)
    witems, wperm, vals = ref_pit(name, p64, t.double(), pit)
    if pit and S > 1 and margin:  # the inputs decide the pairing by a wide margin (fp64)
        srt = vals.detach().sort(1).values
        if name == "mse":
            assert ((srt[:, 1] - srt[:, 0]) > 0.1 * srt[:, 0].abs()).all(), srt
        else:
            assert ((srt[:, 1] - srt[:, 0]) > 1.0).all(), srt
    witems.mean().backward()
    witems, want = witems.detach(), witems.detach().mean()
    loss, perm, dp, items = ops.pit_loss(backend.lib, kind, p.to(backend.device), t.to(backend.device), pit=pit, scale_invariant=si,
                                         need_grad=True, return_items=True)
    print(f"{name} S={S} N={N} pit={pit}: loss {float(loss):.7f} want {float(want):.7f} items_err "
          f"{float((items.cpu().double() - witems).abs().max()):.3e} grad_rel_l2 {rel_l2(dp, p64.grad):.3e}")
    assert abs(float(loss) - float(want)) < 2e-5 * max(1.0, abs(float(want)))
    assert torch.equal(perm.cpu().long(), wperm)
    for b in range(B):
        assert abs(float(items[b]) - float(witems[b])) < 2e-5 * max(1.0, abs(float(witems[b]))), (b, float(items[b]), float(witems[b]))
    assert rel_l2(dp, p64.grad) < 2e-5
    return loss, perm, dp


@pytest.mark.parametrize("pit", [True, False], ids=["pit", "nopit"])
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("name", list(KINDS))
def test_parity_with_fp64(backend, name, S, pit):
    """2. loss, per-item losses, perm and dpreds of every kind against the fp64 comparator with autograd (the bars of
    tests/test_signal_loss_optim.py::test_pit_neg_sisdr)"""
    for N in PARITY_N:
        p, t = parity_inputs(S, N, seed=S * 1000 + N % 997)
        check_against_comparator(backend, name, p, t, pit)


def test_four_speakers_and_limits(backend):
    """S = 4 (24 permutations) and the refusals: S > 4, the scale-invariant flag on another kind"""
    p, t = parity_inputs(4, 2000, seed=4)
    for name in KINDS:
        check_against_comparator(backend, name, p, t, True)
    from nbss_amd._lib import NbssError
    p5 = torch.zeros(1, 5, 64, device=backend.device)
    with pytest.raises(NbssError, match="UNSUPPORTED"):
        ops.pit_loss(backend.lib, NBSS_LOSS_SNR, p5, p5)
    p2 = torch.zeros(1, 2, 64, device=backend.device)
    with pytest.raises(NbssError, match="EINVAL"):
        ops.pit_loss(backend.lib, NBSS_LOSS_SNR, p2, p2, scale_invariant=True)


def db_err(name, got, want64):
    """error in dB: of the value itself for the log kinds, of 10 log10 of the value for the MSE (its relative error on the dB scale)"""
    got, want64 = got.detach().cpu().double(), want64.detach().double()
    if name == "mse":
        return float((10 * torch.log10(got / want64)).abs().max())
    return float((got - want64).abs().max())


@pytest.mark.parametrize("name", ["snr", "sa_sdr", "mse"])
def test_high_snr_conditioning(backend, name):
    """3. p = t + 1e-3 rms(t) noise (about 60 dB), N = 32 000: the kinds whose distortion is t - p must subtract element-wise.  Comparator: fp64.
    Yardstick: the error of the reference's own arithmetic (the torchmetrics formula evaluated by torch in fp32 on the CPU); the kernel's
    per-item error must be within 4x that, with a floor of 1e-5 dB (the 4x allows for another summation order; forming |t - p|^2 from fp32 dot
    products misses by orders of magnitude: a few 1e-6 |t|^2 against a distortion of 1e-6 |t|^2).
    Measured (reference fp32 error dB, kernel error dB; largest of 4 items), MI355X and host emulator alike: snr (3.2e-06, 1.9e-06),
    sa_sdr (2.9e-06 on the MI355X host / 3.4e-06, 1.3e-06), mse (3.3e-07 / 3.7e-07, 2.2e-07); also in profiles/README.md."""
    B, S, N = 4, 2, 32000
    g = torch.Generator().manual_seed(60)
    t = torch.randn(B, S, N, generator=g)
    p = t + 1e-3 * t.pow(2).mean(-1, keepdim=True).sqrt() * torch.randn(B, S, N, generator=g)
    want = ref_items(name, p.double(), t.double())
    ref_err = db_err(name, ref_items(name, p, t), want)
    kind, si = KINDS[name]
    _, _, _, items = ops.pit_loss(backend.lib, kind, p.to(backend.device), t.to(backend.device), pit=False, scale_invariant=si, need_grad=False,
                                  return_items=True)
    err = db_err(name, items, want)
    print(f"high-SNR {name} [{backend.name}]: value {float(want[0]):.4f}, reference fp32 error {ref_err:.3e} dB, kernel error {err:.3e} dB")
    assert err <= max(4 * ref_err, 1e-5), (err, ref_err)
    # ... and under PIT the same items come out (the identity is the winning pairing here)
    _, perm, _, items_pit = ops.pit_loss(backend.lib, kind, p.to(backend.device), t.to(backend.device), pit=True, scale_invariant=si, need_grad=False,
                                         return_items=True)
    assert perm.cpu().tolist() == [[0, 1]] * B and torch.equal(items_pit, items)


@pytest.mark.parametrize("name", list(KINDS))
def test_bitwise_repeatable(backend, name):
    """4. two calls on the same inputs: bitwise equal loss, perm and dpreds"""
    kind, si = KINDS[name]
    p, t = parity_inputs(3, 5000, seed=11)
    p, t = p.to(backend.device), t.to(backend.device)
    a = ops.pit_loss(backend.lib, kind, p, t, pit=True, scale_invariant=si, return_items=True)
    b = ops.pit_loss(backend.lib, kind, p, t, pit=True, scale_invariant=si, return_items=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("S", [1, 2, 3])
def test_si_sdr_kind_agrees_with_the_shipped_kernel(backend, S):
    """6. ops.pit_neg_sisdr (untouched: its own dots / finalize kernels) and ops.pit_loss(kind=SI_SDR, pit=True) on case 2's inputs.  The two are
    SEPARATE kernels (the family's dots kernel is specialised per S and loads vectors, so its summation order differs): agreement is within the
    existing bar of test_pit_neg_sisdr, not bitwise."""
    for N in PARITY_N:
        p, t = parity_inputs(S, N, seed=S * 1000 + N % 997)
        p, t = p.to(backend.device), t.to(backend.device)
        l0, perm0, dp0 = ops.pit_neg_sisdr(backend.lib, p, t)
        l1, perm1, dp1 = ops.pit_loss(backend.lib, NBSS_LOSS_SI_SDR, p, t, pit=True)
        assert abs(float(l0) - float(l1)) < 2e-5 * max(1.0, abs(float(l0)))
        assert torch.equal(perm0, perm1) and rel_l2(dp1, dp0) < 2e-5


# ---- 5. the drop-in surface: models/io/loss.py ----
class FakeSTFT:
    """stands in for models.io.stft.STFT in the cc_mse test: a fixed linear 'transform' to [B,S,F,T] complex"""

    def __init__(self, F, T):
        self.F, self.T = F, T

    def stft(self, y):
        B, S, N = y.shape
        return torch.view_as_complex(y[..., :self.F * self.T * 2].reshape(B, S, self.F, self.T, 2).contiguous()), N


def dropin_cases():
    from models.io.loss import cc_mse, neg_snr
    return {"snr": (neg_snr, True, {}, "snr", False, "neg_snr"),
            "sa_sdr_si": ("models.io.loss.neg_sa_sdr", True, {"scale_invariant": True}, "sa_sdr_si", True, "neg_sa_sdr"),
            "mse": (cc_mse, False, {}, "mse", False, "cc_mse")}


@pytest.mark.parametrize("case", ["snr", "sa_sdr_si", "mse"])
def test_loss_module(backend, case):
    from models.io.loss import Loss
    func, pit, kwargs, name, scale_inv, fname = dropin_cases()[case]
    L = Loss(func, pit=pit, loss_func_kwargs=kwargs)
    assert L.name == fname and L.is_scale_invariant_loss is scale_inv and L.mask is None and L.pit is pit
    kw = "".join(f"{k}={v}," for k, v in kwargs.items())
    assert L.extra_repr() == f"loss_func={fname}({kw}), pit={pit}, mask=None"
    B, S, N = 4, 2, 3000
    p, t = parity_inputs(S, N, seed=21)
    dev = backend.device
    extra = {}
    if case == "mse":  # cc_mse compares view_as_real(out) with view_as_real(stft(yr) / XrMM)
        F, T = 9, 20
        stft = FakeSTFT(F, T)
        g = torch.Generator().manual_seed(3)
        xrmm = (torch.rand(B, 1, F, T, generator=g) + 0.5)
        out_c = torch.view_as_complex(torch.randn(B, S, F, T, 2, generator=g)) + stft.stft(t)[0] / xrmm
        out64 = out_c.to(torch.complex128).requires_grad_(True)
        p64 = torch.view_as_real(out64).reshape(B, S, -1)
        t64 = torch.view_as_real(stft.stft(t.double())[0] / xrmm.double()).reshape(B, S, -1)
        out_d = out_c.to(dev).requires_grad_(True)
        extra = {"out": out_d, "XrMM": xrmm.to(dev), "stft": stft}
        leaf64, leaf = out64, out_d
    else:
        leaf64 = p.double().requires_grad_(True)
        p64, t64 = leaf64, t.double()
        leaf = p.to(dev).requires_grad_(True)
    witems, wperm, _ = ref_pit(name, p64, t64, pit)
    witems.mean().backward()
    witems = witems.detach()
    yr_hat = leaf if case != "mse" else p.to(dev)
    loss, perms, yh = L(yr_hat=yr_hat, yr=t.to(dev), reorder=True, reduce_batch=True, **extra)
    assert loss.shape == () and abs(float(loss.detach()) - float(witems.mean())) < 2e-5 * max(1.0, abs(float(witems.mean())))
    if pit:
        assert perms.dtype == torch.long and torch.equal(perms.cpu(), wperm)
        assert torch.equal(yh.detach().cpu(), torch.gather(p, 1, wperm[..., None].expand_as(p)))  # reorder=True: pit_permutate
    else:
        assert perms is None and yh is yr_hat
    loss.backward()
    assert rel_l2(leaf.grad, leaf64.grad) < 2e-5
    items, _, yh2 = L(yr_hat=yr_hat.detach(), yr=t.to(dev), reorder=False, reduce_batch=False, **extra)
    assert items.shape == (B,) and yh2.shape == p.shape
    assert ((items.detach().cpu().double() - witems.detach()).abs() < 2e-5 * witems.detach().abs().clamp(min=1.0)).all()
    # host tensors take the closed forms in torch: the same numbers within the same bars
    if case != "mse":
        hl, hperms, _ = L(yr_hat=p, yr=t, reorder=False, reduce_batch=False)
        assert ((hl.double() - witems.detach()).abs() < 2e-5 * witems.detach().abs().clamp(min=1.0)).all()
        assert not pit or torch.equal(hperms, wperm)
        # the bare callables: [batch]
        fn = L.loss_func
        got = fn(p.to(dev), t.to(dev), **kwargs)
        want = ref_items(name, p.double(), t.double())
        assert got.shape == (B,) and ((got.cpu().double() - want).abs() < 2e-5 * want.abs().clamp(min=1.0)).all()


def test_cc_mse_needs_its_kwargs_and_cirm_mse_still_raises():
    from models.io import loss as M
    L = M.Loss(M.cc_mse, pit=False)
    y = torch.randn(1, 2, 720)
    for missing in ("out", "XrMM", "stft"):
        kw = {"out": torch.zeros(1, 2, 9, 20, dtype=torch.complex64), "XrMM": torch.ones(1, 1, 9, 20), "stft": FakeSTFT(9, 20)}
        del kw[missing]
        with pytest.raises(ValueError, match=missing):
            L(yr_hat=y, yr=y, **kw)
    with pytest.raises(NotImplementedError, match="cirm"):
        M.cirm_mse(y, y)
    with pytest.raises(NotImplementedError, match="cirm"):
        M.Loss(M.cirm_mse, pit=False)
    assert M.Loss(M.neg_sa_sdr, pit=True).is_scale_invariant_loss is False  # the reference's default: scale_invariant=False
    assert M.Loss(M.neg_si_sdr, pit=True).is_scale_invariant_loss is True
