"""The persistent NB-BLSTM recurrence kernels (csrc/blstm.hip behind nbss_nb_blstm_fwd / _bwd) against a plain fp64 restatement of one bidirectional layer,
entry point by entry point: y, the saved i | f | g | o | c planes of both directions and dG, at every workgroup width (NBSS_BLSTM_NTN forces 1 / 2 / 4 tiles
of 16 sequences per workgroup; the production choice only leaves 1 above 2048 sequences), at T = 1 and 2, at a padded gate stride, for quiet inputs
(relative accuracy of tanh near 0) and for saturated gates (|pre-activation| > 88: __expf overflows).

Layouts (include/nbss_hip.h): gx [n][T][ldg] (direction d at columns d * 4 HD, gate rows i | f | g | o, biases inside), w_hh / w_hh_reverse fp32 [4 HD][HD],
y [n][T][2 HD], save [2][n][T][5 HD], dg [n][T][8 HD] = d sum(y * dy) / d gx.

Every output buffer starts as NaN and ends in sentinel rows past n: inside n everything must come back finite, the sentinels untouched (tail tiles); the pad
columns of a gx with ldg > 8 HD are NaN (a read of them poisons the result).

Bars.  fp32: the ones the path meets through the module (tests/test_blstm_native.py): rel-L2 < 2e-5 on y and on each saved plane, < 1e-4 on dG.
bf16: the comparator is the fp64 loop on the operands as the stream holds them (gx, dy and W_hh rounded to bf16: the kernel packs W_hh to the stream type); the
allowance per tensor is 1.5 x the error the SAME loop run in torch bf16 tensors on the host (autograd for dG) shows against that comparator on the same inputs
(margin and rationale of tests/test_nbc2_large.py, tests/test_bf16_vs_reference.py)."""
from types import SimpleNamespace

import pytest
import torch

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32
from util import rel_l2

PAD = 3          # sentinel sequences past n in every buffer
MAGIC = -1536.0  # sentinel value (exact in bf16)
PLANES = "ifgoc"
F32_FWD, F32_BWD, BF16_MARGIN = 2e-5, 1e-4, 1.5

DTYPES = [pytest.param(NBSS_F32, id="f32"), pytest.param(NBSS_BF16, id="bf16")]
HIDDEN = [pytest.param(128, id="hd128"), pytest.param(256, id="hd256")]


def _td(dt):
    return torch.bfloat16 if dt == NBSS_BF16 else torch.float32


def _inputs(dt, HD, n, T, seed, scale=1.0, saturate=False):
    """(gx [n][T][8 HD], w_hh, w_hh_reverse, dy [n][T][2 HD]) in fp32, holding what the stream of type dt holds (gx, dy rounded to it); W_hh at nn.LSTM's
    init U(-HD^-1/2, HD^-1/2), fp32 as the entry point takes it"""
    g = torch.Generator().manual_seed(seed)
    gx = torch.randn(n, T, 8 * HD, generator=g)
    if saturate:  # half of the entries at 150 x: a quarter of all pre-activations beyond +-100, the rest where the gates still move
        gx = gx * torch.where(torch.rand(n, T, 8 * HD, generator=g) < 0.5, 150.0, 1.0)
    gx = gx * scale
    k = HD ** -0.5
    w0, w1 = ((torch.rand(4 * HD, HD, generator=g) * 2 - 1) * k for _ in range(2))
    dy = torch.randn(n, T, 2 * HD, generator=g)
    td = _td(dt)
    return gx.to(td).float(), w0, w1, dy.to(td).float()


def _loop(gx, w0, w1, dy, HD, dtype):
    """one bidirectional LSTM layer as an explicit loop over frames in `dtype`: G_t = gx_t + W_hh h_{t-1}, c_t = f c_{t-1} + i g, h_t = o tanh(c_t), the reverse
    direction walking t = T-1 .. 0 -> y [n][T][2 HD], save [2][n][T][5 HD], dg [n][T][8 HD] (autograd of sum(y * dy); dG = d / d gx: gx enters additively),
    pre [2][n][T][4 HD] the pre-activations"""
    n, T, _ = gx.shape
    gx = gx.to(dtype).detach().clone().requires_grad_(True)
    ys, saves, pres = [], [], []
    for d, w in enumerate((w0, w1)):
        wt = w.to(dtype).t()
        h = torch.zeros(n, HD, dtype=dtype)
        c = torch.zeros(n, HD, dtype=dtype)
        out, sv, pre = [None] * T, [None] * T, [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            G = gx[:, t, d * 4 * HD:(d + 1) * 4 * HD] + h @ wt
            i, f, g, o = torch.sigmoid(G[:, :HD]), torch.sigmoid(G[:, HD:2 * HD]), torch.tanh(G[:, 2 * HD:3 * HD]), torch.sigmoid(G[:, 3 * HD:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            out[t], sv[t], pre[t] = h, torch.cat([i, f, g, o, c], -1), G
        ys.append(torch.stack(out, 1))
        saves.append(torch.stack(sv, 1))
        pres.append(torch.stack(pre, 1))
    y = torch.cat(ys, -1)
    (y * dy.to(dtype)).sum().backward()
    return y.detach(), torch.stack(saves).detach(), gx.grad, torch.stack(pres).detach()


def _reference(dt, gx, w0, w1, dy, HD):
    """the fp64 comparator on the operands as the stream holds them"""
    if dt == NBSS_BF16:
        w0, w1 = w0.bfloat16().float(), w1.bfloat16().float()
    return _loop(gx, w0, w1, dy, HD, torch.float64)


class Kernels:
    """the two entry points on one backend with poisoned, sentinel-terminated buffers"""

    def __init__(self, backend, dt, HD):
        self.lib, self.dev, self.dt, self.HD, self.td = backend.lib, backend.device, dt, HD, _td(dt)
        nb = self.lib._dll.nbss_nb_blstm_ws_bytes(dt, HD)
        assert nb > 0
        self.ws = ops.scratch(nb, self.dev)

    def _out(self, rows, width):
        """flat output buffer: `rows` rows of NaN, then PAD * T rows of MAGIC"""
        b = torch.full((rows + self.padrows, width), float("nan"), dtype=self.td)
        b[rows:] = MAGIC
        return b.to(self.dev)

    def _check_out(self, b, rows, name):
        b = b.cpu()
        assert torch.isfinite(b[:rows].float()).all(), f"{name}: non-finite (or unwritten) values inside n"
        assert (b[rows:].float() == MAGIC).all(), f"{name}: rows past n were written"
        return b[:rows]

    def _in(self, x, width=None):
        """input buffer: x's rows (padded to `width` columns with NaN), then PAD sequences of NaN"""
        n, T, w = x.shape
        b = torch.full((n + PAD, T, width or w), float("nan"), dtype=self.td)
        b[:n, :, :w] = x.to(self.td)
        return b.to(self.dev)

    def forward(self, gx, w0, w1, ldg=None, train=True):
        n, T, _ = gx.shape
        HD, p = self.HD, lambda t: ops._ptr(self.lib, t)
        self.padrows = PAD * T
        self.n, self.T = n, T
        gxb = self._in(gx, ldg)
        w0d, w1d = w0.to(self.dev).contiguous(), w1.to(self.dev).contiguous()
        y = self._out(n * T, 2 * HD)
        save = self._out(2 * n * T, 5 * HD) if train else None
        self.lib.call("nbss_nb_blstm_fwd", self.dt, n, T, HD, gxb.shape[-1], p(gxb), p(w0d), p(w1d), p(y), p(save), p(self.ws), ops._stream(self.lib, gxb))
        self.save_dev = save
        yc = self._check_out(y, n * T, "y").view(n, T, 2 * HD)
        sc = self._check_out(save, 2 * n * T, "save").view(2, n, T, 5 * HD) if train else None
        return yc, sc

    def backward(self, dy, w0, w1):
        """dG from dy and the save of the last training forward"""
        n, T, HD, p = self.n, self.T, self.HD, lambda t: ops._ptr(self.lib, t)
        dyb = self._in(dy)
        w0d, w1d = w0.to(self.dev).contiguous(), w1.to(self.dev).contiguous()
        dg = self._out(n * T, 8 * HD)
        self.lib.call("nbss_nb_blstm_bwd", self.dt, n, T, HD, p(dyb), p(self.save_dev), p(w0d), p(w1d), p(dg), p(self.ws), ops._stream(self.lib, dyb))
        return self._check_out(dg, n * T, "dg").view(n, T, 8 * HD)


def _errors(got, want, HD):
    """rel-L2 per checked tensor: y, each saved plane per direction, dG"""
    (y, save, dg), (y_w, save_w, dg_w) = got, want[:3]
    e = {"y": rel_l2(y, y_w), "dg": rel_l2(dg, dg_w)}
    for d in range(2):
        for k, name in enumerate(PLANES):
            e[f"{name}{d}"] = rel_l2(save[d, ..., k * HD:(k + 1) * HD], save_w[d, ..., k * HD:(k + 1) * HD])
    return e


def _check_parity(dt, HD, got, ins, label):
    """the bars of the module docstring; prints every figure before it asserts"""
    want = _reference(dt, *ins, HD)
    err = _errors(got, want, HD)
    if dt == NBSS_F32:
        bar = {k: F32_BWD if k == "dg" else F32_FWD for k in err}
        print(f"{label}: kernel y {err['y']:.2e} planes max {max(v for k, v in err.items() if k not in ('y', 'dg')):.2e} dg {err['dg']:.2e}")
    else:
        gx, w0, w1, dy = ins
        t16 = _loop(gx, w0, w1, dy, HD, torch.bfloat16)
        e16 = _errors(t16[:3], want, HD)
        bar = {k: BF16_MARGIN * v for k, v in e16.items()}
        worst = max(err, key=lambda k: err[k] / (e16[k] + 1e-30))
        print(f"{label}: torch bf16 y {e16['y']:.2e} dg {e16['dg']:.2e}; kernel y {err['y']:.2e} dg {err['dg']:.2e}; "
              f"worst ratio {worst} {err[worst]:.2e} / {e16[worst]:.2e}")
    bad = {k: (v, bar[k]) for k, v in err.items() if not v < bar[k]}
    assert not bad, (label, bad)
    return want, err


def _train(K, ins, ldg=None):
    gx, w0, w1, dy = ins
    y, save = K.forward(gx, w0, w1, ldg=ldg)
    return y, save, K.backward(dy, w0, w1)


def _b1_cases(ntn):
    """(n, T, pad columns of gx), NS = 16 ntn: n = 1; a partial last tile; exactly one workgroup; NS + 1: a second workgroup holding one sequence, its other
    tiles wholly past n when ntn > 1; three workgroups.  T = 1, 2 and 5 paired with them, the padded stride at the first and the largest"""
    NS = 16 * ntn
    return [(1, 2, 16), (NS - 1, 5, 0), (NS, 2, 0), (NS + 1, 1, 0), (2 * NS + 1, 5, 16)]


@pytest.mark.parametrize("case", range(5))
@pytest.mark.parametrize("ntn", [1, 2, 4])
@pytest.mark.parametrize("HD", HIDDEN)
@pytest.mark.parametrize("dt", DTYPES)
def test_parity_with_fp64_at_every_width(backend, monkeypatch, dt, HD, ntn, case):
    """B1.  y, the ten saved planes and dG of nbss_nb_blstm_fwd / _bwd against the fp64 loop under a forced workgroup width; the inference call (save = NULL)
    gives bitwise the training y, a second backward call bitwise the first.

    Largest case (HD 256, forced NTN 4, n = 129, T = 5, ldg = 8 HD + 16), rel-L2 against the fp64 comparator:
      bf16, emulator: torch bf16 loop y 4.33e-3, dG 5.36e-3 | kernel y 1.67e-3, dG 3.40e-3
      bf16, MI355X:   not measured
      fp32 (forward at its cap of 2), kernel: emulator y 2.5e-7, planes <= 2.4e-7, dG 3.1e-7; MI355X not measured
    Largest kernel / torch-bf16 ratio of any tensor in any case: 1.00 (emulator), not measured (MI355X) - at T = 1 both round an fp32 gate once."""
    n, T, padc = _b1_cases(ntn)[case]
    monkeypatch.setenv("NBSS_BLSTM_NTN", str(ntn))
    ins = _inputs(dt, HD, n, T, seed=100 * ntn + case)
    gx, w0, w1, dy = ins
    K = Kernels(backend, dt, HD)
    ldg = 8 * HD + padc
    y, save, dg = _train(K, ins, ldg=ldg)
    _check_parity(dt, HD, (y, save, dg), ins, f"{backend.name} dt={dt} HD={HD} ntn={ntn} n={n} T={T} ldg={ldg}")
    dg2 = K.backward(dy, w0, w1)
    assert torch.equal(dg2.view(torch.uint8), dg.view(torch.uint8)), "a second backward call differs"
    y_inf, _ = K.forward(gx, w0, w1, ldg=ldg, train=False)
    assert torch.equal(y_inf.view(torch.uint8), y.view(torch.uint8)), "inference y differs from the training y"


def _bits_equal(a, b):
    return all(torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)) for u, v in zip(a, b))


@pytest.mark.parametrize("HD", HIDDEN)
@pytest.mark.parametrize("dt", DTYPES)
def test_results_do_not_depend_on_width_or_grid(backend, monkeypatch, dt, HD):
    """B2.  "results do not depend on the grid" (blstm.hip): n = 70, T = 3 gives the same bits under forced widths 1, 2 and 4 (fp32 at HD 256: 4 is clamped to
    the cap of 2 and still succeeds), and sequence s of that launch is bitwise the n = 1 launch of that sequence alone"""
    n, T, s = 70, 3, 37
    ins = _inputs(dt, HD, n, T, seed=5)
    gx, w0, w1, dy = ins
    K = Kernels(backend, dt, HD)
    res = {}
    for ntn in (1, 2, 4):
        monkeypatch.setenv("NBSS_BLSTM_NTN", str(ntn))
        res[ntn] = _train(K, ins)
    _check_parity(dt, HD, res[1], ins, f"{backend.name} dt={dt} HD={HD} n={n} T={T}")
    assert _bits_equal(res[1], res[2]), "width 2 differs from width 1"
    assert _bits_equal(res[1], res[4]), "width 4 differs from width 1"
    monkeypatch.delenv("NBSS_BLSTM_NTN")
    y1, save1, dg1 = _train(K, (gx[s:s + 1], w0, w1, dy[s:s + 1]))
    y, save, dg = res[1]
    assert _bits_equal((y1, save1, dg1), (y[s:s + 1], save[:, s:s + 1], dg[s:s + 1])), "a sequence depends on its neighbours"


@pytest.mark.parametrize("scale", [1.0, 1e-2, 1e-4])
def test_small_signals_keep_relative_accuracy(backend, scale):
    """B3.  fp32, HD 128, n = 17, T = 4, gx scaled by s (W_hh at its usual init): g, c and h shrink with s, and the bars are relative.  The same loop in torch
    fp32 on the host must stay far below the bars (they are attainable at reference precision); so must the kernel.

    Measured rel-L2 against fp64, worst of y and the ten planes | dG:
      s       torch fp32 (host)    kernel with the former 2 / (1 + e^-2x) - 1: emulator, MI355X      kernel with this bl_tanh: emulator, MI355X
      1       8.3e-8 | 1.0e-7      2.3e-7 | 2.3e-7, not measured      1.8e-7 | 2.2e-7, not measured
      1e-2    9.6e-8 | 9.8e-8      9.3e-6 | 1.2e-7, not measured      2.7e-7 | 1.1e-7, not measured
      1e-4    8.9e-8 | 8.8e-8      8.6e-4 | 1.1e-7, not measured      2.6e-7 | 9.6e-8, not measured
    The former formula misses the 2e-5 bar at s = 1e-4 (y, and the g and c planes at 4.4e-4) and comes within a factor of two of it at s = 1e-2; what is left
    with the new one is the rounding of 1 + e^-x in the three sigmoids."""
    HD, n, T = 128, 17, 4
    ins = _inputs(NBSS_F32, HD, n, T, seed=11, scale=scale)
    want = _reference(NBSS_F32, *ins, HD)
    e32 = _errors(_loop(*ins, HD, torch.float32)[:3], want, HD)
    fwd32 = max(v for k, v in e32.items() if k != "dg")
    print(f"{backend.name} scale {scale:g}: torch fp32 fwd {fwd32:.2e} dg {e32['dg']:.2e}")
    assert fwd32 < F32_FWD / 20 and e32["dg"] < F32_BWD / 20, e32
    K = Kernels(backend, NBSS_F32, HD)
    _, err = _check_parity(NBSS_F32, HD, _train(K, ins), ins, f"{backend.name} scale {scale:g}")
    print(f"{backend.name} scale {scale:g}: kernel fwd {max(v for k, v in err.items() if k != 'dg'):.2e} dg {err['dg']:.2e}")


@pytest.mark.parametrize("dt", DTYPES)
def test_saturated_gates(backend, dt):
    """B4.  pre-activations far beyond +-88, where __expf overflows to inf: the gates must land on 0 / +-1, every gradient stay finite, and the bars of B1 hold"""
    HD, n, T = 128, 17, 4
    ins = _inputs(dt, HD, n, T, seed=13, saturate=True)
    K = Kernels(backend, dt, HD)
    got = _train(K, ins)  # (finite inside n: checked by Kernels)
    want, _ = _check_parity(dt, HD, got, ins, f"{backend.name} dt={dt} saturated")
    pre = want[3]
    assert (pre > 88).float().mean() > 0.1 and (pre < -88).float().mean() > 0.1
    assert (pre.abs() > 100).float().mean() > 0.2


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2049, 4097])
@pytest.mark.parametrize("HD", HIDDEN)
@pytest.mark.parametrize("dt", DTYPES)
def test_production_width_selection_on_the_device(hip_lib, monkeypatch, dt, HD, n):
    """B5.  No knob: bl_ntn doubles the width from 1 while 2 * cdiv(n, 16 ntn) > 256 (both directions of every tile in one round of the 256 CUs) and the
    dtype's cap allows.  n = 2049: 2 * cdiv(2049, 16) = 258 > 256 -> 2, 2 * cdiv(2049, 32) = 130 -> NTN = 2, and 2049 = 64 * 32 + 1: the last workgroup
    holds one sequence.  n = 4097: 258 at 32 sequences per workgroup as well (cdiv(4097, 32) = 129) -> NTN = 4 where the cap allows (fp32 at HD 256 stays
    at 2, in 129 workgroups per direction).  A change to that rule makes these two counts the wrong ones: rethink them with it."""
    monkeypatch.delenv("NBSS_BLSTM_NTN", raising=False)
    T = 2
    ins = _inputs(dt, HD, n, T, seed=n)
    K = Kernels(SimpleNamespace(name="hip", lib=hip_lib, device=torch.device("cuda:0")), dt, HD)
    _check_parity(dt, HD, _train(K, ins), ins, f"hip dt={dt} HD={HD} n={n} T={T}")


def test_argument_checks(emu_lib):
    """B6.  NBSS_EINVAL for ldg < 8 hidden, T = 0, nseq = 0; unsupported for hidden = 64; ws_bytes = -1 for a bad hidden or dtype"""
    EINVAL, EUNSUPPORTED = -1, -2
    dll, HD = emu_lib._dll, 128
    assert dll.nbss_nb_blstm_ws_bytes(NBSS_F32, 64) == -1 and dll.nbss_nb_blstm_ws_bytes(NBSS_BF16, 192) == -1
    assert dll.nbss_nb_blstm_ws_bytes(2, HD) == -1 and dll.nbss_nb_blstm_ws_bytes(-1, 256) == -1
    assert dll.nbss_nb_blstm_ws_bytes(NBSS_F32, HD) == 2 * dll.nbss_nb_blstm_ws_bytes(NBSS_BF16, HD) > 0
    gx, y, save, dg = torch.zeros(1, 1, 8 * HD), torch.zeros(1, 1, 2 * HD), torch.zeros(2, 1, 1, 5 * HD), torch.zeros(1, 1, 8 * HD)
    w = torch.zeros(4 * HD, HD)
    ws = torch.zeros(dll.nbss_nb_blstm_ws_bytes(NBSS_F32, HD), dtype=torch.uint8)
    p = [t.data_ptr() for t in (gx, w, w, y, save, ws)]

    def fwd(n=1, T=1, hidden=HD, ldg=8 * HD, dt=NBSS_F32):
        return dll.nbss_nb_blstm_fwd(dt, n, T, hidden, ldg, *p, None)

    def bwd(n=1, T=1, hidden=HD, dt=NBSS_F32):
        return dll.nbss_nb_blstm_bwd(dt, n, T, hidden, y.data_ptr(), save.data_ptr(), w.data_ptr(), w.data_ptr(), dg.data_ptr(), ws.data_ptr(), None)

    assert fwd() == 0 and bwd() == 0
    assert fwd(ldg=8 * HD - 8) == EINVAL and fwd(T=0) == EINVAL and fwd(n=0) == EINVAL and fwd(dt=2) == EINVAL
    assert bwd(T=0) == EINVAL and bwd(n=0) == EINVAL and bwd(dt=2) == EINVAL
    assert fwd(hidden=64, ldg=8 * HD) == EUNSUPPORTED and bwd(hidden=64) == EUNSUPPORTED
