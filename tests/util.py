"""helpers shared by the kernel parity tests"""
import copy

import torch

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32, make_cfg
from oracle import spatialnet_ref as ref


def _t(a):
    import numpy as np
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    a = a.detach().cpu()
    if a.is_complex():
        a = torch.view_as_real(a.to(torch.complex128))
    return a.double()


def rel_l2(a, b):
    a = _t(a)
    b = _t(b)
    return float((a - b).norm() / (b.norm() + 1e-30))


def max_abs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def _sliced_sums(t, dims, blocks):
    """sum of t over every axis not in dims, the kept axes cut into blocks of blocks[axis] entries (a ragged last block) -> sums, element counts"""
    t = _t(t)
    dims = tuple(d % t.dim() for d in dims)
    drop = [d for d in range(t.dim()) if d not in dims]
    s = t.sum(dim=drop) if drop else t.clone()
    n = torch.full_like(s, float(t.numel() // max(s.numel(), 1)))
    blocks = {d % t.dim(): b for d, b in (blocks or {}).items()}
    for i, d in enumerate(sorted(dims)):
        blk = blocks.get(d, 1)
        if blk > 1:
            idx = torch.arange(s.shape[i]) // blk
            shape = list(s.shape)
            shape[i] = int(idx[-1]) + 1
            s = torch.zeros(shape, dtype=s.dtype).index_add_(i, idx, s)
            n = torch.zeros(shape, dtype=n.dtype).index_add_(i, idx, n)
    return s, n


SLICE_MIN = 64  # fewer elements than this is a sample, not a slice: its rms fluctuates by more than 1 / sqrt(2 x 64) = 9 %


def sliced_err(got, want, dims, blocks=None):
    """the error of `got` (a kernel's tensor) against `want` (the fp64 oracle's) slice by slice: the axes `dims` are kept — `blocks` {axis: n} cuts a kept
    axis into blocks of n entries, the last one ragged — and every other axis is reduced.  Per slice s: rms(got - want over s) / max(rms(want over s),
    rms(want over everything)), so a slice that is legitimately near zero does not divide by nothing and a slice larger than the average is judged against
    itself.  fp64 on the host.  A slice holds at least SLICE_MIN elements (asserted: the caller coarsens `blocks`)."""
    got, want = _t(got), _t(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    e2, n = _sliced_sums((got - want) ** 2, dims, blocks)
    w2, _ = _sliced_sums(want ** 2, dims, blocks)
    assert float(n.min()) >= SLICE_MIN, f"slices of {int(n.min())} elements: coarsen (shape {tuple(want.shape)}, dims {dims}, blocks {blocks})"
    whole = (want ** 2).mean()
    return torch.sqrt(e2 / n) / torch.sqrt(torch.maximum(w2 / n, whole)).clamp_min(1e-300)


def worst_slice(got, want, dims, blocks=None):
    """-> (index tuple along the kept axes, in blocks; value) of the largest sliced_err"""
    err = sliced_err(got, want, dims, blocks)
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)  # a NaN from the kernel is the worst slice, not an ignored one
    i = int(err.argmax())
    return tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape)) if err.dim() else (), float(err.reshape(-1)[i])


# ---- the native blocks inside models.arch.OnlineSpatialNet (tests/test_online_*_train_module.py) ---------------------------------------------------------
ONLINE_SWITCHES = ("NBSS_ONLINE_NATIVE_XBAND", "NBSS_ONLINE_NATIVE_TRAIN", "NBSS_ONLINE_NATIVE_RET")


def online_net(seed, num_freqs, **kw):
    """a small OnlineSpatialNet in train mode at the kernels' geometry, with non-trivial norm weights and biases"""
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    torch.manual_seed(seed)
    args = dict(dim_input=4, dim_output=4, num_layers=1, dim_squeeze=8, num_freqs=num_freqs, dim_hidden=96, dim_ffn=192, num_heads=4, attention="ret(2)")
    args.update(kw)
    net = OnlineSpatialNet(**args).train()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.2 * torch.randn_like(p))
    return net


def grad_fns(t):
    """names of every node of the autograd graph behind t"""
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo += [g for g, _ in f.next_functions]
    return names


def fp64_reference(net, B, F, T):
    """-> net, x, r, y, {name: grad}: the run of `net` (switches off) in fp64 on the CPU on random x [B,F,T,4], loss = sum(y r)"""
    x, r = torch.randn(B, F, T, 4), torch.randn(B, F, T, 4)
    n64 = copy.deepcopy(net).double()
    y = n64(x.double())
    (y * r.double()).sum().backward()
    return net, x, r, y.detach(), {k: p.grad for k, p in n64.named_parameters()}


def check_against_fp64(y, grads, wy, wg, fwd_tol, grad_tol, also=()):
    """y and every gradient of {name: grad} against the fp64 run, rel-L2"""
    ey = rel_l2(y.detach().cpu(), wy)
    errs = {k: rel_l2(g.cpu(), wg[k]) for k, g in grads.items()}
    print(f"y {ey:.1e}; worst grad {max(errs, key=errs.get)} {max(errs.values()):.1e}" + "".join(f"; {k} {errs[k]:.1e}" for k in also))
    assert set(errs) == set(wg) and ey <= fwd_tol, ey
    assert max(errs.values()) <= grad_tol, {k: v for k, v in errs.items() if v > grad_tol}


def fit_with_switch(monkeypatch, argv, on, node):
    """`TrainCLI fit` twice, with every switch off and with those of `on` set: four steps in two epochs each on the device, no step of the first run and
    every step of the second has `node` in the graph of its loss, the first step's loss is the switch-off run's to 1e-4 relative, and the loss decreases"""
    import SharedTrainer
    from SharedTrainer import TrainCLI
    steps = []
    orig = SharedTrainer.TrainModule.training_step

    def recording(self, *a, **k):
        loss = orig(self, *a, **k)
        steps.append((float(loss.detach()), node in grad_fns(loss)))
        return loss

    monkeypatch.setattr(SharedTrainer.TrainModule, "training_step", recording)
    for s in ONLINE_SWITCHES:
        monkeypatch.delenv(s, raising=False)
    TrainCLI(argv=argv)
    off, steps[:] = list(steps), []
    for s in on:
        monkeypatch.setenv(s, "1")
    log = TrainCLI(argv=argv).result["log"]
    on = list(steps)
    print("switch off:", off, "\nswitch on: ", on)
    assert len(log) == 2 and len(on) == len(off) == 4 and log[0]["device"].startswith("cuda")
    assert not any(n for _, n in off) and all(n for _, n in on)
    assert abs(on[0][0] - off[0][0]) <= 1e-4 * abs(off[0][0]), (on[0], off[0])
    key = next(k for k in log[0] if k.startswith("train/"))
    assert log[1][key] < log[0][key], log


class Case:
    """one (cfg, params, packed) bundle on a backend"""

    GEO = {"small": dict(H=96, FFN=192, SQ=8), "large": dict(H=192, FFN=384, SQ=16)}  # configs/SpatialNet.yaml:16-24 and its "for large" comments

    def __init__(self, backend, B, F, T, dtype, L=1, C_in=12, C_out=4, seed=0, geo="small"):
        self.be = backend
        self.lib = backend.lib
        g = self.GEO[geo]
        self.cfg = make_cfg(B, F, T, C_in, C_out, L=L, dtype=dtype, **g)
        self.p = ref.init_params(num_layers=L, num_freqs=F, dim_input=C_in, dim_output=C_out, seed=seed, dim_hidden=g["H"], dim_ffn=g["FFN"],
                                 dim_squeeze=g["SQ"])
        self.p64 = {k: v.double() for k, v in self.p.items()}
        self.flat = ops.flatten_params(self.lib, self.cfg, self.p, backend.device)
        self.packed = ops.pack_params(self.lib, self.cfg, self.flat)
        self.sdtype = ops.stream_dtype(self.cfg)
        # tolerances: fp32 path vs fp64 oracle ; bf16 path vs fp64 oracle fed with bf16-rounded input
        self.tol = 2e-5 if dtype == NBSS_F32 else 1.5e-2

    def stream(self, seed=1, H=None, scale=1.0):
        H = self.cfg.H if H is None else H
        g = torch.Generator().manual_seed(seed)
        x = scale * torch.randn(self.cfg.B, self.cfg.F, self.cfg.T, H, generator=g)
        xs = x.to(self.sdtype)
        return xs.to(self.be.device), xs.double()
