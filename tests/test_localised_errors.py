"""Localised errors of the fused SpatialNet blocks, forward and backward, emulator and device.

The block parity tests (test_kernels_fwd.py, test_kernels_bwd.py, test_large.py) reduce every tensor to ONE rel-L2 figure.  At the bf16 bars a defect confined
to one strip seam, one tile edge, one channel or one token's share of a weight gradient is a per-cent of that figure and passes.  Two instruments show such a
defect at its full size:

  * test_sliced_parity: the same figures slice by slice (util.sliced_err) — per batch element, frequency, frame, channel, 16 x 16 (F tile x T strip) cell, (frame,
    head), (frequency, conv group), and the parameter gradients per row / tap / group / head — on grids where one tile is a small share of the tensor;
  * test_token_impulse_backward: an upstream gradient that is zero except at ONE token.  The backward is linear in dy, so dx is that token's row of the
    Jacobian and every parameter gradient is that token's contribution alone.

Bars.  Every bar is the one the project already applies to the whole tensor (y: 2e-5 | 1.5e-2, y - x: 3 x; dx and parameter gradients 1e-4 | 3e-2, F-conv bf16 5e-2,
dx - dy: 3 x).  fp32: they hold per slice.  bf16: a small slice fluctuates more than the whole, so the bar of a slicing is max(project bar, 1.5 x the worst
slice of the ORACLE's own block evaluated in torch.bfloat16 on the host against the fp64 oracle) — the rule of tests/test_bf16_vs_reference.py, computed at run
time from the reference side alone, never from the kernel.

The F-conv PReLU kink.  A pre-activation that rounding moves across zero takes the other PReLU branch than the fp64 oracle's; per slice or per token that is a
large share.  Nothing is masked and no bar is loosened: the INPUT is chosen, on the fp64 oracle alone, so that no pre-activation that matters is near zero.
The F-conv block does not couple frames, so x is assembled frame by frame: a frame whose pre-activations fail the condition is redrawn with the next seed
(0, 1, 2, ... at most 64).
  * sliced parity, fp32: no pre-activation of the whole grid within 1e-5 x rms(a) of zero.  (One seed for the whole tensor cannot do this: the grids hold 1e5 to
    2.5e6 pre-activations, 1 to 20 of which lie that close to zero for any seed; per frame it is a 1e4-element condition.)
  * token impulse: the backward of one token's dy evaluates PReLU' only at that token's own H pre-activations (the conv spreads the result over five rows of
    dx afterwards), so the condition is placed on those: |a| >= 0.01 x rms(a).  A wider net (five rows, 0.05) holds for no draw: of 480 unit normals 19 lie
    within 0.05 of zero.  0.01 x rms(a) is six times the rms rounding error of a, a sum of 60 (large: 120) products of two bf16-rounded factors:
    2^-9 sqrt(2/3) rms(a) = 1.6e-3 rms(a).  A weaker input condition can make a correct kernel fail, never a wrong one pass.
"""
import math

import pytest
import torch
import torch.nn.functional as Fn

from nbss_amd import ops
from nbss_amd._lib import NBSS_BF16, NBSS_F32
from nbss_amd.params import param_table
from oracle import spatialnet_ref as ref
from test_kernels_bwd import _FC_NAMES, FULL_NAMES, MH_NAMES, TF_NAMES
from util import SLICE_MIN, Case, rel_l2, sliced_err, worst_slice

DT = {"f32": NBSS_F32, "bf16": NBSS_BF16}
# block -> (the oracle's block, its parameters, the project's bf16 backward bar: tests/test_kernels_bwd.py)
BLOCKS = {
    "fconv0": (lambda x, p: ref.fconv(x, p, "layers.0.fconv1"), _FC_NAMES[0], 5e-2),
    "fconv1": (lambda x, p: ref.fconv(x, p, "layers.0.fconv2"), _FC_NAMES[1], 5e-2),
    "full": (lambda x, p: ref.full(x, p, "layers.0"), FULL_NAMES, 3e-2),
    "mhsa": (lambda x, p: ref.mhsa(x, p, "layers.0"), MH_NAMES, 3e-2),
    "tconvffn": (lambda x, p: ref.tconvffn(x, p, "layers.0"), TF_NAMES, 3e-2),
    "tconvffn_saved": (lambda x, p: ref.tconvffn(x, p, "layers.0"), TF_NAMES, 3e-2)}  # bf16, small geometry: ops.tconvffn_save / t_save=
# grid -> (B, F, T, geometry, backends): see the table in the docstring of test_sliced_parity
GRIDS = {"B2_F37_T70": (2, 37, 70, "small", ("emu", "hip")), "F2_T251": (1, 2, 251, "small", ("emu", "hip")), "B2_F129_T100": (2, 129, 100, "small", ("hip",)),
         "large_F18_T35": (1, 18, 35, "large", ("emu", "hip")), "F257_T3": (1, 257, 3, "small", ("emu", "hip"))}


def _runs(block, dname, grid):
    geo = GRIDS[grid][3]
    if block == "tconvffn_saved" and (dname != "bf16" or geo != "small"):
        return False  # nbss_tconvffn_save_bytes == 0: that stream / geometry recomputes (test_tconvffn_save_is_refused_where_backward_recomputes)
    if grid == "F2_T251":
        return dname == "bf16"
    if grid == "F257_T3":  # the 17-tile F axis: the cross-band blocks; fp32 only where it is served (test_fp32_backward_stops_at_160_frequencies)
        return block in ("fconv0", "fconv1", "full") and (dname == "bf16" or block == "full")
    return True


def _backend_param(be, *rest, id):
    return pytest.param(be, *rest, id=f"{id}-{be}", marks=[pytest.mark.gpu] if be == "hip" else [])


# ---- the blocks ------------------------------------------------------------------------------------------------------------------------------------
def _fconv_preact(x64, p64, pre):
    """the fp64 oracle's F-conv pre-activations a (the input of the PReLU), [B, F, T, H]: oracle/spatialnet_ref.py: fconv, up to the conv"""
    B, F, T, H = x64.shape
    u = ref.layer_norm_h(x64, p64[pre + ".0.weight"], p64[pre + ".0.bias"]).permute(0, 2, 3, 1).reshape(B * T, H, F)
    a = Fn.conv1d(u, p64[pre + ".1.weight"], p64[pre + ".1.bias"], padding="same", groups=8)
    return a.reshape(B, T, H, F).permute(0, 3, 1, 2)


def _clear_of_the_kink(cs, block, x64, margin, where=None):
    """x64 with frames redrawn (seeds 0, 1, ... < 64) until, on the fp64 oracle, |a| >= margin x rms(a) at every pre-activation — `where` (b, f, t): only at
    that token's H pre-activations.  Chosen on the oracle alone; asserted on the result."""
    pre = "layers.0.fconv1" if block == "fconv0" else "layers.0.fconv2"
    x64 = x64.clone()

    def near(x):
        a = _fconv_preact(x, cs.p64, pre)
        lim = margin * float(a.pow(2).mean().sqrt())
        if where is not None:
            b, f, t = where
            bad = torch.zeros(a.shape[0], a.shape[2], dtype=torch.bool)
            bad[b, t] = bool((a[b, f, t].abs() < lim).any())
            return bad
        return (a.abs() < lim).any(dim=3).any(dim=1)  # [B, T]: frames with a pre-activation near zero

    for seed in range(64):
        bad = near(x64)
        if not bad.any():
            break
        cand = cs.stream(seed=seed)[1]
        x64 = torch.where(bad[:, None, :, None], cand, x64)
    bad = near(x64)
    assert not bad.any(), f"no draw of {int(bad.sum())} frame(s) clear of the PReLU kink within 64 seeds ({block}, margin {margin})"
    return x64


def _kernel(cs, block, x, dy, state=None):
    """forward + backward of one block through the C ABI -> y, dx, flat gradient, state (saved forward state, reusable for another dy on the same x)"""
    lib, cfg, dev = cs.lib, cs.cfg, cs.be.device
    G = torch.zeros_like(cs.flat)
    ws = ops.workspace(lib, cfg, dev)
    y, save = state if state is not None else (None, None)
    if block == "mhsa":
        if state is None:
            save = ops.mhsa_save(lib, cfg, dev)
            y = ops.mhsa_fwd(lib, cfg, cs.flat, cs.packed, 0, x, o_save=save)
        dx = ops.mhsa_bwd(lib, cfg, cs.flat, G, cs.packed, 0, x, dy, save, ws)
    elif block == "tconvffn":
        if state is None:
            y = ops.tconvffn_fwd(lib, cfg, cs.flat, cs.packed, 0, x)
        dx = ops.tconvffn_bwd(lib, cfg, cs.flat, G, cs.packed, 0, x, dy, ws)
    elif block == "tconvffn_saved":
        if state is None:
            save = ops.tconvffn_save(lib, cfg, dev)
            assert save is not None
            y = ops.tconvffn_fwd(lib, cfg, cs.flat, cs.packed, 0, x, t_save=save)
        dx = ops.tconvffn_bwd(lib, cfg, cs.flat, G, cs.packed, 0, x, dy, ws, t_save=save)
    elif block == "full":
        if state is None:
            y = ops.full_fwd(lib, cfg, cs.flat, cs.packed, 0, x)
        dx = ops.full_bwd(lib, cfg, cs.flat, G, cs.packed, 0, x, dy, ws)
    else:
        which = int(block[-1])
        if state is None:
            y = ops.fconv_fwd(lib, cfg, cs.flat, cs.packed, 0, which, x)
        dx = ops.fconv_bwd(lib, cfg, cs.flat, G, cs.packed, 0, which, x, dy, ws)
    return y, dx, G, (y, save)


def _leaves(p, names, dtype):
    out, leaves = dict(p), {}
    for n in names:
        out[n] = leaves.setdefault(id(p[n]), p[n].to(dtype).clone().requires_grad_(True))
    return {k: (v if k in names else v.to(dtype)) for k, v in out.items()}


def _oracle(block, x64, p64, dy64, dtype=torch.float64):
    """the oracle's block in `dtype` on the host (inputs and parameters cast to it, gradients from autograd) -> {tensor name: tensor} in fp64"""
    fwd_ref, names, _ = BLOCKS[block]
    x = x64.to(dtype).clone().requires_grad_(True)
    p = _leaves(p64, names, dtype)
    out = {}
    if block == "mhsa":
        y, o, lse = ref.mhsa(x, p, "layers.0", return_saved=True)
        out["o"], out["lse"] = o.detach().double(), lse.detach().double()
    else:
        y = fwd_ref(x, p)
    grads = torch.autograd.grad(y, [x] + [p[n] for n in names], dy64.to(dtype))
    out.update(y=y.detach().double(), dx=grads[0].double())
    out.update({n: g.double() for n, g in zip(names, grads[1:])})
    return out


# ---- the slicings ----------------------------------------------------------------------------------------------------------------------------------
def _fit(shape, dims, blocks):
    """`blocks` coarsened (the first kept axis that still can be doubled, and again) until the smallest slice holds SLICE_MIN elements"""
    blocks = {d: blocks.get(d, 1) for d in dims}

    def smallest():
        n = 1
        for d, s in enumerate(shape):
            n *= s if d not in blocks else min(blocks[d], s % blocks[d] or blocks[d])
        return n

    while smallest() < SLICE_MIN:
        d = next((d for d in dims if blocks[d] < shape[d]), None)
        if d is None:
            break
        blocks[d] = min(2 * blocks[d], shape[d])
    return blocks


def _stream_slicings(block, cfg):
    """label -> (kept axes, blocks) of a [B, F, T, H] tensor"""
    s = {"b": ((0,), {}), "f": ((1,), {}), "t": ((2,), {}), "channel": ((3,), {}), "cell": ((1, 2), {1: 16, 2: 16})}
    if block == "mhsa":
        s["t,head"] = ((2, 3), {3: cfg.H // 4})
    if block.startswith("fconv"):
        s["f,group"] = ((1, 3), {3: cfg.H // 8})
    return s


def _param_slicings(name, shape, cfg):
    """[(label, view shape, kept axes, blocks)] of one parameter gradient; "whole" is the rel-L2 of the existing tests"""
    out = [("whole", shape, (), {})]
    n0 = shape[0]
    if name.endswith(".full.weight"):
        return out + [("squeeze channel", shape, (0,), {}), ("output row", shape, (1,), {}), ("input column", shape, (2,), {})]
    if len(shape) == 1:
        return out + ([("blocks", shape, (0,), {0: -(-n0 // (n0 // SLICE_MIN))})] if n0 >= 2 * SLICE_MIN else [])  # blocks of at least 64 entries; below 128: whole
    out.append(("row", shape, (0,), {}))
    if len(shape) == 3 and shape[2] > 1:  # the grouped convs
        out += [("tap", shape, (2,), {}), ("group", shape, (0,), {0: n0 // 8})]
    if name.endswith("in_proj_weight"):
        out += [("q|k|v", (3, 4, cfg.H // 4, cfg.H), (0,), {}), ("q|k|v,head", (3, 4, cfg.H // 4, cfg.H), (0, 1), {})]
    return out


def _figures(block, cs, got, want, x64, dy64):
    """{(tensor, slicing): (worst slice index, its figure)} of `got` against `want` (both {name: fp64 tensor}, as _oracle returns)"""
    cfg = cs.cfg
    fig = {}
    streams = {"y": (got["y"], want["y"]), "y - x": (got["y"] - x64, want["y"] - x64), "dx": (got["dx"], want["dx"]),
               "dx - dy": (got["dx"] - dy64, want["dx"] - dy64)}
    for tname, (g, w) in streams.items():
        for label, (dims, blocks) in _stream_slicings(block, cfg).items():
            fig[(tname, label)] = worst_slice(g, w, dims, _fit(w.shape, dims, blocks))
    if "o" in want and "o" in got:  # the attention output before out_proj, per (strip, head)
        dims, blocks = (2, 3), {2: 16, 3: cfg.H // 4}
        fig[("o", "strip,head")] = worst_slice(got["o"], want["o"], dims, _fit(want["o"].shape, dims, blocks))
    for n in BLOCKS[block][1]:
        w = want[n]
        if float(w.abs().max()) == 0:  # as check_param_grads: an exactly-zero gradient is judged by the largest entry
            fig[(n, "zero")] = ((), float(got[n].abs().max()))
            continue
        for label, shape, dims, blocks in _param_slicings(n, tuple(w.shape), cfg):
            if not dims:  # the whole tensor, however few entries: the figure of check_param_grads
                fig[(n, label)] = ((), rel_l2(got[n], w))
                continue
            if math.prod(shape) < SLICE_MIN:  # (full.weight at F = 2: 32 entries) nothing to slice, "whole" stands
                continue
            fig[(n, label)] = worst_slice(got[n].reshape(shape), w.reshape(shape), dims, _fit(shape, dims, blocks))
    return fig


def _project_bar(block, dtype, cs, tname):
    btol = 1e-4 if dtype == NBSS_F32 else BLOCKS[block][2]
    return {"y": cs.tol, "o": cs.tol, "y - x": 3 * cs.tol, "dx": btol, "dx - dy": 3 * btol}.get(tname, btol)


_sliced_oracle = {}  # (block's oracle, grid, dtype) -> x64, dy64, fp64 oracle tensors, the bf16 oracle's worst slices: computed once, shared by both backends, never written


def _sliced_case(backend, block, dname, grid):
    B, F, T, geo, _ = GRIDS[grid]
    dtype = DT[dname]
    cs = Case(backend, B, F, T, dtype, geo=geo)
    key = ("tconvffn" if block == "tconvffn_saved" else block, dname, grid)
    if key not in _sliced_oracle:
        x64 = cs.stream(seed=11)[1]
        if block.startswith("fconv") and dtype == NBSS_F32:
            x64 = _clear_of_the_kink(cs, block, x64, 1e-5)
        dy64 = cs.stream(seed=111, scale=0.5)[1]
        want = _oracle(block, x64, cs.p64, dy64)
        ref16 = None
        if dtype == NBSS_BF16:
            ref16 = _figures(block, cs, _oracle(block, x64, cs.p64, dy64, torch.bfloat16), want, x64, dy64)
        _sliced_oracle[key] = (x64, dy64, want, ref16)
    x64, dy64, want, ref16 = _sliced_oracle[key]
    return cs, x64.to(cs.sdtype).to(backend.device), x64, dy64.to(cs.sdtype).to(backend.device), dy64, want, ref16


def _got(cs, block, y, dx, G, save=None):
    got = {"y": y.double().cpu(), "dx": dx.double().cpu()}
    table = param_table(cs.lib, cs.cfg)
    for n in BLOCKS[block][1]:
        off, shape = table[n]
        got[n] = G[off:off + math.prod(shape)].reshape(shape).double().cpu()
    if block == "mhsa" and cs.cfg.H == 96:  # the save buffer of the small geometry: O | log2-sum-exp rows (layout.h: mhsa_lse_offset), as test_mhsa reads it
        n, esz, H = cs.cfg.B * cs.cfg.F * cs.cfg.T, y.element_size(), cs.cfg.H
        got["o"] = save[: n * H * esz].view(y.dtype).view(cs.cfg.B, cs.cfg.F, cs.cfg.T, H).double().cpu()
        off = (n * H * esz + 255) // 256 * 256
        got["lse"] = save[off: off + n * 4 * 4].view(torch.float32).view(cs.cfg.B, cs.cfg.F, cs.cfg.T, 4).double().cpu()
    return got


SLICED_CASES = [_backend_param(be, block, dname, grid, id=f"{block}-{dname}-{grid}") for grid in GRIDS for block in BLOCKS for dname in DT
                for be in GRIDS[grid][4] if _runs(block, dname, grid)]


@pytest.mark.parametrize("backend,block,dname,grid", SLICED_CASES, indirect=["backend"])
def test_sliced_parity(backend, block, dname, grid):
    """forward and backward of one fused block, every figure of test_layernorm_row_edges slice by slice (module docstring: slicings and bars).  Grids:
      (2, 37, 70)              F: three 16-row tiles, the last with 5 rows; T: five 16-frame strips (an odd count), the last with 6 frames, two 64-query dS chunks
      (1, 2, 251) bf16         the full-length specialisations: all 16 strips, the last with 11 frames
      (2, 129, 100) device     258 sequences (nseq % 8 == 2, more sequences than CUs) and 200 frames of slabs
      (1, 18, 35) large        the generic path and, on bf16, tchain / fconv_g
      (1, 257, 3)              the 17-tile F axis: fconv*, full on bf16; full on fp32 too
    mhsa (small geometry) also: the saved attention output per (strip, head), and the saved log2-sum-exp rows as a largest absolute error per (strip, head)
    at the bars of test_mhsa (2e-4 | 5e-2)."""
    cs, x, x64, dy, dy64, want, ref16 = _sliced_case(backend, block, dname, grid)
    dtype = DT[dname]
    y, dx, G, (_, save) = _kernel(cs, block, x, dy)
    got = _got(cs, block, y, dx, G, save)
    bad = []
    for (tname, label), (idx, err) in _figures(block, cs, got, want, x64, dy64).items():
        bar = _project_bar(block, dtype, cs, tname)
        if ref16 is not None and label != "zero":
            bar = max(bar, 1.5 * ref16[(tname, label)][1])
        print(f"sliced {backend.name} {block} {grid} {dname} {tname} per {label}: worst {idx} {err:.3e} (bar {bar:.1e})")
        if not err < bar:
            bad.append((tname, label, idx, err, bar))
    if "lse" in got:
        e = (got["lse"] - want["lse"]).abs()  # [B, F, T, heads]
        T = e.shape[2]
        per = torch.stack([e[:, :, s:s + 16].amax(dim=(0, 1, 2)) for s in range(0, T, 16)])  # [strips, heads]
        idx, err, bar = divmod(int(per.argmax()), 4), float(per.max()), 2e-4 if dtype == NBSS_F32 else 5e-2
        print(f"sliced {backend.name} {block} {grid} {dname} lse per strip,head: worst {idx} {err:.3e} abs (bar {bar:.1e})")
        if not err < bar:
            bad.append(("lse", "strip,head", idx, err, bar))
    assert not bad, bad


# ---- single-token upstream gradients -----------------------------------------------------------------------------------------------------------------
IMPULSE_GRIDS = [(2, 18, 35, "small"), (1, 18, 35, "large")]
IMPULSE_F, IMPULSE_T = (0, 15, 16, 17), (0, 15, 16, 31, 32, 34)  # first and last rows, both sides of every tile / strip seam, the ragged last strip


def _impulse_tokens(backend, block):
    tokens = [(f, t) for f in (IMPULSE_F[0], IMPULSE_F[-1]) for t in (IMPULSE_T[0], IMPULSE_T[-1])]  # the four corners: every block, both backends
    if backend.name == "emu":  # the sweep along the axis the block couples (narrow-band: T at the last row; cross-band: F at the last frame)
        tokens += [(IMPULSE_F[-1], t) for t in IMPULSE_T[1:-1]] if block in ("mhsa", "tconvffn", "tconvffn_saved") else [(f, IMPULSE_T[-1]) for f in IMPULSE_F[1:-1]]
    return tokens


_impulse_oracle = {}  # (block's oracle, dtype, geometry, token) -> x64, dy64, the fp64 oracle's dx and parameter gradients: shared by both backends, never written


def _impulse_wants(cs, block, dname, geo, tokens):
    """per token: x64, dy64, {dx and parameter gradients of the fp64 oracle}.  One oracle graph per (block, dtype, geometry), one autograd.grad per token —
    the F-conv blocks: one graph per token, since each token's frame of x is drawn clear of the PReLU kink (module docstring)."""
    fwd_ref, names, _ = BLOCKS[block]
    B, F, T, H = cs.cfg.B, cs.cfg.F, cs.cfg.T, cs.cfg.H
    base = ("tconvffn" if block == "tconvffn_saved" else block, dname, geo)
    x64 = cs.stream(seed=11)[1]
    graph = None
    out = []
    for i, (f, t) in enumerate(tokens):
        key = base + ((f, t),)
        if key not in _impulse_oracle:
            g = torch.Generator().manual_seed(1000 + 64 * f + t)
            dy64 = torch.zeros(B, F, T, H, dtype=torch.float64)
            dy64[B - 1, f, t] = torch.randn(H, generator=g).to(cs.sdtype).double()
            xt = x64
            if block.startswith("fconv"):
                xt = _clear_of_the_kink(cs, block, x64, 0.01, where=(B - 1, f, t))
                graph = None
            if graph is None:
                x = xt.clone().requires_grad_(True)
                p = _leaves(cs.p64, names, torch.float64)
                graph = (x, p, fwd_ref(x, p))
            x, p, y = graph
            grads = torch.autograd.grad(y, [x] + [p[n] for n in names], dy64, retain_graph=True)
            _impulse_oracle[key] = (xt, dy64, dict(zip(["dx"] + names, grads)))
        out.append(_impulse_oracle[key])
    return out


IMPULSE_CASES = [_backend_param(be, block, dname, id=f"{block}-{dname}") for block in BLOCKS for dname in DT for be in ("emu", "hip")
                 if block != "tconvffn_saved" or dname == "bf16"]


@pytest.mark.parametrize("backend,block,dname", IMPULSE_CASES, indirect=["backend"])
def test_token_impulse_backward(backend, block, dname):
    """dy zero except at ONE token of the last batch element (H seeded normal values), grids (2, 18, 35) and large (1, 18, 35); tokens: the four corners of
    f in {0, 15, 16, 17} x t in {0, 15, 16, 31, 32, 34} and, on the emulator, the sweep over t at f = 17 (mhsa, tconvffn*) or over f at t = 34 (fconv*, full).
    Per impulse: dx at the dx bar of run_block_bwd; every parameter gradient at that bar (bf16, few tokens: 4 x, as
    test_block_forward_backward_random_small_grids; an exactly-zero oracle gradient: largest entry, as check_param_grads); fconv* and full, which do not
    couple frames: dx at every other frame is exactly zero."""
    dtype = DT[dname]
    bad = []
    for (B, F, T, geo) in IMPULSE_GRIDS:
        if block == "tconvffn_saved" and geo != "small":
            continue  # nbss_tconvffn_save_bytes == 0 at the large geometry
        cs = Case(backend, B, F, T, dtype, geo=geo)
        tokens = _impulse_tokens(backend, block)
        table = param_table(cs.lib, cs.cfg)
        btol = 1e-4 if dtype == NBSS_F32 else BLOCKS[block][2]
        gtol = btol if dtype == NBSS_F32 else 4 * btol
        state, x_of_state = None, None
        for (f, t), (x64, dy64, want) in zip(tokens, _impulse_wants(cs, block, dname, geo, tokens)):
            if x_of_state is not x64:
                state, x_of_state, x = None, x64, x64.to(cs.sdtype).to(backend.device)
            _, dx, G, state = _kernel(cs, block, x, dy64.to(cs.sdtype).to(backend.device), state)
            dx = dx.double().cpu()
            figures = [("dx", rel_l2(dx, want["dx"]), btol)]
            for n in BLOCKS[block][1]:
                off, shape = table[n]
                g = G[off:off + math.prod(shape)].reshape(shape)
                figures.append((n, rel_l2(g, want[n]) if float(want[n].abs().max()) > 0 else float(g.abs().max()), gtol))
            if block in ("fconv0", "fconv1", "full"):
                rest = dx.clone()
                rest[B - 1, :, t] = 0
                figures.append(("dx at the other frames, nonzero entries", float((rest != 0).sum()) + float(rest.isnan().sum()), 0.5))
            worst = max(figures, key=lambda v: v[1] / v[2])
            print(f"impulse {backend.name} {block} {geo} {dname} token (f {f}, t {t}): dx {figures[0][1]:.3e} (bar {btol:.1e}); worst {worst[0]} {worst[1]:.3e} (bar {worst[2]:.1e})")
            bad += [(geo, f, t, n, err, bar) for n, err, bar in figures if not err < bar]
    assert not bad, bad
