"""Two builds of the library in ONE process, the same inputs to nbss_{mhsa,tconvffn,fconv,full}_{fwd,bwd}, every output compared byte for byte:
y, dx, the flat gradient buffer, the saved-state buffers (attention output / log-sum-exp / LayerNorm statistics, T-ConvFFN pre-activations) and
the workspace (row statistics, weight-gradient operands and partials).  For a refactor that must not change a bit.

    tools/build_prev.sh <rev>                              # the other build: lib/libnbss_hip_prev.so
    python tools/ln_bitwise.py hip|emu [prev library] [current library]

An output the PREVIOUS build does not reproduce from one run to the next (atomicAdd partials) is held to that build's own run-to-run difference
instead: the previous build runs three times first, its figure is the largest max|d| among its own runs, and the current build may not be further
from the first of them.  Byte buffers (workspace, saved state) hold fp32 and bf16 regions side by side: they are read as fp32 words for that figure
(a changed bf16 value still changes its word), NaN words counting as equal only to the same bits.  Exit status 1 when a reproducible output
differs or a non-reproducible one differs by more than the previous build from itself.
The emulator leg leaves out the grids that take it minutes — (2, 129, 251), SpatialNet-large at (1, 129, 251), T = 600 — and keeps one long
sequence of 300 frames; the device leg runs them all."""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from nbss_amd import ops  # noqa: E402
from nbss_amd._lib import NBSS_BF16, NBSS_F32, Lib, make_cfg  # noqa: E402

GEO = {"small": dict(H=96, FFN=192, SQ=8), "large": dict(H=192, FFN=384, SQ=16)}
EDGE = [(2, 1, 1), (2, 17, 15), (2, 16, 17), (2, 5, 33)]
GRIDS = {"emu": [("small", g) for g in EDGE] + [("large", (1, 5, 19))],
         "hip": [("small", g) for g in EDGE] + [("small", (2, 129, 251)), ("large", (1, 5, 19)), ("large", (1, 129, 251))]}
LONG = {"emu": [("small", (1, 2, 300))], "hip": [("small", (1, 129, 600)), ("large", (1, 2, 300))]}  # forwards only: the mhsa_kv / flash and chunked T-ConvFFN paths


def fresh(n, dev):
    return torch.full((int(n),), 0xFF, dtype=torch.uint8, device=dev)


def run_block(lib, cfg, dev, flat, packed, x, dy, block, bwd=True):
    """-> {name: tensor} of everything the block's entry points write"""
    out = {}
    G = torch.zeros_like(flat)
    ws = fresh(ops.workspace(lib, cfg, dev).numel(), dev)
    if block == "mhsa":
        o = fresh(ops.mhsa_save(lib, cfg, dev).numel(), dev)  # (beyond 256 frames this buffer is the K | V scratch)
        out["y"] = ops.mhsa_fwd(lib, cfg, flat, packed, 0, x, o_save=o)
        out["o_save"] = o.clone()
        if bwd:
            out["dx"] = ops.mhsa_bwd(lib, cfg, flat, G, packed, 0, x, dy, o, ws)
    elif block in ("tconvffn", "tconvffn_saved"):
        sv = ops.tconvffn_save(lib, cfg, dev) if block == "tconvffn_saved" else None
        if block == "tconvffn_saved" and sv is None:
            return None  # this stream type / geometry recomputes
        if sv is not None:
            sv.fill_(0xFF)
        out["y"] = ops.tconvffn_fwd(lib, cfg, flat, packed, 0, x, t_save=sv)
        if sv is not None:
            out["t_save"] = sv.clone()
        if bwd:
            out["dx"] = ops.tconvffn_bwd(lib, cfg, flat, G, packed, 0, x, dy, ws, t_save=sv)
    elif block == "full":
        out["y"] = ops.full_fwd(lib, cfg, flat, packed, 0, x)
        if bwd:
            out["dx"] = ops.full_bwd(lib, cfg, flat, G, packed, 0, x, dy, ws)
    else:
        which = int(block[-1])
        out["y"] = ops.fconv_fwd(lib, cfg, flat, packed, 0, which, x)
        if bwd:
            out["dx"] = ops.fconv_bwd(lib, cfg, flat, G, packed, 0, which, x, dy, ws)
    if bwd:
        out["G"] = G
        out["ws"] = ws
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return out


def nbytes_differ(a, b):
    return int((a.contiguous().view(torch.uint8) != b.contiguous().view(torch.uint8)).sum())


def max_diff(a, b):
    if a.dtype == torch.uint8:  # as fp32 words
        n = a.numel() // 4 * 4
        wa, wb = a[:n].view(torch.int32), b[:n].view(torch.int32)
        a, b = a[:n].view(torch.float32), b[:n].view(torch.float32)
        d = (a - b).abs()
        d[wa == wb] = 0.0
        return float("inf") if bool((~torch.isfinite(d)).any()) else float(d.max()) if n else 0.0
    d = (a.float() - b.float()).abs()
    return float(d[torch.isfinite(d)].max()) if bool(torch.isfinite(d).any()) else 0.0


def main():
    backend = sys.argv[1] if len(sys.argv) > 1 else "hip"
    libdir = ROOT / ("nbss_amd/lib" if backend == "hip" else "tests/hipemu")
    stem = "libnbss_hip" if backend == "hip" else "libnbss_emu"
    prev = Lib(sys.argv[2] if len(sys.argv) > 2 else libdir / f"{stem}_prev.so")
    cur = Lib(sys.argv[3] if len(sys.argv) > 3 else libdir / f"{stem}.so")
    dev = torch.device("cuda:0" if backend == "hip" else "cpu")
    ncmp = nbad = nloose = 0
    cases = [(geo, g, True) for geo, g in GRIDS[backend]] + [(geo, g, False) for geo, g in LONG[backend]]
    for geo, (B, F, T), bwd in cases:
        for dtype, nm in ((NBSS_F32, "f32"), (NBSS_BF16, "bf16")):
            cfg = make_cfg(B, F, T, 12, 4, L=1, dtype=dtype, **GEO[geo])
            gen = torch.Generator().manual_seed(1)
            flat = ops.random_params(prev, cfg, dev)
            flat += 0.1 * torch.randn(flat.numel(), generator=gen).to(dev)  # (no LayerNorm weight stays at exactly 1)
            npk = ops.pack_params(prev, cfg, flat).numel()
            packed = ops.pack_params(prev, cfg, flat, out=torch.zeros(npk, dtype=torch.uint8, device=dev))
            assert torch.equal(packed, ops.pack_params(cur, cfg, flat, out=torch.zeros(npk, dtype=torch.uint8, device=dev)))
            sd = ops.stream_dtype(cfg)
            x = torch.randn(B, F, T, cfg.H, generator=gen).to(sd).to(dev)
            dy = (0.5 * torch.randn(B, F, T, cfg.H, generator=gen)).to(sd).to(dev)
            blocks = ["mhsa", "tconvffn"] if not bwd else ["mhsa", "tconvffn", "tconvffn_saved", "fconv0", "fconv1", "full"]
            for block in blocks:
                p1 = run_block(prev, cfg, dev, flat, packed, x, dy, block, bwd)
                if p1 is None:
                    continue
                p2 = run_block(prev, cfg, dev, flat, packed, x, dy, block, bwd)
                p3 = run_block(prev, cfg, dev, flat, packed, x, dy, block, bwd)
                c = run_block(cur, cfg, dev, flat, packed, x, dy, block, bwd)
                for k in p1:
                    selfb, curb = max(nbytes_differ(p1[k], p2[k]), nbytes_differ(p1[k], p3[k])), nbytes_differ(p1[k], c[k])
                    ncmp += 1
                    if selfb == 0 and curb == 0:
                        continue
                    selfd, curd = max(max_diff(p1[k], p2[k]), max_diff(p1[k], p3[k]), max_diff(p2[k], p3[k])), max_diff(p1[k], c[k])
                    ok = selfb > 0 and curd <= selfd
                    nloose += ok
                    nbad += not ok
                    print(f"{'not reproducible' if ok else 'DIFFERENT'}: {geo} B{B} F{F} T{T} {nm} {block}.{k}: previous build against itself {selfb} bytes (max|d| {selfd:.3e}), "
                          f"current against previous {curb} bytes (max|d| {curd:.3e})", flush=True)
    print(f"{backend}: {ncmp} outputs compared, {ncmp - nbad - nloose} equal byte for byte, {nloose} within the previous build's own run-to-run difference, {nbad} different")
    return 1 if nbad else 0


if __name__ == "__main__":
    sys.exit(main())
