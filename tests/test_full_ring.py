"""The full-band block at 8-frame slabs, bit for bit against the build BEFORE its row slots (LDS-DMA) and its LDS parameter rows (full.hip).

The change moves no operand and no arithmetic, so y, dx, the saved (mean, rstd) and the five weight-gradient operands (s, dz, z, dy_pre, ds_pre) must keep
their bits.  tests/golden/full_ring_bits.json holds the SHA-256 of each tensor as the parent build (its "parent" entry) produced it, per backend (the
emulator's and the device's bits differ): `python tests/test_full_ring.py child <emu|hip> - <library of the parent build>` for the per-block entry points,
and the same call with 0 / 1 in place of - (and NBSS_FLIP set to it) for the walk-order case, both rounds per knob.

The slab width is a per-process choice (full.hip: full_tt reads NBSS_FULL_TT once) and these grids are far too small for 8 frames by themselves, so
the kernels run in child processes with NBSS_FULL_TT=8: one per backend for the per-block shapes, and one each with NBSS_FLIP=0 / 1 for the walks."""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "full_ring_bits.json"
# (B, F, T), H = 96, squeeze 8, bf16: one row | one full slab, the last frequency tile holds one bin | two slabs + a 3-frame remainder |
# fewer tiles than waves x 2, a one-frame remainder slab, two utterances | the walk-order case
SHAPES = [(1, 1, 1), (1, 129, 8), (1, 129, 19), (2, 17, 9), (3, 129, 8)]
FLIP_SHAPE = (3, 129, 8)
NAMES = ["y", "dx", "stats", "s", "dz", "z", "dy_pre", "ds_pre"]


def _key(shape):
    return "x".join(map(str, shape))


def _digests(backend_name, lib, device, shape):
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    from nbss_amd import ops
    from nbss_amd._lib import NBSS_BF16
    from util import Case

    class Be:
        pass
    be = Be()
    be.name, be.lib, be.device = backend_name, lib, device
    B, F, T = shape
    cs = Case(be, B, F, T, NBSS_BF16)
    x, _ = cs.stream(seed=3)
    dy, _ = cs.stream(seed=4)
    y = ops.full_fwd(lib, cs.cfg, cs.flat, cs.packed, 0, x)
    G = torch.zeros_like(cs.flat)
    ws = ops.workspace(lib, cs.cfg, device)
    dx = ops.full_bwd(lib, cs.cfg, cs.flat, G, cs.packed, 0, x, dy, ws)
    if device.type == "cuda":
        torch.cuda.synchronize()
    # workspace of the block (full.hip: full_bwd_impl): stats [N][2] fp32 | s [B T][8][FKP] | dz [B T][8][FKP] | z [N][8] | dy_pre [N][96] | ds_pre [N][8], 256-byte aligned
    N, BT, FKP, esz = B * F * T, B * T, (F + 3) & ~3, 2
    al = lambda b: (b + 255) & ~255
    sizes = [("stats", N * 2 * 4), ("s", BT * 8 * FKP * esz), ("dz", BT * 8 * FKP * esz), ("z", N * 8 * esz), ("dy_pre", N * 96 * esz), ("ds_pre", N * 8 * esz)]
    raw = ws.cpu().numpy().tobytes()
    out = {"y": y.cpu().view(torch.int16).numpy().tobytes(), "dx": dx.cpu().view(torch.int16).numpy().tobytes()}
    off = 0
    for name, n in sizes:
        out[name] = raw[off:off + n]
        off += al(n)
    return {k: hashlib.sha256(out[k]).hexdigest() for k in NAMES}


WALK_NAMES = ["out", "acts", "grads"]


def _walk_digests(lib, device):
    """FLIP_SHAPE through the forward and backward WALKS (one layer): only these open a WalkFlipScope (launch.h), the per-block entry points run
    unflipped whatever NBSS_FLIP says.  A walk launches an odd number of direction-taking kernels per forward (five per layer) and the counter runs on from
    call to call, so round "a" (counter at 0) and round "b" (after a + one more forward: an odd count) give every kernel of the walk, full_fwd and
    full_bwd among them, BOTH directions when NBSS_FLIP=1 (and neither when it is 0)."""
    import torch
    from nbss_amd._lib import NBSS_BF16
    from nbss_amd.engine import SpatialNetEngine
    from oracle import spatialnet_ref as ref
    B, F, T = FLIP_SHAPE
    p = ref.init_params(num_layers=1, num_freqs=F, dim_input=12, dim_output=4, seed=4)
    eng = SpatialNetEngine(lib, device, dim_input=12, dim_output=4, num_freqs=F, num_layers=1, dtype=NBSS_BF16)
    eng.load_params(p)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, F, T, 12, generator=g).to(eng.stream_dtype()).to(device)
    dout = torch.randn(B, F, T, 4, generator=g).to(device)
    sb, n = (B * F * T * 96 * 2 + 255) // 256 * 256, B * F * T * 96 * 2  # the saved block inputs: 5 L + 1 stream tensors at a 256-byte stride

    def one_round():
        eng.grads.zero_()
        out = eng.forward(x, train=True)
        eng.backward(x, dout)
        if device.type == "cuda":
            torch.cuda.synchronize()
        acts = eng.acts.cpu().numpy().tobytes()
        t = {"out": out.cpu().numpy().tobytes(), "acts": b"".join(acts[i * sb:i * sb + n] for i in range(6)), "grads": eng.grads.cpu().numpy().tobytes()}
        return {k: hashlib.sha256(t[k]).hexdigest() for k in WALK_NAMES}

    a = one_round()
    eng.forward(x, train=True)
    return {"a": a, "b": one_round()}


def _child_main(argv):
    backend_name, flip = argv[0], argv[1]
    libpath = argv[2] if len(argv) > 2 else None
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    from nbss_amd._lib import Lib
    if backend_name == "emu":
        from nbss_amd.build import build_emu
        lib, device = Lib(Path(libpath) if libpath else build_emu()), torch.device("cpu")
    else:
        from nbss_amd._lib import hip
        lib, device = Lib(Path(libpath)) if libpath else hip(), torch.device("cuda:0")
    if flip in ("0", "1"):
        res = {"walk_" + _key(FLIP_SHAPE): _walk_digests(lib, device)}
    else:
        res = {_key(s): _digests(backend_name, lib, device, s) for s in SHAPES}
    print("DIGESTS " + json.dumps(res))


_RUNS = {}


_PROCS = {}


def start_child(backend_name, flip="-"):
    if (backend_name, flip) not in _RUNS and (backend_name, flip) not in _PROCS:
        env = dict(os.environ, NBSS_FULL_TT="8", PYTHONPATH=str(ROOT))
        env.pop("NBSS_FLIP", None)
        if flip != "-":
            env["NBSS_FLIP"] = flip
        _PROCS[(backend_name, flip)] = subprocess.Popen([sys.executable, str(Path(__file__).resolve()), "child", backend_name, flip], env=env,
                                                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def run_child(backend_name, flip="-"):
    """digests of one child process (shared by the tests of a session)"""
    if (backend_name, flip) not in _RUNS:
        start_child(backend_name, flip)
        pr = _PROCS.pop((backend_name, flip))
        out, _ = pr.communicate(timeout=600)
        assert pr.returncode == 0, out
        line = [l for l in out.splitlines() if l.startswith("DIGESTS ")][-1]
        _RUNS[(backend_name, flip)] = json.loads(line[len("DIGESTS "):])
    return _RUNS[(backend_name, flip)]


@pytest.mark.parametrize("shape", SHAPES, ids=_key)
def test_full_block_keeps_the_parent_bits(backend, shape):
    want = json.loads(GOLDEN.read_text())[backend.name][_key(shape)]
    got = run_child(backend.name)[_key(shape)]
    print({k: got[k][:12] for k in NAMES})
    assert got == want, [k for k in NAMES if got[k] != want[k]]


def test_full_block_bits_do_not_depend_on_the_walk_order(backend):
    """out and the saved block inputs (full_fwd's y among them) are the parent's with NBSS_FLIP=0 whatever the direction; the parameter gradients are
    the parent's of the same knob and round (some of the parent's gradient sums outside this block follow the directions of a round)"""
    key = "walk_" + _key(FLIP_SHAPE)
    want = json.loads(GOLDEN.read_text())[backend.name][key]  # the parent's walks: NBSS_FLIP + round
    start_child(backend.name, "0")
    start_child(backend.name, "1")  # (the two children run side by side)
    runs = {f + r: run_child(backend.name, f)[key][r] for f in "01" for r in "ab"}
    print({k: {n: v[n][:12] for n in WALK_NAMES} for k, v in runs.items()})
    for k, got in runs.items():
        assert [got[n] for n in ("out", "acts")] == [want["0a"][n] for n in ("out", "acts")], k
        assert got["grads"] == want[k]["grads"], k


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "child":
    _child_main(sys.argv[2:])
