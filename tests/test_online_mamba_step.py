"""nbss_online_mamba_step (csrc/online_mamba_step.hip: one residual Mamba block of the native OnlineSpatialNet streaming step) through the C ABI against
the module in fp64: copy.deepcopy(LayerNorm / models.arch.base.mamba.Mamba).double() on the whole stream.

As in tests/test_online_kernels.py the kernel is driven over ONE stream of BF = 15 sequences cut into the irregular partition PART (1, 25 and 32 frames,
two equal neighbours, sizes that are no multiple of the 8-frame register tile), the two states persisting across the calls; the chunk's output AND both
states after every call are compared with the reference (the states transposed to the module's [BF,E,3] / [BF,E,16]).  Tolerance: rel-L2 <= 2e-5, the
project's bound for an fp32 kernel against fp64 (tests/util.py: Case.tol).  The chunk buffer is NaN bytes outside the frames of the call (the kernel has
no scratch in global memory).  The recurrence uses the accurate expf (shared with the training kernels); SiLU uses __expf like the rest of the step."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as Fn

from nbss_amd import ops
from nbss_amd._lib import NbssError
from util import rel_l2

TOL = 2e-5
PART = [1, 32, 7, 25, 8, 3, 32, 16, 16, 5, 2]  # 147 frames
T_ALL = sum(PART)
BF = 15
EINVAL, EUNSUPPORTED = -1, -2


def _bounds(part):
    out, t = [], 0
    for C in part:
        out.append((t, C))
        t += C
    return out


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(ln, mamba) in fp32, the stream x [BF, T_ALL, 96] and the fp64 reference: out [BF, T, 96] = x + mamba(ln(x)), the states after every frame count that
    any partition used here reaches, and the dt pre-activations.  Computed once per kind and left unchanged."""
    from models.arch.base.mamba import Mamba
    torch.manual_seed({"perturbed": 11, "long_memory": 12, "softplus": 13}[kind])
    m, ln = Mamba(d_model=96, d_state=16, d_conv=4).eval(), torch.nn.LayerNorm(96)
    with torch.no_grad():  # not only the defaults: A_log (log 1..16 in every channel), D (ones), the taps, both 1-D biases, the LayerNorm's affine
        m.A_log.add_(0.1 * torch.randn_like(m.A_log))
        m.D.add_(0.1 * torch.randn_like(m.D))
        m.conv1d.weight.add_(0.1 * torch.randn_like(m.conv1d.weight))
        m.conv1d.bias.add_(0.1 * torch.randn_like(m.conv1d.bias))
        m.dt_proj.bias.add_(0.1 * torch.randn_like(m.dt_proj.bias))
        ln.weight.add_(0.1 * torch.randn_like(ln.weight))
        ln.bias.add_(0.1 * torch.randn_like(ln.bias))
        if kind == "long_memory":  # dt ~ 1e-3 with A[:, 0] ~ -1: exp(dt A[0]) ~ 0.999, the state of 147 frames ago is still there at the end
            m.dt_proj.bias.copy_(math.log(math.expm1(1e-3)) + 0.1 * torch.randn_like(m.dt_proj.bias))
        if kind == "softplus":  # pre-activations of both signs far beyond torch's threshold of 20
            m.dt_proj.weight.mul_(600.0)
    x = torch.randn(BF, T_ALL, 96)
    m64, ln64 = copy.deepcopy(m).double(), copy.deepcopy(ln).double()
    with torch.no_grad():
        u = ln64(x.double())
        out = x.double() + m64(u)
        st, states, ys = m64.init_state(BF, dtype=torch.float64), {}, []
        for t in range(T_ALL):
            ys.append(m64.step(u[:, t:t + 1], st))
            states[t + 1] = (st["conv"].clone(), st["ssm"].clone())
        assert rel_l2(x.double() + torch.cat(ys, 1), out) < 1e-10  # the step form IS the whole-sequence form
        xr = m64.in_proj(u)[..., :192]
        xc = Fn.silu(Fn.conv1d(Fn.pad(xr.transpose(1, 2), (3, 0)), m64.conv1d.weight, m64.conv1d.bias, groups=192).transpose(1, 2))
        pre = Fn.linear(Fn.linear(xc, m64.x_proj.weight)[..., :6], m64.dt_proj.weight, m64.dt_proj.bias)
        decay0 = torch.exp(Fn.softplus(pre) * -torch.exp(m64.A_log[:, 0]))
    return {"m": m, "ln": ln, "x": x, "out": out, "states": states, "pre": pre, "decay0": decay0, "xr": xr}


class Block:
    """the entry point on a backend: the module's weights laid out as nbss_amd/online.py lays them out, and the two caller-owned states"""

    def __init__(self, backend, case, rows=slice(None)):
        self.lib, self.dev = backend.lib, backend.device
        m, ln = case["m"], case["ln"]
        dv = lambda t: t.detach().float().contiguous().to(self.dev)  # noqa: E731
        self.w = [dv(t) for t in (ln.weight, ln.bias, m.in_proj.weight.t(), m.conv1d.weight[:, 0], m.conv1d.bias, m.x_proj.weight.t(), m.dt_proj.weight,
                                  m.dt_proj.bias, m.A_log, m.D, m.out_proj.weight.t())]
        self.x = case["x"][rows]
        self.n = self.x.shape[0]
        self.conv, self.ssm = torch.zeros(self.n, 3, 192, device=self.dev), torch.zeros(self.n, 16, 192, device=self.dev)
        self.buf = torch.empty(self.n * 32 * 96, device=self.dev)
        self.st = ops._stream(self.lib, self.buf)

    def f(self, t):
        return ops._ptr(self.lib, t, torch.float32)

    def call(self, t0, C):
        """frames t0 .. t0 + C - 1 in place in a NaN-poisoned buffer -> (output [n, C, 96], conv [n, 192, 3], ssm [n, 192, 16]) on the host"""
        self.buf.view(torch.uint8).fill_(0xFF)
        xc = self.buf[:self.n * C * 96].view(self.n, C, 96)
        xc.copy_(self.x[:, t0:t0 + C])
        self.lib.call("nbss_online_mamba_step", self.n, C, *(self.f(t) for t in self.w), self.f(self.conv), self.f(self.ssm), self.f(xc), self.st)
        assert torch.isnan(self.buf[self.n * C * 96:]).all()  # nothing written behind the chunk
        return xc.cpu().clone(), self.conv.cpu().transpose(1, 2).clone(), self.ssm.cpu().transpose(1, 2).clone()

    def stream(self, part=PART):
        return [self.call(t0, C) for t0, C in _bounds(part)]


def _check_stream(backend, kind):
    case = _case(kind)
    blk = Block(backend, case)
    worst = [0.0, 0.0, 0.0]
    for t0, C in _bounds(PART):
        out, conv, ssm = blk.call(t0, C)
        cref, sref = case["states"][t0 + C]
        e = (rel_l2(out, case["out"][:, t0:t0 + C]), rel_l2(conv, cref), rel_l2(ssm, sref))
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert max(e) <= TOL, (kind, t0, C, e)
    print(f"{backend.name} {kind}: worst rel-L2 over the calls: out {worst[0]:.2e}, conv state {worst[1]:.2e}, ssm state {worst[2]:.2e}")
    return case


def test_step_perturbed_parameters(backend):
    """A_log, D, the conv taps, both 1-D biases and the LayerNorm affine perturbed: output, conv state and h after every one of the eleven calls"""
    _check_stream(backend, "perturbed")


def test_step_long_memory(backend):
    """dt_proj.bias = softplus^-1(1e-3): the slowest state of a channel decays by ~0.999 per frame (asserted on the fp64 reference), so what the earlier
    calls left in ssm_state carries the output of the later ones — a state lost or rounded badly between calls shows at 2e-5"""
    case = _case("long_memory")
    d = case["decay0"]
    assert 0.9985 < float(d.median()) < 0.9995 and float(d.min()) > 0.995, (float(d.median()), float(d.min()))
    _check_stream(backend, "long_memory")


def test_step_both_softplus_branches(backend):
    """dt_proj.weight x 600: a fair share of the pre-activations lies beyond torch's softplus threshold of 20 (there softplus(p) = p), the rest below it —
    both shares asserted on the fp64 reference"""
    case = _case("softplus")
    above = float((case["pre"] > 20).double().mean())
    assert 0.1 < above < 0.9, above
    assert float((case["pre"] < 0).double().mean()) > 0.1
    _check_stream(backend, "softplus")


def test_conv_state_is_a_copy(backend):
    """the conv state holds the kernel's own fp32 in_proj outputs (which a caller cannot see: compared at 2e-5 against fp64), MOVED, never recomputed: after
    a one-frame call its two older rows are, bit for bit, the two newer rows of the state before; rows no frame has reached are still zero; and since a
    frame's in_proj sum does not depend on the chunk it arrives in, calls of 3 + 1 frames leave the very bits of one call of 4"""
    case = _case("perturbed")
    a = Block(backend, case)
    _, c1, _ = a.call(0, 1)  # the partition's first call: one frame on the empty state
    assert not c1[..., :2].any() and c1[..., 2].any()
    assert rel_l2(c1[..., 2], case["xr"][:, 0]) <= TOL
    _, c3, _ = a.call(1, 2)
    assert torch.equal(c3[..., 0], c1[..., 2])
    _, c4, _ = a.call(3, 1)
    assert torch.equal(c4[..., :2], c3[..., 1:])
    assert rel_l2(c4, case["xr"][:, 1:4].transpose(1, 2)) <= TOL
    b = Block(backend, case)
    _, c4b, _ = b.call(0, 4)
    assert torch.equal(c4, c4b)


def test_repeatable_and_batch_invariant(backend):
    """two passes from a zeroed state give the same bits (outputs and both states after every call), and sequence 7 alone (BF = 1) gives the bits of row 7
    of the BF = 15 run: no atomics, no sum whose order depends on the grid"""
    case = _case("perturbed")
    blk = Block(backend, case)
    first = blk.stream()
    blk.conv.zero_(), blk.ssm.zero_()
    again = blk.stream()
    for i, (a, b) in enumerate(zip(first, again)):
        assert all(torch.equal(p, q) for p, q in zip(a, b)), i
    one = Block(backend, case, rows=slice(7, 8)).stream()
    for i, (a, b) in enumerate(zip(first, one)):
        assert all(torch.equal(p[7:8], q) for p, q in zip(a, b)), i


def test_refusals(backend):
    """NBSS_EINVAL for BF or C <= 0 and for a NULL pointer (a state pointer, a weight), NBSS_EUNSUPPORTED for C > 32; none of them launches anything"""
    dev = backend.device
    lib = backend.lib
    # every weight and the chunk are NaN (1 MiB; the largest need is 96 x 384 floats), the two states zeros: a launch would carry NaN into the states
    buf, conv, ssm = torch.full((1 << 18,), float("nan"), device=dev), torch.zeros(3 * 192, device=dev), torch.zeros(16 * 192, device=dev)
    p, cp, sp = (ops._ptr(lib, t, torch.float32) for t in (buf, conv, ssm))
    st = ops._stream(lib, buf)

    def call(BF=1, C=8, conv=cp, ssm=sp, w=p, x=p):
        return lib.nbss_online_mamba_step(BF, C, w, p, p, p, p, p, p, p, p, p, p, conv, ssm, x, st)

    assert call(C=0) == EINVAL and call(BF=0) == EINVAL and call(C=-1) == EINVAL
    assert call(C=33) == EUNSUPPORTED
    assert call(conv=None) == EINVAL and call(ssm=None) == EINVAL and call(w=None) == EINVAL and call(x=None) == EINVAL
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        lib.call("nbss_online_mamba_step", 1, 33, *([p] * 11), cp, sp, p, st)
    with pytest.raises(NbssError, match="EINVAL"):
        lib.call("nbss_online_mamba_step", 1, 0, *([p] * 11), cp, sp, p, st)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert not conv.any() and not ssm.any()  # nothing ran
