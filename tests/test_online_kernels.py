"""The five entry points of csrc/online.hip (the native OnlineSpatialNet streaming step) one by one, through the C ABI, against plain fp64 torch
written here: nbss_online_encoder_step, nbss_online_ret_step, nbss_online_mhsa_step, nbss_online_advance, nbss_online_tconvffn_step.

Every kernel is driven over ONE stream cut into an irregular partition of chunk sizes (PART: 1, 25 and 32 — from 25 frames on the dynamic LDS of
online_ret_kernel, (672 C + 192) * 4 bytes, passes 64 KiB — two equal neighbours, sizes that are no multiple of the 8-frame register tile), the state
persisting across the calls; every chunk's output AND the state after every call are compared with the reference of the whole stream.
Tolerance: rel-L2 <= 2e-5, the project's bound for an fp32 kernel against fp64 (tests/util.py: Case.tol).  Weights are random fp32 with the
1-D parameters perturbed (tests/test_online.py: _native_net) and transposed as nbss_amd/online.py transposes them.  Scratch (a3, gn_sums) and the
output buffers are NaN bytes before every call."""
import copy
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
EINVAL, EUNSUPPORTED = -1, -2


# ---- thin helpers around the C ABI -------------------------------------------------------------------------------------------------------------
class K:
    def __init__(self, backend):
        self.lib, self.dev = backend.lib, backend.device
        self.st = ops._stream(self.lib, torch.zeros(1, device=self.dev))

    def f(self, t):
        return ops._ptr(self.lib, t, torch.float32)

    def i(self, t):
        return ops._ptr(self.lib, t, torch.int32)

    def dv(self, t):
        return t.detach().float().contiguous().to(self.dev)

    def zeros(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device=self.dev)

    def poisoned(self, *shape):
        return ops.scratch(4 * math.prod(shape), self.dev).view(torch.float32).view(*shape)


def _poison(*ts):
    for t in ts:
        t.view(torch.uint8).fill_(0xFF)


def _perturb(*mods):
    with torch.no_grad():
        for m in mods:
            for p in m.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))


def _chunks(part=PART):
    t0 = 0
    for C in part:
        yield t0, C
        t0 += C


def _layer(F, attention="ret(2,share_qk)"):
    from models.arch.OnlineSpatialNet import SpatialNetLayer
    layer = SpatialNetLayer(dim_hidden=96, dim_ffn=192, dim_squeeze=8, num_freqs=F, num_heads=4, attention=attention).eval()
    _perturb(layer)
    return layer


# ---- encoder -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_in", [1, 4, 12, 32])
def test_encoder_step(backend, C_in):
    """causal Conv1d(C_in -> 96, k = 5): every chunk against the fp64 convolution of the whole stream; the state is a copy, so it EQUALS the last
    four input frames (zeros before the start) — also after a one-frame call, where three of its four rows come from the old state"""
    from models.arch.OnlineSpatialNet import CausalConv1d
    torch.manual_seed(100 + C_in)
    conv = CausalConv1d(C_in, 96, kernel_size=5)
    _perturb(conv)
    BF = 15
    x = torch.randn(BF, T_ALL, C_in)
    with torch.no_grad():
        want = copy.deepcopy(conv).double()(x.double().transpose(1, 2)).transpose(1, 2)
    xpad = torch.cat([torch.zeros(BF, 4, C_in), x], 1)
    k = K(backend)
    w, b, state, y = k.dv(conv.weight), k.dv(conv.bias), k.zeros(BF, 4, C_in), k.poisoned(BF, 32, 96)
    for t0, C in _chunks():
        xc, yc = k.dv(x[:, t0:t0 + C]), y.view(-1)[:BF * C * 96].view(BF, C, 96)
        _poison(y)
        k.lib.call("nbss_online_encoder_step", BF, C, C_in, k.f(w), k.f(b), k.f(xc), k.f(state), k.f(yc), k.st)
        e = rel_l2(yc, want[:, t0:t0 + C])
        assert e <= TOL, (t0, C, e)
        assert torch.equal(state.cpu(), xpad[:, t0 + C:t0 + C + 4]), (t0, C)


# ---- retention ---------------------------------------------------------------------------------------------------------------------------------
def _retention_ref(ln, m, gamma, x, bounds):
    """x + out_proj(SiLU(g) * RMSNorm_head(recurrent retention(q, k, v))) of LayerNorm(x) in fp64, written out (base/retention.py: forward +
    recurrent_forward).  The state is kept in the module's — and the kernel's (online.hip: `carry`, `inv`) — normalisation:
        scale_t = gamma scale_{t-1} + 1 = sum_{i <= t} gamma^i,     kv_t = kv_{t-1} sqrt(scale_{t-1}) gamma / sqrt(scale_t) + k_t^T v_t / sqrt(scale_t),
    i.e. kv_t sqrt(scale_t) = S_t = gamma S_{t-1} + k_t^T v_t, the plain recurrent state; scale_{-1} = 0, kv_{-1} = 0 is the empty stream (the first
    frame then gets carry 0 and divisor 1, the module's `scale = 1` branch).  Returns the output [N, T, 96] and {t: (kv [N,4,24,48], scale [4])} after
    the frames `bounds`."""
    x = x.double()
    N, T, _ = x.shape
    W = lambda lin: lin.weight.detach().double()  # noqa: E731
    u = Fn.layer_norm(x, (96,), ln.weight.detach().double(), ln.bias.detach().double(), ln.eps)
    q = (u @ W(m.q_proj).T).view(N, T, 4, 24)
    kk = q if m.k_proj is None else ((u @ W(m.k_proj).T) * 24 ** -0.5).view(N, T, 4, 24)
    v, g = (u @ W(m.v_proj).T).view(N, T, 4, 48), u @ W(m.g_proj).T
    gam = gamma.double().view(1, 4, 1, 1)
    kv, scale = torch.zeros(N, 4, 24, 48, dtype=torch.float64), torch.zeros(1, 4, 1, 1, dtype=torch.float64)
    o, states = torch.empty(N, T, 4, 48, dtype=torch.float64), {}
    for t in range(T):
        new = scale * gam + 1
        kv = kv * (scale.sqrt() * gam / new.sqrt()) + kk[:, t, :, :, None] * v[:, t, :, None, :] / new.sqrt()
        scale = new
        o[:, t] = (q[:, t, :, None, :] @ kv)[:, :, 0]
        if t + 1 in bounds:
            states[t + 1] = (kv.clone(), scale.reshape(4).clone())
    o = o * torch.rsqrt(o.pow(2).mean(-1, keepdim=True) + 1e-6)
    return x + (Fn.silu(g) * o.reshape(N, T, 192)) @ W(m.out_proj).T, states


def _retention_parts(share, seed):
    from models.arch.base.retention import MultiScaleRetention, RetNetRelPos
    torch.manual_seed(seed)
    m, ln = MultiScaleRetention(96, 4, value_factor=2, share_qk=share).eval(), torch.nn.LayerNorm(96)
    _perturb(ln)
    pos = RetNetRelPos(96, 4, recurrent_chunk_size=64, decay=[4, 5, 9, 10])
    return m, ln, pos


@pytest.mark.parametrize("share", [True, False])
def test_retention_reference_is_the_modules_recurrent_form(share):
    """the written-out reference above == MultiScaleRetention in .double(), frame by frame with its incremental state (output to 1e-6: the module's
    RMSNorm passes through fp32; the state to 1e-12)"""
    m, ln, pos = _retention_parts(share, 7)
    x = torch.randn(3, 20, 96)
    m64, ln64, pos64 = copy.deepcopy(m).double(), copy.deepcopy(ln).double(), copy.deepcopy(pos).double()
    got, states = _retention_ref(ln, m, pos64.decay.exp(), x, {20})
    with torch.no_grad():
        u, st = ln64(x.double()), {}
        y = torch.cat([m64(u[:, t:t + 1], rel_pos=pos64(slen=t + 1, activate_recurrent=True), incremental_state=st, rope=False) for t in range(20)], 1)
    assert rel_l2(got, x.double() + y) < 1e-6
    assert rel_l2(states[20][0], st["prev_key_value"]) < 1e-12 and rel_l2(states[20][1], st["scale"]) < 1e-12


def _run_retention(backend, share, BF, part, seed):
    m, ln, pos = _retention_parts(share, seed)
    T = sum(part)
    x = torch.randn(BF, T, 96)
    gamma = pos.decay.detach().float().exp()  # what nbss_amd/online.py hands to the kernel: the reference takes the same fp32 values
    bounds = {t0 + C for t0, C in _chunks(part)}
    want, states = _retention_ref(ln, m, gamma, x, bounds)
    k = K(backend)
    lw, lb, wq, wv, wg, wo = (k.dv(t) for t in (ln.weight, ln.bias, m.q_proj.weight.t(), m.v_proj.weight.t(), m.g_proj.weight.t(), m.out_proj.weight.t()))
    wk = None if share else k.dv(m.k_proj.weight.t())
    dec, kv, scale = k.dv(gamma), k.zeros(BF, 4, 24, 48), k.zeros(BF, 4)
    worst = 0.0
    for t0, C in _chunks(part):
        xc = k.dv(x[:, t0:t0 + C])
        k.lib.call("nbss_online_ret_step", BF, C, k.f(lw), k.f(lb), k.f(wq), k.f(wk) if wk is not None else None, k.f(wv), k.f(wg), k.f(wo), k.f(dec),
                   k.f(kv), k.f(scale), k.f(xc), k.st)
        kv_ref, scale_ref = states[t0 + C]
        e = (rel_l2(xc, want[:, t0:t0 + C]), rel_l2(kv, kv_ref), rel_l2(scale[0], scale_ref))
        worst = max(worst, *e)
        assert max(e) <= TOL, (t0, C, e)
        assert torch.equal(scale, scale[:1].expand_as(scale)), (t0, C)  # one copy per sequence, all the same
    return worst


@pytest.mark.parametrize("share", [True, False], ids=["share_qk", "own_k"])
def test_retention_step(backend, share):
    """wk_t = NULL (k = q) and a separate k projection (scaled by 24^-1/2), decays 1 - 2^-(4, 5, 9, 10): output, kv and scale after every call"""
    _run_retention(backend, share, BF=15, part=PART, seed=21 + share)


def test_retention_step_long_stream(backend):
    """544 frames in 32-frame calls (one short call in the middle): drift of the carried fp32 state (the slowest head forgets over 1024 frames) would
    show at the same tolerance"""
    _run_retention(backend, True, BF=2, part=[32] * 8 + [1] + [32] * 8 + [31], seed=23)


# ---- windowed attention ------------------------------------------------------------------------------------------------------------------------
def attention_ref(u, mha, scope, block=64):
    """causal windowed multi-head attention of the (already normalised) sequences u [N, T, E] in fp64, written out:
    out_proj(softmax(q k^T / sqrt(dh) + window mask) v) with a BOOL window (key j is visible to query i iff 0 <= i - j < scope).
    Returns (output [N, T, E], k [N, T, E], v [N, T, E]); evaluated in blocks of queries against the keys their windows reach."""
    u = u.double()
    N, T, E = u.shape
    nh = mha.num_heads
    dh = E // nh
    q, k, v = Fn.linear(u, mha.in_proj_weight.detach().double(), mha.in_proj_bias.detach().double()).chunk(3, -1)
    heads = lambda z: z.reshape(N, -1, nh, dh).transpose(1, 2)  # noqa: E731
    o = torch.empty(N, T, E, dtype=torch.float64)
    for q0 in range(0, T, block):
        q1, k0 = min(T, q0 + block), max(0, q0 - scope + 1)
        s = heads(q[:, q0:q1]) @ heads(k[:, k0:q1]).transpose(-1, -2) / math.sqrt(dh)
        rel = torch.arange(q0, q1)[:, None] - torch.arange(k0, q1)[None, :]
        p = torch.softmax(s.masked_fill(~((rel >= 0) & (rel < scope)), -torch.inf), -1)
        o[:, q0:q1] = (p @ heads(v[:, k0:q1])).transpose(1, 2).reshape(N, q1 - q0, E)
    return Fn.linear(o, mha.out_proj.weight.detach().double(), mha.out_proj.bias.detach().double()), k, v


def test_mhsa_module_in_double_uses_its_window():
    """OnlineSpatialNet in .double(): the additive window mask has the module's dtype (an fp32 mask on fp64 queries is silently mis-applied by
    nn.MultiheadAttention) — a layer's attention equals the written-out fp64 attention to 1e-10, the fp64 net its fp32 self to 1e-5"""
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    torch.manual_seed(5)
    net = OnlineSpatialNet(dim_input=4, dim_output=4, num_layers=2, dim_squeeze=8, num_freqs=9, dim_hidden=96, dim_ffn=192, num_heads=4, attention="mhsa(3)").eval()
    _perturb(net)
    x = torch.randn(2, 9, 20, 4)
    net64 = copy.deepcopy(net).double()
    mask = net64.get_causal_mask(slen=20, device=x.device)
    assert mask.dtype == torch.float64 and net.get_causal_mask(slen=20).dtype == torch.float32
    layer = net64.layers[0]
    h = torch.randn(2, 9, 20, 96, dtype=torch.float64)
    with torch.no_grad():
        got, _ = layer._tsa(h, mask, True)
        want, _, _ = attention_ref(layer.norm_mhsa(h).reshape(18, 20, 96), layer.mhsa, 3)
        assert rel_l2(got.reshape(18, 20, 96), want) < 1e-10
        assert rel_l2(net(x), net64(x.double())) < 1e-5


class _AttnLayer:
    """one layer's windowed attention on a backend: weights, its K / V rings, and the fp64 reference of a whole stream"""

    def __init__(self, k, x, scope, ring):
        self.k, self.scope, self.ring, BF = k, scope, ring, x.shape[0]
        self.mha, self.ln = torch.nn.MultiheadAttention(96, 4, batch_first=True).eval(), torch.nn.LayerNorm(96)
        _perturb(self.mha, self.ln)
        u = Fn.layer_norm(x.double(), (96,), self.ln.weight.detach().double(), self.ln.bias.detach().double(), self.ln.eps)
        a, self.kref, self.vref = attention_ref(u, self.mha, scope)
        self.want = x.double() + a
        self.w = [k.dv(t) for t in (self.ln.weight, self.ln.bias, self.mha.in_proj_weight.t(), self.mha.in_proj_bias, self.mha.out_proj.weight.t(),
                                    self.mha.out_proj.bias)]
        self.kring, self.vring = k.zeros(BF, ring, 96), k.zeros(BF, ring, 96)

    def step(self, x, t0, C, pos):
        """one call on frames t0 .. t0 + C - 1 (pos holds t0): the chunk's output, then the rings"""
        k, BF = self.k, x.shape[0]
        xc = k.dv(x[:, t0:t0 + C])
        k.lib.call("nbss_online_mhsa_step", BF, C, self.scope, self.ring, *(k.f(t) for t in self.w), k.f(self.kring), k.f(self.vring), k.i(pos), k.f(xc), k.st)
        e = rel_l2(xc, self.want[:, t0:t0 + C])
        assert e <= TOL, (t0, C, e)
        # slot t mod ring holds frame t, for the window before the chunk and the chunk itself; slots no frame has reached yet are still zero
        frames = torch.arange(max(0, t0 - (self.scope - 1)), t0 + C)
        for ring, ref in ((self.kring, self.kref), (self.vring, self.vref)):
            ring = ring.cpu()
            e = rel_l2(ring[:, frames % self.ring], ref[:, frames])
            assert e <= TOL, (t0, C, e)
            if t0 + C < self.ring:
                assert not ring[:, t0 + C:].any(), (t0, C)


@pytest.mark.parametrize("extra", [0, 5], ids=["minimal_ring", "ring_plus_5"])
@pytest.mark.parametrize("scope", [1, 3, 11, 40])
def test_mhsa_step(backend, scope, extra):
    """windows of 1 frame, 3 (< C), 11 and 40 frames over a ring of scope - 1 + max C (+ 5) slots, the chunk size changing from call to call; two
    'layers' read the same frame counter in every step and one nbss_online_advance then adds exactly C to it"""
    torch.manual_seed(300 + scope)
    BF = 6
    x = torch.randn(BF, T_ALL, 96)
    k = K(backend)
    layers = [_AttnLayer(k, x, scope, scope - 1 + max(PART) + extra) for _ in range(2)]
    pos = k.zeros(1, dtype=torch.int32)
    for t0, C in _chunks():
        for layer in layers:
            layer.step(x, t0, C, pos)
            assert int(pos) == t0  # the kernel only reads it
        k.lib.call("nbss_online_advance", k.i(pos), C, k.st)
        assert int(pos) == t0 + C


@pytest.mark.parametrize("backend", [pytest.param("emu", id="emu", marks=pytest.mark.slow), pytest.param("hip", id="hip", marks=pytest.mark.gpu)], indirect=True)
def test_mhsa_step_large_window(backend):
    """scope 2600 at C = 32: (2 * 32 * 96 + 4 * 2631 + 8) * 4 = 66 704 bytes of dynamic LDS, the one run of online_mhsa_kernel above 64 KiB — 90 calls,
    2880 frames: the window fills (frame 2599) and the ring wraps (frame 2631)"""
    torch.manual_seed(41)
    BF, C, scope, calls = 2, 32, 2600, 90
    x = torch.randn(BF, C * calls, 96)
    k = K(backend)
    layer = _AttnLayer(k, x, scope, scope - 1 + C)
    pos = k.zeros(1, dtype=torch.int32)
    for t0, _ in _chunks([C] * calls):
        layer.step(x, t0, C, pos)
        k.lib.call("nbss_online_advance", k.i(pos), C, k.st)
    assert int(pos) == C * calls


# ---- T-ConvFFN ---------------------------------------------------------------------------------------------------------------------------------
def _tconv_ref(layer, x, dtype):
    """the module's own _tconvffn on the whole stream x [B, F, T, 96] in `dtype`: x + T-ConvFFN(x), the inputs of the three causal convs
    (-> s1, s2, s3), and the pre-GroupNorm activation a3 [B*F, 192, T]"""
    from models.arch.OnlineSpatialNet import CausalConv1d
    layer = copy.deepcopy(layer).to(dtype)
    seen, hooks = {"conv_in": []}, []
    for m in layer.tconvffn:
        if isinstance(m, CausalConv1d):
            hooks.append(m.register_forward_pre_hook(lambda mod, args: seen["conv_in"].append(args[0].detach())))
        elif "GroupNorm" in type(m).__name__:
            hooks.append(m.register_forward_pre_hook(lambda mod, args: seen.__setitem__("gn_in", args[0].detach())))
    with torch.no_grad():
        out = x.to(dtype) + layer._tconvffn(x.to(dtype))
    for h in hooks:
        h.remove()
    B, F, T, _ = x.shape
    r = {"out": out.reshape(B * F, T, 96), "gn_in": seen["gn_in"]}  # gn_in [B*T, 192, F]
    for name, h in zip(("s1", "s2", "s3"), seen["conv_in"]):  # [B*F, 192, T] -> frames -2 .. T-1, time-major
        r[name] = torch.cat([torch.zeros(B * F, 2, 192, dtype=dtype), h.transpose(1, 2)], 1)
    return r


def _run_tconvffn(backend, layer, x, bound):
    """the kernel over the stream x [B, F, T, 96] in PART's chunks; `bound`: {quantity: rel-L2 bound}.  Returns the worst error per quantity."""
    B, F, T, _ = x.shape
    BF = B * F
    want = _tconv_ref(layer, x, torch.float64)
    k, tc = K(backend), layer.tconvffn
    w = [k.dv(t) for t in (tc[0].weight, tc[0].bias, tc[1].weight[:, :, 0].t(), tc[1].bias, tc[3].weight, tc[3].bias, tc[5].weight, tc[5].bias,
                           tc[6].weight, tc[6].bias, tc[8].weight, tc[8].bias, tc[10].weight[:, :, 0].t(), tc[10].bias)]
    s = {n: k.zeros(BF, 2, 192) for n in ("s1", "s2", "s3")}
    a3, gn_sums = k.poisoned(BF, 32, 192), k.poisoned(B + BF, 32, 8, 2)
    xs = x.reshape(BF, T, 96)
    worst = {n: 0.0 for n in bound}
    for t0, C in _chunks():
        xc = k.dv(xs[:, t0:t0 + C])
        _poison(a3, gn_sums)
        k.lib.call("nbss_online_tconvffn_step", B, F, C, *(k.f(t) for t in w), k.f(s["s1"]), k.f(s["s2"]), k.f(s["s3"]), k.f(a3), k.f(gn_sums), k.f(xc), k.st)
        e = {"out": rel_l2(xc, want["out"][:, t0:t0 + C])}
        e.update({n: rel_l2(s[n], want[n][:, t0 + C:t0 + C + 2]) for n in s})  # rows t0 + C - 2, t0 + C - 1 of the stream (+ 2 rows of padding)
        for n, v in e.items():
            worst[n] = max(worst[n], v)
            assert v <= bound[n], (t0, C, n, v, bound[n])
    return worst


def _tconv_input(B, F):
    """a different level per batch item and channel (LayerNorm removes a per-frame constant, not this): the items' GroupNorm statistics differ, so
    statistics leaking from one item into another would show"""
    return torch.randn(B, F, T_ALL, 96) + 1.5 * torch.arange(B).view(B, 1, 1, 1) * torch.randn(B, 1, 1, 96)


@pytest.mark.parametrize("B,F", [(3, 5), (2, 1)])
def test_tconvffn_step(backend, B, F):
    """output and s1 / s2 / s3 (the last two input frames of the three convs) after every call"""
    torch.manual_seed(500 + F)
    _run_tconvffn(backend, _layer(F), _tconv_input(B, F), {n: TOL for n in ("out", "s1", "s2", "s3")})


def test_tconvffn_step_shifted_groupnorm(backend):
    """GroupNorm input with |mean| / std ~ 100 (a per-group constant on the bias of the second causal conv): the statistics must not be formed as
    E[a^2] - mean^2 from fp32 sums.  Bound per quantity: max(2e-5, 4 e_ref), e_ref = the error of the torch fp32 module's own _tconvffn against
    fp64 on the same inputs (the factor 4: __expf in SiLU, another summation order).

    Measured (B = 3, F = 5, 147 frames, |mean| / std: median 99.9, minimum 86.5; rel-L2 against fp64, the worst chunk for the kernel):
                                                           out        s3 (= SiLU(GroupNorm(..)), the input of the third conv)
        e_ref (torch fp32 module, whole stream)            2.8e-7     6.2e-6      -> bounds 2e-5 / 2.5e-5
        kernel with E[a^2] - mean^2 (emulator)             4.0e-5     9.9e-4      (MI355X: fails at the first chunk, out 2.8e-5)
        kernel with (mean, M2) from deviations (emulator)  1.5e-7     3.6e-6      (MI355X: 1.5e-7 / 3.6e-6)
    (the conv that feeds the GroupNorm also adds its bias last: starting the 72-term sum at a bias of 100 std alone left s3 at 2.0e-5)"""
    torch.manual_seed(505)
    B, F = 3, 5
    layer, x = _layer(F), _tconv_input(B, F)
    a = _tconv_ref(layer, x, torch.float64)["gn_in"].reshape(B * T_ALL, 8, 24 * F)
    with torch.no_grad():  # per group: 100 x the typical standard deviation of a frame's group, alternating in sign
        shift = 100.0 * a.std(-1, unbiased=False).mean(0) * torch.tensor([1.0, -1.0] * 4, dtype=torch.float64)
        layer.tconvffn[5].bias.add_(shift.float().repeat_interleave(24))
    ref64, ref32 = _tconv_ref(layer, x, torch.float64), _tconv_ref(layer, x, torch.float32)
    g = ref64["gn_in"].reshape(B * T_ALL, 8, 24 * F)
    ratio = (g.mean(-1).abs() / g.std(-1, unbiased=False))
    assert float(ratio.min()) >= 50, float(ratio.min())  # every (item, frame, group): the case cannot go soft
    e_ref = {n: rel_l2(ref32[n], ref64[n]) for n in ("out", "s1", "s2", "s3")}
    bound = {n: max(TOL, 4 * e_ref[n]) for n in e_ref}
    worst = _run_tconvffn(backend, layer, x, bound)
    print(f"shifted GroupNorm: |mean|/std median {float(ratio.median()):.1f} min {float(ratio.min()):.1f}; e_ref {e_ref}; kernel {worst}")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(backend):
    """bad arguments are refused before anything is launched: NBSS_EINVAL for C outside 1..32, C_in outside 1..32, scope 0, a ring one slot short, a
    NULL required pointer; NBSS_EUNSUPPORTED for a ring whose LDS need exceeds 160 KiB; through Lib.call they raise NbssError"""
    k = K(backend)
    lib, st = k.lib, k.st
    buf = k.zeros(1 << 21)  # 8 MiB of zeros: every pointer argument of the calls below, none of which may launch
    p, ip = k.f(buf), k.i(k.zeros(1, dtype=torch.int32))
    enc = lambda C=8, C_in=4, w=p: lib.nbss_online_encoder_step(1, C, C_in, w, p, p, p, p, st)  # noqa: E731
    ret = lambda C=8, dec=p: lib.nbss_online_ret_step(1, C, p, p, p, None, p, p, p, dec, p, p, p, st)  # noqa: E731
    att = lambda C=8, scope=11, ring=18, pos=ip: lib.nbss_online_mhsa_step(1, C, scope, ring, p, p, p, p, p, p, p, p, pos, p, st)  # noqa: E731
    ffn = lambda C=8, gn=p: lib.nbss_online_tconvffn_step(1, 1, C, *([p] * 18), gn, p, st)  # noqa: E731
    for C in (0, 33):
        assert enc(C=C) == EINVAL and ret(C=C) == EINVAL and att(C=C, ring=64) == EINVAL and ffn(C=C) == EINVAL, C
    assert enc(C_in=33) == EINVAL and enc(C_in=0) == EINVAL
    assert att(scope=0) == EINVAL
    assert att(C=8, scope=11, ring=11 - 2 + 8) == EINVAL
    assert enc(w=None) == EINVAL and ret(dec=None) == EINVAL and att(pos=None) == EINVAL and ffn(gn=None) == EINVAL
    assert lib.nbss_online_advance(None, 8, st) == EINVAL and lib.nbss_online_advance(ip, 0, st) == EINVAL
    # (2 * 8 * 96 + 4 * 10307 + 8) * 4 = 171 088 bytes > 160 KiB; one slot less than this ring would be EINVAL, not EUNSUPPORTED
    assert att(C=8, scope=10300, ring=10307) == EUNSUPPORTED
    with pytest.raises(NbssError, match="EINVAL"):
        lib.call("nbss_online_encoder_step", 1, 33, 4, p, p, p, p, p, st)
    with pytest.raises(NbssError, match="EUNSUPPORTED"):
        lib.call("nbss_online_mhsa_step", 1, 8, 10300, 10307, p, p, p, p, p, p, p, p, ip, p, st)
    assert not buf.any()  # nothing ran
