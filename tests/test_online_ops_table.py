"""The driver of the online training blocks in nbss_amd/ops.py (one `OnlineBlock` record per block with parameters, `_online_fwd` / `_online_bwd`, the
workspace cache): the arguments it passes are those of the C ABI as nbss_amd/_lib.py declares it, every block refuses a parameter or gradient buffer of the
wrong size before anything is launched, and the cached workspace is one buffer per (library, device, dtype, extra key) that a new shape replaces."""
import ctypes as C
import weakref

import pytest
import torch

from nbss_amd import online_train, ops
from nbss_amd._lib import NBSS_F32, SIGNATURES


class _Spy:
    """stands in for a library: keeps the arguments of every call; a size function answers 256 bytes"""
    _is_emu = True  # (takes CPU tensors)

    def __init__(self):
        self.args = {}

    def call(self, name, *args):
        self.args[name] = args

    def __getattr__(self, name):
        def sizer(*args):
            self.args[name] = args
            return 256
        return sizer


def _named(args, tensors):
    """every argument as the name of the tensor it points at, 'null' for None, 'int' for anything else"""
    names = {t.data_ptr(): n for n, t in tensors.items() if t is not None}
    return ["null" if a is None else names.get(a, "int") for a in args]


def test_the_table_agrees_with_the_abi():
    """what the driver passes to the four symbols of every record: the integers and pointers the symbol's argtypes list, in number and kind, and every tensor
    in the slot the record and the header's common order (inputs, then save, dy, dx, the gradients, ws, stream) give it"""
    records = [v for v in vars(ops).values() if isinstance(v, ops.OnlineBlock)]
    assert len(records) == 4
    for rec in records:
        spy = _Spy()
        params = [None if i in rec.optional else torch.zeros(n) for i, n in enumerate(rec.sizes(2))]
        x, ws = torch.zeros(*((1, 2, 3) if rec.ranks == (4,) else (1, 2)), rec.width), torch.zeros(256, dtype=torch.uint8)
        ops._online_fwd(rec, spy, params, x)  # (sizes its own workspace: the call of ws_bytes)
        y, save = ops._online_fwd(rec, spy, params, x, ws=ws)
        dy = torch.zeros_like(y)
        dx, grads = ops._online_bwd(rec, spy, params, x, save, dy, ws=ws)
        assert set(spy.args) == {rec.fwd, rec.bwd, rec.save_bytes, rec.ws_bytes}
        tensors = {"x": x, "y": y, "save": save, "dy": dy, "dx": dx, "ws": ws, **{f"p{i}": p for i, p in enumerate(params)},
                   **{f"g{i}": g for i, g in enumerate(grads)}}
        lead = ["int"] * (4 if rec.ranks == (4,) else 3)
        ps = ["null" if p is None else f"p{i}" for i, p in enumerate(params)]
        ins = ["x"] + ps if rec.x_first else ps + ["x"]
        gs = ["null" if p is None else f"g{i}" for i, p in enumerate(params)][:len(params) - rec.consts]
        want = {rec.fwd: lead + ins + ["y", "save", "ws", "null"], rec.bwd: lead + ins + ["save", "dy", "dx"] + gs + ["ws", "null"],
                rec.save_bytes: lead + ["int"] * len(rec.size_extra(params)), rec.ws_bytes: lead + ["int"] * len(rec.size_extra(params))}
        for name, args in spy.args.items():
            got = _named(args, tensors)
            assert got == want[name], (rec.what, name)
            assert [g == "int" for g in got] == [t is not C.c_void_p for t in SIGNATURES[name][1]], (rec.what, name)


def _valid(which, device):
    """(fwd, bwd, params, x) of the smallest valid call of a block, the parameters taken from the torch modules"""
    torch.manual_seed(0)
    if which == "mamba":
        from models.arch.base.mamba import Mamba
        params = online_train.mamba_params(Mamba(d_model=96, d_state=16, d_conv=4, layer_idx=0))
        params = [p.to(device) for p in online_train._kernel_params(params)]
        return ops.online_mamba_train_fwd, ops.online_mamba_train_bwd, params, torch.randn(1, 2, 384, device=device)
    from models.arch.OnlineSpatialNet import SpatialNetLayer
    layer = SpatialNetLayer(dim_hidden=96, dim_ffn=192, dim_squeeze=8, num_freqs=2, num_heads=4, attention="ret(2,share_qk)")
    if which == "tsa":
        params = online_train.tsa_params(layer, (None, ("chunk", 64, torch.tensor([0.9, 0.8, 0.7, 0.6]))))
        x = torch.randn(1, 2, 96, device=device)
    else:
        params, x = getattr(online_train, which + "_params")(layer), torch.randn(1, 2, 3, 96, device=device)
    params = [None if p is None else p.to(device) for p in online_train._kernel_params(params)]
    return getattr(ops, f"online_{which}_train_fwd"), getattr(ops, f"online_{which}_train_bwd"), params, x


def _short(t):
    return t.reshape(-1)[:-1].contiguous()


@pytest.mark.parametrize("which", ["tconvffn", "xband", "tsa", "mamba"])
def test_size_refusals_are_uniform(backend, which):
    """a parameter with one element too few is refused by the forward, a gradient buffer with one element too few by the backward: every slot in turn"""
    fwd, bwd, params, x = _valid(which, backend.device)
    y, save = fwd(backend.lib, params, x)
    dy = torch.randn_like(y)
    dx, grads = bwd(backend.lib, params, x, save, dy)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all() and len(grads) == len(params)
    for i, p in enumerate(params):
        if p is not None:
            with pytest.raises(ops.NbssError):
                fwd(backend.lib, [_short(q) if j == i else q for j, q in enumerate(params)], x)
    for i, g in enumerate(grads):
        if g is not None:
            with pytest.raises(ops.NbssError):
                bwd(backend.lib, params, x, save, dy, [_short(h) if j == i else h for j, h in enumerate(grads)])


def test_workspace_cache(backend):
    lib, dev = backend.lib, backend.device

    def xband(T, dtype=torch.float32):
        return ops.online_xband_ws(lib, torch.empty(1, 2, T, 96, dtype=dtype, device=dev))

    def tsa(T, share=0):
        return ops.online_tsa_ws(lib, NBSS_F32, 2, T, share, dev)

    for ws in (xband, tsa):
        a = ws(3)
        assert ws(3) is a
        other = ws(3, torch.bfloat16) if ws is xband else ws(3, 1)  # another dtype, the other key form: a buffer of its own, side by side
        assert other is not a and ws(3) is a
        gone = weakref.ref(a)
        del a
        b = ws(4)
        assert gone() is None  # the new shape took the slot: nothing holds the first buffer
        assert ws(4) is b and (ws(3, torch.bfloat16) if ws is xband else ws(3, 1)) is other
        assert ws(3) is not b
