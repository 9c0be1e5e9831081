"""Records the sequence of `lib.call(...)` launches of one step of the native streamers (nbss_amd/online.py: NativeOnlineStreamer.step, nbss_amd/online_io.py:
NativeWaveStreamer.push) at small seeded geometries -> tests/golden/online_call_trace.json, the fixture of tests/test_online_call_trace.py: what is launched,
in which order, with which integers and WHICH tensor in every pointer slot.  Only the public surface is used (constructor with `lib=` and `use_graph=False`,
one step / push), so the same script runs on any commit; the committed fixture comes from the commit named in its "parent" field, on the host emulator.

One record = [symbol, arg, arg, ...]: integers and floats by value, the nbss_cfg passed by reference as "cfg", null for a None pointer, and every other
pointer as [shape, dtype, digest, ordinal]: before the step every tensor reachable from the streamer object (attributes, lists, tuples, dicts, recursively;
modules are not entered) is mapped from its data_ptr() to its shape, dtype and the first 12 hex digits of the SHA-256 of its bytes (taken from a host copy,
so one fixture serves the emulator and the device); `ordinal` counts the distinct pointers of the trace in the order of their first appearance.  The weights
are random, so the digest pins which weight sits in which slot; state and scratch are all zeros, so shape and ordinal pin them.  A pointer that resolves to
no tensor is recorded as "unresolved" (the test fails on it).  The trailing stream argument of every entry point is left out: it is None on the emulator
and a stream handle on the device.

usage: python tests/golden/make_online_call_trace.py <commit hash of the tree it runs in>"""
import ctypes as C
import hashlib
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

OUT = Path(__file__).resolve().parent / "online_call_trace.json"
SWITCHES = {"NBSS_ONLINE_NATIVE_MAMBA_STEP": "1", "NBSS_ONLINE_MAMBA": "1"}  # what the 'mamba(..)' cases run with

# the 2-layer, 9-frequency, 4 -> 4 net of tests/test_online.py (NATIVE_KW) and the 1-layer, 129-frequency one of tests/test_online_wave.py (_module)
NET_KW = dict(dim_input=4, dim_output=4, num_layers=2, dim_squeeze=8, num_freqs=9, encoder_kernel_size=5, dim_hidden=96, dim_ffn=192, num_heads=4,
              dropout=(0, 0, 0), kernel_size=(5, 3), conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], full_share=0, decay=[4, 5, 9, 10], rope=False)
WAVE_KW = dict(num_layers=1, num_freqs=129)
CASES = [("step", a) for a in ("ret(2)", "ret(2,not_share_qk)", "mhsa(7)", "mamba(16,4)", "mamba(16,4,not_replace_ffn)")] + \
        [("wave", a) for a in ("ret(2)", "mamba(16,4)")]


def tensors_of(obj, found=None, top=True):
    """data_ptr -> [shape, dtype, digest] of every tensor reachable from `obj` through attributes (of `obj` itself), lists, tuples and dicts"""
    found = {} if found is None else found
    if isinstance(obj, torch.Tensor):
        if obj.numel():
            host = obj.detach().cpu().contiguous()
            digest = hashlib.sha256(host.view(torch.uint8).numpy().tobytes()).hexdigest()[:12]
            found.setdefault(obj.data_ptr(), [list(obj.shape), str(obj.dtype).replace("torch.", ""), digest])
    elif isinstance(obj, dict):
        for v in obj.values():
            tensors_of(v, found, False)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            tensors_of(v, found, False)
    elif top:
        tensors_of(vars(obj), found, False)
    return found


class RecordingLib:
    """forwards everything to the library it wraps and records each `call` made after `arm(tensors)`"""

    def __init__(self, lib):
        self._lib, self.records, self.tensors, self.ordinal = lib, [], None, {}

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def arm(self, tensors):
        self.tensors = tensors

    def call(self, name, *args):
        if self.tensors is not None:
            from nbss_amd._lib import SIGNATURES
            types = SIGNATURES[name][1]
            assert len(types) == len(args) and types[-1] is C.c_void_p, name  # (the last argument of every launching entry point is the stream)
            rec = [name]
            for ty, a in zip(types[:-1], args[:-1]):
                if ty is C.c_void_p:
                    if a is None:
                        rec.append(None)
                    else:
                        rec.append(self.tensors.get(a, ["unresolved"]) + [self.ordinal.setdefault(a, len(self.ordinal))])
                elif ty is C.c_float:
                    rec.append(C.c_float(a.value if isinstance(a, C.c_float) else a).value)
                elif ty in (C.c_int, C.c_int64):
                    rec.append(int(a))
                else:
                    rec.append("cfg")
            self.records.append(rec)
        return self._lib.call(name, *args)


def _net(attention, **over):
    """seeded, with the 1-D parameters perturbed as tests/test_online_mamba_stream.py: _net does (norm weights / biases away from 1 / 0).  Mamba
    initialises A_log and dt_proj.bias through log / exp, whose last bit depends on the host's vector math library: they are drawn again as uniform
    numbers of the same range (exact arithmetic), or the digests would hold on the recording machine only."""
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    torch.manual_seed(5)
    net = OnlineSpatialNet(**{**NET_KW, "attention": attention, **over}).eval()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("A_log"):
                p.copy_(2.75 * torch.rand_like(p))  # log(1 .. 16)
            elif name.endswith("dt_proj.bias"):
                p.copy_(-6.9 + 4.6 * torch.rand_like(p))  # softplus^-1 of dt in 1e-3 .. 1e-1
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return net


def trace(lib, device, kind, attention):
    """the records of one step: `kind` "step" = NativeOnlineStreamer(batch 2, chunk 4).step, "wave" = NativeWaveStreamer(batch 1, chunk 4, n_fft 256).push"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ.update(SWITCHES)
    try:
        rec = RecordingLib(lib)
        g = torch.Generator().manual_seed(12)
        if kind == "step":
            from nbss_amd.online import NativeOnlineStreamer
            s = NativeOnlineStreamer(_net(attention).to(device), 2, 4, device=device, use_graph=False, lib=rec)
            rec.arm(tensors_of(s))
            s.step(torch.randn(2, 9, 4, 4, generator=g).to(device))
        else:
            from models.io.stft import STFT
            from nbss_amd.online_io import NativeWaveStreamer
            s = NativeWaveStreamer(_net(attention, **WAVE_KW).to(device), 1, 4, STFT(n_fft=256, n_hop=128, win_len=256), "frequency", [0, 1], 1, device=device,
                                   use_graph=False, lib=rec)
            rec.arm(tensors_of(s))
            s.push(torch.randn(1, 2, 4 * 128, generator=g).to(device))
        return rec.records
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


def main():
    from nbss_amd._lib import Lib
    from nbss_amd.build import build_emu
    lib = Lib(build_emu())
    out = {"parent": sys.argv[1], "cases": {"/".join(c): trace(lib, torch.device("cpu"), *c) for c in CASES}}
    lines = ["{", f' "parent": {json.dumps(out["parent"])},', ' "cases": {']
    for i, (k, recs) in enumerate(out["cases"].items()):
        lines.append(f"  {json.dumps(k)}: [")
        lines += ["   " + json.dumps(r) + ("," if j + 1 < len(recs) else "") for j, r in enumerate(recs)]
        lines.append("  ]" + ("," if i + 1 < len(out["cases"]) else ""))
    lines += [" }", "}"]
    OUT.write_text("\n".join(lines) + "\n")
    print(f"{OUT}: {sum(len(v) for v in out['cases'].values())} records in {len(out['cases'])} cases")


if __name__ == "__main__":
    main()
