"""Records the sequence of `lib.call(...)` launches of the three native narrow-band runners (nbss_amd/nbc2.py, nbc.py, blstm.py) at small seeded geometries
-> tests/golden/nb_call_trace.json, the fixture of tests/test_nb_call_trace.py: what is launched, in which order, with which arguments.  Only the public
surface is used (`NativeX(net, lib).forward`, `.forward_train` + `.backward()`), so the same script runs on any commit; the committed fixture comes from the
commit named in its "parent" field, on the host emulator.

One record = [symbol, arg, arg, ...]: integers and floats by value (floats as the fp32 the C ABI receives), pointers as "p" / null (null = None was
passed).  The trailing stream argument of every entry point is left out: it is None on the emulator and a stream handle on the device.

usage: python tests/golden/make_nb_call_trace.py <commit hash of the tree it runs in>"""
import ctypes as C
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

OUT = Path(__file__).resolve().parent / "nb_call_trace.json"


class RecordingLib:
    """forwards everything to the library it wraps and records each `call`"""

    def __init__(self, lib):
        self._lib, self.records = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        from nbss_amd._lib import SIGNATURES
        types = SIGNATURES[name][1]
        assert len(types) == len(args) and types[-1] is C.c_void_p, name  # (the last argument of every launching entry point is the stream)
        rec = [name]
        for ty, a in zip(types[:-1], args[:-1]):
            if ty is C.c_void_p:
                rec.append(None if a is None else "p")
            elif ty is C.c_float:
                rec.append(C.c_float(a.value if isinstance(a, C.c_float) else a).value)
            else:
                rec.append(int(a))
        self.records.append(rec)
        return self._lib.call(name, *args)


def _nbc2(mode):
    """5 input channels for inference; 4 for training, as in the existing small tests: the weight-gradient kernel takes channel counts that are multiples
    of 4 and NBC2's encoder backward passes the unpadded count (nbss_nb_conv_t_bwd refuses 5) — both are padded to 8 columns"""
    from models.arch.NBC2 import NBC2
    from nbss_amd.nbc2 import NativeNBC2
    cin = 5 if mode == "infer" else 4
    bk = {"n_heads": 2, "dropout": 0, "conv_kernel_size": 3, "n_conv_groups": 8, "norms": ("LN", "GBN", "GBN"),
          "group_batch_norm_kwargs": {"share_along_sequence_dim": False}}
    net = NBC2(dim_input=cin, dim_output=3, n_layers=2, encoder_kernel_size=5, dim_hidden=48, dim_ffn=64, num_freqs=3, block_kwargs=bk).train()
    return net, NativeNBC2, (1, 3, 5, cin)


def _nbc(mode):
    from models.arch.NBC import NBC
    from nbss_amd.nbc import NativeNBC
    net = NBC(dim_input=5, dim_output=3, n_layers=2, encoder_kernel_size=4, n_heads=2, hidden_size=48, ffn_size=64).train()  # (train(): dropout 0.1 is active)
    return net, NativeNBC, (1, 3, 7, 5)


def _blstm(mode):
    from models.arch.blstm2_fc1 import BLSTM2_FC1
    from nbss_amd.blstm import NativeBLSTM
    net = BLSTM2_FC1(dim_input=5, dim_output=3, hidden_size=(128, 128)).train()
    return net, NativeBLSTM, (1, 3, 2, 5)


ARCHS = {"nbc2": _nbc2, "nbc": _nbc, "blstm": _blstm}
CASES = [(arch, dtype, mode) for arch in ARCHS for dtype in ("f32", "bf16") for mode in ("infer", "train")]


def trace(lib, device, arch, dtype, mode):
    """the records of one run: `mode` "infer" = runner.forward(x), "train" = runner.forward_train(x) and the backward of sum(y * r)"""
    torch.manual_seed(11)
    net, cls, shape = ARCHS[arch](mode)
    g = torch.Generator().manual_seed(12)
    x, r = torch.randn(*shape, generator=g), torch.randn(*shape[:3], 3, generator=g)
    x = x.to(torch.bfloat16 if dtype == "bf16" else torch.float32).to(device)
    rec = RecordingLib(lib)
    run = cls(net.to(device), rec)
    torch.manual_seed(13)  # (NBC draws its dropout masks from torch's generator)
    if mode == "infer":
        with torch.no_grad():
            run.forward(x)
    else:
        (run.forward_train(x).float() * r.to(device)).sum().backward()
    return rec.records


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
