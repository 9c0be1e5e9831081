"""Generate tests/golden/nb_long.npz FROM THE REFERENCE ITSELF (run in the build container, where /root/reference exists): the reference's NBC2 and NBC
on a sequence longer than the whole-head attention kernels take — 1 x 5 frequencies x 300 frames (five 64-key blocks; the last one 44 keys) — at the
smallest widths the native paths have kernels for, run in fp64 in eval mode: input, parameters and output.
  nbc2_24 / nbc2_48 / nbc2_96   one NBC2 layer, one attention head of width 24 / 48 / 96 (dim_hidden = the head width, dim_ffn 32 in 4 conv groups)
  nbc                           one NBC layer, hidden 48 / 2 heads (head width 24), ffn 64
tests/test_nb_long.py compares the native inference paths (nbss_amd/nbc2.py, nbc.py with NBSS_NB_LONG=1) with THESE numbers on both backends.

Also stored per case, as in make_golden_nbc2_wide.py: `ref32/y`, the error of the reference module itself run in fp32 on the same data — what single
precision costs at this length whatever the implementation.  It must lie under the bars of the test (5e-6 NBC2, 2e-5 NBC): asserted here.
Small: parameters are rounded to fp16 VALUES before the reference runs and stored as fp16 (exact); NBC's sinusoid table (a constructor constant) is not stored."""
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
BARS = {"nbc2_24": 5e-6, "nbc2_48": 5e-6, "nbc2_96": 5e-6, "nbc": 2e-5}
B, F, T = 1, 5, 300


def main():
    assert REF.exists(), "the reference tree is needed to (re)generate the fixture"
    for m in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[m]
    sys.path.insert(0, str(REF))
    tm = types.ModuleType("torchmetrics"); tmf = types.ModuleType("torchmetrics.functional"); tma = types.ModuleType("torchmetrics.functional.audio")
    tma.permutation_invariant_training = tma.scale_invariant_signal_distortion_ratio = lambda *a, **k: None
    sys.modules.update({"torchmetrics": tm, "torchmetrics.functional": tmf, "torchmetrics.functional.audio": tma})
    from models.arch.NBC import NBC  # noqa: E402  (reference)
    from models.arch.NBC2 import NBC2  # noqa: E402
    assert str(REF) in sys.modules["models.arch.NBC2"].__file__ and str(REF) in sys.modules["models.arch.NBC"].__file__
    torch.manual_seed(300)
    torch.set_num_threads(1)
    bk = {"n_heads": 1, "dropout": 0, "conv_kernel_size": 3, "n_conv_groups": 4, "norms": ("LN", "GBN", "GBN"),
          "group_batch_norm_kwargs": {"share_along_sequence_dim": False}}
    cases = {f"nbc2_{dh}": NBC2(dim_input=4, dim_output=4, n_layers=1, dim_hidden=dh, dim_ffn=32, num_freqs=F, block_kwargs=bk) for dh in (24, 48, 96)}
    cases["nbc"] = NBC(dim_input=4, dim_output=4, n_layers=1, encoder_kernel_size=4, n_heads=2, hidden_size=48, ffn_size=64)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    out = {}
    for name, net in cases.items():
        net.eval()  # (NBC's blocks carry dropout 0.1: inactive in eval mode; neither network has mode-dependent statistics)
        x = torch.randn(B, F, T, 4)
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))
                p.copy_(p.half().float())
            sd32 = {k: v.clone() for k, v in net.state_dict().items() if not k.endswith("rel_pos.pe")}
            y32 = net(x)
            y = net.double()(x.double())
        e32 = rel(y32, y)
        assert e32 < BARS[name], (name, e32)  # (shrink the case rather than widen the bar)
        out[f"{name}/x"], out[f"{name}/y"], out[f"{name}/ref32/y"] = x.numpy(), y.float().numpy(), np.float64(e32)
        for k, v in sd32.items():
            assert torch.equal(v.half().float(), v)
            out[f"{name}/param/{k}"] = v.numpy().astype(np.float16)
        print(f"{name}: reference fp32 error {e32:.3e} (bar {BARS[name]:.0e})")
    np.savez_compressed(HERE / "nb_long.npz", **out)
    print("written: nb_long.npz", (HERE / "nb_long.npz").stat().st_size // 1024, "KB")


if __name__ == "__main__":
    main()
