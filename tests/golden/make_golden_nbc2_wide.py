"""Generate tests/golden/nbc2_head96.npz FROM THE REFERENCE ITSELF (run in the build container, where /root/reference exists): the reference's NBC2 at
attention head width 96 (dim_hidden 192, 2 heads: the NBC2-large attention geometry) with a small feed-forward (dim_ffn 64, 4 conv groups), one layer,
5 frequencies x 33 frames (one 16-frame tile past two), run in fp64: input, output, r, parameters and the gradient of sum(y * r) w.r.t. every parameter.
tests/test_nbc2_large.py compares the native path (nbss_amd/nbc2.py) with THESE numbers on both backends.

Kept under 1 MB: one layer; the parameters are rounded to fp16 VALUES before the reference runs and stored as fp16 (exact), the gradients are stored as
fp32 and of in_proj_weight (576 rows) every second row.  Also stored: the error of the reference module itself run in fp32 on the same fixture
(`ref32/y`, `ref32/grad`: rel_l2 of the output, largest rel_l2 over the parameter gradients) — what single precision costs at this width whatever
the implementation."""
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")


def main():
    for m in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[m]
    sys.path.insert(0, str(REF))
    tm = types.ModuleType("torchmetrics"); tmf = types.ModuleType("torchmetrics.functional"); tma = types.ModuleType("torchmetrics.functional.audio")
    tma.permutation_invariant_training = tma.scale_invariant_signal_distortion_ratio = lambda *a, **k: None
    sys.modules.update({"torchmetrics": tm, "torchmetrics.functional": tmf, "torchmetrics.functional.audio": tma})
    from models.arch.NBC2 import NBC2  # noqa: E402  (reference)
    assert str(REF) in sys.modules["models.arch.NBC2"].__file__
    torch.manual_seed(96)
    torch.set_num_threads(1)
    bk = {"n_heads": 2, "dropout": 0, "conv_kernel_size": 3, "n_conv_groups": 4, "norms": ("LN", "GBN", "GBN"),
          "group_batch_norm_kwargs": {"share_along_sequence_dim": False}}
    net = NBC2(dim_input=4, dim_output=4, n_layers=1, dim_hidden=192, dim_ffn=64, num_freqs=5, block_kwargs=bk).eval()
    x = torch.randn(2, 5, 33, 4)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
            p.copy_(p.half().float())
    sd32 = {k: v.clone() for k, v in net.state_dict().items()}
    r = torch.randn(2, 5, 33, 4)
    # the reference in single precision on the same fixture
    y32 = net(x)
    (y32 * r).sum().backward()
    g32 = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad()
    net = net.double()
    y = net(x.double())
    (y * r.double()).sum().backward()
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    out = {"x": x.numpy(), "y": y.detach().float().numpy(), "r": r.numpy(),
           "ref32/y": np.float64(rel(y32.detach(), y.detach())),
           "ref32/grad": np.float64(max(rel(g32[k], p.grad) for k, p in net.named_parameters()))}
    for k, v in sd32.items():
        assert torch.equal(v.half().float(), v)
        out[f"param/{k}"] = v.numpy().astype(np.float16)
    for k, p in net.named_parameters():
        g = p.grad.float().numpy()
        if g.ndim == 2 and g.shape[0] >= 512:
            g = g[::2]
        out[f"grad/{k}"] = g
    np.savez_compressed(HERE / "nbc2_head96.npz", **out)
    print("written: nbc2_head96.npz", sum(np.asarray(v).nbytes for v in out.values()) // 1024, "KB uncompressed;", "reference fp32 error: y", out["ref32/y"], "grad",
          out["ref32/grad"])


if __name__ == "__main__":
    main()
