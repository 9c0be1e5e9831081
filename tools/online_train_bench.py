"""One OnlineSpatialNet training step (forward + backward + AdamW) of the shipped 8-layer configs/onlineSpatialNet.yaml model in five settings in the same
process — every switch off, the native T-ConvFFN (NBSS_ONLINE_NATIVE_TRAIN), the native T-ConvFFN + the native retention core (NBSS_ONLINE_NATIVE_RET),
those two + the native cross-band trio (NBSS_ONLINE_NATIVE_XBAND), and T-ConvFFN + the whole retention block as one node (NBSS_ONLINE_NATIVE_TSA) + the
cross-band trio — then the T-ConvFFN block alone against the module's `_tconvffn`, the retention block alone (`layer._tsa`: LayerNorm, projections,
retention, out_proj) against the module's MultiScaleRetention, the retention block with its residual (`x + _tsa(x)`) with the native core against the
one-node form, and the cross-band trio alone (`layer._xband`: fconv1, full-band, fconv2 with their residuals) against the module's `_fconv` / `_full`
chain, each forward and forward + backward.  With `--variant mamba` instead: the 8-layer 'mamba(16,4)' model (NBSS_ONLINE_MAMBA=1) with the native cross-band
trio alone (the torch module's Mamba blocks at the fastest cross-band path) against the trio + the native Mamba core (NBSS_ONLINE_NATIVE_MAMBA), then one
Mamba block alone (`layer._mamba`: LayerNorm, in_proj, the core, out_proj), forward and forward + backward.

    python tools/online_train_bench.py [--variant ret|mamba] [--batches 2 4] [--seconds 4] [--steps 10] [--warmup 3] [--layers 8]

HIP events around `steps` iterations after `warmup` discarded ones; the variants alternate in blocks so that clock drift hits both; peak memory is
torch's allocator peak over the timed iterations.  Prints one JSON line per setting."""
import argparse
import json
import os
import sys
from pathlib import Path

import torch
import yaml

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, torch.cuda.max_memory_allocated() / 2 ** 20


def _switch(on, ret=False, xband=False, tsa=False):
    os.environ["NBSS_ONLINE_NATIVE_TRAIN"] = "1" if on else "0"
    os.environ["NBSS_ONLINE_NATIVE_RET"] = "1" if ret else "0"
    os.environ["NBSS_ONLINE_NATIVE_XBAND"] = "1" if xband else "0"
    os.environ["NBSS_ONLINE_NATIVE_TSA"] = "1" if tsa else "0"


def _mamba(a):
    """the 'mamba(16,4)' model: XBAND alone against XBAND + MAMBA, then one Mamba block alone; the same protocol as the settings of `main`"""
    os.environ["NBSS_ONLINE_MAMBA"] = "1"
    os.environ["NBSS_ONLINE_NATIVE_XBAND"] = "1"
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    arch = yaml.safe_load((ROOT / "configs" / "onlineSpatialNet.yaml").read_text())["model"]["arch"]["init_args"]
    arch.update(num_layers=a.layers, dim_input=12, dim_output=4, num_freqs=129, attention="mamba(16,4)")
    dev = torch.device("cuda", 0)
    T = int(a.seconds * 8000) // 128 + 1
    torch.manual_seed(2)
    net = OnlineSpatialNet(**arch).to(dev).train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-3)

    def native(on):
        os.environ["NBSS_ONLINE_NATIVE_MAMBA"] = "1" if on else "0"

    for B in a.batches:
        x, r = torch.randn(B, 129, T, 12, device=dev), torch.randn(B, 129, T, 4, device=dev)
        for prec in ("32", "bf16-mixed"):
            def step():
                opt.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    y = net(x)
                ((y.float() - r) ** 2).mean().backward()
                opt.step()
            res = {}
            for _ in range(a.rounds):
                for k, on in (("xband", False), ("xband_mamba", True)):
                    native(on)
                    ms, mb = _timed(step, a.steps, a.warmup)
                    res[k] = (min(ms, res[k][0]), max(mb, res[k][1])) if k in res else (ms, mb)
            print(json.dumps({"what": "mamba(16,4) train step", "layers": a.layers, "B": B, "T": T, "precision": prec, "rounds": a.rounds,
                              "xband_ms": round(res["xband"][0], 2), "xband_mamba_ms": round(res["xband_mamba"][0], 2),
                              "xband_over_xband_mamba": round(res["xband"][0] / res["xband_mamba"][0], 3), "xband_peak_MiB": round(res["xband"][1]),
                              "xband_mamba_peak_MiB": round(res["xband_mamba"][1])}), flush=True)
        layer = net.layers[0]
        for prec in ("32", "bf16-mixed"):
            h = torch.randn(B, 129, T, 96, device=dev, requires_grad=True)
            g = torch.randn(B, 129, T, 96, device=dev)

            def fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    layer._mamba(h, layer.mhsa, layer.norm_mhsa, layer.dropout_mhsa)

            def fwd_bwd():
                net.zero_grad(set_to_none=True)
                h.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    y = layer._mamba(h, layer.mhsa, layer.norm_mhsa, layer.dropout_mhsa)
                y.backward(g.to(y.dtype))
            out = {"what": "Mamba block", "B": B, "T": T, "precision": prec}
            for name, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                for on in (False, True):
                    native(on)
                    ms, mb = _timed(fn, a.steps, a.warmup)
                    out[f"{name}_{'on' if on else 'off'}_ms"], out[f"{name}_{'on' if on else 'off'}_peak_MiB"] = round(ms, 3), round(mb)
                out[f"{name}_off_over_on"] = round(out[f"{name}_off_ms"] / out[f"{name}_on_ms"], 3)
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("ret", "mamba"), default="ret", help="the shipped ret(2) model and its four blocks, or the mamba(16,4) model")
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2, help="blocks of the settings per case (the minimum of the rounds is reported; for the two fastest "
                    "settings also the maximum)")
    a = ap.parse_args()
    if a.variant == "mamba":
        return _mamba(a)
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    arch = yaml.safe_load((ROOT / "configs" / "onlineSpatialNet.yaml").read_text())["model"]["arch"]["init_args"]
    arch.update(num_layers=a.layers, dim_input=12, dim_output=4, num_freqs=129)
    dev = torch.device("cuda", 0)
    T = int(a.seconds * 8000) // 128 + 1
    torch.manual_seed(2)
    net = OnlineSpatialNet(**arch).to(dev).train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-3)
    for B in a.batches:
        x, r = torch.randn(B, 129, T, 12, device=dev), torch.randn(B, 129, T, 4, device=dev)
        for prec in ("32", "bf16-mixed"):
            def step():
                opt.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    y = net(x)
                ((y.float() - r) ** 2).mean().backward()
                opt.step()
            res, hi = {}, {}
            for _ in range(a.rounds):
                for k, on, ret, xb, tsa in (("off", False, False, False, False), ("on", True, False, False, False), ("on_ret", True, True, False, False),
                                            ("on_ret_xband", True, True, True, False), ("on_tsa_xband", True, False, True, True)):
                    _switch(on, ret, xb, tsa)
                    ms, mb = _timed(step, a.steps, a.warmup)
                    res[k] = (min(ms, res[k][0]), max(mb, res[k][1])) if k in res else (ms, mb)
                    hi[k] = max(ms, hi.get(k, 0.0))
            print(json.dumps({"what": "train step", "layers": a.layers, "B": B, "T": T, "precision": prec, "rounds": a.rounds, "off_ms": round(res["off"][0], 2),
                              "on_ms": round(res["on"][0], 2), "on_ret_ms": round(res["on_ret"][0], 2), "on_ret_xband_ms": round(res["on_ret_xband"][0], 2),
                              "off_over_on": round(res["off"][0] / res["on"][0], 3), "on_over_on_ret": round(res["on"][0] / res["on_ret"][0], 3),
                              "on_ret_over_on_ret_xband": round(res["on_ret"][0] / res["on_ret_xband"][0], 3), "off_peak_MiB": round(res["off"][1]),
                              "on_peak_MiB": round(res["on"][1]), "on_ret_peak_MiB": round(res["on_ret"][1]),
                              "on_ret_xband_peak_MiB": round(res["on_ret_xband"][1]), "on_ret_xband_max_ms": round(hi["on_ret_xband"], 2),
                              "on_tsa_xband_ms": round(res["on_tsa_xband"][0], 2), "on_tsa_xband_max_ms": round(hi["on_tsa_xband"], 2),
                              "on_tsa_xband_peak_MiB": round(res["on_tsa_xband"][1])}), flush=True)
        # the block alone: x + _tconvffn(x), forward and forward + backward
        layer = net.layers[0]
        for prec in ("32", "bf16-mixed"):
            h = torch.randn(B, 129, T, 96, device=dev, requires_grad=True)
            g = torch.randn(B, 129, T, 96, device=dev)

            def fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    layer._tconvffn(h, residual=True)

            def fwd_bwd():
                net.zero_grad(set_to_none=True)
                h.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    y = layer._tconvffn(h, residual=True)
                y.backward(g)
            out = {"what": "T-ConvFFN block", "B": B, "T": T, "precision": prec}
            for name, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                for on in (False, True):
                    _switch(on)
                    out[f"{name}_{'on' if on else 'off'}_ms"] = round(_timed(fn, a.steps, a.warmup)[0], 3)
                out[f"{name}_off_over_on"] = round(out[f"{name}_off_ms"] / out[f"{name}_on_ms"], 3)
            print(json.dumps(out), flush=True)
        # the retention block alone: layer._tsa (LayerNorm, the projections, retention, out_proj), forward and forward + backward
        pos = net.get_causal_mask(slen=T, device=dev, chunkwise_recurrent=True, batch_size=B * 129)
        for prec in ("32", "bf16-mixed"):
            h = torch.randn(B, 129, T, 96, device=dev, requires_grad=True)
            g = torch.randn(B, 129, T, 96, device=dev)

            def fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    layer._tsa(h, pos, True, net.rope)

            def fwd_bwd():
                net.zero_grad(set_to_none=True)
                h.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    y = layer._tsa(h, pos, True, net.rope)[0]
                y.backward(g.to(y.dtype))
            out = {"what": "retention block", "B": B, "T": T, "precision": prec}
            for name, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                for ret in (False, True):
                    _switch(False, ret)
                    out[f"{name}_{'on' if ret else 'off'}_ms"] = round(_timed(fn, a.steps, a.warmup)[0], 3)
                out[f"{name}_off_over_on"] = round(out[f"{name}_off_ms"] / out[f"{name}_on_ms"], 3)
            print(json.dumps(out), flush=True)
        # the retention block with its residual, x + _tsa(x) as SpatialNetLayer.forward evaluates it: the native core between torch's LayerNorm and GEMMs (RET)
        # against the one native node (TSA)
        from nbss_amd import online_train

        def block(h):
            if online_train.take(online_train.TSA, layer, h, False, pos, True, net.rope):
                return online_train.tsa_residual(layer, h, pos, True, net.rope)
            return h + layer._tsa(h, pos, True, net.rope)[0]

        for prec in ("32", "bf16-mixed"):
            h = torch.randn(B, 129, T, 96, device=dev, requires_grad=True)
            g = torch.randn(B, 129, T, 96, device=dev)

            def fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    block(h)

            def fwd_bwd():
                net.zero_grad(set_to_none=True)
                h.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    y = block(h)
                y.backward(g.to(y.dtype))
            out = {"what": "retention block with residual, RET against TSA", "B": B, "T": T, "precision": prec}
            for name, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                for tsa in (False, True):
                    _switch(False, not tsa, False, tsa)
                    ms, mb = _timed(fn, a.steps, a.warmup)
                    out[f"{name}_{'tsa' if tsa else 'ret'}_ms"], out[f"{name}_{'tsa' if tsa else 'ret'}_peak_MiB"] = round(ms, 3), round(mb)
                out[f"{name}_ret_over_tsa"] = round(out[f"{name}_ret_ms"] / out[f"{name}_tsa_ms"], 3)
            print(json.dumps(out), flush=True)
        # the cross-band trio alone: layer._xband (x + fconv1, + full-band, + fconv2), forward and forward + backward
        for prec in ("32", "bf16-mixed"):
            h = torch.randn(B, 129, T, 96, device=dev, requires_grad=True)
            g = torch.randn(B, 129, T, 96, device=dev)

            def fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    layer._xband(h)

            def fwd_bwd():
                net.zero_grad(set_to_none=True)
                h.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec != "32"):
                    y = layer._xband(h)
                y.backward(g.to(y.dtype))
            out = {"what": "cross-band trio", "B": B, "T": T, "precision": prec}
            for name, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                for xb in (False, True):
                    _switch(False, False, xb)
                    out[f"{name}_{'on' if xb else 'off'}_ms"] = round(_timed(fn, a.steps, a.warmup)[0], 3)
                out[f"{name}_off_over_on"] = round(out[f"{name}_off_ms"] / out[f"{name}_on_ms"], 3)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
