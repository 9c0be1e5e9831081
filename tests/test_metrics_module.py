"""models/utils/metrics.py — the drop-in for the reference's cal_metrics_functional / recover_scale: key names, improvements, chunk suffixes, refusals,
on the host path; a gpu-marked twin runs the same calls on the device kernels and compares them with the host results (1e-4 dB)."""
import pytest
import torch

from models.utils.metrics import cal_metrics_functional, recover_scale

SERVED = ["sdr", "si_sdr", "snr", "si_snr"]
NAMES = ["SDR", "SI_SDR", "SNR", "SI_SNR", "NB_PESQ"]


def signals(S=2, N=4001, seed=3):
    g = torch.Generator().manual_seed(seed)
    target = torch.randn(S, N, generator=g)
    target = target + 0.5 * torch.roll(target, 1, -1)  # a little colour
    original = (target.sum(0, keepdim=True) + 0.05 * torch.randn(1, N, generator=g)).expand(S, N).contiguous()
    preds = 0.7 * target + 0.1 * torch.randn(S, N, generator=g)
    return preds, target, original


def check_result(res, S=2, suffixes=("",)):
    metrics, input_metrics, imp = res
    want_m = {f"{m}{sf}{a}" for m in SERVED for sf in suffixes for a in ("", "_all")}
    assert set(metrics) == want_m
    assert set(input_metrics) == {"input_" + k for k in want_m}
    assert set(imp) == {f"{m}{sf}{a}" for m in SERVED for sf in suffixes for a in ("_i", "_all_i")}
    for m in SERVED:
        for sf in suffixes:
            k = m + sf
            assert isinstance(metrics[k], float) and metrics[k] == metrics[k]
            assert len(metrics[k + "_all"]) == S and len(input_metrics["input_" + k + "_all"]) == S and len(imp[k + "_all_i"]) == S
            assert imp[k + "_i"] == metrics[k] - input_metrics["input_" + k]
            assert abs(metrics[k] - sum(metrics[k + "_all"]) / S) < 1e-5
            for a, b, c in zip(metrics[k + "_all"], input_metrics["input_" + k + "_all"], imp[k + "_all_i"]):
                assert abs((a - b) - c) < 1e-5


def run(device):
    preds, target, original = (t.to(device) for t in signals())
    return cal_metrics_functional(NAMES, preds, target, original, 8000, device_only="gpu")


def test_key_set_and_improvements_on_the_host():
    res = run("cpu")
    check_result(res)
    assert res[0]["sdr"] > res[1]["input_sdr"]  # the estimate is better than the mixture


def test_values_are_the_closed_forms():
    from test_metrics_kernels import ref_ratios, ref_sdr
    preds, target, original = signals()
    m, im, _ = cal_metrics_functional(["SDR", "SI_SDR", "SNR", "SI_SNR"], preds, target, original, 8000, device_only="gpu")
    r, ri = ref_ratios(preds, target), ref_ratios(original, target)
    for s in range(2):
        assert abs(m["sdr_all"][s] - float(ref_sdr(preds, target)[s])) <= 1e-4
        assert abs(im["input_sdr_all"][s] - float(ref_sdr(original, target)[s])) <= 1e-4
        for col, name in enumerate(("snr", "si_sdr", "si_snr")):
            assert abs(m[name + "_all"][s] - float(r[s, col])) <= 1e-4
            assert abs(im["input_" + name + "_all"][s] - float(ri[s, col])) <= 1e-4


def test_chunk_suffixes():
    """chunk = (0.25 s, 0.125 s) at 8 kHz on 4001 samples: int((4001 / 8000 - 0.25) / 0.125) + 1 = 3 chunks, named as the reference names them"""
    preds, target, original = signals()
    res = cal_metrics_functional(NAMES, preds, target, original, 8000, device_only="gpu", chunk=(0.25, 0.125))
    sfx = [f"_{i*0.125+1}s-{i*0.125+0.25}s" for i in range(3)]
    assert sfx == ["_1.0s-0.25s", "_1.125s-0.375s", "_1.25s-0.5s"]
    check_result(res, suffixes=["", *sfx])
    one = cal_metrics_functional(["SI_SDR"], preds[..., 1000:3000], target[..., 1000:3000], None, 8000, device_only="gpu")
    assert res[0]["si_sdr" + sfx[1]] == one[0]["si_sdr"] and one[1] == {} and one[2] == {}


def test_refusals():
    preds, target, original = signals(N=1000)
    for name, pkg in (("NB_PESQ", "pesq"), ("STOI", "pystoi"), ("ESTOI", "pystoi"), ("DNSMOS", "onnxruntime")):
        for dev in (None, "cpu"):
            with pytest.raises(NotImplementedError, match=pkg):
                cal_metrics_functional([name], preds, target, original, 16000, device_only=dev)
        assert cal_metrics_functional([name], preds, target, original, 16000, device_only="gpu") == ({}, {}, {})
    with pytest.raises(NotImplementedError, match="pesq"):
        cal_metrics_functional(["WB_PESQ"], preds, target, original, 16000)
    assert cal_metrics_functional(["WB_PESQ"], preds, target, original, 8000) == ({}, {}, {})  # narrow band only at 8 kHz: skipped, as in the reference
    with pytest.raises(ValueError, match="Unkown audio metric"):
        cal_metrics_functional(["SDRR"], preds, target, original, 8000, device_only="gpu")
    assert set(cal_metrics_functional(["SDR"], preds, target, None, 8000)[0]) == {"sdr", "sdr_all"}  # device_only=None serves the native ones too
    assert cal_metrics_functional(["SDR"], preds, target, None, 8000, device_only="cpu") == ({}, {}, {})  # ... the cpu pass leaves them to the device pass


def test_recover_scale_on_the_host():
    g = torch.Generator().manual_seed(5)
    preds = torch.randn(2, 2, 1000, generator=g)
    mixture = 2.0 * preds[:, 0] - 0.5 * preds[:, 1]
    out = recover_scale(preds, mixture, scale_src_together=False, norm_if_exceed_1=False)
    assert torch.allclose(out[:, 0], 2.0 * preds[:, 0], atol=1e-5) and torch.allclose(out[:, 1], -0.5 * preds[:, 1], atol=1e-5)
    want = preds * torch.linalg.lstsq(preds.sum(1, keepdim=True).transpose(-1, -2), mixture[..., None]).solution
    assert torch.allclose(recover_scale(preds, mixture, True, False), want, atol=1e-5)
    assert float(recover_scale(preds, mixture, False, True).abs().max()) <= 1.0 + 1e-6


@pytest.mark.gpu
def test_device_results_equal_host_results(hip_lib):
    host, dev = run("cpu"), run("cuda:0")
    check_result(dev)
    for h, d in zip(host, dev):
        assert set(h) == set(d)
        for k in h:
            a, b = torch.tensor(h[k], dtype=torch.float64), torch.tensor(d[k], dtype=torch.float64)
            print(k, h[k], d[k])
            assert float((a - b).abs().max()) <= 1e-4, k
    preds, target, original = signals()
    res = cal_metrics_functional(NAMES, preds.cuda(), target.cuda(), original.cuda(), 8000, device_only="gpu", chunk=(0.25, 0.125))
    check_result(res, suffixes=["", "_1.0s-0.25s", "_1.125s-0.375s", "_1.25s-0.5s"])
    g = torch.Generator().manual_seed(5)
    p = torch.randn(2, 2, 1000, generator=g)
    x = 2.0 * p[:, 0] - 0.5 * p[:, 1] + 0.1 * torch.randn(2, 1000, generator=g)
    for together in (False, True):
        a, b = recover_scale(p, x, together, True), recover_scale(p.cuda(), x.cuda(), together, True).cpu()
        assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
