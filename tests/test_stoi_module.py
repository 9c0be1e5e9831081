"""STOI / eSTOI through models/utils/metrics.py: the host closed form against the restatement of tests/test_stoi_kernels.py, the switch
NBSS_NATIVE_STOI (off: today's refusals; on: the reference's keys, shapes, chunk suffixes, improvements and the device_only routing) and, under
-m gpu, device tensors against the host form within the kernel bar."""
import numpy as np
import pytest
import torch

from models.utils.metrics import cal_metrics_functional, get_metric_list_on_device, native_stoi
from test_stoi_kernels import GRID, ar2_pair, bar, grid_refs, ref_batch


def signals(B=2, S=2, N=8000):
    target, preds = ar2_pair(B, S, N)
    g = torch.Generator().manual_seed(3)
    original = (target + 0.1 * torch.randn(B, S, N, generator=g)).contiguous()  # noisier than the estimates of the high-SNR pairs
    return preds, target, original


@pytest.mark.parametrize("N,fs", GRID)
def test_host_form_matches_restatement(N, fs):
    target, preds = ar2_pair(2, 2, N)
    for ext in (False, True):
        got = native_stoi(preds, target, fs, ext)
        assert got.shape == (2, 2) and got.dtype == torch.float32
        err = float(np.abs(got.double().numpy() - grid_refs()[N, fs, ext][0]).max())
        print(N, fs, ext, err)
        assert err <= 6e-8  # two fp64 evaluations of one definition: the fp32 rounding of a value below 1 (half an ulp: 3e-8) and nothing else


def test_host_form_edges():
    target, preds = ar2_pair(1, 2, 2400)
    assert torch.equal(native_stoi(preds, target, 8000, True), torch.full((1, 2), 1e-5))
    assert native_stoi(preds[0, 0], target[0, 0], 8000, False).shape == ()
    with pytest.raises(ValueError, match="sampling rate"):
        native_stoi(preds, target, 44100, False)
    with pytest.raises(ValueError, match="same shape"):
        native_stoi(preds, target[..., :-1], 8000, False)


@pytest.mark.parametrize("value", [None, "0", "true", "11"])
def test_switch_off(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("NBSS_NATIVE_STOI", raising=False)
    else:
        monkeypatch.setenv("NBSS_NATIVE_STOI", value)
    preds, target, original = signals(N=4001)
    for dev in (None, "cpu"):
        with pytest.raises(NotImplementedError, match="pystoi") as e:
            cal_metrics_functional(["ESTOI"], preds, target, original, 8000, device_only=dev)
        assert "NBSS_NATIVE_STOI=1" in str(e.value) and "not pinned" in str(e.value)
    assert cal_metrics_functional(["ESTOI"], preds, target, original, 8000, device_only="gpu") == ({}, {}, {})
    assert "ESTOI" not in get_metric_list_on_device("gpu") and "STOI" not in get_metric_list_on_device("gpu")


def test_switch_on_keys_shapes_and_improvement(monkeypatch):
    monkeypatch.setenv("NBSS_NATIVE_STOI", "1")
    preds, target, original = signals()
    assert {"STOI", "ESTOI"} <= set(get_metric_list_on_device("gpu"))
    m, im, imp = cal_metrics_functional(["SI_SDR", "STOI", "eSTOI"], preds, target, original, 8000)
    for name, ext in (("stoi", False), ("estoi", True)):
        want = ref_batch(preds, target, 8000, ext)
        want_in = ref_batch(original, target, 8000, ext)
        assert np.abs(np.array(m[name + "_all"]) - want).max() <= 6e-8 and np.abs(np.array(im[f"input_{name}_all"]) - want_in).max() <= 6e-8
        assert np.array(m[name + "_all"]).shape == (2, 2)
        assert abs(m[name] - np.mean(m[name + "_all"])) <= 1e-12 and abs(im["input_" + name] - np.mean(im[f"input_{name}_all"])) <= 1e-12
        assert imp[name + "_i"] == m[name] - im["input_" + name]
        assert np.abs(np.array(imp[name + "_all_i"]) - (np.array(m[name + "_all"]) - np.array(im[f"input_{name}_all"]))).max() <= 1e-12
    assert "si_sdr" in m and "input_si_sdr" in im
    m, im, imp = cal_metrics_functional(["ESTOI"], preds, target, None, 8000)
    assert set(m) == {"estoi", "estoi_all"} and im == {} and imp == {}


def test_switch_on_chunks(monkeypatch):
    monkeypatch.setenv("NBSS_NATIVE_STOI", "1")
    preds, target, original = signals(N=12000)  # 1.5 s at 8 kHz: chunks of 1 s at hop 0.5 s -> two
    m, im, imp = cal_metrics_functional(["ESTOI"], preds, target, original, 8000, chunk=(1.0, 0.5))
    for sfx in ("", "_1.0s-1.0s", "_1.5s-1.5s"):
        assert {"estoi" + sfx, "estoi" + sfx + "_all"} <= set(m) and "input_estoi" + sfx in im and "estoi" + sfx + "_i" in imp, (sfx, sorted(m))
    assert abs(m["estoi_1.5s-1.5s"] - float(ref_batch(preds[..., 4000:12000], target[..., 4000:12000], 8000, True, margin=False).mean())) <= 6e-8


def test_switch_on_device_only_routing(monkeypatch):
    monkeypatch.setenv("NBSS_NATIVE_STOI", "1")
    preds, target, original = signals()
    for dev in ("gpu", "cpu"):  # host tensors in both passes here: the 'gpu' pass evaluates where the tensors live
        m, im, imp = cal_metrics_functional(["SDR", "ESTOI", "NB_PESQ"] if dev == "gpu" else ["SDR", "ESTOI"], preds, target, original, 8000, device_only=dev)
        assert {"estoi", "estoi_all"} <= set(m) and "input_estoi" in im and "estoi_i" in imp
        assert ("sdr" in m) == (dev == "gpu") and not any("pesq" in k or k.startswith("stoi") for k in m)
    with pytest.raises(NotImplementedError, match="pesq"):
        cal_metrics_functional(["ESTOI", "NB_PESQ"], preds, target, original, 8000, device_only="cpu")


@pytest.mark.gpu
def test_device_tensors_agree_with_the_host_form(hip_lib, monkeypatch):
    monkeypatch.setenv("NBSS_NATIVE_STOI", "1")
    preds, target, original = signals()
    dev = torch.device("cuda:0")
    for ext in (False, True):
        host = native_stoi(preds, target, 8000, ext)
        got = native_stoi(preds.to(dev), target.to(dev), 8000, ext)
        assert got.is_cuda and got.shape == (2, 2)
        assert float((got.cpu().double() - host.double()).abs().max()) <= bar() + 6e-8  # the kernel bar, and the host form's own fp32 rounding
    m_host = cal_metrics_functional(["ESTOI"], preds, target, original, 8000, device_only="gpu")
    m_dev = cal_metrics_functional(["ESTOI"], preds.to(dev), target.to(dev), original.to(dev), 8000, device_only="gpu")
    m_cpu = cal_metrics_functional(["ESTOI"], preds.to(dev), target.to(dev), original.to(dev), 8000, device_only="cpu")
    assert abs(m_dev[0]["estoi"] - m_host[0]["estoi"]) <= bar() + 6e-8 and abs(m_dev[2]["estoi_i"] - m_host[2]["estoi_i"]) <= 2 * (bar() + 6e-8)
    assert m_cpu[0]["estoi"] == m_host[0]["estoi"]  # the 'cpu' pass moves device tensors to the host
