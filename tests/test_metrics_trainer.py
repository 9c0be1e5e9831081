"""The metrics through the trainer: `validate` logs val/sdr, val/neg_si_sdr and val/metric, `test` recovers the scale and reports every served metric of
`model.metrics` with its input value and improvement (and writes test_results.json), `fit` logs val/sdr, val/si_sdr and val/metric and rejects an
unknown `val_metric`.  On the host with NBC2 through the generic path; gpu-marked: the fused SpatialNet path."""
import itertools
import json
import math
from pathlib import Path

import pytest
import torch

from SharedTrainer import TrainCLI, _instantiate, parse_cli

ROOT = Path(__file__).resolve().parent.parent
SYN = str(ROOT / "configs" / "datasets" / "synthetic.yaml")
DATA = ["--data.audio_time_len=[1.0,1.0,1.0]", "--data.num_samples=[4,2,4]", "--trainer.max_epochs=1"]
NBC2 = ["--config", str(ROOT / "configs" / "NBC2.yaml"), "--config", SYN, "--model.arch.dim_input=12", "--model.arch.dim_output=4", "--trainer.accelerator=cpu",
        "--model.arch.n_layers=1", "--model.arch.dim_hidden=16", "--model.arch.dim_ffn=32"] + DATA
SPATIAL = ["--config", str(ROOT / "configs" / "SpatialNet.yaml"), "--config", SYN, "--model.arch.dim_input=12", "--model.arch.dim_output=4",
           "--model.arch.num_layers=1"] + DATA


def finite(v):
    return isinstance(v, float) and math.isfinite(v)


def check_validate(args):
    rec = TrainCLI(argv=["validate"] + args).result
    assert finite(rec["val/sdr"]) and finite(rec["val/metric"])
    assert rec["val/metric"] == -rec["val/neg_si_sdr"]  # `val_metric: loss` as shipped; the loss is neg_si_sdr itself
    rec2 = TrainCLI(argv=["validate"] + args + ["--model.val_metric=sdr"]).result
    assert rec2["val/metric"] == rec2["val/sdr"] == rec["val/sdr"]
    rec3 = TrainCLI(argv=["validate"] + args + ["--model.loss.init_args.loss_func=models.io.loss.neg_snr", "--model.val_metric=si_sdr"]).result
    assert finite(rec3["val/neg_si_sdr"]) and rec3["val/metric"] == -rec3["val/neg_si_sdr"] and finite(rec3["val/sdr"])
    return rec


def check_test(args, tmp_path, utterances=4, S=2):
    rec = TrainCLI(argv=["test"] + args + [f"--trainer.default_root_dir={tmp_path}"]).result
    for m in ("sdr", "si_sdr"):  # the shipped `metrics` list: SDR, SI_SDR served, NB_PESQ / WB_PESQ / eSTOI left to a pass that is not ported
        assert finite(rec[f"test/{m}"]) and finite(rec[f"test/input_{m}"]) and finite(rec[f"test/{m}_i"]), rec
        assert abs(rec[f"test/{m}_i"] - (rec[f"test/{m}"] - rec[f"test/input_{m}"])) <= 1e-9
    assert "test/snr" not in rec and not any("pesq" in k or "stoi" in k for k in rec)
    assert finite(rec["test/neg_si_sdr"]) and finite(rec["test/si_sdr_improvement_dB"]) and rec["batches"] == utterances // 2
    rows = json.loads((tmp_path / "test_results.json").read_text())
    assert len(rows) == utterances and [r["id"] for r in rows] == list(range(utterances))
    for r in rows:
        assert finite(r["neg_si_sdr"]) and all(len(r[k]) == S for k in ("sdr_all", "input_sdr_all", "sdr_all_i", "si_sdr_all"))
    assert abs(sum(sum(r["sdr_all"]) / S for r in rows) / utterances - rec["test/sdr"]) <= 1e-5
    rec2 = TrainCLI(argv=["test"] + args + ["--model.metrics=[SNR,SDR]"]).result
    assert all(finite(rec2[k]) for k in ("test/snr", "test/input_snr", "test/snr_i", "test/sdr")) and "test/si_sdr" not in rec2
    return rec


def test_validate_on_the_host():
    check_validate(NBC2)


def test_test_on_the_host(tmp_path):
    check_test(NBC2, tmp_path)


def test_fit_logs_val_metric_on_the_host():
    log = TrainCLI(argv=["fit"] + NBC2 + ["--model.val_metric=sdr"]).result["log"]
    assert len(log) == 1 and finite(log[0]["val/sdr"]) and finite(log[0]["val/si_sdr"]) and log[0]["val/metric"] == log[0]["val/sdr"]
    log = TrainCLI(argv=["fit"] + NBC2).result["log"]
    assert log[0]["val/metric"] == -log[0]["val/neg_si_sdr"]


def test_unknown_val_metric_raises():
    for sub in ("fit", "validate"):
        with pytest.raises(ValueError, match="loss, si_sdr, sdr"):
            TrainCLI(argv=[sub] + NBC2 + ["--model.val_metric=pesq"])


@pytest.mark.gpu
def test_validate_and_fit_on_the_fused_path(hip_lib):
    check_validate(SPATIAL)
    log = TrainCLI(argv=["fit"] + SPATIAL + ["--model.val_metric=sdr", "--trainer.precision=bf16-mixed"]).result["log"]
    assert len(log) == 1 and finite(log[0]["val/sdr"]) and finite(log[0]["val/si_sdr"]) and log[0]["val/metric"] == log[0]["val/sdr"]
    with pytest.raises(ValueError, match="loss, si_sdr, sdr"):
        TrainCLI(argv=["fit"] + SPATIAL + ["--model.val_metric=pesq"])


@pytest.mark.gpu
def test_test_on_the_fused_path_and_sdr_of_the_predicted_waveforms(hip_lib, tmp_path):
    """test/sdr recomputed from `predict`'s waveforms with the fp64 restatement: best SI-SDR pairing per utterance (what the uPIT loss picks), SDR of the
    paired signals (SDR normalises both signals, so the recovered scale does not enter), mean over the split; 1e-3 dB"""
    from test_metrics_kernels import ref_ratios, ref_sdr
    rec = check_test(SPATIAL, tmp_path)
    outs = TrainCLI(argv=["predict"] + SPATIAL).result["yr_hat"]
    _, cfg = parse_cli(["predict"] + SPATIAL)
    data = _instantiate(cfg["data"])
    vals = []
    for yr_hat, (x, ys, _) in zip(outs, data.batches(2, 0, 1, 0)):
        yr = ys[:, :, 0]
        for b in range(yr.shape[0]):
            best = max(itertools.permutations(range(yr.shape[1])), key=lambda pm: float(ref_ratios(yr_hat[b, list(pm)], yr[b])[:, 1].mean()))
            vals.append(float(ref_sdr(yr_hat[b, list(best)], yr[b]).mean()))
    print("test/sdr", rec["test/sdr"], "recomputed", sum(vals) / len(vals))
    assert len(vals) == 4 and abs(sum(vals) / len(vals) - rec["test/sdr"]) <= 1e-3
