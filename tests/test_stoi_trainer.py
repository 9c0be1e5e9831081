"""eSTOI through the trainer: with NBSS_NATIVE_STOI=1 a `test` run on the synthetic data module with the shipped metrics list (SDR, SI_SDR, NB_PESQ,
WB_PESQ, eSTOI) logs test/estoi, test/input_estoi and test/estoi_i and writes estoi rows to test_results.json; without the switch it writes none.
On the host with NBC2 through the generic path; gpu-marked: the fused SpatialNet path."""
import json
import math

import pytest

from SharedTrainer import TrainCLI
from test_metrics_trainer import NBC2, SPATIAL


def run_test(args, tmp_path):
    rec = TrainCLI(argv=["test"] + args + [f"--trainer.default_root_dir={tmp_path}"]).result
    return rec, json.loads((tmp_path / "test_results.json").read_text())


def check_on(args, tmp_path, S=2):
    rec, rows = run_test(args, tmp_path)
    for k in ("test/estoi", "test/input_estoi", "test/estoi_i", "test/sdr", "test/si_sdr"):
        assert isinstance(rec[k], float) and math.isfinite(rec[k]), (k, rec)
    assert -1.0 <= rec["test/estoi"] <= 1.0 and abs(rec["test/estoi_i"] - (rec["test/estoi"] - rec["test/input_estoi"])) <= 1e-9
    assert not any("pesq" in k for k in rec)
    assert len(rows) == 4
    for r in rows:
        assert all(len(r[k]) == S and all(math.isfinite(v) for v in r[k]) for k in ("estoi_all", "input_estoi_all", "estoi_all_i", "sdr_all"))
    assert abs(sum(sum(r["estoi_all"]) / S for r in rows) / len(rows) - rec["test/estoi"]) <= 1e-6


def check_off(args, tmp_path):
    rec, rows = run_test(args, tmp_path)
    assert not any("stoi" in k for k in rec) and not any("stoi" in k for r in rows for k in r)
    assert "test/sdr" in rec


def test_switch_on_writes_estoi_rows_on_the_host(monkeypatch, tmp_path):
    monkeypatch.setenv("NBSS_NATIVE_STOI", "1")
    check_on(NBC2, tmp_path)


def test_switch_off_writes_none_on_the_host(monkeypatch, tmp_path):
    monkeypatch.delenv("NBSS_NATIVE_STOI", raising=False)
    check_off(NBC2, tmp_path)


@pytest.mark.gpu
def test_fused_path_with_and_without_the_switch(hip_lib, monkeypatch, tmp_path):
    monkeypatch.setenv("NBSS_NATIVE_STOI", "1")
    (tmp_path / "on").mkdir(), (tmp_path / "off").mkdir()
    check_on(SPATIAL, tmp_path / "on")
    monkeypatch.delenv("NBSS_NATIVE_STOI")
    check_off(SPATIAL, tmp_path / "off")
