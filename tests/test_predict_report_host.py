"""Host side of the whole predict report (no GPU): processor.predict_case + processor.write_reports on CPU tensors, every
kernel wrapper replaced by its numpy yardstick, for the 16 combinations of regions / densitometry / core_peel / clusters
with and without region names -- held string for string (metric order included: output_json is dumped in insertion
order) to tests/golden/predict_report.json, which tests/golden/make_golden_report.py recorded at the commit before the
report path was rewritten over one section table."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_report", os.path.join(GOLDEN, "make_golden_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "predict_report.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded(gen):
    return gen.record()


def test_the_fixture_reaches_every_corner(gen, golden):
    """what the golden is worth: None entries, all four error lines, a NaN cluster fit, a mean that prints -0.000"""
    assert len(golden) == 32
    full = json.loads(golden["1111/named"]["entry"])
    m, errors = full["metrics"], full["error_messages"]
    assert [e.split(":")[0].split(" ", 1)[1] for e in errors] == [
        "ess voxels carry a lobe label outside 1..5", "lung voxels carry a lobe label outside 1..5",
        "lung voxels carry a lobe label outside 1..5", "low-attenuation voxels carry a lobe label outside 1..5"]
    assert errors[1].endswith("their density is in no region") and errors[2].endswith("peel or core")
    assert m["region_voxels"]["4"] == "0" and m["cle_lesion_percentage_per_region"]["4"] is None     # a lobe without voxels
    assert m["mean_lung_density_per_region"]["4"] is None and m["volume_ml_per_region_core"]["5"] == "0.0"
    assert m["laa950_cluster_d_per_region"] == {"RUL": "0.792", "2": None, "RLL": None, "4": None, "5": None}
    assert m["laa950_clusters_per_region"]["2"] == "4"                       # clusters, yet no fit: D is NaN, not absent
    assert m["mean_lung_density_per_lung"] == "-0.000"                       # densitometry keeps the sign
    assert list(m)[:4] == ["cle_severity_score", "cle_lesion_percentage_per_lung", "pse_severity_score",
                           "pse_lesion_percentage_per_lung"]
    assert json.loads(golden["0000/plain"]["entry"]) == {"metrics": {k: m[k] for k in list(m)[:4]}, "error_messages": []}
    assert set(golden["0000/plain"]["refused"]) == set(gen.SWITCH_ARG.values()) and not golden["1111/plain"]["refused"]
    assert set(golden["1111/plain"]["files"]) == set(gen.BASE_ARGS) | set(gen.SWITCH_ARG.values())


def test_every_combination_equals_the_recorded_report(recorded, golden):
    assert sorted(recorded) == sorted(golden)
    for run in sorted(golden):
        got, want = recorded[run], golden[run]
        assert got["entry"] == want["entry"], run
        assert sorted(got["files"]) == sorted(want["files"]), run
        for arg in want["files"]:
            assert got["files"][arg] == want["files"][arg], (run, arg)
        assert got["refused"] == want["refused"], run


def test_densitometry_keeps_the_sign_of_zero_and_the_clusters_drop_it():
    """the one difference between the two formatters' callers, asserted directly"""
    import torch
    from bodyct_dram_emph_subtype_amd import processor
    t = lambda v, dt=torch.float64: torch.tensor(v, dtype=dt)
    dens = {"mean_density": t([-0.0004, -0.0004, 0.0004]), "volume_ml": t([0.0, -0.04, 1.0]), "laa": t([[0.0, 0.5, -0.0]]),
            "perc": t([[float("nan"), -0.0, 3.0]]), "thresholds": (-950,), "percentiles": (15,),
            "whole_lung": {"mean_density": t(-0.0004), "volume_ml": t(1.0), "laa": t([-0.0001]), "perc": t([-900.0])}}
    m = processor.densitometry_metrics(dens)
    assert m["mean_lung_density_per_lung"] == "-0.000" and m["mean_lung_density_per_region"] == {"1": "-0.000", "2": "0.000"}
    assert m["laa950_fraction_per_lung"] == "-0.000" and m["volume_ml_per_region"]["1"] == "-0.0"
    assert m["perc15_hu_per_region"] == {"1": "0", "2": "3"}
    assert processor._fmt(-0.0004, "{:.3f}") == "-0.000" and processor._fmt(-0.0004, "{:.3f}", unsigned_zero=True) == "0.000"
    assert processor._fmt(-0.0006, "{:.3f}", unsigned_zero=True) == "-0.001"
    assert processor._fmt(float("nan"), "{:d}", int) is None and processor._fmt(None, "{:d}", int) is None
    with pytest.raises(ValueError, match="densitometry_metrics: the result must hold rows 0..n_regions"):
        processor.densitometry_metrics(dict(dens, mean_density=t([1.0])))
    with pytest.raises(ValueError, match="laa_cluster_metrics: the result must hold rows 0..n_regions"):
        processor.laa_cluster_metrics({"threshold": -950, "connectivity": 6, "clusters": t([1], torch.int64),
                                       "largest_ml": t([1.0]), "d": t([1.0]),
                                       "whole_lung": {"clusters": t(1, torch.int64), "largest_ml": t(1.0), "d": t(1.0)}})
