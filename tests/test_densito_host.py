"""Host side of the per-lobe densitometry (no GPU): the header declares dram_lobe_hist_nblk / dram_lobe_hist and the
built library exports them; the launcher's argument checks are reached through ctypes with dummy pointers (no launch);
processor.densitometry_from_hist -- the tensor math between the histogram and the report -- on CPU tensors against the
flattened-selection yardstick of tests/densito_ref.py (counts and percentiles exactly, ratios to one float64
rounding); densitometry_metrics' formats and names; write_reports(densitometry_json=...); and the register / LDS /
spill audit of csrc/densito.hip."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import densito_ref as DR
from conftest import ROOT

ENTRY_POINTS = ("dram_lobe_hist_nblk", "dram_lobe_hist")


def test_entry_points_are_declared_and_exported():
    from ctypes import c_int as I, c_longlong as LL, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _build, _lib
    expect = {"dram_lobe_hist_nblk": [LL], "dram_lobe_hist": [P, P, I, LL, LL, P, P, P, P] + [I] * 6 + [P]}
    for name in ENTRY_POINTS:
        res, args = _lib.SIGNATURES[name]
        assert res is I and list(args) == expect[name], name
    path = _build.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRY_POINTS) <= exported, set(ENTRY_POINTS) - exported


def test_nblk_rule():
    """ceil(voxels / 8192) clamped to 1..256: 1024 threads x 8 voxels per workgroup and step"""
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    sizes = (0, 1, 8192, 8193, 255 * 8192 + 1, 256 * 8192 + 1, 350 * 300 * 400, (1 << 31) - 1)
    assert [lib.dram_lobe_hist_nblk(v) for v in sizes] == [1, 1, 1, 2, 256, 256, 256, 256]


def test_lobe_hist_refuses_bad_and_unsupported_arguments_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    one = ctypes.c_void_p(16)                   # never dereferenced: the argument checks come first

    def call(image=one, labels=one, code=1, sz=77, sy=11, ph=one, ps=one, hist=one, sums=one, size=(5, 7, 11), n=5,
             lo=-1024, nbins=1024):
        return lib.dram_lobe_hist(image, labels, code, sz, sy, ph, ps, hist, sums, *size, n, lo, nbins, None)

    for k in ("image", "labels", "ph", "ps", "hist", "sums"):
        assert call(**{k: None}) == BAD, k
    for code in (0, 3, -1):
        assert call(code=code) == BAD, code
    assert call(sz=-77) == BAD and call(sy=-11) == BAD
    for axis in range(3):
        for v in (0, -1):
            assert call(size=tuple(v if a == axis else s for a, s in enumerate((5, 7, 11)))) == BAD, (axis, v)
    for n in (0, -1, 16, 255):
        assert call(n=n) == BAD, n
    assert call(size=(2048, 1024, 1024)) == UNS and call(size=(1 << 30, 2, 1)) == UNS
    for nbins in (0, -64, 32, 100, 1000, 2112, 4096):
        assert call(nbins=nbins) == UNS, nbins
    assert call(n=15, nbins=2048 + 64) == UNS                         # 16 rows x 2048 bins is the largest image
    assert call(lo=-32769) == UNS and call(lo=32767 - 1022) == UNS    # bins outside int16
    assert call(size=(2048, 1024, 1024), n=16) == BAD                 # a bad argument is named first


def test_python_wrapper_refuses_before_any_launch():
    from bodyct_dram_emph_subtype_amd import ops
    img, lab = torch.zeros(2, 3, 4, dtype=torch.int16), torch.zeros(2, 3, 4, dtype=torch.uint8)
    for n in (0, 16):
        with pytest.raises(ValueError, match="n_regions"):
            ops.lobe_histogram(img, lab, n_regions=n)
    with pytest.raises(TypeError):
        ops.lobe_histogram(img, lab.float())
    with pytest.raises(TypeError):
        ops.lobe_histogram(img, lab.to(torch.int32))
    with pytest.raises(ValueError):
        ops.lobe_histogram(img, lab[:, :, :3])
    with pytest.raises(ValueError):
        ops.lobe_histogram(img[0], lab[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lobe_histogram(img, lab)


# ------------------------------------------------------------------------------------------------ the tensor math
def from_numpy_hist(scan, labels, spacing, n, thresholds, percentiles, hu_lo, nbins):
    """processor.densitometry_from_hist on CPU tensors, fed with a histogram counted by np.bincount"""
    from bodyct_dram_emph_subtype_amd import processor
    hu = np.asarray(scan).astype(np.int64).ravel()
    row = DR.rows_of(labels, n).ravel()
    keep = row >= 0
    key = row[keep] * nbins + np.clip(hu[keep], hu_lo, hu_lo + nbins - 1) - hu_lo
    hist = np.bincount(key, minlength=(n + 1) * nbins).reshape(n + 1, nbins).astype(np.int64)
    sums = np.stack([np.bincount(row[keep], minlength=n + 1),
                     np.array([hu[row == r].sum() for r in range(n + 1)])], axis=1).astype(np.int64)
    return processor.densitometry_from_hist(torch.from_numpy(hist), torch.from_numpy(sums), spacing, thresholds,
                                            percentiles, hu_lo)


def test_math_equals_the_yardstick_on_a_lung_like_volume():
    scan, labels = DR.lung_like((6, 40, 50), 5, seed=3)
    labels[labels == 4] = 0                                   # an empty region
    labels[0, 0, 10] = 9                                      # lung outside 1..5 -> row 0
    labels = labels.astype(np.int16)
    labels[0, 0, 11] = -3                                     # not lung
    kw = dict(n=5, thresholds=(-950, -910, -1023, -1), percentiles=(15, 1, 50, 99), hu_lo=-1024, nbins=1024)
    want = DR.densitometry(scan, labels, (2.5, 0.7, 0.8), **kw)
    got = from_numpy_hist(scan, labels, (2.5, 0.7, 0.8), **kw)
    DR.assert_matches(got, want, "lung-like")
    assert int(want["voxels"][4]) == 0 and np.isnan(want["mean_density"][4]) and np.isnan(want["perc"][0, 4])
    assert int(want["voxels"][0]) == 1 and int(want["whole_lung"]["voxels"]) == int((labels > 0).sum())
    assert np.isfinite(want["perc"][0, 1]) and -1024 < want["perc"][0, 1] < -1                # Perc15 inside the bins
    assert got["thresholds"] == (-950, -910, -1023, -1) and got["percentiles"] == (15, 1, 50, 99)


def test_math_edges_one_voxel_end_bins_rank_and_thresholds():
    hu_lo, nbins = -1024, 64                                  # bins -1024 .. -961; end bins -1024 and -961
    hi = hu_lo + nbins - 1
    scan = np.full((1, 4, 200), -1000, dtype=np.int16)
    labels = np.zeros((1, 4, 200), dtype=np.uint8)
    labels[0, 0, 0] = 1                                       # region 1: one voxel
    scan[0, 0, 0] = -990
    labels[0, 1, :] = 2                                       # region 2: 200 voxels -1010 .. -1001, 20 of each
    scan[0, 1, :] = np.repeat(np.arange(-1010, -1000), 20)
    labels[0, 2, :101] = 3                                    # region 3: 101 voxels, 15 in the low tail, 16 in the high
    scan[0, 2, :101] = -1000
    scan[0, 2, :15] = -2000
    scan[0, 2, 15:31] = 500
    labels[0, 3, :100] = 4                                    # region 4: 100 voxels = 15 x -1020, 85 x -1000
    scan[0, 3, :15] = -1020
    kw = dict(n=5, thresholds=(hu_lo + 1, hi), percentiles=(15, 16, 85, 10, 11), hu_lo=hu_lo, nbins=nbins)
    want = DR.densitometry(scan, labels, (1.0, 1.0, 1.0), **kw)
    got = from_numpy_hist(scan, labels, (1.0, 1.0, 1.0), **kw)
    DR.assert_matches(got, want, "edges")
    perc, P = got["perc"], {p: i for i, p in enumerate(kw["percentiles"])}
    assert perc[:, 1].tolist() == [-990.0] * 5                                  # one voxel: every percentile is it
    assert int(got["voxels"][5]) == 0 and bool(perc[:, 5].isnan().all())        # the empty region
    # region 2, N = 200: 10 % -> k = 20 exactly (the last -1010), 11 % -> k = 22 (the second -1009)
    assert perc[P[10], 2].item() == -1010.0 and perc[P[11], 2].item() == -1009.0
    # region 4, N = 100: p N divisible by 100: k = 15 -> the 15th value (-1020); 16 -> just above (-1000)
    assert perc[P[15], 4].item() == -1020.0 and perc[P[16], 4].item() == -1000.0
    # region 3, N = 101: k(15) = 16 > 15 voxels of the low tail -> inside; k(10) = 11 in the low end bin, k(85) = 86 in
    # the high end bin -> NaN
    assert perc[P[15], 3].item() == -1000.0 and math_isnan(perc[P[10], 3]) and math_isnan(perc[P[85], 3])
    # thresholds at hu_lo + 1 (counts the low end bin alone) and at hu_lo + nbins - 1 (everything but the high end bin)
    assert got["laa_counts"][:, 3].tolist() == [15, 85] and got["laa_counts"][:, 2].tolist() == [0, 200]
    assert got["mean_density"][3].item() == (15 * -2000 + 16 * 500 + 70 * -1000) / 101     # raw values, not clamped


def math_isnan(t):
    return bool(torch.isnan(t))


def test_thresholds_and_percentiles_outside_their_range_raise():
    from bodyct_dram_emph_subtype_amd import processor
    hist, sums = torch.zeros(3, 64, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int64)
    ok = processor.densitometry_from_hist(hist, sums, (1, 1, 1), (-1023, -961), (15,), -1024)
    assert bool(ok["laa"].isnan().all()) and ok["volume_ml"].tolist() == [0.0, 0.0, 0.0]
    for t in (-1024, -960, -2000, 0):
        with pytest.raises(ValueError, match="threshold"):
            processor.densitometry_from_hist(hist, sums, (1, 1, 1), (t,), (15,), -1024)
    for p in (0, 100, 15.5, -1):
        with pytest.raises(ValueError, match="percentile"):
            processor.densitometry_from_hist(hist, sums, (1, 1, 1), (-1000,), (p,), -1024)
    with pytest.raises(ValueError):
        processor.densitometry_from_hist(hist.int(), sums, (1, 1, 1))
    with pytest.raises(ValueError):
        processor.densitometry_from_hist(hist, sums[:2], (1, 1, 1))
    with pytest.raises(ValueError):
        processor.densitometry_from_hist(hist, sums, (1, 1))


# ------------------------------------------------------------------------------------------------ the report
def _result():
    nan = float("nan")
    t = lambda v, dt=torch.float64: torch.tensor(v, dtype=dt)
    return {"voxels": t([0, 1000, 0, 7], torch.int64), "volume_ml": t([0.0, 1234.56, 0.0, 0.049]),
            "mean_density": t([nan, -850.12345, nan, -1000.0]),
            "laa": t([[nan, 0.12345, nan, 1.0], [nan, 0.5, nan, 0.0005]]),
            "laa_counts": t([[0, 123, 0, 7], [0, 500, 0, 0]], torch.int64), "perc": t([[nan, -975.0, nan, nan]]),
            "whole_lung": {"voxels": t(1007, torch.int64), "volume_ml": t(1234.609), "mean_density": t(-851.2),
                           "laa": t([0.129, 0.4965]), "laa_counts": t([130, 500], torch.int64), "perc": t([-974.0])},
            "thresholds": (-950, -910), "percentiles": (15,), "hu_lo": -1024, "nbins": 1024}


DENSITO_KEYS = [f"{s}_per_{w}" for w in ("region", "lung")
                for s in ("laa950_fraction", "laa910_fraction", "perc15_hu", "mean_lung_density", "volume_ml")]


def test_densitometry_metrics_formats_names_and_nan():
    from bodyct_dram_emph_subtype_amd import processor
    m = processor.densitometry_metrics(_result())
    assert list(m) == DENSITO_KEYS
    assert m["laa950_fraction_per_region"] == {"1": "0.123", "2": None, "3": "1.000"}
    assert m["laa910_fraction_per_region"] == {"1": "0.500", "2": None, "3": "0.001"}
    assert m["perc15_hu_per_region"] == {"1": "-975", "2": None, "3": None}
    assert m["mean_lung_density_per_region"] == {"1": "-850.123", "2": None, "3": "-1000.000"}
    assert m["volume_ml_per_region"] == {"1": "1234.6", "2": "0.0", "3": "0.0"}
    assert [m[k] for k in DENSITO_KEYS[5:]] == ["0.129", "0.496", "-974", "-851.200", "1234.6"]
    names = {1: "RUL", 2: "RML", 3: "RLL"}
    named = processor.densitometry_metrics(_result(), names)
    assert named["perc15_hu_per_region"] == {"RUL": "-975", "RML": None, "RLL": None}
    assert processor.densitometry_metrics(_result(), ["-", "RUL", "RML", "RLL"]) == named
    assert list(processor.densitometry_metrics(_result(), {1: "RUL"})["volume_ml_per_region"]) == ["RUL", "2", "3"]
    assert json.loads(json.dumps(m))["perc15_hu_per_region"]["2"] is None
    other = dict(_result(), thresholds=(-856, -910), percentiles=(10,))
    assert {"laa856_fraction_per_region", "perc10_hu_per_lung"} <= set(processor.densitometry_metrics(other))


def _prediction():
    return {"cle_dense_outs": torch.zeros(1, 1, 2, 2, 2), "pse_dense_outs": torch.zeros(1, 1, 2, 2, 2),
            "cle_precentages": torch.tensor([0.02]), "pse_precentages": torch.tensor([0.3]),
            "crop_slices": torch.tensor([[[0, 2], [0, 2], [0, 2]]]), "original_size": torch.tensor([[2, 2, 2]]), "uids": ["u"]}


def test_write_reports_densitometry_json(monkeypatch, tmp_path):
    from bodyct_dram_emph_subtype_amd import processor
    monkeypatch.setattr(processor, "resample_paste", lambda d, *a, **k: (None, torch.zeros(2, 2, 2, dtype=torch.uint8)))
    plain = processor.build_outputs([_prediction()])[0]
    dens = processor.build_outputs([_prediction()])[0]
    dens["metrics"].update(processor.densitometry_metrics(_result()))
    names = ("centrilobular_json", "paraseptal_json", "output_json")
    before = {k: str(tmp_path / f"a_{k}") for k in names}
    after = {k: str(tmp_path / f"b_{k}") for k in names}
    processor.write_reports([plain], **before)
    processor.write_reports([plain], **after, densitometry_json=None)
    for k in names:                                                    # without the argument: byte for byte as before
        assert open(before[k], "rb").read() == open(after[k], "rb").read(), k
    assert json.load(open(before["centrilobular_json"])) == {"score": 1, "percentage": 0.02}
    path = str(tmp_path / "densitometry.json")
    processor.write_reports([dens], **after, densitometry_json=path)
    assert json.load(open(path)) == json.loads(json.dumps(processor.densitometry_metrics(_result())))
    assert list(json.load(open(path))) == DENSITO_KEYS
    for k in names[:2]:                                                # the two score files do not see the new keys
        assert open(before[k], "rb").read() == open(after[k], "rb").read(), k
    assert json.load(open(after["output_json"]))[0]["metrics"] == dens["metrics"]
    with pytest.raises(ValueError, match="densitometry_json"):
        processor.write_reports([plain], densitometry_json=path)
    with pytest.raises(ValueError, match="regions_json"):
        processor.write_reports([dens], regions_json=str(tmp_path / "r.json"))


# ------------------------------------------------------------------------------------------------ the kernels' resources
def test_hist_kernels_use_the_lds_their_header_states_and_do_not_spill():
    """tools/isa_waits.py --table on csrc/densito.hip: no spills (the 8 voxels of a group stay in registers), the LDS
    bytes per workgroup the file header records -- the counter image of 8192 / 16384 / 32768 counters + 4224 B for the
    excess sums and the fold -- and at most 128 VGPRs (1024 threads per workgroup)."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not present")
    src = os.path.join(ROOT, "bodyct-dram-emph-subtype_amd", "csrc", "densito.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_waits.py"), "--table", src],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for l in r.stdout.splitlines():
        if " vgpr " not in l:
            continue
        name = l.split("vgpr")[0].split(None, 1)[1].strip()
        vgpr, lds, spills = (int(l.split(k)[1].split()[0]) for k in ("vgpr", "lds", "spills"))
        assert spills == 0 and vgpr <= 128, l
        seen[name] = lds
    assert seen.pop("lobe_hist_fold_kernel") == 16 * 64 * 8
    assert len(seen) == 6 and all(n.startswith("lobe_hist_kernel<") for n in seen), r.stdout
    for name, lds in seen.items():
        counters = int(name.rstrip(">").split(",")[1])
        assert lds == 4 * counters + 16 * 8 + 16 * 16 * 2 * 8 and lds <= 160 * 1024, (name, lds)
    assert sorted(set(seen.values())) == [36992, 69760, 135296]
