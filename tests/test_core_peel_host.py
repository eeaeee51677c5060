"""Host side of the core / peel split (no GPU): the yardstick of tests/edt_ref.py against the definition (a brute force
over all background voxels) and, where scipy is present, against scipy.ndimage.distance_transform_edt; the header's
entry points and the launcher's argument checks through ctypes with dummy pointers (no launch); ops.lung_zones'
argument errors, which fire before the device is touched; the per-zone tensor math of processor.core_peel on CPU
tensors; core_peel_metrics / zone_region_metrics / fold_zone_table formats and names; write_reports(core_peel_json)."""
import ctypes
import json
import math
import subprocess

import numpy as np
import pytest
import torch

import case_prep_ref as CR
import densito_ref as DR
import edt_ref as ER

TINY = {"5x7x11": ((5, 7, 11), (2.5, 0.7, 0.65)), "6x9x13": ((6, 9, 13), (0.8, 1.4, 0.6))}


def tiny_lung(shape, seed):
    return np.random.default_rng(seed).random(shape) < 0.8


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("max_mm", [math.inf, 1.5], ids=["full", "capped"])
@pytest.mark.parametrize("sid", sorted(TINY))
def test_yardstick_equals_the_brute_force(sid, max_mm):
    shape, spacing = TINY[sid]
    lung = tiny_lung(shape, seed=len(sid) + shape[0])
    s, _, mx = ER.units(spacing, 1.5, max_mm)
    got, want = ER.dist2(lung, s, mx), ER.brute(lung, s, mx)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(got == 0, ~lung)
    n_inf = int((got == ER.INF).sum())
    print(f"[{sid} {max_mm}] lung {int(lung.sum())}, +inf {n_inf}, largest finite {int(got[got != ER.INF].max())} um^2")
    assert (n_inf > 0) == (mx is not None)                 # 1.5 mm caps some voxels, the full transform reaches all
    one = lung.copy()                                      # a lung voxel beside a background one: d2 = s_a^2
    one[:] = True
    one[2, 3, 4] = False
    d = ER.dist2(one, s)
    assert [int(d[3, 3, 4]), int(d[2, 4, 4]), int(d[2, 3, 5])] == [s[0] ** 2, s[1] ** 2, s[2] ** 2]
    assert bool((ER.dist2(np.ones(shape, bool), s) == ER.INF).all())          # no background: +inf everywhere


def test_yardstick_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    cases = [(tiny_lung(shape, 3), spacing) for shape, spacing in TINY.values()]
    for name in ("blobs_u8", "lobes_i16"):
        _, lobes, spacing, _ = CR.fixture_cases()[name]
        cases.append((lobes.numpy() > 0, spacing))
    for lung, spacing in cases:
        s, _, _ = ER.units(spacing)
        want = np.rint(ndi.distance_transform_edt(lung, sampling=[float(v) for v in s]) ** 2).astype(np.int64)
        assert np.array_equal(ER.dist2(lung, s), want), lung.shape


def test_zones_and_labels_of_the_yardstick():
    d2 = np.array([[[0, 25, 26, ER.INF, 9, 9]]], dtype=np.int64)
    lab = np.array([[[0, 1, 2, 3, 9, -4]]], dtype=np.int16)
    lung = lab > 0
    d2 = np.where(lung, d2, 0)
    z = ER.zones(d2, lung, 5)
    assert z.tolist() == [[[0, 1, 2, 2, 1, 0]]]                                # equality is peel, +inf is core
    assert ER.zone_labels(lab, z, 3).tolist() == [[[0, 1, 5, 6, 255, 0]]]
    assert ER.dist_mm(np.array([4000000, ER.INF, 7]), np.array([True, True, False])).tolist() == [2.0, math.inf, 0.0]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_and_exported():
    from ctypes import c_int as I, c_longlong as LL, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _build, _lib
    assert _lib.SIGNATURES["dram_lung_zones_workspace"] == (LL, [I, I, I, LL])
    res, args = _lib.SIGNATURES["dram_lung_zones"]
    assert res is I and list(args) == [P, I, LL, LL, P, P, P, P] + [I] * 6 + [LL, LL, I, P]
    out = subprocess.run(["nm", "-D", "--defined-only", _build.build_library()], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"dram_lung_zones", "dram_lung_zones_workspace"} <= exported


def test_workspace_rule():
    """two work volumes, each rounded up to 256 bytes: uint32 up to max_um = 65535, uint64 above"""
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    up = lambda b: -(-b // 256) * 256
    assert lib.dram_lung_zones_workspace(5, 7, 11, 10000) == 2 * up(385 * 4)
    assert lib.dram_lung_zones_workspace(5, 7, 11, 65535) == 2 * up(385 * 4)
    assert lib.dram_lung_zones_workspace(5, 7, 11, 65536) == 2 * up(385 * 8)
    assert lib.dram_lung_zones_workspace(64, 256, 300, 1 << 26) == 2 * 64 * 256 * 300 * 8
    assert lib.dram_lung_zones_workspace(0, 7, 11, 10000) == 0 and lib.dram_lung_zones_workspace(2048, 1024, 1024, 1) == 0


def test_lung_zones_refuses_bad_and_unsupported_arguments_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    one = ctypes.c_void_p(256)                  # never dereferenced: the argument checks come first

    def call(labels=one, code=1, sz=77, sy=11, zones=one, zl=one, dist=one, ws=one, size=(5, 7, 11), sp=(2500, 700, 650),
             peel=3000, mx=3000, n=5):
        return lib.dram_lung_zones(labels, code, sz, sy, zones, zl, dist, ws, *size, *sp, peel, mx, n, None)

    for k in ("labels", "zones", "ws"):
        assert call(**{k: None}) == BAD, k
    for code in (0, 3, -1):
        assert call(code=code) == BAD, code
    assert call(sz=-77) == BAD and call(sy=-11) == BAD
    for axis in range(3):
        for v in (0, -1):
            assert call(size=tuple(v if a == axis else s for a, s in enumerate((5, 7, 11)))) == BAD, (axis, v)
    for n in (0, -1, 8, 15):
        assert call(n=n) == BAD, n
    assert call(zl=None, n=5) == BAD                                          # regions without a place for their labels
    assert call(peel=-1) == BAD and call(peel=3001) == BAD                    # max_um < peel_um
    assert call(size=(2048, 1024, 1024)) == UNS
    for axis in range(3):
        for v in (0, -5, 20001):
            assert call(sp=tuple(v if a == axis else s for a, s in enumerate((2500, 700, 650)))) == UNS, (axis, v)
    assert call(size=(5, 7, 1 + (1 << 25) // 650 + 1)) == UNS                 # (W - 1) * sx >= 2^25
    assert call(size=(1 + (1 << 25) // 2500 + 1, 7, 11)) == UNS
    assert call(size=(2048, 1024, 1024), n=8) == BAD                          # a bad argument is named first


def test_python_wrapper_refuses_before_the_device_is_touched():
    from bodyct_dram_emph_subtype_amd import ops
    lab = torch.zeros(2, 3, 4, dtype=torch.uint8)
    sp = (1.0, 0.7, 0.7)
    for n in (0, 8, -1):
        with pytest.raises(ValueError, match="n_regions"):
            ops.lung_zones(lab, sp, 3.0, n_regions=n)
    with pytest.raises(ValueError, match="max_mm"):
        ops.lung_zones(lab, sp, 3.0, max_mm=2.0)
    for bad in ((0.0, 0.7, 0.7), (1.0, -0.7, 0.7), (1.0, 0.7, math.inf), (1.0, math.nan, 0.7), (1.0, 0.7), (25.0, 1.0, 1.0),
                (1.0, 1.0, 0.0004)):
        with pytest.raises(ValueError, match="spacing"):
            ops.lung_zones(lab, bad, 3.0)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="peel_mm"):
            ops.lung_zones(lab, sp, bad)
    with pytest.raises(ValueError, match="2\\^25"):
        ops.lung_zones(torch.zeros(1, 1, 1680, dtype=torch.uint8).expand(2, 3, 1680), (1.0, 1.0, 20.0), 3.0)
    with pytest.raises(TypeError):
        ops.lung_zones(lab.to(torch.int32), sp, 3.0)
    with pytest.raises(TypeError):
        ops.lung_zones(lab.float(), sp, 3.0)
    with pytest.raises(ValueError):
        ops.lung_zones(lab[0], sp, 3.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lung_zones(lab, sp, 3.0, n_regions=5, max_mm=math.inf, want_dist=True)
    s_um, peel_um, max_um = ops.lung_zones_units((1.25, 0.7, 0.65), 10.0)
    assert (s_um, peel_um, max_um) == ((1250, 700, 650), 10000, 10000)
    assert ops.lung_zones_units(sp, 10.0, math.inf)[2] == ops.EDT_FULL_UM == 1 << 26
    assert ops.lung_zones_units(sp, 10.0, 70.0)[2] == 70000


# ------------------------------------------------------------------------------------------------ the tensor math
def test_per_zone_math_equals_the_yardstick(monkeypatch):
    """processor.core_peel on CPU tensors, its two kernels replaced by the yardstick's label volume and np.bincount:
    the row slicing, the zero row 0 and each zone's whole_lung"""
    from bodyct_dram_emph_subtype_amd import ops, processor
    shape, spacing, n = (6, 40, 50), (2.5, 0.7, 0.8), 5
    scan, labels = DR.lung_like(shape, n, seed=3)
    labels = labels.astype(np.int16)
    labels[labels == 4] = 0                                   # an absent lobe
    labels[2, 20, 10:14] = 9                                  # lung outside 1..5
    labels[0, 0, 11] = -3
    want = ER.core_peel(scan, labels, spacing, 2.0, n)

    def zones_stub(lab, sp, peel_mm, n_regions=None, **kw):
        assert n_regions == n and peel_mm == 2.0
        return torch.from_numpy(want["zones"]), torch.from_numpy(want["zone_labels"]), None

    def hist_stub(image, zl, rows, hu_lo, nbins):
        assert rows == 2 * n
        h, s = DR.histogram(image.numpy(), zl.numpy(), rows, hu_lo, nbins)
        return torch.from_numpy(h), torch.from_numpy(s)

    monkeypatch.setattr(ops, "lung_zones", zones_stub)
    monkeypatch.setattr(ops, "lobe_histogram", hist_stub)
    got = processor.core_peel(torch.from_numpy(scan), torch.from_numpy(labels), spacing, 2.0, n)
    assert set(got) == {"peel", "core", "outside_voxels", "zones", "zone_labels", "peel_mm", "n_regions"}
    for zone in ("peel", "core"):
        DR.assert_matches(got[zone], want[zone], zone)
        assert int(got[zone]["voxels"][0]) == 0 and int(got[zone]["voxels"][4]) == 0
        assert int(got[zone]["voxels"][1]) > 0, zone            # both zones are populated
    assert got["outside_voxels"].dim() == 0 and got["outside_voxels"].dtype == torch.int64
    assert int(got["outside_voxels"]) == want["outside_voxels"] == 4
    whole = DR.densitometry(scan, labels, spacing, n)
    assert np.array_equal((got["peel"]["voxels"] + got["core"]["voxels"]).numpy()[1:], whole["voxels"][1:])
    assert np.array_equal((got["peel"]["laa_counts"] + got["core"]["laa_counts"]).numpy()[:, 1:], whole["laa_counts"][:, 1:])
    other = processor.core_peel(torch.from_numpy(scan), torch.from_numpy(labels), spacing, 2.0, n, thresholds=(-856,),
                                percentiles=(10, 50), hu_lo=-1100, nbins=2048)
    want2 = ER.core_peel(scan, labels, spacing, 2.0, n, thresholds=(-856,), percentiles=(10, 50), hu_lo=-1100, nbins=2048)
    DR.assert_matches(other["core"], want2["core"], "other bins")


# ------------------------------------------------------------------------------------------------ the report
def _dens(scale):
    nan = float("nan")
    t = lambda v, dt=torch.float64: torch.tensor(v, dtype=dt)
    return {"voxels": t([0, 1000 * scale, 0, 7], torch.int64), "volume_ml": t([0.0, 1234.56 * scale, 0.0, 0.049]),
            "mean_density": t([nan, -850.12345, nan, -1000.0]),
            "laa": t([[nan, 0.12345, nan, 1.0], [nan, 0.5, nan, 0.0005]]),
            "laa_counts": t([[0, 123, 0, 7], [0, 500, 0, 0]], torch.int64), "perc": t([[nan, -975.0, nan, nan]]),
            "whole_lung": {"voxels": t(1007, torch.int64), "volume_ml": t(1234.609), "mean_density": t(-851.2),
                           "laa": t([0.129, 0.4965]), "laa_counts": t([130, 500], torch.int64), "perc": t([nan])},
            "thresholds": (-950, -910), "percentiles": (15,), "hu_lo": -1024, "nbins": 1024}


def _result():
    return {"peel": _dens(1), "core": _dens(2), "outside_voxels": torch.tensor(0), "peel_mm": 7.5, "n_regions": 3}


STEMS = ("laa950_fraction", "laa910_fraction", "perc15_hu", "mean_lung_density", "volume_ml")


def test_core_peel_metrics_formats_names_and_none():
    from bodyct_dram_emph_subtype_amd import processor
    m = processor.core_peel_metrics(_result())
    want_keys = {f"{s}_per_{w}_{z}" for s in STEMS for w in ("region", "lung") for z in ("peel", "core")} | {"peel_mm"}
    assert set(m) == want_keys and len(m) == 21
    assert m["peel_mm"] == "7.500"
    assert m["laa950_fraction_per_region_peel"] == {"1": "0.123", "2": None, "3": "1.000"}
    assert m["perc15_hu_per_region_core"] == {"1": "-975", "2": None, "3": None}
    assert m["volume_ml_per_region_peel"] == {"1": "1234.6", "2": "0.0", "3": "0.0"}
    assert m["volume_ml_per_region_core"] == {"1": "2469.1", "2": "0.0", "3": "0.0"}
    assert m["mean_lung_density_per_lung_core"] == "-851.200" and m["perc15_hu_per_lung_peel"] is None
    for zone in ("peel", "core"):                              # densitometry_metrics' own formats, renamed
        plain = processor.densitometry_metrics(_result()[zone])
        assert {k[:-len(zone) - 1]: v for k, v in m.items() if k.endswith("_" + zone)} == plain
    named = processor.core_peel_metrics(_result(), {1: "RUL", 2: "RML", 3: "RLL"})
    assert named["perc15_hu_per_region_peel"] == {"RUL": "-975", "RML": None, "RLL": None}
    assert json.loads(json.dumps(m))["perc15_hu_per_region_peel"]["2"] is None
    other = dict(_result(), peel=dict(_dens(1), thresholds=(-856, -910)), core=dict(_dens(2), thresholds=(-856, -910)))
    assert "laa856_fraction_per_lung_core" in processor.core_peel_metrics(other)


TABLE = [[5.0, 6.0, 7.0, 100.0],            # row 0
         [10.0, 1.0, 3.0, 40.0], [0.0, 0.0, 0.0, 0.0],          # peel of lobes 1, 2
         [2.5, 0.5, 1.0, 10.0], [0.0, 0.0, 0.0, 0.0]]           # core of lobes 1, 2


def test_zone_region_metrics_and_the_fold():
    from bodyct_dram_emph_subtype_amd import processor
    m = processor.zone_region_metrics(torch.tensor(TABLE, dtype=torch.float64), {1: "RUL"})
    assert set(m) == {f"{h}_lesion_percentage_per_{w}_{z}" for h in ("cle", "pse") for w in ("region", "lung")
                      for z in ("peel", "core")} | {"region_voxels_peel", "region_voxels_core"}
    assert m["cle_lesion_percentage_per_region_peel"] == {"RUL": "0.250", "2": None}
    assert m["pse_lesion_percentage_per_region_core"] == {"RUL": "0.050", "2": None}
    assert m["region_voxels_peel"] == {"RUL": "40", "2": "0"} and m["region_voxels_core"] == {"RUL": "10", "2": "0"}
    assert m["cle_lesion_percentage_per_lung_peel"] == "0.250" and m["pse_lesion_percentage_per_lung_core"] == "0.050"
    empty = [r if i < 3 else [0.0] * 4 for i, r in enumerate(TABLE)]
    e = processor.zone_region_metrics(empty)
    assert e["cle_lesion_percentage_per_lung_core"] is None and e["region_voxels_core"] == {"1": "0", "2": "0"}
    assert not any("severity" in k for k in m)
    folded = processor.fold_zone_table(TABLE)
    assert folded.dtype == torch.float64 and folded.tolist() == [TABLE[0], [12.5, 1.5, 4.0, 50.0], [0.0] * 4]
    assert processor.region_metrics(folded)["cle_lesion_percentage_per_region"] == {"1": "0.250", "2": None}
    for bad in (TABLE[:4], TABLE[:1], [r[:3] for r in TABLE]):
        with pytest.raises(ValueError):
            processor.zone_region_metrics(bad)
    with pytest.raises(ValueError):
        processor.fold_zone_table(TABLE[:4])


def _prediction():
    return {"cle_dense_outs": torch.zeros(1, 1, 2, 2, 2), "pse_dense_outs": torch.zeros(1, 1, 2, 2, 2),
            "cle_precentages": torch.tensor([0.02]), "pse_precentages": torch.tensor([0.3]),
            "crop_slices": torch.tensor([[[0, 2], [0, 2], [0, 2]]]), "original_size": torch.tensor([[2, 2, 2]]), "uids": ["u"]}


def test_write_reports_core_peel_json(monkeypatch, tmp_path):
    from bodyct_dram_emph_subtype_amd import processor
    monkeypatch.setattr(processor, "resample_paste", lambda d, *a, **k: (None, torch.zeros(2, 2, 2, dtype=torch.uint8)))
    plain = processor.build_outputs([_prediction()])[0]
    cp = processor.build_outputs([_prediction()])[0]
    added = dict(processor.core_peel_metrics(_result()), **processor.zone_region_metrics(TABLE))
    cp["metrics"].update(added)
    names = ("centrilobular_json", "paraseptal_json", "output_json")
    before = {k: str(tmp_path / f"a_{k}") for k in names}
    after = {k: str(tmp_path / f"b_{k}") for k in names}
    processor.write_reports([plain], **before)
    processor.write_reports([plain], **after, core_peel_json=None)
    for k in names:                                                    # without the argument: byte for byte as before
        assert open(before[k], "rb").read() == open(after[k], "rb").read(), k
    path = str(tmp_path / "core_peel.json")
    processor.write_reports([cp], **after, core_peel_json=path)
    assert json.load(open(path)) == json.loads(json.dumps(added)) and len(added) == 31
    for k in names[:2]:                                                # the two score files do not see the new keys
        assert open(before[k], "rb").read() == open(after[k], "rb").read(), k
    assert json.load(open(after["output_json"]))[0]["metrics"] == cp["metrics"]
    with pytest.raises(ValueError, match="core_peel_json"):
        processor.write_reports([plain], core_peel_json=path)
    half = processor.build_outputs([_prediction()])[0]
    half["metrics"].update(processor.core_peel_metrics(_result()))     # the scan side alone is not the report
    with pytest.raises(ValueError, match="core_peel_json"):
        processor.write_reports([half], core_peel_json=path)
    with pytest.raises(ValueError, match="densitometry_json"):         # the zone keys are not the plain densitometry's
        processor.write_reports([cp], densitometry_json=str(tmp_path / "d.json"))
