"""Host side of the fissural rind (no GPU): the yardstick of tests/fissure_ref.py (one binary transform per class)
against the definition (a brute force over all sites of another class); the header's entry points and the launcher's
argument checks through ctypes with dummy pointers (no launch); ops.lobe_zones' argument errors, which fire before the
device is touched; the three-zone tensor math of processor.core_peel(fissure_mm=...) on CPU tensors; the formats of
core_peel_metrics / zone_region_metrics / fold_zone_table with three zones and their unchanged defaults;
predict_case's refusals before any device work; the section table and write_reports(core_peel_json)."""
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
import fissure_ref as FR

TINY = {"5x7x11": ((5, 7, 11), (2.5, 0.7, 0.65)), "6x9x13": ((6, 9, 13), (0.8, 1.4, 0.6)), "4x4x9": ((4, 4, 9), (1.0, 1.0, 1.0))}


def tiny_labels(shape, n, seed):
    """x-runs of classes 1..n (ties: equal distances to several classes) with background holes inside the runs, a label
    above n (n + 1 and 300: lung, no site) and negatives (not lung)"""
    rng = np.random.default_rng(seed)
    lab = np.resize(np.repeat(rng.integers(1, n + 1, size=40), 3), math.prod(shape)).reshape(shape).astype(np.int16)
    lab[rng.random(shape) < 0.15] = 0
    flat = lab.reshape(-1)
    pos = rng.choice(flat.size, size=max(6, flat.size // 30), replace=False)
    flat[pos] = np.resize(np.array([300, -1, n + 1, -32768, n + 1, -7], dtype=np.int16), pos.size)
    return lab


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("max_mm", [math.inf, 1.5], ids=["full", "capped"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("sid", sorted(TINY))
def test_yardstick_equals_the_brute_force(sid, n, max_mm):
    shape, spacing = TINY[sid]
    lab = tiny_labels(shape, n, seed=n + shape[2])
    cls = FR.classes(lab, n)
    assert (lab < 0).any() and (lab == 300).any() and (cls == n + 1).any() and (cls == 0).any()
    assert sorted(set(cls.ravel().tolist())) == list(range(n + 2))               # every class 0..n+1 is present
    s, _, _, mx = FR.units(spacing, 1.5, 1.5, max_mm)
    got, want = FR.f2(lab, s, n, mx), FR.brute(lab, s, n, mx)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert bool((got[cls == 0] == 0).all()) and bool((got[cls > 0] > 0).all())
    fin = got[(cls > 0) & (got != FR.INF)]
    print(f"[{sid} n={n} {max_mm}] lung {int((cls > 0).sum())}, +inf {int((got == FR.INF).sum())}, "
          f"finite {fin.size}, largest {int(fin.max()) if fin.size else None} um^2")
    if n == 1:                                                                   # one class: only class n + 1 has a foreign site
        assert bool((got[cls == 1] == FR.INF).all()) and (got[cls == 2] != FR.INF).any()


def test_yardstick_by_hand():
    s = (2500, 700, 650)
    lab = np.full((5, 7, 11), 1, dtype=np.int16)
    lab[2, 3, 4] = 2
    f = FR.f2(lab, s, 5)
    assert [int(f[3, 3, 4]), int(f[2, 4, 4]), int(f[2, 3, 5])] == [s[0] ** 2, s[1] ** 2, s[2] ** 2]   # beside a foreign voxel
    assert int(f[2, 3, 4]) == s[2] ** 2                                        # the lone voxel: its nearest neighbour
    assert bool((FR.f2(np.full((3, 4, 5), 2, np.int16), s, 5) == FR.INF).all())  # one class only: +inf everywhere
    lab = np.full((1, 1, 6), 1, dtype=np.int16)
    lab[0, 0, 3:] = [6, 6, 2]                                                  # a label above n between two lobes
    f = FR.f2(lab, (1000, 1000, 1000), 5)[0, 0]
    assert f.tolist() == [25_000_000, 16_000_000, 9_000_000, 1_000_000, 1_000_000, 9_000_000]   # 6 is no site, but has f2
    z = FR.zones(np.array([0, 9, 26, 26, 26, 26]), np.array([0, 1, 16, 17, FR.INF, 1]), np.array([0, 1, 1, 1, 1, 1], bool), 5, 4)
    assert z.tolist() == [0, 1, 3, 2, 2, 3]                                    # the peel wins; equality is rind; +inf is core
    assert ER.zone_labels(np.array([0, 1, 2, 3, 9, 3]), z, 3).tolist() == [0, 1, 8, 6, 255, 9]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_and_exported():
    from ctypes import c_int as I, c_longlong as LL, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _build, _lib
    assert _lib.SIGNATURES["dram_lobe_zones_workspace"] == (LL, [I, I, I, LL])
    res, args = _lib.SIGNATURES["dram_lobe_zones"]
    assert res is I and list(args) == [P, I, LL, LL, P, P, P, P, P] + [I] * 6 + [LL, LL, LL, I, P]
    out = subprocess.run(["nm", "-D", "--defined-only", _build.build_library()], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"dram_lobe_zones", "dram_lobe_zones_workspace"} <= exported


def test_workspace_rule():
    """dram_lung_zones' two work volumes, then two volumes of 16-byte pairs, each rounded up to 256 bytes"""
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    up = lambda b: -(-b // 256) * 256
    for mx, elem in ((10000, 4), (65535, 4), (65536, 8), (1 << 26, 8)):
        assert lib.dram_lobe_zones_workspace(5, 7, 11, mx) == 2 * up(385 * elem) + 2 * up(385 * 16), mx
        assert lib.dram_lobe_zones_workspace(5, 7, 11, mx) == lib.dram_lung_zones_workspace(5, 7, 11, mx) + 2 * up(385 * 16)
    assert lib.dram_lobe_zones_workspace(0, 7, 11, 10000) == 0 and lib.dram_lobe_zones_workspace(2048, 1024, 1024, 1) == 0


def test_lobe_zones_refuses_bad_and_unsupported_arguments_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    one = ctypes.c_void_p(256)                  # never dereferenced: the argument checks come first

    def call(labels=one, code=1, sz=77, sy=11, zones=one, zl=one, pl=one, fo=one, ws=one, size=(5, 7, 11),
             sp=(2500, 700, 650), peel=3000, fis=2000, mx=3000, n=5):
        return lib.dram_lobe_zones(labels, code, sz, sy, zones, zl, pl, fo, ws, *size, *sp, peel, fis, mx, n, None)

    for k in ("labels", "zones", "ws"):
        assert call(**{k: None}) == BAD, k
    for code in (0, 3, -1):
        assert call(code=code) == BAD, code
    assert call(sz=-77) == BAD and call(sy=-11) == BAD
    for axis in range(3):
        for v in (0, -1):
            assert call(size=tuple(v if a == axis else s for a, s in enumerate((5, 7, 11)))) == BAD, (axis, v)
    for n in (0, -1, 6, 7, 15):
        assert call(n=n) == BAD, n
        assert call(n=n, zl=None) == BAD, n                                   # the classes need n with or without labels
    assert call(peel=-1) == BAD and call(fis=-1) == BAD
    assert call(peel=3001) == BAD and call(fis=3001) == BAD                   # max_um below either width
    assert call(size=(2048, 1024, 1024)) == UNS
    for axis in range(3):
        for v in (0, -5, 20001):
            assert call(sp=tuple(v if a == axis else s for a, s in enumerate((2500, 700, 650)))) == UNS, (axis, v)
    assert call(size=(5, 7, 1 + (1 << 25) // 650 + 1)) == UNS                 # (W - 1) * sx >= 2^25
    assert call(size=(2048, 1024, 1024), n=6) == BAD                          # a bad argument is named first


def test_python_wrapper_refuses_before_the_device_is_touched():
    from bodyct_dram_emph_subtype_amd import ops
    lab = torch.zeros(2, 3, 4, dtype=torch.uint8)
    sp = (1.0, 0.7, 0.7)
    for n in (0, 6, 7, -1):
        with pytest.raises(ValueError, match="n_regions"):
            ops.lobe_zones(lab, sp, 3.0, 2.0, n_regions=n)
    for kw in (dict(max_mm=2.5), dict(max_mm=math.nan)):
        with pytest.raises(ValueError, match="max_mm"):
            ops.lobe_zones(lab, sp, 3.0, 2.0, **kw)
    with pytest.raises(ValueError, match="max_mm"):
        ops.lobe_zones(lab, sp, 2.0, 3.0, max_mm=2.5)                          # below the fissure width
    for bad in ((0.0, 0.7, 0.7), (1.0, 0.7, math.inf), (1.0, 0.7), (25.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            ops.lobe_zones(lab, bad, 3.0, 2.0)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="peel_mm"):
            ops.lobe_zones(lab, sp, bad, 2.0)
        with pytest.raises(ValueError, match="fissure_mm"):
            ops.lobe_zones(lab, sp, 3.0, bad)
    with pytest.raises(ValueError, match="2\\^25"):
        ops.lobe_zones(torch.zeros(1, 1, 1680, dtype=torch.uint8).expand(2, 3, 1680), (1.0, 1.0, 20.0), 3.0, 2.0)
    with pytest.raises(TypeError):
        ops.lobe_zones(lab.to(torch.int32), sp, 3.0, 2.0)
    with pytest.raises(ValueError):
        ops.lobe_zones(lab[0], sp, 3.0, 2.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lobe_zones(lab, sp, 3.0, 2.0, n_regions=5, max_mm=math.inf, want_dist=True)
    assert ops.lobe_zones_units((1.25, 0.7, 0.65), 10.0, 4.0) == ((1250, 700, 650), 10000, 4000, 10000)
    assert ops.lobe_zones_units((1.25, 0.7, 0.65), 4.0, 10.0) == ((1250, 700, 650), 4000, 10000, 10000)
    assert ops.lobe_zones_units(sp, 10.0, 4.0, math.inf)[3] == ops.EDT_FULL_UM
    assert ops.lobe_zones_units(sp, 10.0, 4.0, 70.0)[3] == 70000
    assert ops.lobe_zones_units(sp, 10.0, 4.0)[:2] == ops.lung_zones_units(sp, 10.0)[:2]


# ------------------------------------------------------------------------------------------------ the tensor math
def lobed(shape=(6, 40, 50), n=5):
    scan, labels = DR.lung_like(shape, n, seed=3)
    labels = labels.astype(np.int16)
    labels[labels == 4] = 0                                   # an absent lobe: 3 and 5 have a gap between them
    labels[2, 20, 12:16] = 9                                  # lung outside 1..5
    labels[0, 0, 11] = -3
    return scan, labels


def test_three_zone_math_equals_the_yardstick(monkeypatch):
    """processor.core_peel(fissure_mm=...) on CPU tensors, its two kernels replaced by the yardstick's label volume and
    np.bincount: the row slicing of three zones, the zero row 0 and each zone's whole_lung"""
    from bodyct_dram_emph_subtype_amd import ops, processor
    spacing, n = (2.5, 0.7, 0.8), 5
    scan, labels = lobed()
    want = FR.core_peel(scan, labels, spacing, 2.0, 1.5, n)
    calls = []

    def zones_stub(lab, sp, peel_mm, fissure_mm, n_regions=None, **kw):
        assert n_regions == n and (peel_mm, fissure_mm) == (2.0, 1.5) and not kw
        calls.append("lobe_zones")
        return torch.from_numpy(want["zones"]), torch.from_numpy(want["zone_labels"]), None, None

    def hist_stub(image, zl, rows, hu_lo, nbins):
        assert rows == 3 * n
        calls.append("lobe_histogram")
        h, s = DR.histogram(image.numpy(), zl.numpy(), rows, hu_lo, nbins)
        return torch.from_numpy(h), torch.from_numpy(s)

    def never(*a, **k):
        raise AssertionError("lung_zones is not called with fissure_mm")

    monkeypatch.setattr(ops, "lobe_zones", zones_stub)
    monkeypatch.setattr(ops, "lung_zones", never)
    monkeypatch.setattr(ops, "lobe_histogram", hist_stub)
    got = processor.core_peel(torch.from_numpy(scan), torch.from_numpy(labels), spacing, 2.0, n, fissure_mm=1.5)
    assert calls == ["lobe_zones", "lobe_histogram"]                           # ONE histogram with 3n rows
    assert set(got) == {"peel", "core", "fissure", "outside_voxels", "zones", "zone_labels", "peel_mm", "n_regions",
                        "fissure_mm", "zone_names"}
    assert got["zone_names"] == ("peel", "core", "fissure") == processor.FISSURE_ZONES and got["fissure_mm"] == 1.5
    for zone in FR.ZONE_NAMES:
        DR.assert_matches(got[zone], want[zone], zone)
        assert int(got[zone]["voxels"][0]) == 0 and int(got[zone]["voxels"][4]) == 0
        assert int(got[zone]["voxels"][1]) > 0, zone            # all three zones are populated
    print("[three zones]", {z: want[z]["voxels"].tolist() for z in FR.ZONE_NAMES})
    assert int(got["outside_voxels"]) == want["outside_voxels"] == 4
    whole = DR.densitometry(scan, labels, spacing, n)
    total = lambda k: sum(got[z][k] for z in FR.ZONE_NAMES).numpy()
    assert np.array_equal(total("voxels")[1:], whole["voxels"][1:])
    assert np.array_equal(total("laa_counts")[:, 1:], whole["laa_counts"][:, 1:])
    two = ER.core_peel(scan, labels, spacing, 2.0, n)                          # the peel is the two-zone peel, the other
    assert np.array_equal(want["zones"] == 1, two["zones"] == 1)               # two zones are its core
    assert np.array_equal((want["zones"] == 2) | (want["zones"] == 3), two["zones"] == 2)
    DR.assert_matches(got["peel"], two["peel"], "peel of the two-zone split")
    other = processor.core_peel(torch.from_numpy(scan), torch.from_numpy(labels), spacing, 2.0, n, fissure_mm=1.5,
                                thresholds=(-856,), percentiles=(10, 50), hu_lo=-1100, nbins=2048)
    want2 = FR.core_peel(scan, labels, spacing, 2.0, 1.5, n, thresholds=(-856,), percentiles=(10, 50), hu_lo=-1100, nbins=2048)
    DR.assert_matches(other["fissure"], want2["fissure"], "other bins")


# ------------------------------------------------------------------------------------------------ the report
STEMS = ("laa950_fraction", "laa910_fraction", "perc15_hu", "mean_lung_density", "volume_ml")
ZONES3 = ("peel", "core", "fissure")
SCAN_KEYS3 = {f"{s}_per_{w}_{z}" for s in STEMS for w in ("region", "lung") for z in ZONES3} | {"peel_mm", "fissure_mm"}
NET_KEYS3 = {f"{h}_lesion_percentage_per_{w}_{z}" for h in ("cle", "pse") for w in ("region", "lung") for z in ZONES3} | \
    {f"region_voxels_{z}" for z in ZONES3}


def yardstick_result():
    """lobes 1 | 2 | 3 touch along y planes; 4 is absent, which leaves 5.6 mm of background between 3 and 5: with a rind
    of 1.5 mm lobe 5 has a peel and a core, and no fissural rind"""
    scan, labels = lobed()
    return scan, labels, FR.core_peel(scan, labels, (2.5, 0.7, 0.8), 2.0, 1.5, 5)


def test_core_peel_metrics_with_three_zones():
    from bodyct_dram_emph_subtype_amd import processor
    _, _, res = yardstick_result()
    vox = {z: res[z]["voxels"].tolist() for z in ZONES3}
    print("[metrics]", vox)
    assert vox["fissure"][1] > 0 and vox["fissure"][2] > 0 and vox["fissure"][3] > 0    # 1 | 2 and 2 | 3 touch
    assert vox["fissure"][5] == 0 and vox["core"][5] > 0 and vox["peel"][5] > 0         # 5 stands alone
    m = processor.core_peel_metrics(res, {1: "RUL"})
    assert set(m) == SCAN_KEYS3 and len(m) == 32
    assert m["peel_mm"] == "2.000" and m["fissure_mm"] == "1.500"
    for zone in ZONES3:                                        # densitometry_metrics' own formats, renamed
        plain = processor.densitometry_metrics(res[zone], {1: "RUL"})
        assert {k[:-len(zone) - 1]: v for k, v in m.items() if k.endswith("_" + zone)} == plain, zone
    assert m["mean_lung_density_per_region_fissure"]["5"] is None and m["mean_lung_density_per_region_fissure"]["4"] is None
    assert m["laa950_fraction_per_region_fissure"]["5"] is None and m["perc15_hu_per_region_fissure"]["5"] is None
    assert m["volume_ml_per_region_fissure"]["5"] == "0.0"
    assert m["volume_ml_per_region_fissure"]["RUL"] == "{:.1f}".format(vox["fissure"][1] * 2.5 * 0.7 * 0.8 / 1000.0)
    assert json.loads(json.dumps(m))["mean_lung_density_per_region_fissure"]["5"] is None
    # a result without 'zone_names' is today's: the two zones, no fissure key
    two = {k: v for k, v in res.items() if k not in ("zone_names", "fissure_mm", "fissure")}
    m2 = processor.core_peel_metrics(two, {1: "RUL"})
    assert set(m2) == {k for k in SCAN_KEYS3 if not k.endswith("_fissure")} - {"fissure_mm"} and len(m2) == 21
    assert all(m2[k] == m[k] for k in m2)
    # an empty third zone altogether: every per-lung value of it is None but the volume
    empty = dict(res, fissure=DR.densitometry(np.zeros((1, 1, 2), np.int16), np.zeros((1, 1, 2), np.int16), (2.5, 0.7, 0.8), 5))
    me = processor.core_peel_metrics(empty)
    assert me["mean_lung_density_per_lung_fissure"] is None and me["laa910_fraction_per_lung_fissure"] is None
    assert me["volume_ml_per_lung_fissure"] == "0.0"


TABLE = [[5.0, 6.0, 7.0, 100.0],            # row 0
         [10.0, 1.0, 3.0, 40.0], [0.0, 0.0, 0.0, 0.0],          # peel of lobes 1, 2
         [2.5, 0.5, 1.0, 10.0], [0.0, 0.0, 0.0, 0.0]]           # core of lobes 1, 2
TABLE3 = TABLE + [[1.0, 2.0, 4.0, 8.0], [0.0, 0.0, 0.0, 0.0]]   # fissural rind of lobes 1, 2


def test_zone_region_metrics_and_the_fold_with_three_zones():
    from bodyct_dram_emph_subtype_amd import processor
    m = processor.zone_region_metrics(torch.tensor(TABLE3, dtype=torch.float64), {1: "RUL"}, zones=ZONES3)
    assert set(m) == NET_KEYS3 and len(m) == 15
    assert m["cle_lesion_percentage_per_region_fissure"] == {"RUL": "0.125", "2": None}
    assert m["pse_lesion_percentage_per_region_fissure"] == {"RUL": "0.250", "2": None}
    assert m["region_voxels_fissure"] == {"RUL": "8", "2": "0"}
    assert m["cle_lesion_percentage_per_lung_fissure"] == "0.125" and m["pse_lesion_percentage_per_lung_fissure"] == "0.250"
    two = processor.zone_region_metrics(torch.tensor(TABLE, dtype=torch.float64), {1: "RUL"})
    assert all(m[k] == two[k] for k in two) and set(two) == {k for k in NET_KEYS3 if not k.endswith("_fissure")}
    assert processor.zone_region_metrics(TABLE3, zones=processor.FISSURE_ZONES) == \
        processor.zone_region_metrics(TABLE3, None, ZONES3)
    empty = [r if i < 5 else [0.0] * 4 for i, r in enumerate(TABLE3)]          # an empty third zone
    e = processor.zone_region_metrics(empty, zones=ZONES3)
    assert e["cle_lesion_percentage_per_lung_fissure"] is None and e["pse_lesion_percentage_per_lung_fissure"] is None
    assert e["region_voxels_fissure"] == {"1": "0", "2": "0"} and e["cle_lesion_percentage_per_region_fissure"] == {"1": None, "2": None}
    assert not any("severity" in k for k in m)
    folded = processor.fold_zone_table(TABLE3, n_zones=3)
    assert folded.dtype == torch.float64 and folded.tolist() == [TABLE3[0], [13.5, 3.5, 8.0, 58.0], [0.0] * 4]
    assert processor.region_metrics(folded)["region_voxels"] == {"1": "58", "2": "0"}
    # a row count alone is ambiguous: 7 rows are 3 lobes in two zones as well
    assert processor.fold_zone_table(TABLE3).shape == (4, 4) and processor.fold_zone_table(TABLE3, 3).shape == (3, 4)
    assert set(processor.zone_region_metrics(TABLE3)["region_voxels_core"]) == {"1", "2", "3"}
    for bad in (TABLE3[:6], TABLE3[:1], TABLE, [r[:3] for r in TABLE3]):
        with pytest.raises(ValueError):
            processor.zone_region_metrics(bad, zones=ZONES3)
    with pytest.raises(ValueError):
        processor.fold_zone_table(TABLE, n_zones=3)
    with pytest.raises(ValueError):
        processor.fold_zone_table(TABLE3, n_zones=4)
    with pytest.raises(ValueError):
        processor.zone_region_metrics(TABLE3, zones=("peel",))


def test_defaults_return_what_they_returned():
    """the literals tests/test_core_peel_host.py pins for the two-zone forms, through the new signatures' defaults"""
    from bodyct_dram_emph_subtype_amd import processor
    assert processor.ZONES == ("peel", "core")
    m = processor.zone_region_metrics(torch.tensor(TABLE, dtype=torch.float64), {1: "RUL"})
    assert m == {"cle_lesion_percentage_per_region_peel": {"RUL": "0.250", "2": None},
                 "pse_lesion_percentage_per_region_peel": {"RUL": "0.025", "2": None},
                 "region_voxels_peel": {"RUL": "40", "2": "0"},
                 "cle_lesion_percentage_per_lung_peel": "0.250", "pse_lesion_percentage_per_lung_peel": "0.025",
                 "cle_lesion_percentage_per_region_core": {"RUL": "0.250", "2": None},
                 "pse_lesion_percentage_per_region_core": {"RUL": "0.050", "2": None},
                 "region_voxels_core": {"RUL": "10", "2": "0"},
                 "cle_lesion_percentage_per_lung_core": "0.250", "pse_lesion_percentage_per_lung_core": "0.050"}
    assert list(m) == list(processor.zone_region_metrics(TABLE, {1: "RUL"}, processor.ZONES))     # the order of the report
    assert processor.fold_zone_table(TABLE).tolist() == [TABLE[0], [12.5, 1.5, 4.0, 50.0], [0.0] * 4]
    assert processor.fold_zone_table(TABLE).tolist() == processor.fold_zone_table(TABLE, 2).tolist()
    scan, labels = lobed()
    two = ER.core_peel(scan, labels, (2.5, 0.7, 0.8), 2.0, 5)
    m = processor.core_peel_metrics(dict(two, peel_mm=2.0))
    assert set(m) == {k for k in SCAN_KEYS3 if not k.endswith("_fissure")} - {"fissure_mm"}
    for zone in ("peel", "core"):
        assert {k[:-len(zone) - 1]: v for k, v in m.items() if k.endswith("_" + zone)} == processor.densitometry_metrics(two[zone])


# ------------------------------------------------------------------------------------------------ predict_case, the sections
class _Module:
    def __init__(self, n):
        self.args = type("Args", (), {"n_regions": n})()

    def predict_step(self, batch, i):
        raise AssertionError("predict_step is never reached")


def test_predict_case_refuses_before_any_device_work(monkeypatch):
    from bodyct_dram_emph_subtype_amd import ops, processor, transforms
    touched = []
    monkeypatch.setattr(transforms, "prepare_case", lambda *a, **k: touched.append("prepare_case"))
    monkeypatch.setattr(ops, "_L", lambda: touched.append("_L"))
    scan, lobes = torch.zeros(4, 5, 6, dtype=torch.int16), torch.ones(4, 5, 6, dtype=torch.uint8)
    args = (scan, lobes, (1.0, 1.0, 1.0), (4, 4, 4))
    with pytest.raises(ValueError, match="core_peel"):
        processor.predict_case(_Module(5), *args, fissure_mm=3.0)
    with pytest.raises(ValueError, match="core_peel"):
        processor.predict_case(_Module(5), *args, regions=True, densitometry=True, fissure_mm=3.0)
    for n in (6, 7, 0):
        with pytest.raises(ValueError, match="n_regions"):
            processor.predict_case(_Module(n), *args, core_peel=True, peel_mm=3.0, fissure_mm=3.0)
    assert touched == []


def test_section_table_and_the_key_pattern():
    from bodyct_dram_emph_subtype_amd import processor
    assert list(processor._SECTIONS) == ["regions", "densitometry", "core_peel", "clusters"]
    assert processor._SECTIONS["core_peel"].required == ("mean_lung_density_per_region_peel", "region_voxels_peel", "peel_mm")
    key = processor._CORE_PEEL_KEY
    _, _, res = yardstick_result()
    new = set(processor.core_peel_metrics(res)) | set(processor.zone_region_metrics(TABLE3, zones=ZONES3))
    assert new == SCAN_KEYS3 | NET_KEYS3 and all(key.fullmatch(k) for k in new)
    scan, labels = lobed()
    others = set(processor.REGION_KEYS) | set(processor.densitometry_metrics(DR.densitometry(scan, labels, (2.5, 0.7, 0.8), 5)))
    others |= {"laa950_clusters_per_region", "laa950_largest_cluster_ml_per_lung", "laa950_cluster_d_per_region",
               "laa_cluster_connectivity", "scan_filter", "cle_severity_score", "cle_lesion_percentage_per_lung",
               "pse_lesion_percentage_per_lung", "pse_severity_score"}
    assert len(others) > 20 and not any(key.fullmatch(k) for k in others)
    for name, section in processor._SECTIONS.items():
        if name != "core_peel" and not isinstance(section.select, tuple):
            assert not any(section.select.fullmatch(k) for k in new), name
    for k in ("fissure", "fissure_mm_per_region", "volume_ml_per_lung_rind", "region_voxels", "xfissure_mm"):
        assert not key.fullmatch(k), k


def _prediction():
    return {"cle_dense_outs": torch.zeros(1, 1, 2, 2, 2), "pse_dense_outs": torch.zeros(1, 1, 2, 2, 2),
            "cle_precentages": torch.tensor([0.02]), "pse_precentages": torch.tensor([0.3]),
            "crop_slices": torch.tensor([[[0, 2], [0, 2], [0, 2]]]), "original_size": torch.tensor([[2, 2, 2]]), "uids": ["u"]}


def test_write_reports_carries_the_new_keys(monkeypatch, tmp_path):
    from bodyct_dram_emph_subtype_amd import processor
    monkeypatch.setattr(processor, "resample_paste", lambda d, *a, **k: (None, torch.zeros(2, 2, 2, dtype=torch.uint8)))
    _, _, res = yardstick_result()
    entry = processor.build_outputs([_prediction()])[0]
    added = dict(processor.core_peel_metrics(res), **processor.zone_region_metrics(TABLE3, zones=ZONES3))
    entry["metrics"].update(added)
    path = str(tmp_path / "core_peel.json")
    processor.write_reports([entry], core_peel_json=path)
    assert json.load(open(path)) == json.loads(json.dumps(added)) and len(added) == 47 and set(added) == SCAN_KEYS3 | NET_KEYS3
    with pytest.raises(ValueError, match="densitometry_json"):         # the zone keys are not the plain densitometry's
        processor.write_reports([entry], densitometry_json=str(tmp_path / "d.json"))
