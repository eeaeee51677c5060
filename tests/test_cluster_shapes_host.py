"""CPU: the yardstick of the per-component table (tests/shapes_ref.py) held to scipy.ndimage, to a per-voxel loop over
the definition of the faces and to closed forms; processor.shapes_from_rows against its yardstick; the report keys of
the cluster shapes; predict_case with the kernel wrappers replaced by the yardsticks."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import ccl_ref as CC
import shapes_ref as SR
from conftest import GOLDEN

SPACING = (1.5, 0.8, 0.8)


def _golden_tools():
    spec = importlib.util.spec_from_file_location("make_golden_report", os.path.join(GOLDEN, "make_golden_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _random_comp(shape=(4, 7, 9), p=0.5, seed=0, connectivity=6):
    rng = np.random.default_rng(seed)
    key = np.where(rng.random(shape) < p, rng.integers(1, 4, shape), 0).astype(np.uint8)
    return key, CC.label(key, connectivity, 5)[0]


# ------------------------------------------------------------------------------------------------ the yardstick itself
def test_header_binding_and_column_names():
    from bodyct_dram_emph_subtype_amd import _lib, ops
    import ctypes
    I, LL, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    assert _lib.SIGNATURES["dram_component_shapes_workspace"] == (LL, [I, I, I])
    assert _lib.SIGNATURES["dram_component_rank"] == (I, [P, P, P, I, I, I, P])
    assert _lib.SIGNATURES["dram_component_shapes"] == (I, [P, P, I, LL, LL, P, P, P, LL, P, I, I, I, P])
    assert ops.SHAPE_COLS == SR.COLS == 18
    names = ("ROOT", "CLASS", "VOXELS", "Z0", "Z1", "Y0", "Y1", "X0", "X1", "SUM_Z", "SUM_Y", "SUM_X", "FACES_Z", "FACES_Y",
             "FACES_X", "ZONE1", "ZONE2", "ZONE3")
    assert [getattr(ops, "SHAPE_" + n) for n in names] == [getattr(SR, n) for n in names] == list(range(18))


@pytest.mark.parametrize("connectivity,p", [(6, 0.4), (26, 0.1)])
def test_yardstick_voxels_boxes_and_sums_against_scipy(connectivity, p):
    import scipy.ndimage as ndi
    mask = np.random.default_rng(2).random((6, 11, 13)) < p
    comp = CC.label(mask.astype(np.uint8), connectivity, 1)[0]
    rows = SR.rows(comp)
    structure = np.ones((3, 3, 3)) if connectivity == 26 else None
    lab, n = ndi.label(mask, structure=structure)
    assert n == rows.shape[0] > 5
    # scipy numbers the objects in raster order of their first voxel: the ascending root order of the rows
    assert np.array_equal(lab.ravel()[rows[:, SR.ROOT]], np.arange(1, n + 1))
    idx = np.arange(1, n + 1)
    assert np.array_equal(rows[:, SR.VOXELS], ndi.sum(mask, lab, idx).astype(np.int64))
    for r, sl in zip(rows, ndi.find_objects(lab)):
        assert [r[SR.Z0], r[SR.Z1], r[SR.Y0], r[SR.Y1], r[SR.X0], r[SR.X1]] == [v for s in sl for v in (s.start, s.stop)]
    z, y, x = np.indices(mask.shape)
    for col, g in ((SR.SUM_Z, z), (SR.SUM_Y, y), (SR.SUM_X, x)):
        assert np.array_equal(rows[:, col], ndi.sum(g, lab, idx).astype(np.int64))
    com = np.array(ndi.center_of_mass(mask, lab, idx))
    assert np.allclose(rows[:, SR.SUM_Z:SR.SUM_X + 1] / rows[:, [SR.VOXELS]], com, rtol=1e-12, atol=0)


def _faces_by_the_definition(comp):
    """{root: [fz, fy, fx]} by a loop over every counted voxel and its six neighbours"""
    ok = SR.counted(comp)
    out = {}
    D, H, W = comp.shape
    for z, y, x in zip(*np.nonzero(ok)):
        f = out.setdefault(int(comp[z, y, x]), [0, 0, 0])
        for a, (dz, dy, dx) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            for sgn in (-1, 1):
                u = (z + sgn * dz, y + sgn * dy, x + sgn * dx)
                outside = not (0 <= u[0] < D and 0 <= u[1] < H and 0 <= u[2] < W)
                f[a] += int(outside or comp[u] != comp[z, y, x])
    return out


@pytest.mark.parametrize("seed,connectivity", [(0, 6), (1, 26), (2, 6)])
def test_yardstick_faces_against_the_definition(seed, connectivity):
    key, comp = _random_comp(seed=seed, connectivity=connectivity)
    if seed == 2:                                               # hostile contents: the rule decides, not the labelling
        comp = comp.copy()
        comp.ravel()[[3, 50, 100, 200]] = [comp.size, -9, 2 ** 31 - 1, 1]
    rows = SR.rows(comp, key)
    want = _faces_by_the_definition(comp)
    assert sorted(want) == rows[:, SR.ROOT].tolist()
    assert [want[int(r[SR.ROOT])] for r in rows] == rows[:, SR.FACES_Z:SR.FACES_X + 1].tolist()
    assert np.array_equal(rows[:, SR.CLASS], key.ravel()[rows[:, SR.ROOT]])


def test_closed_forms_of_the_faces():
    a, b, c = 2, 3, 5
    comp = np.full((6, 7, 9), -1, dtype=np.int64)
    root = (1 * 7 + 2) * 9 + 3
    comp[1:1 + a, 2:2 + b, 3:3 + c] = root
    (r,) = SR.rows(comp)
    assert r[SR.FACES_Z:SR.FACES_X + 1].tolist() == [2 * b * c, 2 * a * c, 2 * a * b] and r[SR.VOXELS] == a * b * c
    assert r[[SR.Z0, SR.Z1, SR.Y0, SR.Y1, SR.X0, SR.X1]].tolist() == [1, 1 + a, 2, 2 + b, 3, 3 + c]
    one = np.full((3, 3, 3), -1, dtype=np.int64)
    one[1, 1, 1] = 13
    assert SR.rows(one)[0, SR.FACES_Z:SR.FACES_X + 1].tolist() == [2, 2, 2]
    # two boxes that touch along x: both count the shared face, so each keeps the faces of a free box
    two = np.full((2, 2, 6), -1, dtype=np.int64)
    two[:, :, 0:3] = 0
    two[:, :, 3:6] = 3
    r0, r1 = SR.rows(two)
    assert r0[SR.FACES_Z:SR.FACES_X + 1].tolist() == r1[SR.FACES_Z:SR.FACES_X + 1].tolist() == [12, 12, 8]
    # at the edge of the volume a face is exposed as well
    full = np.zeros((2, 3, 4), dtype=np.int64)
    assert SR.rows(full)[0, SR.FACES_Z:SR.FACES_X + 1].tolist() == [24, 16, 12]


def test_zone_columns_count_only_zones_1_to_3():
    key, comp = _random_comp(seed=5)
    zones = np.random.default_rng(5).integers(0, 5, comp.shape).astype(np.uint8)
    rows = SR.rows(comp, key, zones)
    for k in (1, 2, 3):
        assert int(rows[:, SR.ZONE1 + k - 1].sum()) == int(((zones == k) & (comp >= 0)).sum())
    assert int(rows[:, SR.ZONE1:].sum()) < int(rows[:, SR.VOXELS].sum())
    assert not SR.rows(comp, key)[:, SR.ZONE1:].any()


# ------------------------------------------------------------------------------------------------ shapes_from_rows
def _row(root, cls, voxels, box=(0, 1, 0, 1, 0, 1), sums=(0, 0, 0), faces=(2, 2, 2), zones=(0, 0, 0)):
    return [root, cls, voxels, *box, *sums, *faces, *zones]


def test_shapes_from_rows_against_the_yardstick():
    from bodyct_dram_emph_subtype_amd import processor
    key, comp = _random_comp((5, 12, 20), 0.55, 8)
    key[:, 3, :] = np.where(key[:, 3, :] > 0, 9, 0)             # a class outside 1..n: row 0
    comp = CC.label(key, 6, 5)[0]
    zones = np.random.default_rng(1).integers(0, 4, comp.shape).astype(np.uint8)
    rows = SR.rows(comp, key, zones)
    for nz in (0, 2, 3):
        got = processor.shapes_from_rows(torch.from_numpy(rows), SPACING, 5, bulla_mm=2.5, top=4, origin=(10, 20, 30), n_zones=nz)
        SR.assert_shapes(got, SR.from_rows(rows, SPACING, 5, 2.5, 4, (10, 20, 30), nz), nz)
        assert ("zone_clusters" in got) == bool(nz)
    assert int(got["region"].eq(0).sum()) > 0 and 0 < int(got["bullae"].sum()) < rows.shape[0]
    empty = processor.shapes_from_rows(torch.zeros((0, 18), dtype=torch.int64), SPACING, 5, n_zones=2)
    SR.assert_shapes(empty, SR.from_rows(np.zeros((0, 18)), SPACING, 5, n_zones=2), "empty")
    assert bool(torch.isnan(empty["bulla_laa_share"]).all()) and empty["largest"].numel() == 0
    for bad in (torch.from_numpy(rows[:, :17]), torch.from_numpy(rows).double(), torch.from_numpy(rows)[0]):
        with pytest.raises(ValueError):
            processor.shapes_from_rows(bad, SPACING, 5)
    with pytest.raises(ValueError):
        processor.shapes_from_rows(torch.from_numpy(rows), SPACING, 5, n_zones=1)
    with pytest.raises(ValueError):
        processor.shapes_from_rows(torch.from_numpy(rows), SPACING, 5, bulla_mm=0.0)


def test_bulla_boundary_is_an_exact_integer_comparison():
    from bodyct_dram_emph_subtype_amd import processor
    need = processor.bulla_min_voxels(SPACING, 10.0)
    assert need == math.ceil(math.pi / 6.0 * 1000.0 / 0.96) == SR.bulla_min_voxels(SPACING, 10.0) == 546
    assert processor.bulla_min_voxels((10.0, 10.0, 10.0), 1.0) == 1                # never below one voxel
    rows = torch.tensor([_row(0, 1, need), _row(5, 1, need - 1), _row(9, 2, need - 1)], dtype=torch.int64)
    got = processor.shapes_from_rows(rows, SPACING, 2)
    assert got["bulla_min_voxels"] == need and got["is_bulla"].tolist() == [True, False, False]
    assert got["bullae"].tolist() == [0, 1, 0] and got["bulla_voxels"].tolist() == [0, need, 0]
    assert got["bulla_laa_share"].tolist()[1] == need / (2 * need - 1) and got["bulla_laa_share"].tolist()[2] == 0.0
    assert math.isnan(got["bulla_laa_share"].tolist()[0])
    # the equivalent-sphere diameter says the same
    assert float(got["diameter_mm"][0]) >= 10.0 > float(got["diameter_mm"][1])


def test_home_zone_ties_and_top_ordering():
    from bodyct_dram_emph_subtype_amd import processor
    rows = torch.tensor([_row(0, 1, 7, zones=(3, 3, 1)), _row(2, 1, 9, zones=(0, 4, 4)), _row(4, 2, 9, zones=(0, 0, 0)),
                         _row(6, 2, 9, zones=(1, 2, 3)), _row(8, 7, 2, zones=(2, 2, 2)), _row(11, 1, 30, zones=(0, 0, 5))],
                        dtype=torch.int64)
    got = processor.shapes_from_rows(rows, (1.0, 1.0, 1.0), 2, bulla_mm=2.0, top=4, n_zones=3)
    assert got["home_zone"].tolist() == [1, 2, 0, 3, 1, 3]
    assert got["largest"].tolist() == [5, 1, 2, 3]                                 # equal sizes: root ascending
    assert got["region"].tolist() == [1, 1, 2, 2, 0, 1]
    assert got["zone_clusters"].tolist() == [[1, 0, 0], [1, 1, 1], [0, 0, 1]]
    two = processor.shapes_from_rows(rows, (1.0, 1.0, 1.0), 2, bulla_mm=2.0, n_zones=2)    # a home zone of 3 counts nowhere
    assert two["zone_clusters"].tolist() == [[1, 0], [1, 1], [0, 0]]
    SR.assert_shapes(got, SR.from_rows(rows.numpy(), (1.0, 1.0, 1.0), 2, 2.0, 4, (0, 0, 0), 3), "ties")


def test_sphericity_of_a_cube_and_units():
    from bodyct_dram_emph_subtype_amd import processor
    n = 6
    comp = np.full((8, 8, 8), -1, dtype=np.int64)
    comp[1:1 + n, 1:1 + n, 1:1 + n] = (1 * 8 + 1) * 8 + 1
    got = processor.shapes_from_rows(torch.from_numpy(SR.rows(comp)), (0.5, 0.5, 0.5), 1, origin=(100, 0, 50))
    assert abs(float(got["sphericity"][0]) - (math.pi / 6.0) ** (1.0 / 3.0)) < 1e-12
    assert "{:.3f}".format(float(got["sphericity"][0])) == "0.806"
    assert got["extent_mm"].tolist() == [[3.0, 3.0, 3.0]] and got["centroid"].tolist() == [[103.5, 3.5, 53.5]]
    assert abs(float(got["surface_mm2"][0]) - 6 * 9.0) < 1e-12 and abs(float(got["volume_ml"][0]) - 0.027) < 1e-15
    assert abs(float(got["diameter_mm"][0]) - (6.0 * 27.0 / math.pi) ** (1.0 / 3.0)) < 1e-12
    # anisotropic faces: each axis' faces carry the area of the other two spacings
    aniso = processor.shapes_from_rows(torch.tensor([_row(0, 1, 1)], dtype=torch.int64), (2.0, 3.0, 5.0), 1)
    assert float(aniso["surface_mm2"][0]) == 2 * 15.0 + 2 * 10.0 + 2 * 6.0


# ------------------------------------------------------------------------------------------------ the report
def _wrappers(monkeypatch, ops):
    def laa_components(image, labels, threshold, n_regions, connectivity, by_lobe=True, want_sizes=False):
        key = CC.laa_key(image.numpy(), labels.numpy(), threshold, n_regions, by_lobe)
        comp, t, _ = CC.label(key, connectivity, n_regions)
        return torch.from_numpy(comp.astype(np.int32)), torch.from_numpy(t), None

    def component_shapes(components, labels=None, zones=None, max_components=None):
        r = SR.rows(components.numpy(), None if labels is None else labels.numpy(), None if zones is None else zones.numpy())
        return torch.from_numpy(r), torch.tensor([r.shape[0]] * 2, dtype=torch.int64)

    monkeypatch.setattr(ops, "laa_components", laa_components)
    monkeypatch.setattr(ops, "component_shapes", component_shapes)


def _result(monkeypatch, zoned, bulla_mm=3.0, top=3):
    from bodyct_dram_emph_subtype_amd import ops, processor
    _wrappers(monkeypatch, ops)
    rng = np.random.default_rng(21)
    shape = (6, 20, 24)
    lab = CC.slab_lobes(shape, 5)
    lab[lab == 4] = 0                                           # lobe 4 is empty: NaN share -> None
    lab[2, 1, :12] = 9
    hu = np.where(rng.random(shape) < 0.4, -960, -900).astype(np.int16)
    kw = {}
    if zoned:
        kw = dict(zones=torch.from_numpy(rng.integers(0, 4, shape).astype(np.uint8)), zone_names=processor.FISSURE_ZONES)
    return processor.laa_clusters(torch.from_numpy(hu), torch.from_numpy(lab), SPACING, shapes=True, bulla_mm=bulla_mm,
                                  top=top, origin=(5, 6, 7), **kw)


def test_laa_clusters_without_shapes_is_what_it_was(monkeypatch):
    from bodyct_dram_emph_subtype_amd import processor
    with_shapes = _result(monkeypatch, False)
    hu_lab = np.random.default_rng(21)
    shape = (6, 20, 24)
    lab = CC.slab_lobes(shape, 5)
    lab[lab == 4] = 0
    lab[2, 1, :12] = 9
    hu = np.where(hu_lab.random(shape) < 0.4, -960, -900).astype(np.int16)
    plain = processor.laa_clusters(torch.from_numpy(hu), torch.from_numpy(lab), SPACING)
    assert list(plain) == [k for k in with_shapes if k != "shapes"] and "shapes" not in plain
    m = processor.laa_cluster_metrics(plain)
    assert set(m) == CC.CLUSTER_KEYS and len(m) == 7
    m_shapes = processor.laa_cluster_metrics(with_shapes)
    assert {k: m_shapes[k] for k in m} == m and list(m_shapes)[:7] == list(m)
    with pytest.raises(ValueError, match="zone_names"):
        processor.laa_clusters(torch.from_numpy(hu), torch.from_numpy(lab), SPACING, shapes=True,
                               zones=torch.zeros(shape, dtype=torch.uint8))


@pytest.mark.parametrize("zoned", [False, True])
def test_metrics_of_a_result_with_shapes(monkeypatch, zoned):
    from bodyct_dram_emph_subtype_amd import processor
    res = _result(monkeypatch, zoned)
    sh = res["shapes"]
    SR.assert_shapes(sh, SR.from_rows(sh["rows"].numpy(), SPACING, 5, 3.0, 3, (5, 6, 7), 3 if zoned else 0), "by lobe")
    SR.assert_shapes(sh["whole_lung"], SR.from_rows(sh["whole_lung_rows"].numpy(), SPACING, 1, 3.0, 3, (5, 6, 7),
                                                    3 if zoned else 0), "whole lung")
    names = {1: "RUL", 3: "RLL"}
    m = processor.laa_cluster_metrics(res, names)
    new = {"laa950_bullae_per_region", "laa950_bulla_ml_per_region", "laa950_bulla_laa_share_per_region",
           "laa950_bullae_per_lung", "laa950_bulla_ml_per_lung", "laa950_bulla_laa_share_per_lung",
           "laa950_largest_clusters", "bulla_mm", "bulla_min_voxels"}
    if zoned:
        new |= {f"laa950_{s}_per_{w}_{z}" for s in ("clusters", "bullae") for w in ("region", "lung")
                for z in ("peel", "core", "fissure")}
    assert set(m) == CC.CLUSTER_KEYS | new
    for k in m:
        assert processor._CLUSTER_KEY.fullmatch(k), k
        assert not processor._DENSITO_KEY.fullmatch(k) and not processor._CORE_PEEL_KEY.fullmatch(k), k
        assert k not in processor.REGION_KEYS
    for k in ("laa950_fraction_per_region", "laa950_fraction_per_region_peel", "peel_mm", "fissure_mm", "region_voxels_peel",
              "laa950_cluster_d_per_region_peel", "laa950_largest_clusters_per_region", "bulla_mm_per_lung"):
        assert not processor._CLUSTER_KEY.fullmatch(k), k
    # formats
    assert list(m["laa950_bullae_per_region"]) == ["RUL", "2", "RLL", "4", "5"]
    assert m["laa950_bullae_per_region"]["RUL"] == "{:d}".format(int(sh["bullae"][1]))
    assert m["laa950_bulla_ml_per_region"]["2"] == "{:.3f}".format(float(sh["bulla_ml"][2]))
    assert m["laa950_bulla_laa_share_per_region"]["4"] is None and m["laa950_bullae_per_region"]["4"] == "0"
    assert m["laa950_bulla_ml_per_region"]["4"] == "0.000"
    assert m["laa950_bullae_per_lung"] == "{:d}".format(int(sh["whole_lung"]["bullae"][0]))
    assert m["laa950_bulla_laa_share_per_lung"] == "{:.3f}".format(float(sh["whole_lung"]["bulla_laa_share"][0]))
    assert m["bulla_mm"] == "3.000" and m["bulla_min_voxels"] == str(SR.bulla_min_voxels(SPACING, 3.0))
    largest = m["laa950_largest_clusters"]
    assert len(largest) == 3
    for entry, i in zip(largest, sh["largest"].tolist()):
        reg = int(sh["region"][i])
        assert entry["region"] == ({1: "RUL", 3: "RLL"}.get(reg, str(reg)) if reg else None)
        assert entry["volume_ml"] == "{:.3f}".format(float(sh["volume_ml"][i]))
        assert entry["diameter_mm"] == "{:.3f}".format(float(sh["diameter_mm"][i]))
        assert entry["extent_mm"] == ["{:.3f}".format(v) for v in sh["extent_mm"][i].tolist()]
        assert entry["centroid"] == ["{:.1f}".format(v) for v in sh["centroid"][i].tolist()]
        assert entry["surface_mm2"] == "{:.3f}".format(float(sh["surface_mm2"][i]))
        assert entry["sphericity"] == "{:.3f}".format(float(sh["sphericity"][i]))
        home = int(sh["home_zone"][i])
        assert entry["zone"] == (processor.FISSURE_ZONES[home - 1] if zoned and home else None)
        assert float(entry["centroid"][0]) >= 5.0                                  # the origin is added
    if zoned:
        assert m["laa950_clusters_per_region_core"]["RUL"] == "{:d}".format(int(sh["zone_clusters"][1, 1]))
        assert m["laa950_bullae_per_lung_fissure"] == "{:d}".format(int(sh["whole_lung"]["zone_bullae"][0, 2]))
    assert json.loads(json.dumps(m)) == m                                          # plain json types
    as_numpy = lambda d: {k: (v.numpy() if torch.is_tensor(v) else as_numpy(v) if isinstance(v, dict) else v)
                          for k, v in d.items()}
    assert processor.laa_cluster_metrics(as_numpy(res), names) == m               # the yardstick's arrays format alike


def test_sections_and_write_reports_carry_the_new_keys(monkeypatch, tmp_path):
    from bodyct_dram_emph_subtype_amd import processor
    assert list(processor._SECTIONS) == ["regions", "densitometry", "core_peel", "clusters"]
    assert processor._LAUNCH_ORDER == ("clusters", "densitometry", "core_peel")
    added = processor.laa_cluster_metrics(_result(monkeypatch, True))
    monkeypatch.setattr(processor, "resample_paste", lambda d, *a, **k: (None, torch.zeros(2, 2, 2, dtype=torch.uint8)))
    pred = {"cle_dense_outs": torch.zeros(1, 1, 2, 2, 2), "pse_dense_outs": torch.zeros(1, 1, 2, 2, 2),
            "cle_precentages": torch.tensor([0.02]), "pse_precentages": torch.tensor([0.3]),
            "crop_slices": torch.tensor([[[0, 2], [0, 2], [0, 2]]]), "original_size": torch.tensor([[2, 2, 2]]), "uids": ["u"]}
    entry = processor.build_outputs([pred])[0]
    entry["metrics"].update(added)
    entry["metrics"]["laa950_fraction_per_region_peel"] = {"1": "0.100"}          # another section's key stays out
    path = str(tmp_path / "clusters.json")
    processor.write_reports([entry], clusters_json=path)
    assert json.load(open(path)) == added and len(added) == 7 + 9 + 12
    with pytest.raises(ValueError, match="core_peel_json"):
        processor.write_reports([entry], core_peel_json=str(tmp_path / "c.json"))


# ------------------------------------------------------------------------------------------------ predict_case
def test_predict_case_shapes_off_equals_today_and_on_keeps_every_old_key(monkeypatch):
    from bodyct_dram_emph_subtype_amd import ops, processor, transforms
    G = _golden_tools()
    for owner, name, new in G.stubs(processor, ops, transforms):
        monkeypatch.setattr(owner, name, new)
    _wrappers(monkeypatch, ops)
    golden = json.load(open(os.path.join(GOLDEN, "predict_report.json")))
    scan = torch.zeros(G.ORIGINAL, dtype=torch.int16)
    order = []
    real_cp, real_cl = processor._SECTIONS["core_peel"].run, processor._SECTIONS["clusters"].run
    spy = lambda tag, fn: (lambda *a, **k: order.append(tag) or fn(*a, **k))
    monkeypatch.setitem(processor._SECTIONS, "core_peel", processor._SECTIONS["core_peel"]._replace(run=spy("core_peel", real_cp)))
    monkeypatch.setitem(processor._SECTIONS, "clusters", processor._SECTIONS["clusters"]._replace(run=spy("clusters", real_cl)))

    def run(core_peel, cluster_kw):
        del order[:]
        e = processor.predict_case(G.Module(), scan, scan.to(torch.uint8), G.SPACING, G.SHAPE, uid="case", region_names=None,
                                   peel_mm=G.PEEL_MM, regions=True, densitometry=True, core_peel=core_peel, clusters=True,
                                   cluster_kw=cluster_kw)
        return e, list(order)

    for core_peel in (False, True):
        want = golden["11{}1/plain".format(int(core_peel))]["entry"]
        for kw in (None, {"shapes": False}):
            off, launched = run(core_peel, kw)
            assert json.dumps({"metrics": off["metrics"], "error_messages": off["error_messages"]}) == want
            assert launched == (["clusters", "core_peel"] if core_peel else ["clusters"])      # today's launch order
        on, launched = run(core_peel, {"shapes": True, "bulla_mm": 1.5, "top": 2})
        assert launched == (["core_peel", "clusters"] if core_peel else ["clusters"])          # the zones come first
        old = json.loads(want)
        assert {k: on["metrics"][k] for k in old["metrics"]} == old["metrics"]
        assert [k for k in on["metrics"] if k in old["metrics"]] == list(old["metrics"])        # and keep their order
        assert on["error_messages"] == old["error_messages"]
        new = set(on["metrics"]) - set(old["metrics"])
        assert new and all(processor._CLUSTER_KEY.fullmatch(k) for k in new)
        assert ("laa950_clusters_per_region_peel" in new) == core_peel and "laa950_bullae_per_region_fissure" not in new
        largest = on["metrics"]["laa950_largest_clusters"]
        # the largest cluster of the fixture: 5 voxels of lobe 1 around (9, 1, 4); the crop starts at (1, 2, 3)
        assert len(largest) == 2 and largest[0]["region"] == "1"
        assert largest[0]["volume_ml"] == "{:.3f}".format(5 * 1.5 * 0.8 * 0.8 / 1000.0)
        assert largest[0]["centroid"] == ["{:.1f}".format(v) for v in (46 / 5 + 1, 4 / 5 + 2, 20 / 5 + 3)]
        assert (largest[0]["zone"] in ("peel", "core")) if core_peel else (largest[0]["zone"] is None)
        assert on["metrics"]["bulla_min_voxels"] == str(SR.bulla_min_voxels(G.SPACING, 1.5))
