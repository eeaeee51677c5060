"""Host side of the LAA cluster analysis (no GPU): the min-propagation yardstick of tests/ccl_ref.py against
scipy.ndimage.label (where scipy is present) and against hand-counted cases; the header's entry points and the
launcher's argument checks through ctypes with dummy pointers (no launch); processor.clusters_from_table on CPU tensors
against the yardstick's np.polyfit D; laa_cluster_metrics formats and names; write_reports(clusters_json)."""
import ctypes
import json
import math
import subprocess

import numpy as np
import pytest
import torch

import ccl_ref as CC

BERNOULLI = [((40, 48, 65), 0.25, 1), ((40, 48, 65), 0.31, 2), ((33, 40, 130), 0.30, 3)]


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("connectivity", [6, 26])
def test_yardstick_equals_scipy(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    shape, p, seed = BERNOULLI[2]
    for key in (CC.bernoulli_key(shape, p, seed), CC.bernoulli_key((9, 10, 11), 0.5, 7, n=2)):
        got, sweeps = CC.components(key, connectivity)
        want = np.full(key.shape, -1, dtype=np.int64)
        index = np.arange(key.size, dtype=np.int64).reshape(key.shape)
        for k in np.unique(key[key > 0]):                  # scipy labels a mask: one key at a time
            lab, n = ndi.label(key == k, structure=structure)
            ids = ndi.minimum(index, lab, np.arange(1, n + 1)).astype(np.int64)
            want = np.where(lab > 0, ids[np.maximum(lab, 1) - 1], want)
        print(f"[{key.shape} c{connectivity}] {sweeps} sweeps, {len(np.unique(got)) - 1} components")
        assert np.array_equal(got, want)


def test_yardstick_on_hand_counted_cases():
    key = np.zeros((2, 3, 4), dtype=np.int64)
    key[0, 0, 0:2] = 1                     # a run of two ...
    key[0, 1, 1] = 1                       # ... joined through a face: size 3, id 0
    key[1, 2, 3] = 1                       # a singleton, id 23
    key[0, 2, 2] = 1                       # touches (0,1,1) by an edge only: id 10 at 6, merged at 26
    key[0, 0, 2] = 2                       # another key beside the run: never merges, id 2
    c6, t6, s6 = CC.label(key, 6, 1)
    assert c6[0, 0, 0] == c6[0, 0, 1] == c6[0, 1, 1] == 0 and c6[0, 2, 2] == 10 and c6[1, 2, 3] == 23 and c6[0, 0, 2] == 2
    assert int((c6 == -1).sum()) == 24 - 6
    assert s6[0, 1, 1] == 3 and s6[0, 2, 2] == 1 and s6[1, 1, 1] == 0
    # row 1 (key 1): sizes 3, 1, 1 -> bins {0: 2, 1: 1}; row 0 (key 2 > n = 1): one singleton
    assert t6[1, :3].tolist() == [2, 1, 0] and t6[1, 32:].tolist() == [3, 5, 3]
    assert t6[0, :3].tolist() == [1, 0, 0] and t6[0, 32:].tolist() == [1, 1, 1]
    c26, t26, _ = CC.label(key, 26, 2)
    assert c26[0, 2, 2] == 0 and c26[1, 2, 3] == 0          # (1,2,3) touches (0,2,2) by an edge
    assert t26[1, :4].tolist() == [0, 0, 1, 0] and t26[1, 32:].tolist() == [1, 5, 5]
    assert t26[2, 32:].tolist() == [1, 1, 1] and t26[0].tolist() == [0] * 35
    empty = CC.label(np.zeros((2, 2, 2), dtype=np.uint8), 6, 3)
    assert bool((empty[0] == -1).all()) and not empty[1].any() and not empty[2].any()
    # size bins: 2^k <= s < 2^(k+1)
    line = np.zeros((1, 1, 40), dtype=np.int16)
    line[0, 0, 0:7] = 1
    line[0, 0, 8:16] = 1
    line[0, 0, 17:18] = 1
    t = CC.label(line, 6, 1)[1]
    assert t[1, :5].tolist() == [1, 0, 1, 1, 0] and t[1, 32:].tolist() == [3, 16, 8]
    # the LAA key: strict comparison, labels <= 0 are no lung
    img = np.array([[[-951, -950, -949, -951, -951]]], dtype=np.int16)
    lab = np.array([[[2, 2, 2, 0, -1]]], dtype=np.int16)
    assert CC.laa_key(img, lab, -950).tolist() == [[[2, 0, 0, 0, 0]]]
    assert CC.laa_key(img, lab, -950, by_lobe=False).tolist() == [[[1, 0, 0, 0, 0]]]
    # D: Y = (4, 2, 1) at k = 0, 1, 2 is an exact power law with exponent 1
    assert abs(CC.d_exponent([2, 1, 1] + [0] * 29) - 1.0) < 1e-12
    assert math.isnan(CC.d_exponent([5, 3] + [0] * 30)) and math.isnan(CC.d_exponent([0] * 32))
    assert not math.isnan(CC.d_exponent([0, 0, 1] + [0] * 29))              # kmax = 2: three points (slope 0)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_and_exported():
    from ctypes import c_int as I, c_longlong as LL, c_size_t as SZ, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _build, _lib
    assert _lib.SIGNATURES["dram_label_components_workspace"] == (SZ, [I, I, I])
    res, args = _lib.SIGNATURES["dram_label_components"]
    assert res is I and list(args) == [P, I, LL, LL, P, I, I, I, I, P, P, P, P, I, I, I, P]
    out = subprocess.run(["nm", "-D", "--defined-only", _build.build_library()], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"dram_label_components", "dram_label_components_workspace"} <= exported


def test_workspace_query_is_monotone_in_volume():
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    up = lambda b: -(-b // 256) * 256
    assert lib.dram_label_components_workspace(5, 7, 11) == up(385 * 4) + up(385 * 2)
    assert lib.dram_label_components_workspace(1, 1, 1) == 512
    shapes = [(1, 1, 1), (1, 1, 64), (1, 3, 65), (2, 3, 65), (5, 7, 11), (33, 40, 130), (40, 48, 65), (300, 350, 450),
              (1024, 1024, 1024), (2047, 1024, 1024)]
    shapes.sort(key=lambda s: s[0] * s[1] * s[2])
    got = [lib.dram_label_components_workspace(*s) for s in shapes]
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] > 0
    assert all(g >= 6 * s[0] * s[1] * s[2] for g, s in zip(got, shapes))
    assert lib.dram_label_components_workspace(0, 7, 11) == 0 and lib.dram_label_components_workspace(2048, 1024, 1024) == 0


def test_label_components_refuses_bad_and_unsupported_arguments_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    one = ctypes.c_void_p(256)                  # never dereferenced: the argument checks come first

    def call(key=one, elem=1, sz=77, sy=11, image=None, t=-950, by_lobe=1, conn=6, n=5, comp=one, sizes=None, table=one,
             work=one, size=(5, 7, 11)):
        return lib.dram_label_components(key, elem, sz, sy, image, t, by_lobe, conn, n, comp, sizes, table, work, *size, None)

    for k in ("key", "comp", "table", "work"):
        assert call(**{k: None}) == BAD, k
    for elem in (0, 3, 4, -1):
        assert call(elem=elem) == BAD, elem
    assert call(sz=-77) == BAD and call(sy=-11) == BAD
    for conn in (0, 4, 8, 18, 27, -6):
        assert call(conn=conn) == BAD, conn
    for n in (0, -1, 16, 100):
        assert call(n=n) == BAD, n
    for axis in range(3):
        for v in (0, -1):
            assert call(size=tuple(v if a == axis else s for a, s in enumerate((5, 7, 11)))) == BAD, (axis, v)
    assert call(image=one, t=40000) == BAD
    assert call(size=(2048, 1024, 1024)) == UNS and call(size=(2048, 1024, 1024), image=one, sizes=one) == UNS
    assert call(size=(2048, 1024, 1024), conn=7) == BAD                       # a bad argument is named first


def test_python_wrappers_refuse_before_the_device_is_touched():
    from bodyct_dram_emph_subtype_amd import ops
    key = torch.zeros(2, 3, 4, dtype=torch.uint8)
    img = torch.zeros(2, 3, 4, dtype=torch.int16)
    for conn in (4, 18, 0):
        with pytest.raises(ValueError, match="connectivity"):
            ops.label_components(key, connectivity=conn)
        with pytest.raises(ValueError, match="connectivity"):
            ops.laa_components(img, key, connectivity=conn)
    for n in (0, 16, -1):
        with pytest.raises(ValueError, match="n_regions"):
            ops.label_components(key, n_regions=n)
        with pytest.raises(ValueError, match="n_regions"):
            ops.laa_components(img, key, n_regions=n)
    for bad in (key.to(torch.int32), key.float(), key.to(torch.int64)):
        with pytest.raises(TypeError):
            ops.label_components(bad)
        with pytest.raises(TypeError):
            ops.laa_components(img, bad)
    with pytest.raises(TypeError):
        ops.laa_components(img.float(), key)
    with pytest.raises(ValueError):
        ops.label_components(key[0])
    with pytest.raises(ValueError, match="shape"):
        ops.laa_components(img[:, :, :3], key)
    with pytest.raises(ValueError, match="threshold"):
        ops.laa_components(img, key, threshold=-950.5)
    with pytest.raises(ValueError, match="threshold"):
        ops.laa_components(img, key, threshold=40000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.label_components(key, 26, 5, want_sizes=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.laa_components(img, key.bool())


# ------------------------------------------------------------------------------------------------ the tensor math
def test_clusters_from_table_equals_the_yardstick():
    from bodyct_dram_emph_subtype_amd import processor
    spacing = (2.5, 0.7, 0.65)
    shape, p, seed = BERNOULLI[0]
    key = CC.bernoulli_key(shape, p, seed)
    key = np.where(key == 1, 9, key)                                 # lobe 1 -> a key above n: row 0
    for conn in (6, 26):
        _, t, _ = CC.label(key, conn, 5)
        want = CC.from_table(t, spacing)
        got = processor.clusters_from_table(torch.from_numpy(t), spacing)
        print(f"[c{conn}] clusters {want['clusters'].tolist()}, largest {want['largest_voxels'].tolist()}, "
              f"D {np.round(want['d'], 4).tolist()}")
        CC.assert_clusters(got, want, f"bernoulli c{conn}")
        assert int(want["clusters"][0]) > 0 and int(want["clusters"][1]) == 0      # row 0 is populated, lobe 1 is empty
        assert np.isfinite(want["d"][2:]).all() and math.isnan(want["d"][1])
    # the NaN rules: an empty row, kmax = 0, kmax = 1 (two points), kmax = 2 (three points: finite)
    t = np.zeros((5, 35), dtype=np.int64)
    t[1, 0], t[1, 32:] = 7, (7, 7, 1)
    t[2, 0], t[2, 1], t[2, 32:] = 4, 2, (6, 10, 3)
    t[3, 0], t[3, 2], t[3, 32:] = 3, 1, (4, 8, 5)
    t[4, 0], t[4, 31], t[4, 32:] = 3, 1, (4, 2 ** 31 + 2, 2 ** 31 - 1)           # the last bin: all 32 points
    got = processor.clusters_from_table(torch.from_numpy(t), (1.0, 1.0, 1.0))
    want = CC.from_table(t, (1.0, 1.0, 1.0))
    CC.assert_clusters(got, want, "rules")
    d = got["d"].tolist()
    assert math.isnan(d[0]) and math.isnan(d[1]) and math.isnan(d[2]) and d[3] > 0 and d[4] > 0
    assert math.isnan(float(got["largest_ml"][0])) and math.isnan(float(got["mean_voxels"][0]))
    assert float(got["largest_ml"][4]) == (2 ** 31 - 1) / 1000.0 and float(got["mean_voxels"][2]) == 10 / 6
    assert set(got) == {"clusters", "voxels", "largest_voxels", "largest_ml", "mean_voxels", "size_hist", "d"}
    for bad in (torch.from_numpy(t[:1]), torch.from_numpy(t[:, :34]), torch.from_numpy(t).double()):
        with pytest.raises(ValueError):
            processor.clusters_from_table(bad, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        processor.clusters_from_table(torch.from_numpy(t), (1.0, 1.0))


def test_laa_clusters_composition_on_cpu_tensors(monkeypatch):
    """processor.laa_clusters with its kernel replaced by the yardstick: the two calls, row 1 of the whole-lung table"""
    from bodyct_dram_emph_subtype_amd import ops, processor
    rng = np.random.default_rng(5)
    shape, spacing = (8, 20, 30), (1.5, 0.8, 0.8)
    lab = CC.slab_lobes(shape, 5)
    img = np.where(rng.random(shape) < 0.35, -960, -900).astype(np.int16)
    calls = []

    def stub(image, labels, threshold, n_regions, connectivity, by_lobe=True, want_sizes=False):
        calls.append((n_regions, by_lobe))
        key = CC.laa_key(image.numpy(), labels.numpy(), threshold, n_regions, by_lobe)
        comp, t, _ = CC.label(key, connectivity, n_regions)
        return torch.from_numpy(comp.astype(np.int32)), torch.from_numpy(t), None

    monkeypatch.setattr(ops, "laa_components", stub)
    got = processor.laa_clusters(torch.from_numpy(img), torch.from_numpy(lab), spacing, connectivity=26)
    assert calls == [(5, True), (1, False)]
    want = CC.laa_clusters(img, lab, spacing, 5, -950, 26)
    CC.assert_clusters(got, want, "by lobe")
    CC.assert_clusters({k: got["whole_lung"][k] for k in want["whole_lung"]}, want["whole_lung"], "whole lung")
    assert got["threshold"] == -950 and got["connectivity"] == 26
    assert got["components"].dtype == torch.int32 and np.array_equal(got["components"].numpy(), want["components"])
    assert int(got["whole_lung"]["voxels"]) == int(got["voxels"].sum()) == int((img < -950).sum())
    assert int(got["whole_lung"]["clusters"]) < int(got["clusters"].sum())          # clusters cross the slab borders


# ------------------------------------------------------------------------------------------------ the report
def _result(threshold=-950):
    nan = float("nan")
    t = lambda v, dt=torch.float64: torch.tensor(v, dtype=dt)
    return {"clusters": t([2, 1234, 0, 1], torch.int64), "voxels": t([2, 99999, 0, 3], torch.int64),
            "largest_voxels": t([1, 50000, 0, 3], torch.int64), "largest_ml": t([0.001, 61.25049, nan, 0.0036]),
            "mean_voxels": t([1.0, 81.03, nan, 3.0]), "size_hist": torch.zeros(4, 32, dtype=torch.int64),
            "d": t([nan, 1.23456, nan, nan]),
            "whole_lung": {"clusters": t(1200, torch.int64), "voxels": t(100004, torch.int64),
                           "largest_voxels": t(70000, torch.int64), "largest_ml": t(85.75), "mean_voxels": t(83.3),
                           "size_hist": torch.zeros(32, dtype=torch.int64), "d": t(0.9876)},
            "threshold": threshold, "connectivity": 26, "components": None}


def test_laa_cluster_metrics_formats_names_and_none():
    from bodyct_dram_emph_subtype_amd import processor
    m = processor.laa_cluster_metrics(_result())
    assert set(m) == CC.CLUSTER_KEYS and len(m) == 7
    assert m["laa950_clusters_per_region"] == {"1": "1234", "2": "0", "3": "1"}
    assert m["laa950_largest_cluster_ml_per_region"] == {"1": "61.250", "2": None, "3": "0.004"}
    assert m["laa950_cluster_d_per_region"] == {"1": "1.235", "2": None, "3": None}
    assert m["laa950_clusters_per_lung"] == "1200" and m["laa950_largest_cluster_ml_per_lung"] == "85.750"
    assert m["laa950_cluster_d_per_lung"] == "0.988" and m["laa_cluster_connectivity"] == "26"
    named = processor.laa_cluster_metrics(_result(), {1: "RUL", 3: "RLL"})
    assert named["laa950_cluster_d_per_region"] == {"RUL": "1.235", "2": None, "RLL": None}
    seq = processor.laa_cluster_metrics(_result(), ["-", "a", "b"])
    assert seq["laa950_clusters_per_region"] == {"a": "1234", "b": "0", "3": "1"}
    assert json.loads(json.dumps(m))["laa950_cluster_d_per_region"]["2"] is None
    assert "laa910_cluster_d_per_lung" in processor.laa_cluster_metrics(_result(-910))
    nanlung = _result()
    nanlung["whole_lung"] = dict(nanlung["whole_lung"], d=torch.tensor(float("nan"), dtype=torch.float64))
    assert processor.laa_cluster_metrics(nanlung)["laa950_cluster_d_per_lung"] is None
    for flat in (-0.0, -1e-17, 1e-17):                                         # a flat line reads 0.000, never -0.000
        nanlung["whole_lung"]["d"] = torch.tensor(flat, dtype=torch.float64)
        assert processor.laa_cluster_metrics(nanlung)["laa950_cluster_d_per_lung"] == "0.000"
    as_numpy = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in _result().items()}
    as_numpy["whole_lung"] = {k: v.numpy() for k, v in _result()["whole_lung"].items()}
    assert processor.laa_cluster_metrics(as_numpy) == m                        # the yardstick's arrays format alike


def test_new_keys_match_neither_existing_pattern():
    from bodyct_dram_emph_subtype_amd import processor
    for t in (-950, -910, -856):
        for k in processor.laa_cluster_metrics(_result(t)):
            assert not processor._DENSITO_KEY.fullmatch(k), k
            assert not processor._CORE_PEEL_KEY.fullmatch(k), k
            assert processor._CLUSTER_KEY.fullmatch(k), k
            assert k not in processor.REGION_KEYS
    for k in ("laa950_fraction_per_region", "volume_ml_per_lung", "laa950_fraction_per_region_peel", "peel_mm",
              "region_voxels", "cle_lesion_percentage_per_lung"):
        assert not processor._CLUSTER_KEY.fullmatch(k), k


def _prediction():
    return {"cle_dense_outs": torch.zeros(1, 1, 2, 2, 2), "pse_dense_outs": torch.zeros(1, 1, 2, 2, 2),
            "cle_precentages": torch.tensor([0.02]), "pse_precentages": torch.tensor([0.3]),
            "crop_slices": torch.tensor([[[0, 2], [0, 2], [0, 2]]]), "original_size": torch.tensor([[2, 2, 2]]), "uids": ["u"]}


def test_write_reports_clusters_json(monkeypatch, tmp_path):
    from bodyct_dram_emph_subtype_amd import processor
    monkeypatch.setattr(processor, "resample_paste", lambda d, *a, **k: (None, torch.zeros(2, 2, 2, dtype=torch.uint8)))
    plain = processor.build_outputs([_prediction()])[0]
    clu = processor.build_outputs([_prediction()])[0]
    added = processor.laa_cluster_metrics(_result())
    clu["metrics"].update(added)
    names = ("centrilobular_json", "paraseptal_json", "output_json")
    before = {k: str(tmp_path / f"a_{k}") for k in names}
    after = {k: str(tmp_path / f"b_{k}") for k in names}
    processor.write_reports([plain], **before)
    processor.write_reports([plain], **after, clusters_json=None)
    for k in names:                                                    # without the argument: byte for byte as before
        assert open(before[k], "rb").read() == open(after[k], "rb").read(), k
    path = str(tmp_path / "clusters.json")
    processor.write_reports([clu], **after, clusters_json=path)
    assert json.load(open(path)) == json.loads(json.dumps(added)) and len(added) == 7
    for k in names[:2]:                                                # the two score files do not see the new keys
        assert open(before[k], "rb").read() == open(after[k], "rb").read(), k
    assert json.load(open(after["output_json"]))[0]["metrics"] == clu["metrics"]
    with pytest.raises(ValueError, match="clusters_json"):
        processor.write_reports([plain], clusters_json=path)
    with pytest.raises(ValueError, match="densitometry_json"):         # the cluster keys are not the densitometry's
        processor.write_reports([clu], densitometry_json=str(tmp_path / "d.json"))
    with pytest.raises(ValueError, match="core_peel_json"):
        processor.write_reports([clu], core_peel_json=str(tmp_path / "c.json"))
