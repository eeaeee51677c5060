"""GPU: the per-component table of csrc/ccl_shapes.hip (dram_component_rank + dram_component_shapes through
ops.component_shapes) against the numpy yardstick of tests/shapes_ref.py, and the cluster shapes of the report built on
it (processor.laa_clusters(shapes=True) -> predict_case(cluster_kw={'shapes': True})).

Rows and count are compared with EXACT integer equality.  Shapes, from the launch rules of csrc/ccl_shapes.hip (rank: a
workgroup per 4096 voxels, one scan workgroup over the workgroup counts; accumulate: one wave per x-row in chunks of 64
voxels, 4 rows per wave, 4 waves per workgroup): a single voxel, rows of 63 / 64 / 65 / 130 voxels filled by one run
(the chunk cuts and the carry), random keys on a ragged row length, a checkerboard whose ranks cross many rank
workgroups, one component with a coordinate sum above 2^32, and `components` contents that name nothing valid.  Every
case runs with torch.empty poisoned (a workspace or output element that is read unwritten shows)."""
import ctypes

import numpy as np
import pytest
import torch

import case_prep_ref as CR
import ccl_ref as CC
import shapes_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -1234567891


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    e0 = torch.empty

    def fill(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(255)
        elif t.dtype in (torch.int32, torch.int64):
            t.fill_(POISON)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(e0(*a, **k)))
    yield
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(ops, comp, labels=None, zones=None, what=""):
    """ops.component_shapes on the device against the yardstick, with the default capacity; -> the yardstick's rows"""
    comp32 = np.asarray(comp).astype(np.int32)
    want = SR.rows(comp32, labels, zones)
    rows, count = ops.component_shapes(dev(comp32), None if labels is None else dev(labels),
                                       None if zones is None else dev(zones))
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (want.shape[0], 18), (what, rows.shape, want.shape)
    assert count.cpu().tolist() == [want.shape[0], want.shape[0]], (what, count)
    got = rows.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, bad[:8], got[bad[:8, 0]], want[bad[:8, 0]])
    assert np.all(np.diff(got[:, 0]) > 0)                                      # ascending root order
    return want


# ------------------------------------------------------------------------------------------------ tiny and ragged x
def test_single_voxel_foreground_and_background(ops):
    want = check(ops, np.zeros((1, 1, 1)), what="foreground")
    assert want.tolist() == [[0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 2, 2, 2, 0, 0, 0]]
    assert check(ops, np.full((1, 1, 1), -1), what="background").shape == (0, 18)


@pytest.mark.parametrize("W", [63, 64, 65, 130])
def test_one_run_across_the_whole_row(ops, W):
    want = check(ops, np.zeros((1, 1, W)), what=W)
    assert want.tolist() == [[0, 0, W, 0, 1, 0, 1, 0, W, 0, 0, W * (W - 1) // 2, 2 * W, 2 * W, 2, 0, 0, 0]]


@pytest.mark.parametrize("W", [65, 130])
def test_runs_that_change_value_at_the_chunk_cut(ops, W):
    """two components per row meeting at x = 64, and a run ending at x = 63 before background: the x faces at the cut"""
    comp = np.full((1, 2, W), -1, dtype=np.int64)
    comp[0, 0, :64] = 0
    comp[0, 0, 64:] = 64
    comp[0, 1, 10:64] = W + 10
    check(ops, comp, what=W)


# ------------------------------------------------------------------------------------------------ random keys
@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(7)
    shape = (3, 5, 67)
    key = np.where(rng.random(shape) < 0.5, rng.integers(1, 4, shape), 0).astype(np.uint8)
    zones = rng.integers(0, 5, shape).astype(np.uint8)
    return key, zones, {c: CC.label(key, c, 5)[0] for c in (6, 26)}


@pytest.mark.parametrize("connectivity", [6, 26])
def test_random_keys_through_label_components(ops, random_case, connectivity):
    key, zones, want_comp = random_case
    comp, table, sizes = ops.label_components(dev(key), connectivity, 5, want_sizes=True)
    assert np.array_equal(comp.cpu().numpy(), want_comp[connectivity])
    want = SR.rows(want_comp[connectivity], key, zones)
    for labels in (dev(key), dev(key.astype(np.int16)), dev(np.repeat(key, 2, axis=1))[:, ::2, :],
                   dev(np.pad(key, ((0, 0), (0, 0), (3, 2))))[:, :, 3:70]):
        rows, count = ops.component_shapes(comp, labels, dev(zones))
        assert np.array_equal(rows.cpu().numpy(), want), (connectivity, labels.dtype, labels.stride())
        assert count.cpu().tolist() == [want.shape[0]] * 2
    # consistency with the labelling: the table's component count and voxels, cluster_voxels at every root
    assert want.shape[0] == int(table[:, 32].sum()) and int(want[:, 2].sum()) == int(table[:, 33].sum())
    assert np.array_equal(want[:, 2], sizes.cpu().numpy().ravel()[want[:, 0]])
    assert int(want[:, 15:].sum()) == int(((zones >= 1) & (zones <= 3) & (key > 0)).sum())   # zones 0 and 4 count nowhere
    without = SR.rows(want_comp[connectivity])
    rows, _ = ops.component_shapes(comp)
    assert np.array_equal(rows.cpu().numpy(), without) and not without[:, 1].any() and not without[:, 15:].any()


def test_int16_labels_keep_their_sign_and_value(ops):
    comp = np.zeros((1, 2, 3), dtype=np.int64)
    comp[0, 1] = 3
    lab = np.array([[[-5, 1, 1], [300, 1, 1]]], dtype=np.int16)
    assert check(ops, comp, lab)[:, 1].tolist() == [-5, 300]


# ------------------------------------------------------------------------------------------------ many and giant
def test_checkerboard_ranks_cross_many_rank_blocks(ops):
    shape = (20, 33, 65)
    z, y, x = np.indices(shape)
    key = ((z + y + x) % 2 == 0).astype(np.uint8)
    comp, table, _ = ops.label_components(dev(key), 6, 1)
    want_comp = np.where(key > 0, np.arange(key.size).reshape(shape), -1)
    assert np.array_equal(comp.cpu().numpy(), want_comp)
    want = check(ops, want_comp, what="checkerboard")
    assert want.shape[0] == 21450 == int(table[1, 32]) and np.all(want[:, 2] == 1) and np.all(want[:, 12:15] == 2)


def test_one_component_whose_sums_pass_32_bits(ops):
    shape = (2, 2, 100003)
    want = check(ops, np.zeros(shape), zones=np.full(shape, 2, dtype=np.uint8), what="giant")
    W = shape[2]
    assert want[0, 11] == 4 * (W * (W - 1) // 2) > 2 ** 34 and want[0, 2] == 4 * W == want[0, 16]
    assert want[0, 12:15].tolist() == [4 * W, 4 * W, 8]


# ------------------------------------------------------------------------------------------------ capacity, empty
def test_capacity_below_equal_and_above_the_count(ops, random_case):
    key, zones, want_comp = random_case
    full = SR.rows(want_comp[6], key, zones)
    m = full.shape[0]
    assert m > 8
    for cap in (0, 1, m - 3, m, m + 5):
        rows, count = ops.component_shapes(dev(want_comp[6].astype(np.int32)), dev(key), dev(zones), max_components=cap)
        want, want_count = SR.with_capacity(full, cap)
        assert tuple(rows.shape) == (cap, 18) and np.array_equal(rows.cpu().numpy(), want), cap
        assert np.array_equal(count.cpu().numpy(), want_count), cap


def test_empty_volume(ops):
    comp = dev(np.full((3, 4, 70), -1, dtype=np.int32))
    rows, count = ops.component_shapes(comp)
    assert tuple(rows.shape) == (0, 18) and count.cpu().tolist() == [0, 0]
    rows, count = ops.component_shapes(comp, max_components=4)
    assert tuple(rows.shape) == (4, 18) and not rows.cpu().numpy().any() and count.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ hostile components
def test_contents_that_name_nothing_valid_are_background(ops, random_case):
    """values >= D*H*W, values < -1 and values naming a non-root: the rule of the header makes them background, and
    the rows of the rest are the yardstick's under the same rule"""
    key, zones, want_comp = random_case
    comp = want_comp[26].astype(np.int64).copy()
    total = comp.size
    flat = comp.ravel()
    rng = np.random.default_rng(3)
    non_roots = np.nonzero((flat >= 0) & (flat != np.arange(total)))[0]
    assert non_roots.size > 20
    picks = rng.choice(total, size=40, replace=False)
    hostile = [total, total + 7, 2 ** 31 - 1, -2, -7, -2 ** 31] + [int(v) for v in non_roots[:6]]
    for i, v in enumerate(picks):
        flat[v] = hostile[i % len(hostile)]
    flat[total - 1] = 2 ** 31 - 1
    flat[0] = -2 ** 31
    assert (~SR.counted(comp) & (comp != -1)).sum() > 40                       # the corruption orphaned voxels as well
    want = check(ops, comp, key, zones, what="hostile")
    assert 0 < want.shape[0]


# ------------------------------------------------------------------------------------------------ determinism
def test_two_calls_are_bit_identical_and_components_is_only_read(ops):
    key = CC.bernoulli_key((9, 21, 130), 0.6, 4)
    comp, _, _ = ops.label_components(dev(key), 26)
    before = comp.clone()
    zones = dev(np.random.default_rng(1).integers(0, 4, key.shape).astype(np.uint8))
    a = ops.component_shapes(comp, dev(key), zones)
    b = ops.component_shapes(comp, dev(key), zones)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(comp, before)
    assert np.array_equal(a[0].cpu().numpy(), SR.rows(comp.cpu().numpy(), key, zones.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refusals(ops):
    from bodyct_dram_emph_subtype_amd import _lib
    L = ops._L()
    BAD, UNSUP = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    comp = torch.full((2, 3, 70), -1, dtype=torch.int32, device=DEV)
    lab = torch.ones((2, 3, 70), dtype=torch.uint8, device=DEV)
    nbytes = L.dram_component_shapes_workspace(2, 3, 70)
    assert nbytes > 420 * 4 and nbytes % 256 == 0
    assert L.dram_component_shapes_workspace(0, 3, 70) == 0 and L.dram_component_shapes_workspace(2048, 1024, 1024) == 0
    work = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    rows = torch.zeros((4, 18), dtype=torch.int64, device=DEV)
    count = torch.zeros(2, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rank = lambda c=p(comp), w=p(work), n=p(count), size=(2, 3, 70): L.dram_component_rank(c, w, n, *size, None)
    assert rank(c=None) == BAD and rank(w=None) == BAD and rank(n=None) == BAD
    for size in ((0, 3, 70), (2, 0, 70), (2, 3, 0), (2, -3, 70)):
        assert rank(size=size) == BAD, size
    assert rank(size=(2048, 1024, 1024)) == UNSUP

    def shapes(c=p(comp), lb=None, elem=1, sz=0, sy=0, zn=None, w=p(work), r=p(rows), cap=4, n=p(count), size=(2, 3, 70)):
        return L.dram_component_shapes(c, lb, elem, sz, sy, zn, w, r, cap, n, *size, None)

    assert shapes(c=None) == BAD and shapes(w=None) == BAD and shapes(n=None) == BAD
    assert shapes(r=None) == BAD and shapes(cap=-1) == BAD
    assert shapes(lb=p(lab), elem=4, sz=210, sy=70) == BAD and shapes(lb=p(lab), elem=0, sz=210, sy=70) == BAD
    assert shapes(lb=p(lab), sz=-210, sy=70) == BAD and shapes(sy=-1) == BAD
    for size in ((0, 3, 70), (2, 0, 70), (2, 3, 0)):
        assert shapes(size=size) == BAD, size
    assert shapes(size=(2048, 1024, 1024)) == UNSUP
    torch.cuda.synchronize()
    assert not rows.any() and not count.any()                                  # a refused call launches nothing
    assert rank() == 0 and shapes(r=None, cap=0) == 0 and shapes(lb=p(lab), elem=1, sz=210, sy=70) == 0
    assert shapes(elem=7) == 0                                                 # lab_elem is not looked at without labels


def test_wrapper_refusals_come_before_any_launch(ops, monkeypatch):
    comp = torch.full((2, 3, 70), -1, dtype=torch.int32, device=DEV)
    L = ops._L()
    launches = []

    class Spy:
        def __getattr__(self, name):
            if name in ("dram_component_rank", "dram_component_shapes"):
                return lambda *a: launches.append(name) or getattr(L, name)(*a)
            return getattr(L, name)

    monkeypatch.setattr(ops, "_L", lambda: Spy())
    with pytest.raises(TypeError):
        ops.component_shapes(comp.long())
    with pytest.raises(ValueError):
        ops.component_shapes(comp[0])
    with pytest.raises(ValueError, match="contiguous"):
        ops.component_shapes(comp.expand(2, 2, 3, 70)[:, :, :, ::2][0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.component_shapes(comp.cpu())
    with pytest.raises(TypeError):
        ops.component_shapes(comp, zones=comp)
    with pytest.raises(ValueError, match="shape"):
        ops.component_shapes(comp, zones=torch.zeros((2, 3, 60), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="contiguous"):
        ops.component_shapes(comp, zones=torch.zeros((2, 3, 140), dtype=torch.uint8, device=DEV)[:, :, ::2])
    with pytest.raises(ValueError, match="shape"):
        ops.component_shapes(comp, labels=torch.zeros((2, 3, 60), dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.component_shapes(comp, labels=comp)
    with pytest.raises(ValueError, match="max_components"):
        ops.component_shapes(comp, max_components=-1)
    with pytest.raises(ValueError, match="max_components"):
        ops.component_shapes(comp, max_components=2.5)
    assert launches == []
    ops.component_shapes(comp, max_components=3)
    assert launches == ["dram_component_rank", "dram_component_shapes"]


# ------------------------------------------------------------------------------------------------ laa_clusters
def yardstick_wrappers(monkeypatch, ops):
    """ops.laa_components and ops.component_shapes on CPU tensors, by the numpy yardsticks"""
    def laa_components(image, labels, threshold, n_regions, connectivity, by_lobe=True, want_sizes=False):
        key = CC.laa_key(image.numpy(), labels.numpy(), threshold, n_regions, by_lobe)
        comp, t, _ = CC.label(key, connectivity, n_regions)
        return torch.from_numpy(comp.astype(np.int32)), torch.from_numpy(t), None

    def component_shapes(components, labels=None, zones=None, max_components=None):
        r = SR.rows(components.numpy(), None if labels is None else labels.numpy(), None if zones is None else zones.numpy())
        return torch.from_numpy(r), torch.tensor([r.shape[0]] * 2, dtype=torch.int64)

    monkeypatch.setattr(ops, "laa_components", laa_components)
    monkeypatch.setattr(ops, "component_shapes", component_shapes)


@pytest.mark.parametrize("zoned", [False, True])
def test_laa_clusters_with_shapes_equals_the_cpu_composition(ops, monkeypatch, zoned):
    from bodyct_dram_emph_subtype_amd import processor
    rng = np.random.default_rng(12)
    shape, spacing = (7, 22, 70), (1.5, 0.8, 0.8)
    lab = CC.slab_lobes(shape, 5)
    lab[:, 9, :30] = 9
    hu = np.where(rng.random(shape) < 0.45, -960, -900).astype(np.int16)
    zones = rng.integers(0, 4, shape).astype(np.uint8)
    kw = dict(n_regions=5, connectivity=6, shapes=True, bulla_mm=3.0, top=5, origin=(3, 20, 100))
    if zoned:
        kw_dev = dict(kw, zones=dev(zones), zone_names=processor.FISSURE_ZONES)
        kw_cpu = dict(kw, zones=torch.from_numpy(zones), zone_names=processor.FISSURE_ZONES)
    else:
        kw_dev = kw_cpu = kw
    got = processor.laa_clusters(dev(hu), dev(lab), spacing, **kw_dev)
    plain = processor.laa_clusters(dev(hu), dev(lab), spacing, n_regions=5, connectivity=6)
    assert set(got) == set(plain) | {"shapes"}
    yardstick_wrappers(monkeypatch, ops)
    want = processor.laa_clusters(torch.from_numpy(hu), torch.from_numpy(lab), spacing, **kw_cpu)
    sg, sw = got["shapes"], want["shapes"]
    assert sg["rows"].is_cuda and sg["sphericity"].is_cuda
    for k in ("rows", "whole_lung_rows"):
        assert torch.equal(sg[k].cpu(), sw[k]), k
    as_np = lambda s: {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in s.items()}
    SR.assert_shapes(sg, as_np(sw), "by lobe")
    SR.assert_shapes(sg["whole_lung"], as_np(sw["whole_lung"]), "whole lung")
    SR.assert_shapes(sg, SR.from_rows(sw["rows"].numpy(), spacing, 5, 3.0, 5, (3, 20, 100), 3 if zoned else 0), "yardstick")
    assert int(sg["bullae"].sum()) > 0 and int(sg["region"].eq(0).sum()) > 0
    m_got, m_want = processor.laa_cluster_metrics(got), processor.laa_cluster_metrics(want)
    assert m_got == m_want and all(processor._CLUSTER_KEY.fullmatch(k) for k in m_got)
    assert ("laa950_bullae_per_region_fissure" in m_got) == zoned
    assert {k: m_got[k] for k in processor.laa_cluster_metrics(plain)} == processor.laa_cluster_metrics(plain)


# ------------------------------------------------------------------------------------------------ predict_case
def test_predict_case_with_cluster_shapes(ops):
    from bodyct_dram_emph_subtype_amd import models, processor
    name = "blobs_u8"
    scan, lobes, spacing, _ = CR.fixture_cases()[name]
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    run = lambda **sw: processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, (16, 32, 32), uid=name,
                                              region_names=names, clusters=True, **sw)
    shape_kw = {"shapes": True, "bulla_mm": 2.0, "top": 2}
    zone_key = lambda k: k.endswith(("_peel", "_core", "_fissure")) and processor._CLUSTER_KEY.fullmatch(k)
    for sw in ({}, {"core_peel": True, "peel_mm": 3.0}):
        off = run(**sw)
        off_kw = run(cluster_kw={"shapes": False}, **sw)
        on = run(cluster_kw=shape_kw, **sw)
        assert off_kw["metrics"] == off["metrics"] and list(off_kw["metrics"]) == list(off["metrics"])
        assert {k: on["metrics"][k] for k in off["metrics"]} == off["metrics"], sw
        assert on["error_messages"] == off["error_messages"]
        for k in ("full_cle", "full_pse"):
            assert torch.equal(on[k], off[k]) and torch.equal(off_kw[k], off[k]), (sw, k)
        new = set(on["metrics"]) - set(off["metrics"])
        assert {"laa950_bullae_per_region", "laa950_bulla_ml_per_lung", "laa950_bulla_laa_share_per_region",
                "laa950_largest_clusters", "bulla_mm", "bulla_min_voxels"} <= new
        assert all(processor._CLUSTER_KEY.fullmatch(k) for k in new)
        zoned = {k for k in new if zone_key(k)}
        if sw:
            assert zoned == {f"laa950_{s}_per_{w}_{z}" for s in ("clusters", "bullae") for w in ("region", "lung")
                             for z in ("peel", "core")}
        else:
            assert zoned == set()
        largest = on["metrics"]["laa950_largest_clusters"]
        assert len(largest) == 2 and on["metrics"]["bulla_mm"] == "2.000"
        assert set(largest[0]) == {"region", "volume_ml", "diameter_mm", "extent_mm", "centroid", "surface_mm2",
                                   "sphericity", "zone"}
        assert float(largest[0]["volume_ml"]) >= float(largest[1]["volume_ml"]) > 0
        assert (largest[0]["zone"] in ("peel", "core")) if sw else (largest[0]["zone"] is None)
