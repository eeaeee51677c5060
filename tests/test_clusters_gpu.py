"""GPU: the connected-component labelling of csrc/ccl.hip (dram_label_components through ops.label_components /
ops.laa_components) against the min-propagation yardstick of tests/ccl_ref.py, and the LAA cluster report built on it
(processor.laa_clusters -> predict_case(clusters=True)).

Every labelling case asserts that `components` (int32, the whole volume), `table` and `cluster_voxels` equal the
yardstick EXACTLY, for connectivity 6 and 26.  Shapes, from the launch rule of csrc/ccl.hip (init: one wave per x-row
in chunks of 64 voxels, 4 rows per workgroup; every other launch: one thread per voxel, 256 per workgroup): single
voxel and W / H / D = 1, row lengths 63 / 64 / 65 / 130 with runs that start and end on lanes 0, 63 and 64, more than
one workgroup in every launch, and one volume above the 2048 workgroups the table launch is capped at.  The yardstick of a case is computed once and shared.  Every case runs with
torch.empty poisoned (a workspace or output element that is read unwritten shows)."""
import functools
import math

import numpy as np
import pytest
import torch

import case_prep_ref as CR
import ccl_ref as CC

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


# ------------------------------------------------------------------------------------------------ the cases
def _rand(shape, p, seed, keys=(1,)):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < p, rng.choice(np.array(keys), size=shape), 0).astype(np.uint8)


def _runs(W):
    """6 x-rows whose runs start and end on lanes 0, 63 and 64 (clipped to the row), in two planes of three rows"""
    key = np.zeros((2, 3, W), dtype=np.uint8)
    rows = key.reshape(6, W)
    rows[0, :] = 1                                         # the whole row: every chunk carries the run on
    rows[1, 0] = 1                                         # lane 0 alone
    rows[1, 62:65] = 1                                     # across lanes 62..64
    rows[2, 63:] = 1                                       # starts on lane 63
    rows[3, 10:63] = 1                                     # ends on lane 62 ...
    rows[3, 64:] = 1                                       # ... and the next starts on lane 64
    rows[4, 1:64] = 1                                      # ends on lane 63
    rows[4, 65:] = 1
    rows[5, ::2] = 1                                       # singletons on every even lane
    rows[5, 1::2] = 2                                      # and another key between them: no background at all
    return key


def _key_change(W=70):
    """runs split by a key change with no background between the two keys, on the lanes around the chunk boundary"""
    key = np.zeros((1, 3, W), dtype=np.uint8)
    key[0, 0, :64], key[0, 0, 64:] = 1, 2
    key[0, 1, :63], key[0, 1, 63:] = 2, 1
    key[0, 2, :] = np.repeat(np.array([1, 2, 3, 1, 1, 2, 2], dtype=np.uint8), 10)[:W]
    return key


def _comb(axis, shape=(9, 10, 70), teeth=None):
    """teeth along `axis` that only join through a bar at the HIGHEST index of that axis (a late merge)"""
    key = np.zeros(shape, dtype=np.uint8)
    D, H, W = shape
    step = slice(None, None, 2) if teeth is None else slice(0, 2 * teeth, 2)
    if axis == 0:
        key[:, 0, step] = 1
        key[D - 1, 0, :(W if teeth is None else 2 * teeth - 1)] = 1
    elif axis == 1:
        key[0, :, step] = 1
        key[0, H - 1, :(W if teeth is None else 2 * teeth - 1)] = 1
    else:
        key[0, step, :] = 1
        key[0, :(H if teeth is None else 2 * teeth - 1), W - 1] = 1
    return key


def _serpentine(shape=(12, 12, 13)):
    """one component that winds through the whole volume: full x-rows on even y of even z, single connector voxels"""
    D, H, W = shape
    key = np.zeros(shape, dtype=np.uint8)
    for z in range(0, D, 2):
        key[z, 0::2, :] = 1
        for y in range(1, H - 1, 2):
            key[z, y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    last_row = (H - 1) // 2 * 2
    end_x = 0 if (last_row // 2) % 2 == 1 else W - 1       # where the plane's last row ends
    for z in range(1, D - 1, 2):
        key[z, last_row if (z // 2) % 2 == 0 else 0, end_x if (z // 2) % 2 == 0 else 0] = 1
    return key


def _two_keys():
    """blocks of different keys that touch on faces, edges and corners, one key above n_regions = 5"""
    key = np.zeros((4, 4, 6), dtype=np.uint8)
    key[0:2, 0:2, 0:3] = 1
    key[0:2, 0:2, 3:6] = 2                                 # a face with the block of key 1
    key[2:4, 2:4, 3:6] = 7                                 # an edge with key 2, a corner with key 1; above n
    key[2:4, 2:4, 0:3] = 1                                 # an edge with the first block of key 1: merges at 26 only
    key[2:4, 0:2, 0:3] = 3
    return key


def _staircases():
    """three diagonals connected only through corners, one per sign of the x / y step"""
    key = np.zeros((8, 8, 70), dtype=np.uint8)
    i = np.arange(8)
    key[i, i, i] = 1
    key[i, i, 69 - i] = 1
    key[i, 7 - i, 30 + i] = 1
    return key


def _checkerboard():
    z, y, x = np.indices((8, 8, 9))
    return ((z + y + x) % 2 == 0).astype(np.uint8)


CASES = {
    "single_voxel": lambda: np.ones((1, 1, 1), dtype=np.uint8),
    "w1": lambda: _rand((5, 6, 1), 0.6, 1, (1, 2)),
    "h1": lambda: _rand((5, 1, 70), 0.6, 2, (1, 2)),
    "d1": lambda: _rand((1, 6, 70), 0.6, 3, (1, 2)),
    "empty": lambda: np.zeros((3, 5, 70), dtype=np.uint8),
    "full": lambda: np.ones((16, 24, 130), dtype=np.uint8),
    "runs_w63": lambda: _runs(63), "runs_w64": lambda: _runs(64), "runs_w65": lambda: _runs(65),
    "runs_w130": lambda: _runs(130),
    "key_change": _key_change,
    "checkerboard": _checkerboard,
    "u_z": lambda: _comb(0, teeth=2), "u_y": lambda: _comb(1, teeth=2), "u_x": lambda: _comb(2, teeth=2),
    "comb_z": lambda: _comb(0), "comb_y": lambda: _comb(1), "comb_x": lambda: _comb(2),
    "serpentine": _serpentine,
    "two_keys": _two_keys,
    "staircases": _staircases,
    "bernoulli_40x48x65_p25": lambda: CC.bernoulli_key((40, 48, 65), 0.25, 1),
    "bernoulli_40x48x65_p31": lambda: CC.bernoulli_key((40, 48, 65), 0.31, 2),
    "bernoulli_33x40x130_p30": lambda: CC.bernoulli_key((33, 40, 130), 0.30, 3),
    # 548 080 voxels = 2141 workgroups of 256: above the 2048 the table launch is capped at, so its threads loop
    # (p below both percolation thresholds: the yardstick converges in a few sweeps)
    "table_stride_34x124x130_p08": lambda: CC.bernoulli_key((34, 124, 130), 0.08, 4),
}
# what the case is there to show: (components at 6, components at 26), counted by hand
EXPECT = {"single_voxel": (1, 1), "empty": (0, 0), "full": (1, 1), "checkerboard": (8 * 8 * 9 // 2, 1),
          "u_z": (1, 1), "u_y": (1, 1), "u_x": (1, 1), "comb_z": (1, 1), "comb_y": (1, 1), "comb_x": (1, 1),
          "serpentine": (1, 1), "two_keys": (5, 4), "staircases": (24, 3)}


@functools.lru_cache(maxsize=None)
def reference(name, connectivity, n=5):
    key = CASES[name]()
    comp, table, sizes = CC.label(key, connectivity, n)
    for a in (key, comp, table, sizes):
        a.setflags(write=False)
    return key, comp, table, sizes


def assert_equal(what, got, want):
    comp, table, sizes = got
    w_comp, w_table, w_sizes = want
    assert comp.dtype == torch.int32 and tuple(comp.shape) == w_comp.shape and comp.is_contiguous(), what
    assert table.dtype == torch.int64 and tuple(table.shape) == w_table.shape, what
    c, t = comp.cpu().numpy(), table.cpu().numpy()
    print(f"[{what}] voxels {w_comp.size}, foreground {int((w_comp >= 0).sum())}, components {int(w_table[:, 32].sum())}, "
          f"largest {int(w_table[:, 34].max())}; differing ids {int((c != w_comp).sum())}, "
          f"table entries {int((t != w_table).sum())}")
    assert np.array_equal(c, w_comp.astype(np.int32)), what
    assert np.array_equal(t, w_table), (what, t, w_table)
    if sizes is not None:
        assert sizes.dtype == torch.int32 and tuple(sizes.shape) == w_sizes.shape, what
        assert np.array_equal(sizes.cpu().numpy(), w_sizes.astype(np.int32)), what


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", sorted(CASES))
def test_components_and_table_equal_the_yardstick(ops, name, connectivity):
    key, comp, table, sizes = reference(name, connectivity)
    if name in EXPECT:
        assert int(table[:, 32].sum()) == EXPECT[name][connectivity == 26], "the case does not show what it is there for"
    got = ops.label_components(torch.from_numpy(key.copy()).to(DEV), connectivity, 5, want_sizes=True)
    assert_equal(f"{name} c{connectivity}", got, (comp, table, sizes))
    if name == "two_keys":
        assert int(table[0, 33]) == 12 and int(table[4:, 32].sum()) == 0          # key 7 is in row 0
    if name.startswith("bernoulli"):
        assert bool((table[1:, :32].sum(0) > 0).sum() >= 3) and bool((table[1:, 34] > 8).all())


def test_without_sizes_the_same_components(ops):
    key, comp, table, _ = reference("bernoulli_40x48x65_p31", 26)
    got = ops.label_components(torch.from_numpy(key.copy()).to(DEV), 26)
    assert got[2] is None
    assert_equal("no sizes", got, (comp, table, None))


# ------------------------------------------------------------------------------------------------ views and key types
@pytest.mark.parametrize("connectivity", [6, 26])
def test_strided_view_int16_and_bool_keys(ops, connectivity):
    rng = np.random.default_rng(11)
    shape = (7, 9, 67)
    key = np.where(rng.random(shape) < 0.45, rng.integers(1, 4, size=shape), 0).astype(np.int16)
    flat = key.reshape(-1)
    pos = rng.choice(flat.size, size=60, replace=False)
    flat[pos] = np.resize(np.array([300, -1, -32768, 32767, 6, -7], dtype=np.int16), pos.size)
    want = CC.label(key, connectivity, 5)
    assert int(want[1][0, 32]) > 0 and bool((want[0][key < 0] == -1).all())
    big = torch.zeros((9, 13, 75), dtype=torch.int16)
    big[1:8, 2:11, 5:72] = torch.from_numpy(key)
    view = big.to(DEV)[1:8, 2:11, 5:72]                                         # a crop view: x stride 1
    assert not view.is_contiguous() and view.stride(2) == 1
    assert_equal("int16 crop view", ops.label_components(view, connectivity, 5, want_sizes=True), want)
    wide = torch.zeros((7, 9, 134), dtype=torch.int16)
    wide[:, :, ::2] = torch.from_numpy(key)
    assert_equal("x stride 2", ops.label_components(wide.to(DEV)[:, :, ::2], connectivity, 5, want_sizes=True), want)
    u8 = np.where(key > 0, np.minimum(key, 255), 0).astype(np.uint8)
    base = torch.zeros((9, 13, 75), dtype=torch.uint8)
    base[1:8, 2:11, 5:72] = torch.from_numpy(u8)
    assert_equal("uint8 crop view", ops.label_components(base.to(DEV)[1:8, 2:11, 5:72], connectivity, 5, want_sizes=True),
                 CC.label(u8, connectivity, 5))
    mask = key > 0
    assert_equal("bool", ops.label_components(torch.from_numpy(mask).to(DEV), connectivity, 1, want_sizes=True),
                 CC.label(mask, connectivity, 1))


# ------------------------------------------------------------------------------------------------ the image form
T = -950


@functools.lru_cache(maxsize=None)
def laa_case():
    rng = np.random.default_rng(21)
    shape, n = (10, 30, 70), 5
    lab = CC.slab_lobes(shape, n).astype(np.int16)
    lab[:, :, :4] = 0
    lab[:, :, 66:] = -2                                    # not lung
    lab[3:5, 8:12, 20:30] = 7                              # lung in no region
    hu = rng.choice(np.array([T - 1, T, T + 1, -1000, -800, -32768, 32767], dtype=np.int16), size=shape,
                    p=[0.2, 0.2, 0.2, 0.15, 0.15, 0.05, 0.05])
    for a in (lab, hu):
        a.setflags(write=False)
    return hu, lab, n


@pytest.mark.parametrize("by_lobe", [True, False], ids=["by_lobe", "whole_lung"])
@pytest.mark.parametrize("connectivity", [6, 26])
def test_image_form_equals_the_yardstick_on_the_laa_key(ops, connectivity, by_lobe):
    hu, lab, n = laa_case()
    rows = n if by_lobe else 1
    key = CC.laa_key(hu, lab, T, n, by_lobe)
    assert int(((hu == T - 1) & (lab > 0)).sum()) > 0 and bool((key[hu >= T] == 0).all()) and bool((key[hu == T - 1][lab[hu == T - 1] > 0] > 0).all())
    want = CC.label(key, connectivity, rows)
    got = ops.laa_components(torch.from_numpy(hu.copy()).to(DEV), torch.from_numpy(lab.copy()).to(DEV), T, n, connectivity,
                             by_lobe=by_lobe, want_sizes=True)
    assert tuple(got[1].shape) == (rows + 1, 35)
    assert_equal(f"laa c{connectivity} by_lobe={by_lobe}", got, want)
    if by_lobe:
        assert int(want[1][0, 33]) > 0                                          # label 7: row 0
    u8 = np.where(lab > 0, lab, 0).astype(np.uint8)                             # uint8 labels, another threshold
    want = CC.label(CC.laa_key(hu, u8, T + 1, n, by_lobe), connectivity, rows)
    got = ops.laa_components(torch.from_numpy(hu.copy()).to(DEV), torch.from_numpy(u8).to(DEV), T + 1, n, connectivity,
                             by_lobe=by_lobe, want_sizes=True)
    assert_equal(f"laa u8 t+1 c{connectivity} by_lobe={by_lobe}", got, want)


@pytest.mark.parametrize("threshold", [-950, -910])
def test_voxel_column_equals_densitometry_laa_counts(ops, threshold):
    """table column 33 against the histogram pass of csrc/densito.hip, row by row"""
    from bodyct_dram_emph_subtype_amd import processor
    rng = np.random.default_rng(31)
    shape, n = (12, 40, 70), 5
    lab = CC.slab_lobes(shape, n)
    lab[:, :, :5] = 0
    lab[2:4, 3:6, 10:20] = 9
    hu = rng.integers(-1010, -880, size=shape).astype(np.int16)
    img, labels = torch.from_numpy(hu).to(DEV), torch.from_numpy(lab).to(DEV)
    dens = processor.densitometry(img, labels, (1.0, 1.0, 1.0), n, thresholds=(threshold,))
    for conn in (6, 26):
        _, table, _ = ops.laa_components(img, labels, threshold, n, conn)
        print(f"[t {threshold} c{conn}] voxels {table[:, 33].tolist()}, laa_counts {dens['laa_counts'][0].tolist()}")
        assert torch.equal(table[:, 33], dens["laa_counts"][0])
        assert int(table[0, 33]) > 0
        _, whole, _ = ops.laa_components(img, labels, threshold, n, conn, by_lobe=False)
        assert int(whole[1, 33]) == int(dens["whole_lung"]["laa_counts"][0]) and int(whole[0, 33]) == 0


def test_two_calls_are_bit_identical(ops):
    key, _, _, _ = reference("bernoulli_33x40x130_p30", 26)
    k = torch.from_numpy(key.copy()).to(DEV)
    a = ops.label_components(k, 26, 5, want_sizes=True)
    b = ops.label_components(k, 26, 5, want_sizes=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_laa_clusters_equals_the_yardstick(ops):
    from bodyct_dram_emph_subtype_amd import processor
    hu, lab, n = laa_case()
    spacing = (2.5, 0.7, 0.65)
    got = processor.laa_clusters(torch.from_numpy(hu.copy()).to(DEV), torch.from_numpy(lab.copy()).to(DEV), spacing, n, T, 26)
    want = CC.laa_clusters(hu, lab, spacing, n, T, 26)
    CC.assert_clusters(got, want, "by lobe")
    CC.assert_clusters({k: got["whole_lung"][k] for k in want["whole_lung"]}, want["whole_lung"], "whole lung")
    assert got["d"].is_cuda and np.array_equal(got["components"].cpu().numpy(), want["components"])
    assert processor.laa_cluster_metrics(got) == processor.laa_cluster_metrics(want)


# ------------------------------------------------------------------------------------------------ predict_case
PLAIN_KEYS = {"cle_severity_score", "cle_lesion_percentage_per_lung", "pse_severity_score", "pse_lesion_percentage_per_lung"}


def test_predict_case_with_clusters(ops, monkeypatch):
    from bodyct_dram_emph_subtype_amd import models, processor, transforms as TR
    name = "blobs_u8"
    scan, lobes, spacing, _ = CR.fixture_cases()[name]
    target, n = (16, 32, 32), 5
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    kw = dict(uid=name, region_names=names)
    calls = []
    real = ops.laa_components

    def spy(*a, **k):
        calls.append((a[2:], k))
        return real(*a, **k)

    monkeypatch.setattr(ops, "laa_components", spy)
    run = lambda **sw: processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, **sw, **kw)
    e_plain = run()
    e_off = run(clusters=False, cluster_kw={"threshold": -900})
    assert calls == []                                                          # off: the kernel is never reached
    assert set(e_plain) == {"entity", "metrics", "error_messages", "full_cle", "full_pse"}
    assert set(e_plain["metrics"]) == PLAIN_KEYS and e_off["metrics"] == e_plain["metrics"]
    assert e_off["error_messages"] == e_plain["error_messages"] == []
    e_clu = run(clusters=True)
    assert len(calls) == 2 and calls[0][1] == {"by_lobe": True} and calls[1][1] == {"by_lobe": False}
    assert set(e_clu["metrics"]) - set(e_plain["metrics"]) == CC.CLUSTER_KEYS and set(e_clu) == set(e_plain)
    for k in ("full_cle", "full_pse"):
        assert torch.equal(e_clu[k], e_plain[k]) and torch.equal(e_off[k], e_plain[k]), k
    assert {k: e_clu["metrics"][k] for k in PLAIN_KEYS} == e_plain["metrics"]

    # the metrics: laa_cluster_metrics of the yardstick on the crop
    case = TR.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid=name, want_lobes=True)
    idx = tuple(slice(int(a_), int(b_)) for a_, b_ in case["crop_slice"].tolist())
    want = CC.laa_clusters(scan[idx].numpy(), lobes[idx].numpy(), spacing, n, -950, 6)
    want_m = processor.laa_cluster_metrics(want, names)
    print(f"[{name}] {want_m}")
    assert set(want_m) == CC.CLUSTER_KEYS and {k: e_clu["metrics"][k] for k in CC.CLUSTER_KEYS} == want_m
    assert int(want["clusters"][1:].min()) > 0 and e_clu["error_messages"] == []

    # other settings travel through cluster_kw; a label above n_regions is reported
    e_26 = run(clusters=True, cluster_kw={"connectivity": 26, "threshold": -910, "n_regions": 4})
    want26 = CC.laa_clusters(scan[idx].numpy(), lobes[idx].numpy(), spacing, 4, -910, 26)
    m26 = processor.laa_cluster_metrics(want26, names)
    assert {k: e_26["metrics"][k] for k in m26} == m26 and "laa910_cluster_d_per_lung" in m26
    outside = int(want26["voxels"][0])
    assert outside > 0 and len(e_26["error_messages"]) == 1 and str(outside) in e_26["error_messages"][0] and \
        "1..4" in e_26["error_messages"][0]

    # the other switches: their keys are their own, with and without the clusters
    for sw in ({"regions": True}, {"densitometry": True}, {"core_peel": True, "peel_mm": 3.0},
               {"regions": True, "densitometry": True, "core_peel": True, "peel_mm": 3.0}):
        e_a, e_b = run(**sw), run(clusters=True, **sw)
        assert set(e_b["metrics"]) == set(e_a["metrics"]) | CC.CLUSTER_KEYS, sw
        assert {k: e_b["metrics"][k] for k in e_a["metrics"]} == e_a["metrics"], sw
        assert {k: e_b["metrics"][k] for k in CC.CLUSTER_KEYS} == want_m, sw
        assert e_b["error_messages"] == e_a["error_messages"], sw
        for k in ("full_cle", "full_pse"):
            assert torch.equal(e_b[k], e_plain[k]) and torch.equal(e_a[k], e_plain[k]), (sw, k)


def test_write_reports_from_a_predicted_case(ops, tmp_path):
    import json
    from bodyct_dram_emph_subtype_amd import models, processor
    scan, lobes, spacing, _ = CR.fixture_cases()["blobs_u8"]
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    e = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, (16, 32, 32), uid="u", clusters=True)
    path = str(tmp_path / "clusters.json")
    processor.write_reports([e], clusters_json=path)
    assert set(json.load(open(path))) == CC.CLUSTER_KEYS


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch(ops, monkeypatch):
    lab = torch.ones((4, 6, 70), dtype=torch.uint8, device=DEV)
    img = torch.zeros((4, 6, 70), dtype=torch.int16, device=DEV)
    L = ops._L()
    launches = []

    class Spy:
        def __getattr__(self, name):
            if name == "dram_label_components":
                return lambda *a: launches.append(name) or L.dram_label_components(*a)
            return getattr(L, name)

    monkeypatch.setattr(ops, "_L", lambda: Spy())
    with pytest.raises(ValueError, match="connectivity"):
        ops.label_components(lab, 18)
    with pytest.raises(ValueError, match="n_regions"):
        ops.label_components(lab, 6, 16)
    with pytest.raises(TypeError):
        ops.label_components(lab.to(torch.int32))
    with pytest.raises(ValueError, match="shape"):
        ops.laa_components(img[:, :, :60], lab)
    with pytest.raises(TypeError):
        ops.laa_components(img.float(), lab)
    with pytest.raises(ValueError, match="contiguous"):
        ops.laa_components(img.expand(2, 4, 6, 70)[:, :, :, ::2][0], lab[:, :, ::2])
    with pytest.raises(ValueError, match="threshold"):
        ops.laa_components(img, lab, threshold=1 << 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.label_components(lab.cpu())
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.laa_components(img.cpu(), lab)
    assert launches == []
    ops.label_components(lab)
    ops.laa_components(img, lab)
    assert launches == ["dram_label_components"] * 2
