"""GPU: the lobe-to-lobe distance map of csrc/edt.hip (dram_lobe_zones through ops.lobe_zones) against the int64 yardstick
of tests/fissure_ref.py (one binary transform per class), and the three-zone split built on it
(processor.core_peel(fissure_mm=...) -> predict_case(core_peel=True, fissure_mm=...)).

Every distance case asserts: zones and zone_labels equal the yardstick EXACTLY; both distance volumes are within one
float32 ulp of float32(sqrt(float64(x)) / 1000.0) (two IEEE operations in double and one rounding to float: the bound of
INTEGRATION.md B7 that tests/test_core_peel_gpu.py asserts); a second call is bit-identical; zones == 1 is
ops.lung_zones' peel and zones 2 | 3 its core on the same input (and pleura_mm its dist_mm, bit for bit, at the same
cap); the call without the distance volumes -- which skips the fissural search inside the peel -- gives the same zones.

Shapes, from the launch rule of csrc/edt.hip: the pleural x pass runs one wave per x-row in chunks of 64 voxels, 4 rows
per workgroup; every other pass, the three of the pairs included, one thread per voxel, 256 per workgroup; the pleural
work volumes are uint32 up to max_um = 65535 and uint64 above, the pair volumes always 16 bytes per voxel.  So: row
lengths 63 / 64 / 65, row counts 3 / 4 / 5, voxel counts 255 / 256 / 257, each full and capped; one long axis per pass;
max_um 65535 / 65536 on one volume.  Every case runs with torch.empty / empty_like poisoned (floats NaN, bytes 0xFF --
+inf in either kind of work volume, so a work element that is read unwritten shows as a distance that is too large);
launch figures are printed before any assertion (pytest -s)."""
import json
import math

import numpy as np
import pytest
import torch

import case_prep_ref as CR
import densito_ref as DR
import edt_ref as ER
import fissure_ref as FR
import regions_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -1234567891
CHUNK, ROWS_PER_WG, TPB, U32_MAX_UM, PAIR_BYTES = 64, 4, 256, 65535, 16


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    e0, el0 = torch.empty, torch.empty_like

    def fill(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(255)
        elif t.dtype in (torch.int32, torch.int64):
            t.fill_(POISON)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(e0(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(el0(*a, **k)))
    yield
    torch.cuda.synchronize()


def figures(ops, shape, spacing, peel_mm, fissure_mm, max_mm):
    D, H, W = shape
    s_um, _, _, max_um = ops.lobe_zones_units(spacing, peel_mm, fissure_mm, max_mm)
    win = [min(n - 1, max_um // s) for n, s in zip(shape, s_um)]
    ws = ops._L().dram_lobe_zones_workspace(D, H, W, max_um)
    return (f"voxels {D * H * W}, pleural x-rows {D * H} in {-(-D * H // ROWS_PER_WG)} workgroups of {-(-W // CHUNK)} "
            f"chunks, {-(-D * H * W // TPB)} workgroups in every other pass, windows (z, y, x) {win}, "
            f"uint{32 if max_um <= U32_MAX_UM else 64} pleural and {PAIR_BYTES}-byte pair work volumes, {ws} B")


def assert_dist(got, want, lung, what):
    """within one float32 ulp of the yardstick's float32; +inf in the same places; 0 exactly outside the lung"""
    fin = np.isfinite(want)
    ulp = np.spacing(np.where(fin, want, np.float32(1.0)).astype(np.float32))
    off = np.abs(np.where(fin & np.isfinite(got), got, 0.0).astype(np.float64) - np.where(fin, want, 0.0).astype(np.float64))
    worst = float((off / ulp).max())
    assert not np.isnan(got).any() and np.array_equal(np.isinf(got), ~fin) and bool((got[~fin] > 0).all()), what
    assert bool((off <= ulp).all()), (what, worst)
    assert bool((got[~lung] == 0).all()) and bool((got[lung] > 0).all()), what
    return worst


def check(ops, what, lab_np, lab_d, spacing, peel_mm, fissure_mm, n=5, max_mm=None):
    print(f"[{what}] {figures(ops, lab_np.shape, spacing, peel_mm, fissure_mm, max_mm)}")
    want = FR.lobe_zones(lab_np, spacing, peel_mm, fissure_mm, n, max_mm)
    lung = lab_np.astype(np.int64) > 0
    kw = dict(n_regions=n, max_mm=max_mm)
    out = ops.lobe_zones(lab_d, spacing, peel_mm, fissure_mm, want_dist=True, **kw)
    zones, zl, pleura, fissure = out
    assert zones.dtype == zl.dtype == torch.uint8 and pleura.dtype == fissure.dtype == torch.float32
    assert all(tuple(t.shape) == lab_np.shape and t.is_contiguous() for t in out)
    z, l, p, f = (t.cpu().numpy() for t in out)
    wz = want["zones"]
    print(f"[{what}] peel {int((wz == 1).sum())}, core {int((wz == 2).sum())}, fissural rind {int((wz == 3).sum())}, "
          f"d2 +inf {int((want['d2'] == FR.INF).sum())}, f2 +inf {int((want['f2'] == FR.INF).sum())}; "
          f"differing zones {int((z != wz).sum())}, zone labels {int((l != want['zone_labels']).sum())}")
    assert np.array_equal(z, wz), what
    assert np.array_equal(l, want["zone_labels"]), what
    worst = [assert_dist(p, want["pleura_mm"], lung, f"{what}: pleura_mm"),
             assert_dist(f, want["fissure_mm"], lung, f"{what}: fissure_mm")]
    print(f"[{what}] worst error: pleura_mm {worst[0]:.3f} ulp, fissure_mm {worst[1]:.3f} ulp")
    again = ops.lobe_zones(lab_d, spacing, peel_mm, fissure_mm, want_dist=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, out)), f"{what}: second call"
    only = ops.lobe_zones(lab_d, spacing, peel_mm, fissure_mm, **kw)             # no distance volumes: the same zones
    assert only[2] is None and only[3] is None and torch.equal(only[0], zones) and torch.equal(only[1], zl), f"{what}: zones alone"
    cap = max(peel_mm, fissure_mm) if max_mm is None else max_mm                 # lung_zones at the same cap
    lz = ops.lung_zones(lab_d, spacing, peel_mm, max_mm=cap, want_dist=True)
    assert torch.equal(zones == 1, lz[0] == 1), f"{what}: the peel is lung_zones' peel"
    assert torch.equal((zones == 2) | (zones == 3), lz[0] == 2), f"{what}: core and rind are lung_zones' core"
    assert torch.equal(pleura, lz[2]), f"{what}: pleura_mm is lung_zones' dist_mm"
    return want


def i16_labels(shape, seed, n=5, p=0.8):
    """random 80 % lung: labels 1..n, with 300 and n + 1 (lung in no region) and negatives (not lung) sprinkled in"""
    rng = np.random.default_rng(seed)
    lab = np.where(rng.random(shape) < p, rng.integers(1, n + 1, size=shape), 0).astype(np.int16)
    flat = lab.reshape(-1)
    pos = rng.choice(flat.size, size=max(6, flat.size // 40), replace=False)
    flat[pos] = np.resize(np.array([300, -1, -32768, n + 1, 32767, -7], dtype=np.int16), pos.size)
    return lab


# ------------------------------------------------------------------------------------------------ (a) tiny shapes
TINY = {"5x7x11": ((5, 7, 11), (2.5, 0.7, 0.65)), "6x9x13": ((6, 9, 13), (0.8, 1.4, 0.6))}


@pytest.mark.parametrize("max_mm", [math.inf, 1.5], ids=["full", "capped"])
@pytest.mark.parametrize("sid", sorted(TINY))
def test_tiny_shapes(ops, sid, max_mm):
    shape, spacing = TINY[sid]
    lab = i16_labels(shape, seed=shape[1])
    assert (lab < 0).any() and (lab == 300).any() and (lab == 6).any()
    want = check(ops, f"{sid} max {max_mm}", lab, torch.from_numpy(lab).to(DEV), spacing, 1.5, 1.2, 5, max_mm)
    s, _, _, mx = FR.units(spacing, 1.5, 1.2, max_mm)
    assert np.array_equal(want["f2"], FR.brute(lab, s, 5, mx))                  # the yardstick is the definition here
    assert np.array_equal(want["d2"], ER.brute(lab > 0, s, mx))
    for n in (1, 3):                                                            # fewer regions: 2..5 / 4, 5 are no sites
        w = check(ops, f"{sid} max {max_mm} n={n}", lab, torch.from_numpy(lab).to(DEV), spacing, 1.5, 1.2, n, max_mm)
        assert np.array_equal(w["f2"], FR.brute(lab, s, n, mx))


# ------------------------------------------------------------------------------------------------ (b) crop view
def test_crop_view_is_read_through_its_strides(ops):
    shape, off = (6, 37, 123), (1, 2, 3)
    rng = np.random.default_rng(5)
    lab = np.where(rng.random(shape) < 0.9, rng.integers(1, 6, size=shape), 0).astype(np.uint8)
    lab[2, 10, 40:44] = [6, 200, 255, 6]
    big = torch.full(tuple(s + o for s, o in zip(shape, off)), 3, dtype=torch.uint8)   # a foreign lung label around it
    big[off[0]:, off[1]:, off[2]:] = torch.from_numpy(lab)
    view = big.to(DEV)[off[0]:, off[1]:, off[2]:]
    assert not view.is_contiguous() and view.stride(2) == 1 and view.storage_offset() % 2 == 1
    assert view.stride(1) > shape[2] and view.stride(0) > shape[1] * view.stride(1)
    for max_mm in (None, math.inf):
        check(ops, f"crop view max {max_mm}", lab, view, (2.5, 0.7, 0.65), 2.0, 1.5, 5, max_mm)
    tr = torch.from_numpy(lab).to(DEV).transpose(1, 2).contiguous().transpose(1, 2)   # x stride != 1: copied, not misread
    assert tr.stride(2) != 1
    want = ops.lobe_zones(view, (2.5, 0.7, 0.65), 2.0, 1.5, want_dist=True)
    got = ops.lobe_zones(tr, (2.5, 0.7, 0.65), 2.0, 1.5, want_dist=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------ (c) long axes, ragged lines
LONG = [(3, 4, 1100), (3, 1100, 5), (1100, 4, 5)]
RAGGED = [(3, 1, 63), (2, 2, 64), (5, 1, 65), (1, 1, 255), (1, 4, 64), (1, 1, 257), (1, 2, 129)]


def runs_of_lobes(shape, seed):
    """labels 1..5 in x-runs of 7 (tied distances to several classes), one background voxel near each end of the longest
    axis and one in the middle"""
    rng = np.random.default_rng(seed)
    lab = np.resize(np.repeat(rng.integers(1, 6, size=64), 7), math.prod(shape)).reshape(shape).astype(np.uint8)
    axis = int(np.argmax(shape))
    n = shape[axis]
    for i in sorted({min(2, n - 1), n // 2, max(n - 3, 0)}):
        idx = [s // 2 for s in shape]
        idx[axis] = i
        lab[tuple(idx)] = 0
    return lab


def far_sites(shape):
    """all one class except one voxel of a second class near each end of the long axis and one in its middle: the nearest
    foreign site lies across every chunk, window and workgroup boundary"""
    lab = np.full(shape, 1, dtype=np.uint8)
    axis = int(np.argmax(shape))
    n = shape[axis]
    for i in (2, n // 2, n - 3):
        idx = [s // 2 for s in shape]
        idx[axis] = i
        lab[tuple(idx)] = 2
    return lab


@pytest.mark.parametrize("shape", LONG, ids=lambda s: "x".join(map(str, s)))
def test_one_long_axis_full_transform(ops, shape):
    lab = far_sites(shape)
    want = check(ops, f"long {shape}", lab, torch.from_numpy(lab).to(DEV), (0.5, 0.5, 0.5), 20.0, 20.0, 5, math.inf)
    f2 = want["f2"]
    assert not (f2 == FR.INF).any() and int(f2.max()) > (200 * 500) ** 2        # hundreds of voxels away, and found
    assert (want["zones"] == 3).any() and (want["zones"] == 2).any() and not (want["zones"] == 1).any()


@pytest.mark.parametrize("max_mm", [math.inf, 4.0], ids=["full", "capped"])
@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_ragged_lines(ops, shape, max_mm):
    lab = runs_of_lobes(shape, seed=shape[2])
    check(ops, f"ragged {shape} max {max_mm}", lab, torch.from_numpy(lab).to(DEV), (0.5, 0.5, 0.5), 3.0, 2.0, 5, max_mm)


def test_launch_forms_are_the_intended_ones(ops):
    L = ops._L()
    widths, rows, voxels = ({s[2] for s in RAGGED}, {s[0] * s[1] for s in RAGGED}, {math.prod(s) for s in RAGGED})
    assert {CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1} <= widths              # below, at and above the chunk of a wave
    assert {ROWS_PER_WG - 1, ROWS_PER_WG, ROWS_PER_WG + 1} <= rows             # ... the rows of a workgroup
    assert {TPB - 1, TPB, TPB + 1} <= voxels                                   # ... the voxels of a workgroup
    assert all(max(s) > 4 * TPB and max(s) > 16 * CHUNK for s in LONG)         # many workgroups / chunks per line
    up = lambda b: -(-b // 256) * 256
    for shape in RAGGED + LONG:              # the pleural element switches at 65535 um, the pairs never do
        v = math.prod(shape)
        assert L.dram_lobe_zones_workspace(*shape, U32_MAX_UM) == 2 * up(4 * v) + 2 * up(PAIR_BYTES * v)
        assert L.dram_lobe_zones_workspace(*shape, U32_MAX_UM + 1) == 2 * up(8 * v) + 2 * up(PAIR_BYTES * v)
    assert ops.lobe_zones_units((0.5,) * 3, 3.0, 2.0, 4.0)[3] <= U32_MAX_UM < ops.lobe_zones_units((0.5,) * 3, 3.0, 2.0, math.inf)[3]


@pytest.mark.parametrize("max_mm", [65.535, 65.536], ids=["u32", "u64"])
def test_both_sides_of_the_element_type_threshold(ops, max_mm):
    """max_um = 65535 is the last transform with uint32 pleural volumes, 65536 the first with uint64 ones; on 3 x 300 x 5
    at 0.5 mm background and the second lobe lie near y = 2 only, so the far voxels are up to 148.5 mm from either,
    beyond the cap"""
    lab = np.full((3, 300, 5), 1, dtype=np.uint8)
    lab[1, 2, 2] = 0
    lab[1, 3, 3] = 2
    want = check(ops, f"threshold {max_mm}", lab, torch.from_numpy(lab).to(DEV), (0.5, 0.5, 0.5), 60.0, 60.0, 5, max_mm)
    cap = int(round(max_mm * 1000)) ** 2
    for k in ("d2", "f2"):
        v = want[k]
        assert (v == FR.INF).any() and int(v[v != FR.INF].max()) > cap - 2 * 500 * 65536, k     # values right up to the cap


# ------------------------------------------------------------------------------------------------ (d) ellipsoid
BIG, BIG_SPACING = (32, 128, 150), (1.25, 0.7, 0.65)


def lobes_of(lung):
    """uint8 labels 1..5 in y-bands inside the lung"""
    H = lung.shape[1]
    band = (np.arange(H) * 5 // H + 1).astype(np.uint8)
    return np.where(lung, band[None, :, None], 0).astype(np.uint8)


def test_ellipsoid_every_pass_capped(ops):
    z, y, x = np.ogrid[:BIG[0], :BIG[1], :BIG[2]]
    lung = ((z - 16) / 15.0) ** 2 + ((y - 64) / 60.0) ** 2 + ((x - 75) / 70.0) ** 2 < 1
    lab = lobes_of(lung)
    s_um, _, _, max_um = ops.lobe_zones_units(BIG_SPACING, 10.0, 4.0, 10.0)
    assert all(max_um // s < n - 1 for s, n in zip(s_um, BIG))                  # every window is the cap's, not the axis'
    zz = check(ops, "ellipsoid", lab, torch.from_numpy(lab).to(DEV), BIG_SPACING, 10.0, 4.0, 5, 10.0)["zones"]
    assert [int((zz == k).sum()) for k in (1, 2, 3)] == [199452, 38829, 25024]


# ------------------------------------------------------------------------------------------------ (e) special volumes
def test_ties_are_rind_and_the_peel_wins(ops):
    """two lobes meeting at the plane y = 12 (and one voxel of lobe 2 inside lobe 1: 3-4-5 triangles), isotropic 1 mm,
    background only at x = 0; peel_mm = fissure_mm = 5"""
    lab = np.full((9, 24, 24), 1, dtype=np.uint8)
    lab[:, 12:, :] = 2
    lab[4, 3, 12] = 2
    lab[:, :, 0] = 0
    for max_mm in (None, math.inf):
        w = check(ops, f"ties max {max_mm}", lab, torch.from_numpy(lab).to(DEV), (1.0, 1.0, 1.0), 5.0, 5.0, 5, max_mm)
        d2, f2, z = w["d2"], w["f2"], w["zones"]
        tie = (f2 == 25_000_000) & (lab > 0)
        assert int(tie.sum()) == 407 and int((tie & (z == 3)).sum()) == 317 and int((tie & (z == 1)).sum()) == 90
        assert bool((z[tie & (d2 > 25_000_000)] == 3).all())                     # exactly 5 mm from the other lobe: rind
        assert bool((z[(f2 > 25_000_000) & (d2 > 25_000_000)] == 2).all()) and ((f2 > 25_000_000) & (d2 > 25_000_000)).any()
        both = (f2 <= 25_000_000) & (d2 <= 25_000_000) & (lab > 0)               # within both widths: the peel wins
        assert int(both.sum()) == 450 and bool((z[both] == 1).all())
        assert (f2 == 26_000_000).any() == (max_mm is not None)                  # the next distance is core; +inf under the cap
        assert int(f2[0, 7, 20]) == 25_000_000 and int(z[0, 7, 20]) == 3 and int(z[0, 6, 20]) == 2


def test_one_class_only(ops):
    lab = np.full((4, 6, 70), 2, dtype=np.uint8)
    lab[2, 3, 40] = 0
    lab[0, 0, :5] = 0
    for max_mm in (None, math.inf):
        w = check(ops, f"one class max {max_mm}", lab, torch.from_numpy(lab).to(DEV), (1.0, 0.8, 0.7), 3.0, 3.0, 5, max_mm)
        assert bool((w["f2"][lab > 0] == FR.INF).all()) and not (w["zones"] == 3).any()
        assert (w["zones"] == 1).any() and (w["zones"] == 2).any()
        assert bool(np.isinf(w["fissure_mm"][lab > 0]).all())


def test_label_above_n_beside_a_lobe(ops):
    """a lung label above n is no site: the lobe beside it has no fissural rind there; its own voxels have an f2 (to the
    lobe) and the composite label 255 whatever their zone"""
    lab = np.full((4, 12, 70), 1, dtype=np.int16)
    lab[:, 6:, :] = 6
    lab[:, 9:, :] = 300
    lab[0, 0, 0] = -5
    for n in (5, 1):
        w = check(ops, f"label above n, n={n}", lab, torch.from_numpy(lab).to(DEV), (1.0, 0.8, 0.7), 2.0, 2.0, n, math.inf)
        lobe, above = lab == 1, lab > n
        assert bool((w["f2"][lobe] == FR.INF).all()) and not (w["zones"][lobe] == 3).any()
        assert bool((w["zone_labels"][above] == 255).all()) and bool((w["f2"][above] != FR.INF).all())
        assert int(w["f2"][2, 6, 30]) == 800 ** 2 and int(w["f2"][2, 9, 30]) == (4 * 800) ** 2
        assert (w["zones"][above] == 3).any() and (w["zones"][above] == 2).any()
    lab2 = np.where(lab == 6, 2, lab)                                          # the same wall as a lobe: now it is a fissure
    w = check(ops, "a lobe in its place", lab2, torch.from_numpy(lab2).to(DEV), (1.0, 0.8, 0.7), 2.0, 2.0, 5, math.inf)
    assert int(w["f2"][2, 5, 30]) == 800 ** 2 and int(w["zones"][2, 5, 30]) == 3 and int(w["zone_labels"][2, 5, 30]) == 11


def test_degenerate_volumes(ops):
    shape, sp = (4, 6, 70), (1.0, 0.8, 0.7)
    rng = np.random.default_rng(2)
    lung = rng.random(shape) < 0.85
    w = check(ops, "bool labels", lung.astype(np.uint8), torch.from_numpy(lung).to(DEV), sp, 2.0, 2.0, 1, None)
    assert not (w["zones"] == 3).any() and np.array_equal(w["zone_labels"], w["zones"])   # n = 1: the label IS the zone
    for max_mm in (None, math.inf):
        none = np.zeros(shape, dtype=np.uint8)
        w = check(ops, f"no lung max {max_mm}", none, torch.from_numpy(none).to(DEV), sp, 3.0, 2.0, 5, max_mm)
        assert bool((w["zones"] == 0).all())
        full = np.full(shape, 2, dtype=np.uint8)
        w = check(ops, f"one lobe, no background max {max_mm}", full, torch.from_numpy(full).to(DEV), sp, 3.0, 2.0, 5, max_mm)
        assert bool((w["zones"] == 2).all()) and bool((w["d2"] == FR.INF).all()) and bool((w["f2"] == FR.INF).all())
        two = full.copy()                                                      # two lobes, no background: rind and core only
        two[:, :, 35:] = 4
        w = check(ops, f"two lobes, no background max {max_mm}", two, torch.from_numpy(two).to(DEV), sp, 3.0, 2.0, 5, max_mm)
        assert int(w["f2"][1, 1, 34]) == 700 ** 2 == int(w["f2"][1, 1, 35])
        assert int(w["f2"][3, 5, 0]) == (FR.INF if max_mm is None else (35 * 700) ** 2)      # 24.5 mm: beyond the 3 mm cap
        assert set(np.unique(w["zones"]).tolist()) == {2, 3} and int((w["zones"] == 3).sum()) == 4 * 6 * 4
    single = np.array([[[3]]], dtype=np.int16)                                 # one voxel, every window 0
    w = check(ops, "1x1x1", single, torch.from_numpy(single).to(DEV), sp, 3.0, 2.0, 5, math.inf)
    assert w["zones"].tolist() == [[[2]]] and w["zone_labels"].tolist() == [[[8]]]


def test_a_rind_below_every_spacing_is_empty(ops):
    lab = lobes_of(np.ones((4, 20, 70), dtype=bool))
    lab[:, :, 0] = 0
    for max_mm in (None, math.inf):
        w = check(ops, f"thin rind max {max_mm}", lab, torch.from_numpy(lab).to(DEV), (1.0, 0.8, 0.7), 2.0, 0.65, 5, max_mm)
        assert not (w["zones"] == 3).any() and (w["zones"] == 2).any() and (w["zones"] == 1).any()
        assert int(w["f2"][lab > 0].min()) == 800 ** 2                           # the lobes do touch


# ------------------------------------------------------------------------------------------------ (f) graph capture
def test_lobe_zones_is_capturable(ops):
    lab = i16_labels((6, 37, 123), seed=4, p=0.9)
    lab_d = torch.from_numpy(lab).to(DEV)
    args = (lab_d, (2.5, 0.7, 0.65), 2.0, 1.5)
    for max_mm in (None, math.inf):
        kw = dict(n_regions=5, max_mm=max_mm, want_dist=True)
        eager = ops.lobe_zones(*args, **kw)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            ops.lobe_zones(*args, **kw)                                        # warm-up on the side stream
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                captured = ops.lobe_zones(*args, **kw)
        for _ in range(2):
            for t in captured:
                t.fill_(0)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(c, e) for c, e in zip(captured, eager)), max_mm


# ------------------------------------------------------------------------------------------------ (g) scan-side composition
ZONES3 = ("peel", "core", "fissure")
PINNED = {"blobs_u8": {"peel": [0, 832, 1312, 720, 1792, 1520], "core": [0, 128, 336, 64, 640, 480],
                       "fissure": [0, 192, 112, 176, 160, 160]},
          "lobes_i16": {"peel": [0, 0, 0, 0, 3440, 0], "core": [0, 0, 0, 0, 400, 0], "fissure": [0, 0, 0, 0, 0, 0]}}


def same(a, b):
    """tensor for tensor (NaN equal to NaN), through the nested dicts of a densitometry result"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        if a.dtype != b.dtype or a.shape != b.shape:
            return False
        return torch.equal(a.nan_to_num(nan=12345.0), b.nan_to_num(nan=12345.0)) if a.is_floating_point() else torch.equal(a, b)
    return a == b


@pytest.mark.parametrize("name", ["blobs_u8", "lobes_i16"])
def test_three_zones_of_a_prepared_case(ops, name):
    """blobs_u8: lobes 2 | 1, 3 meet at a z plane, 1 | 3 at a y plane, 4 | 5 at a z plane, so every lobe has all three
    zones; lobes_i16: the two boxes do not touch and one of them is label 300, so the rind is empty"""
    from bodyct_dram_emph_subtype_amd import processor, transforms as T
    scan, lobes, spacing, _ = CR.fixture_cases()[name]
    case = T.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid=name, want_lobes=True)
    idx = tuple(slice(int(a), int(b)) for a, b in case["crop_slice"].tolist())
    got = processor.core_peel(case["image"], case["lobe_labels"], spacing, peel_mm=3.0, fissure_mm=3.0)
    want = FR.core_peel(scan[idx].numpy(), lobes[idx].numpy(), spacing, 3.0, 3.0, 5)
    print(f"[{name}] crop {tuple(case['image'].shape)}; " + ", ".join(f"{z} {want[z]['voxels'].tolist()}" for z in ZONES3)
          + f", outside {want['outside_voxels']}")
    assert all(v.is_cuda for v in (got["zones"], got["zone_labels"], got["outside_voxels"], got["fissure"]["voxels"]))
    assert np.array_equal(got["zones"].cpu().numpy(), want["zones"])
    assert np.array_equal(got["zone_labels"].cpu().numpy(), want["zone_labels"])
    for zone in ZONES3:
        DR.assert_matches(got[zone], want[zone], f"{name} {zone}")
    assert {z: want[z]["voxels"].tolist() for z in ZONES3} == PINNED[name]
    if name == "blobs_u8":
        assert all(want[z]["voxels"][r] > 0 for z in ZONES3 for r in range(1, 6))           # all three zones in every lobe
    whole = processor.densitometry(case["image"], case["lobe_labels"], spacing)
    for k in ("voxels", "laa_counts"):
        assert torch.equal(sum(got[z][k] for z in ZONES3)[..., 1:], whole[k][..., 1:]), k
    two = processor.core_peel(case["image"], case["lobe_labels"], spacing, peel_mm=3.0)
    assert set(got) == set(two) | {"fissure", "fissure_mm", "zone_names"}
    assert same(got["peel"], two["peel"])                                       # 'peel' is the two-zone peel, tensor for tensor
    assert torch.equal(got["zones"] == 1, two["zones"] == 1)
    assert torch.equal((got["zones"] == 2) | (got["zones"] == 3), two["zones"] == 2)
    assert int(got["outside_voxels"]) == int((lobes > 5).sum()) == int(whole["voxels"][0])
    assert got["peel_mm"] == 3.0 and got["fissure_mm"] == 3.0 and got["n_regions"] == 5 and got["zone_names"] == ZONES3
    m = processor.core_peel_metrics(got)
    if name == "lobes_i16":                                                     # an empty rind: its metrics are None
        assert not (want["zones"] == 3).any()
        assert m["mean_lung_density_per_lung_fissure"] is None and m["laa950_fraction_per_lung_fissure"] is None
        assert all(v is None for v in m["mean_lung_density_per_region_fissure"].values())
        assert m["volume_ml_per_lung_fissure"] == "0.0" and m["mean_lung_density_per_lung_peel"] is not None


# ------------------------------------------------------------------------------------------------ (h) predict_case
DENS_STEMS = ("laa950_fraction", "laa910_fraction", "perc15_hu", "mean_lung_density", "volume_ml")
SCAN_KEYS = {f"{s}_per_{w}_{z}" for s in DENS_STEMS for w in ("region", "lung") for z in ("peel", "core")} | {"peel_mm"}
NET_KEYS = {f"{h}_lesion_percentage_per_{w}_{z}" for h in ("cle", "pse") for w in ("region", "lung")
            for z in ("peel", "core")} | {"region_voxels_peel", "region_voxels_core"}
TWINS = {k[:-len("_core")] + "_fissure" for k in SCAN_KEYS | NET_KEYS if k.endswith("_core")} | {"fissure_mm"}


@pytest.mark.parametrize("name", ["blobs_u8", "lobes_i16"])
def test_predict_case_with_the_fissural_rind(ops, name, monkeypatch, tmp_path):
    from bodyct_dram_emph_subtype_amd import models, processor, transforms as T
    scan, lobes, spacing, _ = CR.fixture_cases()[name]
    target, n = (16, 32, 32), 5
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    kw = dict(uid=name, region_names=names)
    calls = []
    fused = ops.upproject_regions

    def spy(*a, **k):
        out = fused(*a, **k)
        calls.append((a, out))
        return out

    monkeypatch.setattr(ops, "upproject_regions", spy)
    run = lambda **sw: processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, **sw, **kw)
    e_plain = run()
    assert calls == []
    e_cp = run(core_peel=True, peel_mm=3.0)
    assert len(calls) == 1 and calls[0][0][5] == 2 * n
    assert set(e_cp["metrics"]) - set(e_plain["metrics"]) == SCAN_KEYS | NET_KEYS       # without fissure_mm: today's entry
    e_f = run(core_peel=True, peel_mm=3.0, fissure_mm=3.0)
    assert len(calls) == 2                                                      # one fused tail
    (a, (up_c, up_p, table)) = calls[1]
    assert a[5] == 3 * n and tuple(table.shape) == (1, 3 * n + 1, 4)
    assert len(TWINS) == 16 and set(e_f["metrics"]) - set(e_cp["metrics"]) == TWINS     # the _fissure twins and fissure_mm
    assert set(e_cp["metrics"]) <= set(e_f["metrics"]) and set(e_f) == set(e_plain)
    for k in ("full_cle", "full_pse"):
        assert torch.equal(e_f[k], e_plain[k]) and torch.equal(e_cp[k], e_plain[k]), k
    for k in e_plain["metrics"]:
        assert e_f["metrics"][k] == e_plain["metrics"][k], k

    # scan side: core_peel_metrics of the yardstick on the crop; the peel's numbers are those of the two-zone entry
    case = T.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid=name, want_lobes=True)
    idx = tuple(slice(int(a_), int(b_)) for a_, b_ in case["crop_slice"].tolist())
    want = FR.core_peel(scan[idx].numpy(), lobes[idx].numpy(), spacing, 3.0, 3.0, n)
    want_scan = processor.core_peel_metrics(want, names)
    scan_keys = SCAN_KEYS | {k for k in TWINS if "lesion" not in k and "region_voxels" not in k}
    assert set(want_scan) == scan_keys and {k: e_f["metrics"][k] for k in scan_keys} == want_scan
    assert all(e_f["metrics"][k] == e_cp["metrics"][k] for k in SCAN_KEYS if k.endswith("_peel") or k == "peel_mm")
    assert e_f["metrics"]["fissure_mm"] == "3.000"

    # network side: counts against the resized composite labels, sums against the fp64 sums of the stored volumes
    lab = RR.resize_labels(torch.from_numpy(want["zone_labels"]), target)[None]
    assert torch.equal(a[3].cpu(), lab)
    ess = a[2].cpu()
    t = table.cpu()
    mine = RR.table64(up_c.cpu(), up_p.cpu(), ess, lab, 3 * n)
    mag = RR.table64(up_c.cpu().abs(), up_p.cpu().abs(), ess, lab, 3 * n)
    vps = math.prod(target)
    kappa = -(-vps // (ops._L().dram_region_nblk(vps) * 256)) + 9              # the bound of tests/test_core_peel_gpu.py
    assert torch.equal(t[:, :, 2:], mine[:, :, 2:])
    for col, h in ((0, "cle"), (1, "pse")):
        err, bound = (t[:, :, col] - mine[:, :, col]).abs(), kappa * RR.U * mag[:, :, col]
        print(f"[{name}] composite sum {h}: worst error / (kappa={kappa} u sum|o|) "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), h
    net_keys = NET_KEYS | (TWINS - scan_keys)
    assert {k: e_f["metrics"][k] for k in net_keys} == processor.zone_region_metrics(t[0], names, ZONES3)
    for i, zone in enumerate(ZONES3):
        counts = {names[r]: "{:d}".format(int((lab == i * n + r).sum())) for r in range(1, n + 1)}
        assert e_f["metrics"][f"region_voxels_{zone}"] == counts, zone
    print(f"[{name}] network grid: " + ", ".join(f"{z} {e_f['metrics'][f'region_voxels_{z}']}" for z in ZONES3))
    outside = int((lobes > n).sum())
    if outside:                                                                 # the existing line, once
        assert e_f["error_messages"] == e_cp["error_messages"] and len(e_f["error_messages"]) == 1
        assert str(outside) in e_f["error_messages"][0] and "1..5" in e_f["error_messages"][0]
    else:
        assert e_f["error_messages"] == []

    # with regions: still one fused tail; the folded table's counts are those of regions=True alone, sums within 1e-5
    e_reg = run(regions=True)
    t_reg = calls[-1][1][2][0].cpu()
    n_calls = len(calls)
    e_both = run(regions=True, core_peel=True, peel_mm=3.0, fissure_mm=3.0)
    assert len(calls) == n_calls + 1 and calls[-1][0][5] == 3 * n
    folded = processor.fold_zone_table(calls[-1][1][2][0], n_zones=3)
    assert tuple(folded.shape) == (n + 1, 4) and torch.equal(folded[:, 2:], t_reg[:, 2:])
    assert set(e_both["metrics"]) == set(e_reg["metrics"]) | set(e_f["metrics"])
    for k in ("region_voxels", "region_ess_fraction"):
        assert e_both["metrics"][k] == e_reg["metrics"][k], k
    for col in (0, 1):
        a_, b_ = folded[:, col], t_reg[:, col]
        assert bool(((a_ - b_).abs() <= 1e-5 * b_.abs()).all()), col
        la, lb = float(a_.sum()), float(b_.sum())
        print(f"[{name}] column {col}: folded sum {la:.9g}, regions alone {lb:.9g}")
        assert abs(la - lb) <= 1e-5 * abs(lb), col
    assert {k: e_both["metrics"][k] for k in scan_keys} == want_scan
    for k in ("full_cle", "full_pse"):
        assert torch.equal(e_both[k], e_plain[k]), k

    # the noise filter changes the scan side only: the zones depend on the labels alone
    if name == "blobs_u8":
        e_filt = run(core_peel=True, peel_mm=3.0, fissure_mm=3.0, scan_filter=(3, 3, 3))
        assert all(e_filt["metrics"][k] == e_f["metrics"][k] for k in net_keys) and e_filt["metrics"]["scan_filter"] == "median3x3x3"
        assert e_filt["metrics"]["volume_ml_per_region_fissure"] == e_f["metrics"]["volume_ml_per_region_fissure"]
        for k in ("full_cle", "full_pse"):
            assert torch.equal(e_filt[k], e_plain[k]), k

    path = str(tmp_path / "core_peel.json")
    processor.write_reports([e_f], core_peel_json=path)
    assert set(json.load(open(path))) == SCAN_KEYS | NET_KEYS | TWINS
    processor.write_reports([e_cp], core_peel_json=path)
    assert set(json.load(open(path))) == SCAN_KEYS | NET_KEYS


# ------------------------------------------------------------------------------------------------ (i) refusals
def test_refusals_come_before_any_launch(ops, monkeypatch):
    from bodyct_dram_emph_subtype_amd import processor
    lab = torch.ones((4, 6, 70), dtype=torch.uint8, device=DEV)
    img = torch.zeros((4, 6, 70), dtype=torch.int16, device=DEV)
    sp = (1.0, 0.8, 0.7)
    L = ops._L()
    launches = []

    class Spy:
        def __getattr__(self, name):
            if name in ("dram_lobe_zones", "dram_lung_zones", "dram_lobe_hist"):
                return lambda *a: launches.append(name) or getattr(L, name)(*a)
            return getattr(L, name)

    monkeypatch.setattr(ops, "_L", lambda: Spy())
    for n in (0, 6, 7):
        with pytest.raises(ValueError, match="n_regions"):
            ops.lobe_zones(lab, sp, 3.0, 2.0, n_regions=n)
    with pytest.raises(ValueError, match="fissure_mm"):
        ops.lobe_zones(lab, sp, 3.0, 0.0)
    with pytest.raises(ValueError, match="fissure_mm"):
        ops.lobe_zones(lab, sp, 3.0, math.inf)
    with pytest.raises(ValueError, match="max_mm"):
        ops.lobe_zones(lab, sp, 3.0, 2.0, max_mm=2.5)
    with pytest.raises(ValueError, match="max_mm"):
        ops.lobe_zones(lab, sp, 2.0, 3.0, max_mm=2.5)
    with pytest.raises(ValueError, match="spacing"):
        ops.lobe_zones(lab, (1.0, 0.0, 0.7), 3.0, 2.0)
    with pytest.raises(ValueError, match="2\\^25"):
        ops.lobe_zones(torch.ones((1, 1, 1680), dtype=torch.uint8, device=DEV), (1.0, 1.0, 20.0), 3.0, 2.0)
    with pytest.raises(TypeError):
        ops.lobe_zones(lab.to(torch.int32), sp, 3.0, 2.0)
    with pytest.raises(ValueError, match="shape"):
        processor.core_peel(img[:, :, :60], lab, sp, 3.0, fissure_mm=2.0)
    with pytest.raises(ValueError, match="n_regions"):
        processor.core_peel(img, lab, sp, 3.0, n_regions=6, fissure_mm=2.0)
    with pytest.raises(ValueError, match="fissure_mm"):
        processor.core_peel(img, lab, sp, 3.0, fissure_mm=-1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lobe_zones(lab.cpu(), sp, 3.0, 2.0)
    assert launches == []
    ops.lobe_zones(lab, sp, 3.0, 2.0)
    assert launches == ["dram_lobe_zones"]
    processor.core_peel(img, lab, sp, 3.0, fissure_mm=2.0)
    assert launches == ["dram_lobe_zones", "dram_lobe_zones", "dram_lobe_hist"]
