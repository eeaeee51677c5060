"""GPU: the lung distance transform of csrc/edt.hip (dram_lung_zones through ops.lung_zones) against the int64 yardstick
of tests/edt_ref.py, and the core / peel split built on it (processor.core_peel -> predict_case(core_peel=True)).

Every distance case asserts three things: zones and zone_labels equal the yardstick EXACTLY; dist_mm is within one
float32 ulp of float32(sqrt(float64(d2)) / 1000.0) (two IEEE operations in double and one rounding to float); a second
call is bit-identical.

Shapes, from the launch rule of csrc/edt.hip (x pass: one wave per x-row in chunks of 64 voxels, 4 rows per workgroup;
y and z passes: one thread per voxel, 256 per workgroup; work volumes of uint32 up to max_um = 65535, of uint64 above):
the issue's tiny, crop-view, long-axis, ellipsoid, degenerate and tie cases, plus row lengths 63 / 64 / 65, row counts
3 / 4 / 5 and voxel counts 255 / 256 / 257, each full and capped, and max_um 65535 / 65536 on one volume.
Every case runs with torch.empty / empty_like poisoned (floats NaN, bytes 0xFF -- which is +inf in a work volume, so a
work element that is read unwritten shows as a distance that is too large); launch figures are printed before any
assertion (pytest -s)."""
import math

import numpy as np
import pytest
import torch

import case_prep_ref as CR
import densito_ref as DR
import edt_ref as ER
import regions_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -1234567891
CHUNK, ROWS_PER_WG, TPB, U32_MAX_UM = 64, 4, 256, 65535


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


def figures(ops, shape, spacing, peel_mm, max_mm):
    D, H, W = shape
    s_um, peel_um, max_um = ops.lung_zones_units(spacing, peel_mm, max_mm)
    win = [min(n - 1, max_um // s) for n, s in zip(shape, s_um)]
    ws = ops._L().dram_lung_zones_workspace(D, H, W, max_um)
    return (f"voxels {D * H * W}, x-rows {D * H} in {-(-D * H // ROWS_PER_WG)} workgroups of {-(-W // CHUNK)} chunks, "
            f"{-(-D * H * W // TPB)} workgroups in y / z, windows (z, y, x) {win}, "
            f"uint{32 if max_um <= U32_MAX_UM else 64} work volumes, {ws} B")


def check(ops, what, lab_np, lab_d, spacing, peel_mm, n=5, max_mm=None):
    print(f"[{what}] {figures(ops, lab_np.shape, spacing, peel_mm, max_mm)}")
    d2, want_z, want_zl = ER.lung_zones(lab_np, spacing, peel_mm, n, max_mm)
    lung = lab_np.astype(np.int64) > 0
    want_d = ER.dist_mm(d2, lung)
    zones, zl, dist = ops.lung_zones(lab_d, spacing, peel_mm, n_regions=n, max_mm=max_mm, want_dist=True)
    assert zones.dtype == zl.dtype == torch.uint8 and dist.dtype == torch.float32
    assert tuple(zones.shape) == tuple(zl.shape) == tuple(dist.shape) == lab_np.shape
    assert zones.is_contiguous() and zl.is_contiguous() and dist.is_contiguous()
    z, l, d = zones.cpu().numpy(), zl.cpu().numpy(), dist.cpu().numpy()
    fin = np.isfinite(want_d)
    ulp = np.spacing(np.where(fin, want_d, np.float32(1.0)).astype(np.float32))
    off = np.abs(np.where(fin & np.isfinite(d), d, 0.0).astype(np.float64) - np.where(fin, want_d, 0.0).astype(np.float64))
    print(f"[{what}] peel {int((want_z == 1).sum())}, core {int((want_z == 2).sum())}, +inf {int((d2 == ER.INF).sum())}; "
          f"differing zones {int((z != want_z).sum())}, zone labels {int((l != want_zl).sum())}, "
          f"worst dist_mm error {float((off / ulp).max()):.3f} ulp")
    assert np.array_equal(z, want_z), what
    assert np.array_equal(l, want_zl), what
    assert not np.isnan(d).any() and np.array_equal(np.isinf(d), ~fin) and bool((d[~fin] > 0).all()), what
    assert bool((off <= ulp).all()), what
    assert bool((d[~lung] == 0).all()) and bool((d[lung] > 0).all()), what
    again = ops.lung_zones(lab_d, spacing, peel_mm, n_regions=n, max_mm=max_mm, want_dist=True)
    assert all(torch.equal(a, b) for a, b in zip(again, (zones, zl, dist))), f"{what}: second call"
    only = ops.lung_zones(lab_d, spacing, peel_mm, max_mm=max_mm)                # zones alone: the same zones
    assert only[1] is None and only[2] is None and torch.equal(only[0], zones), f"{what}: zones alone"
    return d2, want_z


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
    assert (lab < 0).any() and (lab == 300).any()
    d2, _ = check(ops, f"{sid} max {max_mm}", lab, torch.from_numpy(lab).to(DEV), spacing, 1.5, 5, max_mm)
    s, _, mx = ER.units(spacing, 1.5, max_mm)
    assert np.array_equal(d2, ER.brute(lab > 0, s, mx))                       # the yardstick is the definition here


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
        check(ops, f"crop view max {max_mm}", lab, view, (2.5, 0.7, 0.65), 2.0, 5, max_mm)
    tr = torch.from_numpy(lab).to(DEV).transpose(1, 2).contiguous().transpose(1, 2)   # x stride != 1: copied, not misread
    assert tr.stride(2) != 1
    want = ops.lung_zones(view, (2.5, 0.7, 0.65), 2.0, n_regions=5)
    got = ops.lung_zones(tr, (2.5, 0.7, 0.65), 2.0, n_regions=5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    lung = torch.from_numpy(lab > 0).to(DEV)                                   # bool labels: one region
    zb = ops.lung_zones(lung, (2.5, 0.7, 0.65), 2.0, n_regions=1)
    assert torch.equal(zb[0], want[0]) and torch.equal(zb[1], want[0])         # n = 1: the composite label IS the zone


# ------------------------------------------------------------------------------------------------ (c) long axes, ragged lines
LONG = [(3, 4, 1100), (3, 1100, 5), (1100, 4, 5)]
RAGGED = [(3, 1, 63), (2, 2, 64), (5, 1, 65), (1, 1, 255), (1, 4, 64), (1, 1, 257), (1, 2, 129)]


def sparse_background(shape, seed):
    """all lung (labels 1..5 in x-runs) except one background voxel near each end of the longest axis and one in the
    middle: the nearest background lies across every chunk, window and workgroup boundary"""
    rng = np.random.default_rng(seed)
    lab = np.resize(np.repeat(rng.integers(1, 6, size=64), 7), math.prod(shape)).reshape(shape).astype(np.uint8)
    axis = int(np.argmax(shape))
    n = shape[axis]
    for i in sorted({min(2, n - 1), n // 2, max(n - 3, 0)}):
        idx = [s // 2 for s in shape]
        idx[axis] = i
        lab[tuple(idx)] = 0
    return lab


@pytest.mark.parametrize("shape", LONG, ids=lambda s: "x".join(map(str, s)))
def test_one_long_axis_full_transform(ops, shape):
    lab = sparse_background(shape, seed=shape[0])
    d2, z = check(ops, f"long {shape}", lab, torch.from_numpy(lab).to(DEV), (0.5, 0.5, 0.5), 20.0, 5, math.inf)
    assert int(d2.max()) > (200 * 500) ** 2 and d2.max() != ER.INF              # hundreds of voxels away, and found
    assert (z == 1).any() and (z == 2).any()


@pytest.mark.parametrize("max_mm", [math.inf, 4.0], ids=["full", "capped"])
@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_ragged_lines(ops, shape, max_mm):
    lab = sparse_background(shape, seed=shape[2])
    check(ops, f"ragged {shape} max {max_mm}", lab, torch.from_numpy(lab).to(DEV), (0.5, 0.5, 0.5), 3.0, 5, max_mm)


def test_launch_forms_are_the_intended_ones(ops):
    L = ops._L()
    widths, rows, voxels = ({s[2] for s in RAGGED}, {s[0] * s[1] for s in RAGGED}, {math.prod(s) for s in RAGGED})
    assert {CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1} <= widths              # below, at and above the chunk of a wave
    assert {ROWS_PER_WG - 1, ROWS_PER_WG, ROWS_PER_WG + 1} <= rows             # ... the rows of a workgroup
    assert {TPB - 1, TPB, TPB + 1} <= voxels                                   # ... the voxels of a y / z workgroup
    assert all(max(s) > 16 * CHUNK for s in LONG)                              # many chunks / many workgroups per line
    up = lambda b: -(-b // 256) * 256
    for shape in RAGGED + LONG:                                                # the element type switches at 65535 um
        v = math.prod(shape)
        assert L.dram_lung_zones_workspace(*shape, U32_MAX_UM) == 2 * up(4 * v)
        assert L.dram_lung_zones_workspace(*shape, U32_MAX_UM + 1) == 2 * up(8 * v)
    assert ops.lung_zones_units((0.5, 0.5, 0.5), 3.0, 4.0)[2] <= U32_MAX_UM < ops.lung_zones_units((0.5,) * 3, 3.0, math.inf)[2]


@pytest.mark.parametrize("max_mm", [65.535, 65.536], ids=["u32", "u64"])
def test_both_sides_of_the_element_type_threshold(ops, max_mm):
    """max_um = 65535 is the last uint32 transform (65535^2 < 2^32 - 1, sums formed in 64 bits), 65536 the first uint64
    one; on 3 x 300 x 5 at 0.5 mm the far voxels lie up to 148.5 mm from the background, beyond either cap"""
    lab = sparse_background((3, 300, 5), seed=9)
    lab[1, 150, 2] = 3
    lab[1, 297, 2] = 3                                                          # background only near y = 2
    d2, _ = check(ops, f"threshold {max_mm}", lab, torch.from_numpy(lab).to(DEV), (0.5, 0.5, 0.5), 60.0, 5, max_mm)
    cap = int(round(max_mm * 1000)) ** 2
    assert (d2 == ER.INF).any() and int(d2[d2 != ER.INF].max()) > cap - 2 * 500 * 65536      # values right up to the cap


# ------------------------------------------------------------------------------------------------ (d) ellipsoid
BIG, BIG_SPACING = (64, 256, 300), (1.25, 0.7, 0.65)


def lobes_of(lung):
    """uint8 labels 1..5 in y-bands inside the lung"""
    H = lung.shape[1]
    band = (np.arange(H) * 5 // H + 1).astype(np.uint8)
    return np.where(lung, band[None, :, None], 0).astype(np.uint8)


def test_ellipsoid_every_pass_capped(ops):
    z, y, x = np.ogrid[:BIG[0], :BIG[1], :BIG[2]]
    lung = ((z - 32) / 30.0) ** 2 + ((y - 128) / 120.0) ** 2 + ((x - 150) / 140.0) ** 2 < 1
    lab = lobes_of(lung)
    _, zz = check(ops, "ellipsoid", lab, torch.from_numpy(lab).to(DEV), BIG_SPACING, 10.0, 5, 10.0)
    assert (int((zz == 1).sum()), int((zz == 2).sum())) == (935934, 1174121)


def test_lung_touching_all_six_faces(ops):
    """all lung minus an interior box: the faces of the volume are no pleura, the only peel is the rind of the box"""
    lung = np.ones(BIG, dtype=bool)
    lung[20:44, 90:170, 100:200] = False
    lab = lobes_of(lung)
    _, zz = check(ops, "six faces", lab, torch.from_numpy(lab).to(DEV), BIG_SPACING, 10.0, 5, 10.0)
    assert bool((zz[0] == 2).all()) and bool((zz[:, 0] == 2).all()) and bool((zz[:, :, 0] == 2).all())
    assert bool((zz[-1] == 2).all()) and bool((zz[:, -1] == 2).all()) and bool((zz[:, :, -1] == 2).all())
    assert (zz == 1).any()


# ------------------------------------------------------------------------------------------------ (e) degenerate volumes
def test_degenerate_volumes(ops):
    shape, sp = (4, 6, 70), (1.0, 0.8, 0.7)
    for max_mm in (None, math.inf):
        full = np.full(shape, 2, dtype=np.uint8)
        d2, z = check(ops, f"all lung max {max_mm}", full, torch.from_numpy(full).to(DEV), sp, 3.0, 5, max_mm)
        assert bool((z == 2).all()) and bool((d2 == ER.INF).all())             # dist_mm all +inf: checked against d2
        none = np.zeros(shape, dtype=np.uint8)
        _, z = check(ops, f"no lung max {max_mm}", none, torch.from_numpy(none).to(DEV), sp, 3.0, 5, max_mm)
        assert bool((z == 0).all())
        one = full.copy()
        one[2, 3, 40] = 0
        d2, _ = check(ops, f"one background voxel max {max_mm}", one, torch.from_numpy(one).to(DEV), sp, 3.0, 5, max_mm)
        assert [int(d2[3, 3, 40]), int(d2[2, 4, 40]), int(d2[2, 3, 41])] == [1000 ** 2, 800 ** 2, 700 ** 2]
        row = full.copy()                                                      # a lung row: none in x, some in y
        row[:, 2, :] = 0
        d2, _ = check(ops, f"rows without background in x max {max_mm}", row, torch.from_numpy(row).to(DEV), sp, 3.0, 5, max_mm)
        assert int(d2[0, 3, 0]) == 800 ** 2 and int(d2[3, 0, 69]) == 1600 ** 2
        plane = full.copy()                                                    # a lung plane: none in x or y, some in z
        plane[1] = 0
        d2, _ = check(ops, f"planes without background in x, y max {max_mm}", plane, torch.from_numpy(plane).to(DEV), sp,
                      3.0, 5, max_mm)
        assert int(d2[0, 5, 69]) == 1000 ** 2 and int(d2[3, 0, 0]) == 2000 ** 2
    single = np.array([[[3]]], dtype=np.int16)                                 # one voxel, every window 0
    check(ops, "1x1x1", single, torch.from_numpy(single).to(DEV), sp, 3.0, 5, math.inf)


# ------------------------------------------------------------------------------------------------ (f) ties
def test_ties_are_peel(ops):
    lab = np.full((9, 40, 40), 1, dtype=np.uint8)
    lab[:, 0, :] = 0
    lab[4, 20, 20] = 0
    for max_mm in (None, math.inf):
        d2, z = check(ops, f"ties max {max_mm}", lab, torch.from_numpy(lab).to(DEV), (1.0, 1.0, 1.0), 5.0, 5, max_mm)
        tie = d2 == 25_000_000
        assert int(tie.sum()) == 388 and bool((z[tie] == 1).all())
        assert bool((z[d2 > 25_000_000] == 2).all()) and (d2 > 25_000_000).any()        # the next value is core
        assert (d2 == 26_000_000).any() == (max_mm is not None)                  # ... and +inf under the 5 mm cap


# ------------------------------------------------------------------------------------------------ (g) graph capture
def test_lung_zones_is_capturable(ops):
    lab = i16_labels((6, 37, 123), seed=4, p=0.9)
    lab_d = torch.from_numpy(lab).to(DEV)
    args = (lab_d, (2.5, 0.7, 0.65), 2.0)
    for max_mm in (None, math.inf):
        kw = dict(n_regions=5, max_mm=max_mm, want_dist=True)
        eager = ops.lung_zones(*args, **kw)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            ops.lung_zones(*args, **kw)                                        # warm-up on the side stream
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                captured = ops.lung_zones(*args, **kw)
        for _ in range(2):
            for t in captured:
                t.fill_(0)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(c, e) for c, e in zip(captured, eager)), max_mm


# ------------------------------------------------------------------------------------------------ (h) scan-side composition
@pytest.mark.parametrize("name", ["blobs_u8", "lobes_i16"])
def test_core_peel_of_a_prepared_case(ops, name):
    from bodyct_dram_emph_subtype_amd import processor, transforms as T
    scan, lobes, spacing, _ = CR.fixture_cases()[name]
    case = T.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid=name, want_lobes=True)
    idx = tuple(slice(int(a), int(b)) for a, b in case["crop_slice"].tolist())
    got = processor.core_peel(case["image"], case["lobe_labels"], spacing, peel_mm=3.0)
    want = ER.core_peel(scan[idx].numpy(), lobes[idx].numpy(), spacing, 3.0, 5)
    print(f"[{name}] crop {tuple(case['image'].shape)}; peel {want['peel']['voxels'].tolist()}, core "
          f"{want['core']['voxels'].tolist()}, outside {want['outside_voxels']}")
    assert all(v.is_cuda for v in (got["zones"], got["zone_labels"], got["outside_voxels"], got["peel"]["voxels"]))
    assert np.array_equal(got["zones"].cpu().numpy(), want["zones"])
    assert np.array_equal(got["zone_labels"].cpu().numpy(), want["zone_labels"])
    for zone in ("peel", "core"):
        DR.assert_matches(got[zone], want[zone], f"{name} {zone}")
    present = [r for r in range(1, 6) if bool((lobes == r).any())]
    assert present and all(want[z]["voxels"][r] > 0 for z in ("peel", "core") for r in present)     # both zones everywhere
    first = present[0]
    assert (int(want["peel"]["voxels"][first]), int(want["core"]["voxels"][first])) == \
        {"blobs_u8": (832, 320), "lobes_i16": (3440, 400)}[name]
    whole = processor.densitometry(case["image"], case["lobe_labels"], spacing)
    for k in ("voxels", "laa_counts"):
        assert torch.equal((got["peel"][k] + got["core"][k])[..., 1:], whole[k][..., 1:]), k
    assert got["outside_voxels"].dim() == 0 and got["outside_voxels"].dtype == torch.int64
    assert int(got["outside_voxels"]) == int((lobes > 5).sum()) == int(whole["voxels"][0])
    assert got["peel_mm"] == 3.0 and got["n_regions"] == 5


# ------------------------------------------------------------------------------------------------ (i) predict_case
DENS_STEMS = ("laa950_fraction", "laa910_fraction", "perc15_hu", "mean_lung_density", "volume_ml")
SCAN_KEYS = {f"{s}_per_{w}_{z}" for s in DENS_STEMS for w in ("region", "lung") for z in ("peel", "core")} | {"peel_mm"}
NET_KEYS = {f"{h}_lesion_percentage_per_{w}_{z}" for h in ("cle", "pse") for w in ("region", "lung")
            for z in ("peel", "core")} | {"region_voxels_peel", "region_voxels_core"}


@pytest.mark.parametrize("name", ["blobs_u8", "lobes_i16"])
def test_predict_case_with_core_peel(ops, name, monkeypatch):
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
    assert len(calls) == 1                                                      # one fused tail
    (a, (up_c, up_p, table)) = calls[0]
    assert a[5] == 2 * n and tuple(table.shape) == (1, 2 * n + 1, 4)
    assert set(e_cp["metrics"]) - set(e_plain["metrics"]) == SCAN_KEYS | NET_KEYS
    assert set(e_plain["metrics"]) <= set(e_cp["metrics"]) and set(e_cp) == set(e_plain)
    for k in ("full_cle", "full_pse"):
        assert torch.equal(e_cp[k], e_plain[k]), k

    # scan side: core_peel_metrics of the yardstick on the crop
    case = T.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid=name, want_lobes=True)
    idx = tuple(slice(int(a_), int(b_)) for a_, b_ in case["crop_slice"].tolist())
    want = ER.core_peel(scan[idx].numpy(), lobes[idx].numpy(), spacing, 3.0, n)
    want_scan = processor.core_peel_metrics(dict(want, peel_mm=3.0), names)
    assert set(want_scan) == SCAN_KEYS and {k: e_cp["metrics"][k] for k in SCAN_KEYS} == want_scan

    # network side: counts against the resized composite labels, sums against the fp64 sums of the stored volumes
    lab = RR.resize_labels(torch.from_numpy(want["zone_labels"]), target)[None]
    assert torch.equal(a[3].cpu(), lab)
    ess = a[2].cpu()
    t = table.cpu()
    mine = RR.table64(up_c.cpu(), up_p.cpu(), ess, lab, 2 * n)
    mag = RR.table64(up_c.cpu().abs(), up_p.cpu().abs(), ess, lab, 2 * n)
    vps = math.prod(target)
    kappa = -(-vps // (ops._L().dram_region_nblk(vps) * 256)) + 9
    assert torch.equal(t[:, :, 2:], mine[:, :, 2:])
    for col, h in ((0, "cle"), (1, "pse")):
        err, bound = (t[:, :, col] - mine[:, :, col]).abs(), kappa * RR.U * mag[:, :, col]
        print(f"[{name}] composite sum {h}: worst error / (kappa={kappa} u sum|o|) "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), h
    assert {k: e_cp["metrics"][k] for k in NET_KEYS} == processor.zone_region_metrics(t[0], names)
    for i, zone in enumerate(("peel", "core")):
        counts = {names[r]: "{:d}".format(int((lab == i * n + r).sum())) for r in range(1, n + 1)}
        assert e_cp["metrics"][f"region_voxels_{zone}"] == counts, zone
    print(f"[{name}] network grid: peel {e_cp['metrics']['region_voxels_peel']}, core {e_cp['metrics']['region_voxels_core']}")
    outside = int((lobes > n).sum())
    if outside:
        assert len(e_cp["error_messages"]) == 1 and str(outside) in e_cp["error_messages"][0] and "1..5" in e_cp["error_messages"][0]
    else:
        assert e_cp["error_messages"] == []

    # with regions: still one fused tail; the folded table's counts are those of regions=True alone, sums within 1e-5
    e_reg = run(regions=True)
    t_reg = calls[-1][1][2][0].cpu()
    n_calls = len(calls)
    e_both = run(regions=True, core_peel=True, peel_mm=3.0)
    assert len(calls) == n_calls + 1
    folded = processor.fold_zone_table(calls[-1][1][2][0])
    assert tuple(folded.shape) == (n + 1, 4) and torch.equal(folded[:, 2:], t_reg[:, 2:])
    assert set(e_both["metrics"]) == set(e_reg["metrics"]) | SCAN_KEYS | NET_KEYS
    for k in ("region_voxels", "region_ess_fraction"):
        assert e_both["metrics"][k] == e_reg["metrics"][k], k
    for col in (0, 1):
        a_, b_ = folded[:, col], t_reg[:, col]
        assert bool(((a_ - b_).abs() <= 1e-5 * b_.abs()).all()), col
        pa, pb = a_[1:] / folded[1:, 3], b_[1:] / t_reg[1:, 3]
        ok = (pa - pb).abs() <= 1e-5 * pb.abs()
        assert bool((ok | pb.isnan()).all()) and torch.equal(pa.isnan(), pb.isnan()), col
        la, lb = float(a_.sum()), float(b_.sum())                              # per lung: one divisor for both
        print(f"[{name}] column {col}: folded sum {la:.9g}, regions alone {lb:.9g}")
        assert abs(la - lb) <= 1e-5 * abs(lb), col
    assert e_both["error_messages"][:len(e_reg["error_messages"])] == e_reg["error_messages"]
    assert {k: e_both["metrics"][k] for k in SCAN_KEYS} == want_scan

    # with densitometry as well: its keys come from its own call, unchanged
    e_dens = run(densitometry=True)
    n_calls = len(calls)
    e_all = run(densitometry=True, core_peel=True, peel_mm=3.0)
    assert len(calls) == n_calls + 1
    dens_keys = set(e_dens["metrics"]) - set(e_plain["metrics"])
    assert len(dens_keys) == 10 and {k: e_all["metrics"][k] for k in dens_keys} == {k: e_dens["metrics"][k] for k in dens_keys}
    assert set(e_all["metrics"]) == set(e_dens["metrics"]) | SCAN_KEYS | NET_KEYS
    for e in (e_both, e_all):
        for k in ("full_cle", "full_pse"):
            assert torch.equal(e[k], e_plain[k]), k


def test_write_reports_from_a_predicted_case(ops, tmp_path):
    import json
    from bodyct_dram_emph_subtype_amd import models, processor
    scan, lobes, spacing, _ = CR.fixture_cases()["blobs_u8"]
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    e = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, (16, 32, 32), uid="u", core_peel=True, peel_mm=3.0)
    path = str(tmp_path / "core_peel.json")
    processor.write_reports([e], core_peel_json=path)
    assert set(json.load(open(path))) == SCAN_KEYS | NET_KEYS


# ------------------------------------------------------------------------------------------------ (j) refusals
def test_refusals_come_before_any_launch(ops, monkeypatch):
    from bodyct_dram_emph_subtype_amd import processor
    lab = torch.ones((4, 6, 70), dtype=torch.uint8, device=DEV)
    img = torch.zeros((4, 6, 70), dtype=torch.int16, device=DEV)
    sp = (1.0, 0.8, 0.7)
    L = ops._L()
    launches = []

    class Spy:
        def __getattr__(self, name):
            if name == "dram_lung_zones":
                return lambda *a: launches.append(name) or L.dram_lung_zones(*a)
            return getattr(L, name)

    monkeypatch.setattr(ops, "_L", lambda: Spy())
    with pytest.raises(ValueError, match="n_regions"):
        ops.lung_zones(lab, sp, 3.0, n_regions=8)
    with pytest.raises(ValueError, match="max_mm"):
        ops.lung_zones(lab, sp, 3.0, max_mm=2.5)
    with pytest.raises(ValueError, match="spacing"):
        ops.lung_zones(lab, (1.0, 0.0, 0.7), 3.0)
    with pytest.raises(ValueError, match="2\\^25"):
        ops.lung_zones(torch.ones((1, 1, 1680), dtype=torch.uint8, device=DEV), (1.0, 1.0, 20.0), 3.0)
    with pytest.raises(TypeError):
        ops.lung_zones(lab.to(torch.int32), sp, 3.0)
    with pytest.raises(ValueError, match="shape"):
        processor.core_peel(img[:, :, :60], lab, sp, 3.0)
    with pytest.raises(ValueError, match="n_regions"):
        processor.core_peel(img, lab, sp, 3.0, n_regions=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lung_zones(lab.cpu(), sp, 3.0)
    assert launches == []
    ops.lung_zones(lab, sp, 3.0)
    assert launches == ["dram_lung_zones"]
