"""GPU: the local LAA map of csrc/boxfrac.hip (dram_boxfrac3d through ops.local_fraction3d) against the numpy yardstick of
tests/local_ref.py, exactly (torch.equal) -- the packed counts, the per-mille map and the u8 bytes are each compared --
processor.local_laa against the flattened-selection statistics, and the map in the predict report
(predict_case(local_mm=...)).

Shapes.  The kernel's constants are TX = 64, TY = 16 (outputs per workgroup of the in-plane pass along x and y) and ZSEG =
64 (planes per thread of the z pass).  Besides the single voxel, W = 1 and 2, and volumes thinner than the window (D = 1,
2, 3 under rz = 3; (1,1,1) under (2,5,7)), the three shapes (ZSEG - 1, TY - 1, TX - 1), (ZSEG, TY, TX), (ZSEG + 1, TY + 1,
TX + 1) put every axis one below, at and one above its tile extent and its segment length, so that a last tile holds one
row / one column and a last segment one plane; (3, 33, 130) has three tiles along both in-plane axes.  Radii: (0,0,3),
(3,0,0), (0,2,0), (1,1,1), (2,5,7), and (16,16,16) on 34 x 34 x 35, the smallest volume whose centre box holds 33^3 =
35 937 voxels in both halves of the packed word.  The yardstick of a (shape, content, radius) is computed once."""
import functools

import numpy as np
import pytest
import torch

import case_prep_ref as CR
import local_ref as LR
import median_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TX, TY, ZSEG, RMAX = 64, 16, 64, 16          # csrc/boxfrac.hip
SHAPES = [(1, 1, 1), (1, 1, 2), (3, 5, 1), (2, 3, 2), (5, 9, 67), (3, 33, 130),
          (ZSEG - 1, TY - 1, TX - 1), (ZSEG, TY, TX), (ZSEG + 1, TY + 1, TX + 1)]
RADII = [(0, 0, 3), (3, 0, 0), (0, 2, 0), (1, 1, 1), (2, 5, 7)]
T = -950
SENTINEL = 12345


def _noise(shape, seed):
    return np.rint(np.random.default_rng(seed).normal(T, 30.0, size=shape)).astype(np.int16)


def _all_low(shape, seed):
    return np.full(shape, -1000, dtype=np.int16), np.ones(shape, dtype=np.uint8)


def _no_lung(shape, seed):
    return _noise(shape, seed), np.zeros(shape, dtype=np.uint8)


def _checker(shape, seed):
    z, y, x = np.indices(shape)
    return _noise(shape, seed), (((z + y + x) % 2) * 2).astype(np.uint8)


def _threshold_edge(shape, seed):
    """HU exactly at the threshold and one below it, side by side: only the second counts"""
    z, y, x = np.indices(shape)
    lab = np.ones(shape, dtype=np.uint8)
    lab[..., ::5] = 0
    return (T - (z + y + x) % 2).astype(np.int16), lab


def _extremes(shape, seed):
    rng = np.random.default_rng(seed)
    img = rng.choice(np.array([-32768, 32767, T, T - 1], dtype=np.int16), size=shape)
    return img, rng.choice(np.array([0, 1, 5, 6, 200, 255], dtype=np.uint8), size=shape)        # labels above n_regions too


def _int16_labels(shape, seed):
    rng = np.random.default_rng(seed)
    return _noise(shape, seed), rng.choice(np.array([-32768, -3, 0, 1, 5, 9, 300, 32767], dtype=np.int16), size=shape)


def _blob(shape, seed):
    return LR.lung_blob(shape, seed)


CONTENTS = {"all_low": _all_low, "no_lung": _no_lung, "checker": _checker, "threshold_edge": _threshold_edge,
            "extremes": _extremes, "int16_labels": _int16_labels, "blob": _blob}


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


@functools.lru_cache(maxsize=None)
def volume(shape, content):
    img, lab = CONTENTS[content](shape, 11 + len(content))
    img.setflags(write=False)
    lab.setflags(write=False)
    return img, lab


@functools.lru_cache(maxsize=None)
def reference(shape, content, radius, threshold=T):
    out = LR.fraction_map(*volume(shape, content), threshold, radius)
    for a in out:
        a.setflags(write=False)
    return out


def on_device(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def check(ops, shape, content, radius):
    """one call with every output: out into a sentinel-filled buffer, out_u8 into an offset, strided window of a larger
    zeroed volume, the counts; each against the yardstick, the inputs unchanged, nothing outside the window touched"""
    img, lab = (on_device(a) for a in volume(shape, content))
    keep = img.clone(), lab.clone()
    D, H, W = shape
    out = torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV)
    big = torch.zeros((D + 3, H + 4, W + 5), dtype=torch.uint8, device=DEV)
    window = big[1:1 + D, 3:3 + H, 2:2 + W]
    got, counts = ops.local_fraction3d(img, lab, T, radius, out=out, out_u8=window, want_counts=True)
    want_q, want_c, want_u8 = (torch.from_numpy(np.array(a)) for a in reference(shape, content, radius))
    what = (shape, content, radius)
    assert got is out and counts.dtype == torch.int32 and tuple(counts.shape) == shape and counts.is_contiguous(), what
    assert torch.equal(counts.cpu(), want_c), what
    assert torch.equal(got.cpu(), want_q), what                               # every element written, no sentinel left
    assert torch.equal(window.cpu(), want_u8), what
    outside = big.clone()
    outside[1:1 + D, 3:3 + H, 2:2 + W] = 0
    assert int(outside.sum()) == 0, what                                      # nothing outside the window is touched
    assert torch.equal(img, keep[0]) and torch.equal(lab, keep[1]), what      # the inputs are only read
    fresh = ops.local_fraction3d(img, lab, T, radius)
    assert fresh.dtype == torch.int16 and fresh.is_contiguous() and torch.equal(fresh, got), what
    # |q / 1000 - num / den| <= 0.0005 where the map is defined, in integers: |2000 num - 2 den q| <= den
    c = counts.cpu().to(torch.int64) & 0xffffffff                             # the word is unsigned: num reaches 35 937
    num, den, q = c >> 16, c & 0xffff, got.cpu().to(torch.int64)
    lung = q >= 0
    assert bool((den[lung] >= 1).all()) and bool(((2000 * num - 2 * den * q).abs()[lung] <= den[lung]).all()), what
    assert bool((num <= den).all()) and bool((q[lung] <= 1000).all()), what
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_yardstick(ops, shape):
    for content in CONTENTS:
        for radius in RADII:
            check(ops, shape, content, radius)


def test_sentinel_is_no_value_of_the_map():
    assert SENTINEL > 1000


def test_largest_box_fills_both_halves_of_the_packed_word(ops):
    shape, r = (2 * RMAX + 2, 2 * RMAX + 2, 2 * RMAX + 3), (RMAX, RMAX, RMAX)
    got = check(ops, shape, "all_low", r)
    _, want_c, _ = reference(shape, "all_low", r)
    full = (2 * RMAX + 1) ** 3
    assert full == 35937 and int((want_c.astype(np.int64) & 0xffffffff).max()) == (full << 16 | full)      # the centre boxes are whole
    assert bool((got == 1000).all())
    check(ops, shape, "blob", r)
    check(ops, shape, "checker", (RMAX, 0, RMAX))
    check(ops, (2, 40, 3), "extremes", (RMAX, RMAX, RMAX))                    # the window wider than the volume on z and x


def test_no_lung_and_all_lung(ops):
    shape = (5, 9, 67)
    img, lab = (on_device(a) for a in volume(shape, "no_lung"))
    q, counts = ops.local_fraction3d(img, lab, T, (1, 2, 3), want_counts=True)
    assert bool((q == -1).all()) and bool((counts == 0).all())
    big = torch.zeros((5, 9, 70), dtype=torch.uint8, device=DEV)
    ops.local_fraction3d(img, lab, T, (1, 2, 3), out_u8=big[:, :, 1:68])
    assert int(big.sum()) == 0
    img, lab = (on_device(a) for a in volume(shape, "all_low"))
    for threshold, value in ((-999, 1000), (-1000, 0), (32768, 1000), (-32768, 0)):   # strict; 32768 counts every HU
        q = ops.local_fraction3d(img, lab, threshold, (1, 2, 3))
        assert bool((q == value).all()), threshold
    top = torch.full(shape, 32767, dtype=torch.int16, device=DEV)
    assert bool((ops.local_fraction3d(top, lab, 32767, (0, 0, 1)) == 0).all())
    assert bool((ops.local_fraction3d(top, lab, 32768, (0, 0, 1)) == 1000).all())


def test_threshold_and_one_below_side_by_side(ops):
    img = on_device(np.array([[[T, T - 1, T, T - 1, T, T]]], dtype=np.int16))
    lab = torch.ones((1, 1, 6), dtype=torch.uint8, device=DEV)
    q, counts = ops.local_fraction3d(img, lab, T, (0, 0, 1), want_counts=True)
    assert (counts.cpu() >> 16).tolist() == [[[1, 1, 2, 1, 1, 0]]] and (counts.cpu() & 0xffff).tolist() == [[[2, 3, 3, 3, 3, 2]]]
    assert q.tolist() == [[[500, 333, 667, 333, 333, 0]]]


def test_label_views_are_read_in_place(ops):
    shape, radius = (5, 9, 67), (1, 2, 3)
    img, lab = (on_device(a) for a in volume(shape, "blob"))
    want_q, want_c, _ = (torch.from_numpy(np.array(a)) for a in reference(shape, "blob", radius))
    wide = torch.full((7, 12, 80), 3, dtype=torch.uint8, device=DEV)          # lung all around the view: it must not be read
    wide[1:6, 2:11, 5:72] = lab
    view = wide[1:6, 2:11, 5:72]
    assert not view.is_contiguous() and view.stride(2) == 1
    q, c = ops.local_fraction3d(img, view, T, radius, want_counts=True)
    assert torch.equal(q.cpu(), want_q) and torch.equal(c.cpu(), want_c)
    swapped = lab.permute(2, 1, 0).contiguous().permute(2, 1, 0)              # x stride != 1: made contiguous first
    assert swapped.stride(2) != 1 and torch.equal(ops.local_fraction3d(img, swapped, T, radius).cpu(), want_q)
    assert torch.equal(ops.local_fraction3d(img, lab > 0, T, radius).cpu(), want_q)      # bool labels
    img16, lab16 = (on_device(a) for a in volume(shape, "int16_labels"))
    wide16 = torch.full((5, 9, 70), 7, dtype=torch.int16, device=DEV)
    wide16[:, :, 2:69] = lab16
    want16 = torch.from_numpy(np.array(reference(shape, "int16_labels", radius)[0]))
    assert torch.equal(ops.local_fraction3d(img16, wide16[:, :, 2:69], T, radius).cpu(), want16)
    # an image that starts on an odd element of its storage, and a u8 window at an odd byte
    flat = torch.cat([torch.zeros(1, dtype=torch.int16, device=DEV), img.reshape(-1)])
    odd = flat[1:].view(shape)
    assert odd.data_ptr() % 4 == 2 and torch.equal(ops.local_fraction3d(odd, lab, T, radius).cpu(), want_q)


def test_two_calls_are_bit_identical(ops):
    img, lab = (on_device(a) for a in volume((ZSEG + 1, TY + 1, TX + 1), "blob"))
    for radius in ((2, 5, 7), (16, 3, 0)):
        a, ca = ops.local_fraction3d(img, lab, T, radius, want_counts=True)
        b, cb = ops.local_fraction3d(img, lab, T, radius, want_counts=True)
        assert torch.equal(a, b) and torch.equal(ca, cb)


def test_is_capturable(ops):
    shape, radius = (ZSEG + 1, TY + 1, TX + 1), (2, 5, 7)
    img, lab = (on_device(a) for a in volume(shape, "blob"))
    eager = ops.local_fraction3d(img, lab, T, radius)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.local_fraction3d(img, lab, T, radius)                             # warm-up on the side stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = ops.local_fraction3d(img, lab, T, radius)
    for _ in range(2):
        captured.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
    assert torch.equal(eager.cpu(), torch.from_numpy(np.array(reference(shape, "blob", radius)[0])))


def test_refusals_come_before_any_launch(ops, monkeypatch):
    img = torch.zeros((4, 6, 70), dtype=torch.int16, device=DEV)
    lab = torch.ones((4, 6, 70), dtype=torch.uint8, device=DEV)
    L = ops._L()
    launches = []

    class Spy:
        def __getattr__(self, name):
            if name == "dram_boxfrac3d":
                return lambda *a: launches.append(name) or L.dram_boxfrac3d(*a)
            return getattr(L, name)

    monkeypatch.setattr(ops, "_L", lambda: Spy())
    f = ops.local_fraction3d
    with pytest.raises(ValueError, match="radius"):
        f(img, lab, T, (1, 1, 17))
    with pytest.raises(ValueError, match="threshold"):
        f(img, lab, 40000, (1, 1, 1))
    with pytest.raises(TypeError):
        f(img.float(), lab)
    with pytest.raises(TypeError):
        f(img, lab.float())
    with pytest.raises(ValueError, match="share storage"):
        f(img, lab, out=img)
    with pytest.raises(ValueError, match="out must"):
        f(img, lab, out=torch.zeros((4, 6, 71), dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError, match="device"):
        f(img, lab, out=torch.zeros((4, 6, 70), dtype=torch.int16))
    with pytest.raises(ValueError, match="out_u8.*strides"):
        f(img, lab, out_u8=torch.zeros((70, 6, 4), dtype=torch.uint8, device=DEV).permute(2, 1, 0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(img.cpu(), lab.cpu())
    assert launches == []
    f(img, lab)
    assert launches == ["dram_boxfrac3d"]


# ------------------------------------------------------------------------------------------------ the statistics
def test_local_laa_equals_the_flattened_selection(ops):
    from bodyct_dram_emph_subtype_amd import processor
    shape, spacing, mm = (12, 30, 40), (2.5, 0.7, 0.8), 6.0
    image, labels = (a.copy() for a in LR.lung_blob(shape, seed=4))
    labels[labels == 4] = 0                                                   # an empty region
    labels[6, 15, 20] = 9                                                     # lung outside 1..5 -> row 0
    radius = ops.local_window(spacing, mm)
    assert radius == (1, 4, 3)
    kw = dict(cuts=(0.10, 0.25, 0.50, 1.0), percentiles=(50, 90, 1, 99))
    got = processor.local_laa(on_device(image), on_device(labels), spacing, mm, **kw)
    q, _, _ = LR.fraction_map(image, labels, T, radius)
    assert torch.equal(got["map"].cpu(), torch.from_numpy(q))
    LR.assert_matches(got, LR.local_laa(q, labels, 5, **kw), "blob")
    assert got["radius"] == radius and got["local_mm"] == 6.0 and got["threshold"] == T
    assert int(got["voxels"][4]) == 0 and int(got["voxels"][0]) == 1 and float(got["whole_lung"]["sd"]) > 0.01
    again = processor.local_laa(on_device(image), on_device(labels), spacing, mm, **kw)
    for k in ("voxels", "mean", "sd", "perc", "above", "above_counts"):
        assert torch.equal(got[k].cpu().nan_to_num(-7.0), again[k].cpu().nan_to_num(-7.0)), k
    other = processor.local_laa(on_device(image), on_device(labels), spacing, mm, n_regions=2, threshold=-900, **kw)
    q900, _, _ = LR.fraction_map(image, labels, -900, radius)
    LR.assert_matches(other, LR.local_laa(q900, labels, 2, **kw), "two rows, -900")


# ------------------------------------------------------------------------------------------------ predict_case
def test_predict_case_with_the_local_map(ops, monkeypatch):
    from bodyct_dram_emph_subtype_amd import models, processor, transforms as TR
    _, lobes, spacing, _ = CR.fixture_cases()["blobs_u8"]
    rng = np.random.default_rng(3)
    hu = np.clip(np.rint(rng.normal(-900.0, 12.0, size=tuple(lobes.shape))), -940, -860).astype(np.int16)
    hu[1::3, 2::4, 1::4] = -1000                       # isolated voxels below -950 HU, none next to another
    hu[5:9, 10:22, 7:19] = -990                        # and a pocket wider than the window
    scan = torch.from_numpy(hu)
    target, peel, mm = (16, 32, 32), 3.0, 6.0
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    L = ops._L()
    launched = []                                                             # the launchers, not the size / capture queries

    class Spy:
        def __getattr__(self, name):
            fn = getattr(L, name)
            if not name.startswith("dram_") or name.endswith(("_workspace", "_nblk", "_capture_id")) or not callable(fn):
                return fn
            return lambda *a: launched.append(name) or fn(*a)

    spy = Spy()
    for module in (ops, processor, TR):
        if hasattr(module, "_L"):
            monkeypatch.setattr(module, "_L", lambda: spy)
    run = lambda **kw: processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, uid="u", region_names=names,
                                              regions=True, densitometry=True, core_peel=True, peel_mm=peel, clusters=True,
                                              **kw)
    run()                                                                     # the weights are packed once
    launched.clear()
    raw = run()
    base = list(launched)
    assert "dram_boxfrac3d" not in base and "full_local_laa" not in raw
    launched.clear()
    none = run(local_mm=None, local_kw=None)                                  # off: the entry and the launches of today
    assert launched == base and list(none) == list(raw) and none["metrics"] == raw["metrics"]
    assert list(none["metrics"]) == list(raw["metrics"]) and none["error_messages"] == raw["error_messages"]
    assert torch.equal(none["full_cle"], raw["full_cle"]) and torch.equal(none["full_pse"], raw["full_pse"])
    launched.clear()
    got = run(local_mm=mm)
    # two launchers more: the box count directly behind the densitometry histogram, and the histogram of the map
    i = launched.index("dram_boxfrac3d")
    assert launched[i - 1] == "dram_lobe_hist" and launched[i + 1] == "dram_lobe_hist"
    assert launched[:i] + launched[i + 2:] == base
    for k in ("full_cle", "full_pse"):
        assert torch.equal(got[k], raw[k]), k
    assert got["error_messages"] == raw["error_messages"]

    # the yardstick on the prepared crop
    case = TR.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid="u", want_lobes=True)
    img, lab = case["image"].cpu().numpy(), case["lobe_labels"].cpu().numpy()
    radius = ops.local_window(spacing, mm)
    assert radius == (1, 4, 4)

    def expected(image):
        q, _, u8 = LR.fraction_map(image, lab, T, radius)
        stats = dict(LR.local_laa(q, lab, 5), cuts=(0.10, 0.25, 0.50), percentiles=(50, 90), radius=radius, local_mm=mm,
                     threshold=T)
        full = torch.zeros(tuple(case["original_size"].tolist()), dtype=torch.uint8)
        (z0, z1), (y0, y1), (x0, x1) = case["crop_slice"].tolist()
        full[z0:z1, y0:y1, x0:x1] = torch.from_numpy(u8)
        return processor.local_laa_metrics(stats, names), full

    want, full = expected(img)
    keys, raw_keys = list(got["metrics"]), list(raw["metrics"])
    j = keys.index("local_laa950_mean_per_region")
    assert keys[j:j + len(want)] == list(want) and keys[:j] + keys[j + len(want):] == raw_keys
    assert keys[j - 1] == "volume_ml_per_lung"                                # they follow the densitometry keys
    assert {k: got["metrics"][k] for k in want} == want
    assert {k: got["metrics"][k] for k in raw_keys} == raw["metrics"]
    assert want["local_window_voxels"] == "3x9x9" and want["local_mm"] == "6.00"
    assert float(want["local_laa950_above50_per_lung"]) > 0.0 and float(want["local_laa950_sd_per_lung"]) > 0.0
    assert got["full_local_laa"].dtype == torch.uint8 and torch.equal(got["full_local_laa"].cpu(), full)
    assert int(full.max()) == 255 and int((full > 0).sum()) > 0

    # behind the median: the map of the filtered image where the section is named, of the raw one where it is not
    smooth = MR.median_filter(img, (3, 3, 3))
    want_f, full_f = expected(smooth)
    filt = run(local_mm=mm, scan_filter=(3, 3, 3))
    assert {k: filt["metrics"][k] for k in want_f} == want_f and torch.equal(filt["full_local_laa"].cpu(), full_f)
    assert want_f != want and not torch.equal(full_f, full)
    part = run(local_mm=mm, scan_filter=(3, 3, 3), scan_filter_sections=("clusters", "core_peel"))
    assert {k: part["metrics"][k] for k in want} == want and torch.equal(part["full_local_laa"].cpu(), full)
    assert part["metrics"]["scan_filter"] == "median3x3x3"
