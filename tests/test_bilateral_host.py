"""CPU: the fixed-point bilateral filter's yardstick (tests/bilateral_ref.py) against a triple loop over the definition
 and against a float64 bilateral filter, the host tables against their formulas, the C entry point's
and the Python wrappers' refusals (all before any device work), and the crop property the report relies on."""
import ctypes
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import bilateral_ref as BR
from conftest import GOLDEN


def hu_phantom(shape, seed):
    """a -850 HU plateau with sigma = 30 HU noise, and a slab of 0 HU (chest wall) behind a sharp edge"""
    rng = np.random.default_rng(seed)
    a = np.rint(rng.normal(-850.0, 30.0, size=shape))
    a[:, :, : shape[2] // 4] = np.rint(rng.normal(0.0, 30.0, size=(shape[0], shape[1], shape[2] // 4)))
    return a.astype(np.int16)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_equals_the_definition():
    rng = np.random.default_rng(5)
    a = rng.integers(-32768, 32768, size=(4, 5, 6), dtype=np.int64).astype(np.int16)
    a[1:3, 1:4, 1:5] = rng.integers(-1000, -900, size=(2, 3, 4))
    for sigma, hu in (((0.5, 0.5, 0.5), 0.5), ((0.2, 1.4, 1.4), 60.0), ((2.5, 1.0, 0.6), 289.0)):
        assert np.array_equal(BR.bilateral_filter(a, sigma, hu), BR.brute_force(a, sigma, hu)), (sigma, hu)
    b = np.rint(rng.normal(-900.0, 40.0, size=(3, 6, 7))).astype(np.int16)
    within = rng.integers(0, 3, size=b.shape).astype(np.uint8)
    within[0, 0, 0], within[2, 5, 6] = 0, 2
    for sigma, hu in (((1.0, 1.5, 1.5), 60.0), ((0.5, 0.5, 2.5), 20.0)):
        got = BR.bilateral_filter(b, sigma, hu, within=within)
        assert np.array_equal(got, BR.brute_force(b, sigma, hu, within=within)), (sigma, hu)
        assert np.array_equal(got[within == 0], b[within == 0])
        assert not np.array_equal(got, BR.bilateral_filter(b, sigma, hu))
    # negative labels are inside as well: non-zero is the rule
    signed = within.astype(np.int16) * -1
    assert np.array_equal(BR.bilateral_filter(b, (1.0, 1.5, 1.5), 60.0, within=signed),
                          BR.bilateral_filter(b, (1.0, 1.5, 1.5), 60.0, within=within))


def test_yardstick_against_a_float64_bilateral():
    """The fixed-point filter against the unrounded float64 bilateral on the same support, on a (12, 24, 32) phantom of
    sigma = 30 HU noise around -850 HU with a 0 HU slab, sigma = (1, 1.5, 1.5) voxels, sigma_hu = 60: the largest
    deviation measured on these inputs is 0.5319 HU (0.5 HU of it is the final rounding), asserted at the next quarter
    HU, 0.75.  The noise on the plateau drops from 30 HU to 7.7 HU, and both sides of the 0 / -850 edge keep their means
    within 1 HU."""
    a = hu_phantom((12, 24, 32), 17)
    sigma, hu = (1.0, 1.5, 1.5), 60.0
    got = BR.bilateral_filter(a, sigma, hu).astype(np.float64)
    ref = BR.float_bilateral(a, sigma, hu)
    dev = float(np.abs(got - ref).max())
    plateau = got[2:-2, 3:-3, 12:-3]
    print(f"max |fixed point - float64| = {dev:.4f} HU; plateau std {a[2:-2, 3:-3, 12:-3].std():.2f} -> {plateau.std():.2f} HU; "
          f"means {got[:, :, :8].mean():.2f} / {plateau.mean():.2f} HU")
    assert dev <= 0.75
    assert plateau.std() < 10.0 < 28.0 < a[2:-2, 3:-3, 12:-3].std()
    assert abs(got[:, :, :8].mean() - a[:, :, :8].mean()) < 1.0 and abs(plateau.mean() - a[2:-2, 3:-3, 12:-3].mean()) < 1.0


def test_all_radii_zero_is_the_identity():
    from bodyct_dram_emph_subtype_amd import ops
    a = hu_phantom((3, 5, 9), 2)
    assert ops.bilateral_tables((0.2, 0.1, 0.0), 60.0)[:3] == ([256], [256], [256])
    assert np.array_equal(BR.bilateral_filter(a, (0.2, 0.1, 0.0), 60.0), a)
    full = np.random.default_rng(1).integers(-32768, 32768, size=(3, 4, 5), dtype=np.int64).astype(np.int16)
    assert np.array_equal(BR.bilateral_filter(full, 0.0, 289.0), full)


def test_masked_crop_equals_the_whole_result_at_lung_voxels():
    """what ``processor.bilateral_image`` relies on: on a crop whose non-lung voxels were overwritten with the fill value,
    filtered within the cropped labels, every lung voxel has the value of the whole volume filtered within the labels"""
    rng = np.random.default_rng(9)
    scan = np.rint(rng.normal(-880.0, 35.0, size=(10, 14, 16))).astype(np.int16)
    lobes = np.zeros(scan.shape, dtype=np.uint8)
    lobes[2:8, 3:11, 4:13] = rng.integers(1, 6, size=(6, 8, 9))
    lobes[4, 5:7, 6:9] = 0                                                        # a hole
    lobes[2, 3, 4] = 3
    whole = BR.bilateral_filter(scan, (1.0, 1.5, 1.5), 60.0, within=lobes)
    box = (slice(2, 8), slice(3, 11), slice(4, 13))                               # the lung's bounding box, no border at all
    crop = np.where(lobes[box] != 0, scan[box], -2048).astype(np.int16)
    got = BR.bilateral_filter(crop, (1.0, 1.5, 1.5), 60.0, within=lobes[box])
    lung = lobes[box] != 0
    assert np.array_equal(got[lung], whole[box][lung]) and (got[~lung] == -2048).all()
    assert not np.array_equal(whole[box][lung], scan[box][lung])


# ------------------------------------------------------------------------------------------------ the tables
def test_tables_are_their_formulas():
    from bodyct_dram_emph_subtype_amd import ops
    assert ops.bilateral_radius(0.5) == 1 and ops.bilateral_radius(1.4) == 3 and ops.bilateral_radius(2.5) == 5
    assert ops.bilateral_radius(0.2) == 0 and ops.bilateral_radius(2.74) == 5 and ops.bilateral_radius(2.75) == 6
    assert ops.bilateral_radius(1.0, truncate=4.0) == 4
    for sigma, hu in (((0.5, 1.4, 2.5), 60.0), ((0.2, 2.74, 1.0), 0.5), ((1.0, 1.0, 1.0), 289.0), ((0.0, 0.0, 0.3), 1e-200)):
        tz, ty, tx, R = ops.bilateral_tables(sigma, hu)
        for t, s in zip((tz, ty, tx), sigma):
            r = int(2.0 * s + 0.5)
            assert t == ([math.floor(256.0 * math.exp(-k * k / (2.0 * s * s)) + 0.5) for k in range(r + 1)] if r else [256])
            assert t[0] == 256 and all(isinstance(v, int) for v in t) and len(t) <= ops.BILAT_MAX_RADIUS + 1
        assert BR.spatial_weight(tz, ty, tx, 0, 0, 0) == 256
        assert R[0] == 256 and R[-1] == 0 and all(v > 0 for v in R[:-1]) and len(R) <= ops.BILAT_RANGE_LEN
        if hu > 1e-100:
            assert R == [math.floor(256.0 * math.exp(-d * d / (2.0 * hu * hu)) + 0.5) for d in range(len(R))]
        assert all(isinstance(v, int) for v in R) and all(a >= b for a, b in zip(R, R[1:]))
    assert ops.bilateral_tables(1.0, 60.0) == ops.bilateral_tables((1.0, 1.0, 1.0), 60.0)
    assert ops.bilateral_tables(0.5, 0.5) == ([256, 35], [256, 35], [256, 35], [256, 35, 0])
    assert len(ops.bilateral_tables(1.0, 289.0)[3]) == 1022                      # the cap: 289 is in, 290 (1026) is out
    with pytest.raises(ValueError, match="1024"):
        ops.bilateral_tables(1.0, 290.0)
    with pytest.raises(ValueError, match="1024"):
        ops.bilateral_tables(1.0, 1e12)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma_hu"):
            ops.bilateral_tables(1.0, bad)
    for axis, sigma in zip("zyx", ((2.75, 1.0, 1.0), (1.0, 3.0, 1.0), (1.0, 1.0, 100.0))):
        with pytest.raises(ValueError, match=f"axis {axis} gives radius"):
            ops.bilateral_tables(sigma, 60.0)
    with pytest.raises(ValueError, match="radius 6"):
        ops.bilateral_tables(1.4, 60.0, truncate=4.0)
    for bad in ((1.0, -1.0, 1.0), (1.0, 1.0, float("nan"))):
        with pytest.raises(ValueError, match="sigma must be finite"):
            ops.bilateral_tables(bad, 60.0)
    with pytest.raises(ValueError, match="truncate"):
        ops.bilateral_tables(1.0, 60.0, truncate=0.0)
    # the corners of the box drop out where the product rounds to 0
    tz, ty, tx, _ = ops.bilateral_tables(1.0, 60.0, truncate=2.5)
    assert tz == [256, 155, 35, 3] and BR.spatial_weight(tz, ty, tx, 3, 3, 3) == 0 < BR.spatial_weight(tz, ty, tx, 3, 0, 0)


def test_the_bounds_of_the_sums():
    """den < 2^27 and, because a tap weighs nothing from |d| = L - 1 on, |num| <= den * (L - 2): a 64-bit sum, and a
    row of 11 taps within int32"""
    from bodyct_dram_emph_subtype_amd import ops
    tz, ty, tx, R = ops.bilateral_tables(2.5, 289.0)
    S = sum(BR.spatial_weight(tz, ty, tx, dz, dy, dx) for dz in range(-5, 6) for dy in range(-5, 6) for dx in range(-5, 6))
    assert S * 256 < 2 ** 27 and max(R[d] * d for d in range(len(R))) * S < 2 ** 34
    assert 11 * 65536 * (ops.BILAT_RANGE_LEN - 2) < 2 ** 30


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_point_is_declared_and_exported():
    from ctypes import c_int as I, c_longlong as LL, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _build, _lib
    assert _lib.SIGNATURES["dram_bilateral3d"] == (I, [P, P, P, I, LL, LL, I, I, I, P, P])
    T = _lib.DramBilateral
    assert (_lib.DRAM_BILAT_MAX_RADIUS, _lib.DRAM_BILAT_RANGE_LEN) == (5, 1024)
    assert ctypes.sizeof(T) == 4 * (3 + 18 + 1 + 1024)
    assert (T.radius.offset, T.spatial.offset, T.range_len.offset, T.range.offset) == (0, 12, 84, 88)
    t = T()
    assert len(t.radius) == 3 and len(t.spatial) == 3 and len(t.spatial[0]) == 6 and len(t.range) == 1024
    out = subprocess.run(["nm", "-D", "--defined-only", _build.build_library()], capture_output=True, text=True,
                         check=True).stdout
    assert "dram_bilateral3d" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_bilateral3d_refuses_bad_and_unsupported_arguments_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib, ops
    lib = _lib.load()
    BAD, UNS = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    one, two, three = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(1024)   # never dereferenced

    def table(**edit):
        t = _lib.DramBilateral()
        tz, ty, tx, R = ops.bilateral_tables((0.5, 1.4, 2.5), 60.0)
        for a, s in enumerate((tz, ty, tx)):
            t.radius[a] = len(s) - 1
            t.spatial[a][:len(s)] = s
        t.range_len = len(R)
        t.range[:len(R)] = R
        for k, v in edit.items():
            v(t)
        return t

    def call(src=one, dst=two, within=None, wt=0, sz=0, sy=0, size=(5, 7, 11), t=table()):
        return lib.dram_bilateral3d(src, dst, within, wt, sz, sy, *size, None if t is None else ctypes.byref(t), None)

    assert call(src=None) == BAD and call(dst=None) == BAD and call(t=None) == BAD
    assert call(dst=one) == BAD                                                  # out == in
    for axis in range(3):
        for v in (0, -1):
            assert call(size=tuple(v if a == axis else s for a, s in enumerate((5, 7, 11)))) == BAD, (axis, v)
        for r in (-1, 6, 100):
            assert call(t=table(e=lambda t: t.radius.__setitem__(axis, r))) == BAD, (axis, r)
        assert call(t=table(e=lambda t: t.spatial[axis].__setitem__(0, 255))) == BAD, axis
        assert call(t=table(e=lambda t: t.spatial[axis].__setitem__(0, 257))) == BAD, axis
    assert call(t=table(e=lambda t: t.spatial[2].__setitem__(1, -1))) == BAD
    assert call(t=table(e=lambda t: t.spatial[2].__setitem__(5, 300))) == BAD
    assert call(t=table(e=lambda t: t.range.__setitem__(0, 255))) == BAD          # the centre tap must weigh 65536
    for L in (1, 0, -1, 1025):
        assert call(t=table(e=lambda t: setattr(t, "range_len", L))) == BAD, L
    assert call(t=table(e=lambda t: setattr(t, "range_len", t.range_len - 1))) == BAD    # the last entry is not 0
    assert call(t=table(e=lambda t: t.range.__setitem__(3, 257))) == BAD
    assert call(t=table(e=lambda t: t.range.__setitem__(3, -1))) == BAD
    for wt in (0, 3, 4, -1):
        assert call(within=three, wt=wt, sz=77, sy=11) == BAD, wt
    assert call(within=three, wt=1, sz=-1, sy=11) == BAD and call(within=three, wt=2, sz=77, sy=-1) == BAD
    assert call(size=(2048, 1024, 1024)) == UNS and call(size=(2 ** 31 - 1, 2, 1)) == UNS
    assert call(size=(2048, 1024, 1024), dst=one) == BAD                         # a bad argument is named first


# ------------------------------------------------------------------------------------------------ the Python wrappers
def test_python_wrapper_refuses_before_the_device_is_touched():
    from bodyct_dram_emph_subtype_amd import ops
    img = torch.zeros(4, 5, 6, dtype=torch.int16)
    f = ops.bilateral_filter3d
    for sigma in ((1.0, 1.0), (1.0,) * 4, "a", None, (1.0, "b", 1.0)):
        with pytest.raises(ValueError, match="sigma"):
            f(img, sigma, 60.0)
    with pytest.raises(ValueError, match="sigma"):
        f(img, (1.0, -1.0, 1.0), 60.0)
    with pytest.raises(ValueError, match="axis x gives radius 6"):
        f(img, (1.0, 1.0, 3.0), 60.0)
    with pytest.raises(ValueError, match="truncate"):
        f(img, 1.0, 60.0, truncate=0.0)
    for hu in (0.0, -5.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma_hu"):
            f(img, 1.0, hu)
    with pytest.raises(ValueError, match="1024"):
        f(img, 1.0, 290.0)
    for bad in (img[0], img[:, :, :0], torch.zeros(1, 4, 5, 6, dtype=torch.int16), img.numpy()):
        with pytest.raises(ValueError, match="image"):
            f(bad, 1.0, 60.0)
    for bad in (img.to(torch.int32), img.to(torch.uint8), img.float(), img.double(), img.bool()):
        with pytest.raises(TypeError, match="int16"):
            f(bad, 1.0, 60.0)
    with pytest.raises(TypeError, match="out"):
        f(img, 1.0, 60.0, out=torch.zeros(4, 5, 6))
    with pytest.raises(TypeError, match="out"):
        f(img, 1.0, 60.0, out=np.zeros((4, 5, 6), dtype=np.int16))
    with pytest.raises(ValueError, match="out"):
        f(img, 1.0, 60.0, out=torch.zeros(4, 5, 7, dtype=torch.int16))
    with pytest.raises(ValueError, match="out"):
        f(img, 1.0, 60.0, out=torch.zeros(4, 6, 5, dtype=torch.int16).transpose(1, 2))
    big = torch.zeros(2, 4, 5, 6, dtype=torch.int16)
    for image, out in ((img, img), (big[0], big[1])):
        with pytest.raises(ValueError, match="share storage"):
            f(image, 1.0, 60.0, out=out)
    with pytest.raises(ValueError, match="within"):
        f(img, 1.0, 60.0, within=torch.zeros(4, 5, 7, dtype=torch.uint8))
    with pytest.raises(ValueError, match="within"):
        f(img, 1.0, 60.0, within=np.zeros((4, 5, 6), dtype=np.uint8))
    for bad in (torch.int32, torch.float32, torch.int64):
        with pytest.raises(TypeError, match="within"):
            f(img, 1.0, 60.0, within=torch.zeros(4, 5, 6, dtype=bad))
    # all in order: only the device is missing
    for kw in ({}, {"within": torch.ones(4, 5, 6, dtype=torch.uint8)}, {"within": torch.ones(4, 5, 6, dtype=torch.bool)},
               {"within": torch.ones(4, 5, 12, dtype=torch.int16)[:, :, ::2]}, {"out": torch.zeros(4, 5, 6, dtype=torch.int16)},
               {"truncate": 3.0}):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(img, (0.0, 1.4, 0.5), 289.0, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(img.transpose(0, 2), 0.5, 0.5)


def test_filter_name_and_params():
    from bodyct_dram_emph_subtype_amd import processor
    assert processor.filter_name(("bilateral", 1.0, 60.0)) == "bilateral1.00mm60.0hu"
    assert processor.filter_name(["bilateral", 0.625, 45]) == "bilateral0.62mm45.0hu"
    assert processor.filter_name(("bilateral", 2, 12.25)) == "bilateral2.00mm12.2hu"
    assert processor.bilateral_params("f", ("bilateral", 2, 45)) == (2.0, 45.0)
    for other in (None, (3, 3, 3), ("gaussian", 1.0), ("box", 1.0), "bilateral", ()):
        assert processor.bilateral_params("f", other) is None
    for bad in (("bilateral",), ("bilateral", 1.0), ("bilateral", 0.0, 60.0), ("bilateral", 1.0, 0.0), ("bilateral", -1.0, 60.0),
                ("bilateral", 1.0, -60.0), ("bilateral", float("nan"), 60.0), ("bilateral", 1.0, float("inf")),
                ("bilateral", 1.0, 60.0, 2.0), ("bilateral", "1", 60.0), ("bilateral", True, 60.0), ("bilateral", 1.0, True),
                ("bilateral", (1.0, 1.0, 1.0), 60.0)):
        with pytest.raises(ValueError, match="bilateral"):
            processor.filter_name(bad)
        with pytest.raises(ValueError, match="here: a bilateral"):
            processor.bilateral_params("here", bad)
    # every earlier input as before
    assert processor.filter_name(("gaussian", 1.0)) == "gaussian1.00mm" and processor.filter_name((1, 3, 3)) == "median1x3x3"
    with pytest.raises(ValueError, match="gaussian"):
        processor.filter_name(("gaussian", 0.0))
    with pytest.raises(ValueError, match="size"):
        processor.filter_name(("box", 1.0))
    sig = processor.bilateral_sigma_voxels("f", (2.5, 0.7, 0.5), 1.0)
    assert sig == (1.0 / 2.5, 1.0 / 0.7, 1.0 / 0.5)                              # Python floats, axis by axis
    assert processor.bilateral_sigma_voxels("f", (10.0, 0.7, 0.7), 1.0)[0] == 0.1                 # radius 0: a thick-slice axis
    with pytest.raises(ValueError, match=r"axis x with spacing 0\.3.*radius 7"):
        processor.bilateral_sigma_voxels("f", (0.7, 0.7, 0.3), 1.0)
    with pytest.raises(ValueError, match=r"axis z with spacing 0\.5"):
        processor.bilateral_sigma_voxels("f", (0.5, 0.7, 0.7), 1.4)                # 2.8 voxels: radius 6
    with pytest.raises(ValueError, match="spacing"):
        processor.bilateral_sigma_voxels("f", (0.5, 0.0, 0.7), 1.0)
    img = torch.zeros(4, 5, 6, dtype=torch.int16)
    with pytest.raises(ValueError, match=r"bilateral_image.*axis y"):
        processor.bilateral_image(img, img.to(torch.uint8), (1.0, 0.1, 1.0), 1.0, 60.0)
    with pytest.raises(ValueError, match="1024"):
        processor.bilateral_image(img, img.to(torch.uint8), (1.0, 1.0, 1.0), 1.0, 400.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        processor.bilateral_image(img, img.to(torch.uint8), (1.0, 1.0, 1.0), 1.0, 60.0)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_report", os.path.join(GOLDEN, "make_golden_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_predict_case_refuses_before_any_device_work(gen):
    from bodyct_dram_emph_subtype_amd import processor
    scan = torch.zeros(gen.ORIGINAL, dtype=torch.int16)                          # CPU tensors: prepare_case would refuse them
    run = lambda spacing=gen.SPACING, **kw: processor.predict_case(gen.Module(), scan, scan.to(torch.uint8), spacing,
                                                                   gen.SHAPE, **kw)
    for bad in (("bilateral", 0.0, 60.0), ("bilateral", 1.0, -1.0), ("bilateral",), ("bilateral", 1.0), ("bilateral", True, 60.0),
                ("bilateral", float("inf"), 60.0), ("bilateral", 1.0, 60.0, 1.0)):
        with pytest.raises(ValueError, match="scan_filter.*bilateral"):
            run(scan_filter=bad, clusters=True)
    with pytest.raises(ValueError, match=r"scan_filter.*axis y with spacing 0\.01"):
        run(spacing=(1.0, 0.01, 1.0), scan_filter=("bilateral", 1.0, 60.0), clusters=True)
    with pytest.raises(ValueError, match="1024"):
        run(scan_filter=("bilateral", 1.0, 290.0), clusters=True)
    with pytest.raises(ValueError, match="scan_filter_sections"):
        run(scan_filter=("bilateral", 1.0, 60.0), scan_filter_sections=("regions",), densitometry=True)
    # in order, and the median's precondition does not apply: the first thing missing is the device
    for kw in ({}, {"dilate_iterations": 0}, {"crop_border": 0}):
        with pytest.raises(RuntimeError, match="no CPU path"):
            run(scan_filter=("bilateral", 1.0, 60.0), clusters=True, **kw)
    with pytest.raises(ValueError, match="dilate_iterations"):                   # ... and still does for the median
        run(scan_filter=(3, 3, 3), clusters=True, dilate_iterations=0)
    with pytest.raises(ValueError, match="size"):
        run(scan_filter=("box", 1.0), clusters=True)
