"""Host side of the Gaussian filter (no GPU): the numpy float64 yardstick of tests/gauss_ref.py against the triple sum of
the definition, against scipy.ndimage.correlate1d (where scipy is present) and, with the recorded taps, against the
reference's recorded GaussianSmooth outputs (tests/golden/gauss.npz) within the bound B of gauss_ref.bound;
ops.gaussian_taps against the recorded taps; the entry point's declaration and the launcher's refusals through ctypes with
dummy pointers (no launch); the wrappers' refusals on CPU tensors; filter_name; TrainAugment's random stream with the
smoothing off and on; predict_case's refusals that need no device."""
import ctypes
import importlib.util
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import gauss_ref as GR
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gauss.npz"))


def recorded_taps(gold, sigma):
    i = [float(s) for s in gold["tap_sigmas"]].index(float(sigma))
    return gold[f"taps_{i}"]


# ------------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_equals_the_definition():
    rng = np.random.default_rng(5)
    a = rng.normal(size=(3, 4, 5))
    taps = [np.array([0.25, 0.5, 0.25]), np.array([0.1, 0.2, 0.4, 0.2, 0.1]), np.array([1.0])]
    for mode in GR.MODES:
        for t in (taps, taps[::-1], [taps[1]] * 3):
            got = GR.gaussian_filter(a, t, mode)
            assert got.dtype == np.float64 and got.shape == a.shape
            assert np.abs(got - GR.brute_force(a, t, mode)).max() < 1e-14, mode
        box = [[1, 3], [0, 4], [2, 3]]
        assert np.array_equal(GR.gaussian_filter(a, taps, mode, box), GR.gaussian_filter(a, taps, mode)[1:3, 0:4, 2:3])
    line = np.array([[[4.0, 0.0, 0.0, 8.0]]])
    w = [np.ones(1), np.ones(1), np.array([0.25, 0.5, 0.25])]
    assert GR.gaussian_filter(line, w, "nearest").tolist() == [[[3.0, 1.0, 2.0, 6.0]]]       # the edge voxel counts twice
    assert GR.gaussian_filter(line, w, "zero").tolist() == [[[2.0, 1.0, 2.0, 4.0]]]          # ... or a zero does
    assert GR.rint_i16(np.array([0.5, 1.5, -0.5, 2.5, 40000.0, -40000.0])).tolist() == [0, 2, 0, 2, 32767, -32768]


def test_yardstick_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(6)
    for shape in ((5, 9, 17), (1, 7, 5), (3, 1, 1), (4, 5, 3)):
        a = rng.normal(size=shape)
        for radii in ((1, 2, 3), (0, 2, 0), (8, 8, 8)):
            taps = [rng.random(2 * r + 1) for r in radii]
            taps = [(w + w[::-1]) / (w + w[::-1]).sum() for w in taps]
            for mode, theirs in (("nearest", "nearest"), ("zero", "constant")):
                want = a
                for axis in (2, 1, 0):
                    want = ndi.correlate1d(want, taps[axis], axis=axis, mode=theirs, cval=0.0)
                assert np.abs(GR.gaussian_filter(a, taps, mode) - want).max() < 1e-13, (shape, radii, mode)


def test_yardstick_reproduces_the_recorded_gaussian_smooth(gold):
    img = gold["image"]
    for i, sigma in enumerate(gold["smooth_sigmas"]):
        taps = [recorded_taps(gold, sigma).astype(np.float64)] * 3
        err = np.abs(GR.gaussian_filter(img, taps, "zero") - gold[f"smooth_{i}"].astype(np.float64)).max()
        B = GR.bound(taps, np.abs(img).max())
        print(f"sigma {float(sigma)}: reference GaussianSmooth vs yardstick {err / B:.3f} B")
        assert err <= B, (float(sigma), err, B)
    taps = [recorded_taps(gold, gold["chain_sigma"]).astype(np.float64)] * 3
    err = np.abs(GR.gaussian_filter(gold["after_box"], taps, "zero") - gold["after_smooth"].astype(np.float64)).max()
    assert err <= GR.bound(taps, np.abs(gold["after_box"]).max())


# ------------------------------------------------------------------------------------------------ the taps
def test_gaussian_taps_are_the_references(gold):
    from bodyct_dram_emph_subtype_amd import ops
    for i, sigma in enumerate(gold["tap_sigmas"]):
        want = gold[f"taps_{i}"]
        got = ops.gaussian_taps(float(sigma), 4.0)
        assert got.dtype == torch.float32 and got.device.type == "cpu" and tuple(got.shape) == want.shape, float(sigma)
        assert np.all(np.abs(got.numpy().astype(np.float64) - want) <= 2 * np.spacing(want)), float(sigma)   # 2 float32 ulps
        assert torch.equal(got, got.flip(0)) and abs(float(got.double().sum()) - 1.0) < 1e-6
    for sigma, r in ((0.0, 0), (0.1, 0), (0.124, 0), (0.125, 1), (0.3, 1), (0.374, 1), (0.375, 2), (0.6, 2), (1.0, 4),
                     (2.0, 8), (4.0, 16), (4.124, 16)):
        assert ops.gaussian_radius(sigma) == r and ops.gaussian_taps(sigma).numel() == 2 * r + 1, sigma
    assert ops.gaussian_taps(0.0).tolist() == [1.0] and ops.gaussian_taps(0.1).tolist() == [1.0]
    assert ops.gaussian_taps(1.0, truncate=2.0).numel() == 5 and ops.gaussian_taps(8.0, truncate=2.0).numel() == 33
    assert ops.GAUSS_MAX_RADIUS == 16
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            ops.gaussian_taps(bad)
    for bad in (0.0, -4.0, float("nan")):
        with pytest.raises(ValueError, match="truncate"):
            ops.gaussian_taps(1.0, bad)
    with pytest.raises(ValueError, match="radius 17"):
        ops.gaussian_taps(4.125)
    with pytest.raises(ValueError, match="radius 40"):
        ops.gaussian_taps(10.0)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_and_exported():
    from ctypes import c_int as I, c_longlong as LL, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _build, _lib
    assert _lib.SIGNATURES["dram_gauss3d"] == (I, [P, I, P, I, I, I, I, I, I, I, I, I, I, P, I, P, LL, P])
    assert _lib.SIGNATURES["dram_gauss3d_workspace"] == (LL, [I, I, I, I, I, I])
    T = _lib.DramGaussTaps
    assert ctypes.sizeof(T) == 216 and (T.radius.offset, T.w.offset) == (0, 12)
    t = T()
    assert len(t.radius) == 3 and len(t.w) == 3 and len(t.w[0]) == 17
    assert (_lib.DRAM_GAUSS_NEAREST, _lib.DRAM_GAUSS_ZERO) == (0, 1)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.build_library()], capture_output=True, text=True,
                         check=True).stdout
    assert {"dram_gauss3d", "dram_gauss3d_workspace"} <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_gauss3d_refuses_bad_and_unsupported_arguments_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    one, two, three = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(1024)   # never dereferenced
    taps = _lib.DramGaussTaps()
    for a in range(3):
        taps.radius[a], taps.w[a][0], taps.w[a][1] = 1, 0.5, 0.25

    def call(src=one, it=2, dst=two, ot=2, size=(5, 7, 11), origin=(0, 0, 0), ext=None, t=taps, border=0, work=three,
             nbytes=1 << 40):
        ext = tuple(s - o for s, o in zip(size, origin)) if ext is None else ext
        return lib.dram_gauss3d(src, it, dst, ot, *size, *origin, *ext, None if t is None else ctypes.byref(t), border,
                                work, nbytes, None)

    assert call(src=None) == BAD and call(dst=None) == BAD and call(t=None) == BAD and call(work=None) == BAD
    assert call(dst=one) == BAD                                                  # out == in
    for it, ot in ((4, 2), (2, 1), (1, 2), (8, 4), (0, 0), (4, 8)):
        assert call(it=it, ot=ot) == BAD, (it, ot)
    assert call(border=2) == BAD and call(border=-1) == BAD
    for axis in range(3):
        for v in (0, -1):
            assert call(size=tuple(v if a == axis else s for a, s in enumerate((5, 7, 11)))) == BAD, (axis, v)
            assert call(ext=tuple(v if a == axis else s for a, s in enumerate((5, 7, 11)))) == BAD, (axis, v)
        assert call(origin=tuple(-1 if a == axis else 0 for a in range(3)), ext=(1, 1, 1)) == BAD, axis
        assert call(origin=tuple(1 if a == axis else 0 for a in range(3)), ext=(5, 7, 11)) == BAD, axis      # leaves the volume
        for r in (-1, 17, 100):
            t = _lib.DramGaussTaps()
            t.radius[axis] = r
            assert call(t=t) == BAD, (axis, r)
    need = lib.dram_gauss3d_workspace(5, 0, 5, 7, 11, 1)
    assert need == 5 * 7 * 11 * 4 and call(nbytes=need - 1) == BAD
    assert call(work=ctypes.c_void_p(1028)) == BAD                               # not 16-byte aligned
    # planes [max(0, z0 - rz), min(D, z0 + Do + rz)) of the box's rows and columns, as float32
    assert lib.dram_gauss3d_workspace(10, 2, 5, 4, 6, 3) == 10 * 4 * 6 * 4
    assert lib.dram_gauss3d_workspace(40, 10, 5, 4, 6, 3) == 11 * 4 * 6 * 4
    assert lib.dram_gauss3d_workspace(40, 10, 5, 4, 6, 0) == 5 * 4 * 6 * 4
    for bad in ((10, 2, 9, 4, 6, 3), (10, -1, 5, 4, 6, 3), (10, 2, 5, 0, 6, 3), (10, 2, 5, 4, 6, 17), (10, 2, 5, 4, 6, -1)):
        assert lib.dram_gauss3d_workspace(*bad) == -1, bad
    assert call(size=(2048, 1024, 1024), ext=(1, 1, 1)) == UNS and call(size=(2 ** 31 - 1, 2, 1), ext=(1, 1, 1)) == UNS
    assert call(size=(2048, 1024, 1024), ext=(1, 1, 1), dst=one) == BAD          # a bad argument is named first


def test_python_wrapper_refuses_before_the_device_is_touched():
    from bodyct_dram_emph_subtype_amd import ops
    img = torch.zeros(4, 5, 6, dtype=torch.int16)
    f = ops.gaussian_filter3d
    for sigma in ((1.0, 1.0), (1.0,) * 4, "a", None, (1.0, "b", 1.0)):
        with pytest.raises(ValueError, match="sigma"):
            f(img, sigma)
    with pytest.raises(ValueError, match="sigma"):
        f(img, (1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="radius 20"):
        f(img, (1.0, 1.0, 5.0))
    with pytest.raises(ValueError, match="truncate"):
        f(img, 1.0, truncate=0.0)
    for mode in ("constant", "reflect", None, 0):
        with pytest.raises(ValueError, match="mode"):
            f(img, 1.0, mode=mode)
    for bad in (img[0], img[:, :, :0], torch.zeros(1, 4, 5, 6, dtype=torch.int16), img.numpy()):
        with pytest.raises(ValueError, match="image"):
            f(bad, 1.0)
    for bad in (img.to(torch.int32), img.to(torch.uint8), img.double(), img.bool(), img.to(torch.bfloat16)):
        with pytest.raises(TypeError, match="int16 or float32"):
            f(bad, 1.0)
    with pytest.raises(TypeError, match="out_dtype"):
        f(img.float(), 1.0, out_dtype=torch.int16)
    with pytest.raises(TypeError, match="out_dtype"):
        f(img, 1.0, out_dtype=torch.float64)
    for box in ([[0, 4], [0, 5]], [[0, 5], [0, 5], [0, 6]], [[2, 2], [0, 5], [0, 6]], [[-1, 2], [0, 5], [0, 6]],
                [[0, 4], [0, 5], [3, 7]], [0, 4, 5], "box"):
        with pytest.raises(ValueError, match="box"):
            f(img, 1.0, box=box)
    with pytest.raises(TypeError, match="out"):
        f(img, 1.0, out=torch.zeros(4, 5, 6))                                    # float32 out, int16 asked
    with pytest.raises(TypeError, match="out"):
        f(img, 1.0, out=np.zeros((4, 5, 6), dtype=np.int16))
    with pytest.raises(ValueError, match="out"):
        f(img, 1.0, out=torch.zeros(4, 5, 7, dtype=torch.int16))
    with pytest.raises(ValueError, match="out"):
        f(img, 1.0, box=[[1, 3], [0, 5], [0, 6]], out=torch.zeros(4, 5, 6, dtype=torch.int16))     # the box's shape
    with pytest.raises(ValueError, match="out"):
        f(img, 1.0, out=torch.zeros(4, 6, 5, dtype=torch.int16).transpose(1, 2))
    big = torch.zeros(2, 4, 5, 6, dtype=torch.int16)
    for image, out in ((img, img), (big[0], big[1])):
        with pytest.raises(ValueError, match="share storage"):
            f(image, 1.0, out=out)
    for kw in ({}, {"mode": "zero"}, {"box": torch.tensor([[1, 3], [0, 5], [2, 6]])}, {"out_dtype": torch.float32},
               {"box": [[1, 3], [0, 5], [2, 6]], "out_dtype": torch.float32, "out": torch.zeros(2, 5, 4)}):  # all in order: only the device is missing
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(img, (0.0, 1.5, 4.0), **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(img.float().transpose(0, 2), 0.45, mode="zero")


# ------------------------------------------------------------------------------------------------ the report
def test_filter_name():
    from bodyct_dram_emph_subtype_amd import processor
    assert processor.filter_name(("gaussian", 1.0)) == "gaussian1.00mm"
    assert processor.filter_name(["gaussian", 0.625]) == "gaussian0.62mm" and processor.filter_name(("gaussian", 2)) == "gaussian2.00mm"
    assert processor.filter_name((3, 3, 3)) == "median3x3x3" and processor.filter_name((1, 3, 3)) == "median1x3x3"
    for bad in (("gaussian",), ("gaussian", 0.0), ("gaussian", -1.0), ("gaussian", float("nan")), ("gaussian", 1.0, 2.0),
                ("gaussian", "1"), ("gaussian", True), ("gaussian", (1.0, 1.0, 1.0))):
        with pytest.raises(ValueError, match="gaussian"):
            processor.filter_name(bad)
    with pytest.raises(ValueError, match="size"):
        processor.filter_name(("box", 1.0))
    sig = processor.gaussian_sigma_voxels("f", (2.5, 0.7, 0.5), 1.0)
    assert sig == (1.0 / 2.5, 1.0 / 0.7, 1.0 / 0.5)                              # Python floats, axis by axis
    assert processor.gaussian_sigma_voxels("f", (10.0, 0.7, 0.7), 1.0)[0] == 0.1                  # radius 0: a thick-slice axis
    with pytest.raises(ValueError, match=r"axis x with spacing 0\.05"):
        processor.gaussian_sigma_voxels("f", (0.7, 0.7, 0.05), 1.0)
    with pytest.raises(ValueError, match=r"axis z with spacing 0\.5"):
        processor.gaussian_sigma_voxels("f", (0.5, 0.7, 0.7), 2.1)                # 4.2 voxels: radius 17


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
    for bad in (("gaussian", 0.0), ("gaussian", -1.0), ("gaussian",), ("gaussian", float("inf")), ("gaussian", 1.0, 1.0)):
        with pytest.raises(ValueError, match="scan_filter"):
            run(scan_filter=bad, clusters=True)
    with pytest.raises(ValueError, match=r"scan_filter.*axis y with spacing 0\.01"):
        run(spacing=(1.0, 0.01, 1.0), scan_filter=("gaussian", 1.0), clusters=True)
    with pytest.raises(ValueError, match="scan_filter_sections"):
        run(scan_filter=("gaussian", 1.0), scan_filter_sections=("regions",), densitometry=True)
    # in order, and the median's precondition does not apply: the first thing missing is the device
    for kw in ({}, {"dilate_iterations": 0}, {"crop_border": 0}):
        with pytest.raises(RuntimeError, match="no CPU path"):
            run(scan_filter=("gaussian", 1.0), clusters=True, **kw)
    with pytest.raises(ValueError, match="dilate_iterations"):                   # ... and still does for the median
        run(scan_filter=(3, 3, 3), clusters=True, dilate_iterations=0)


# ------------------------------------------------------------------------------------------------ the augmentation draw
def replay(r, p, smooth_p=0.0, smooth_sigma=(0.3, 0.6)):
    """TrainAugment.draw's consumption of a random.Random, written out"""
    d = dict(noise_sigma=None, box_centers=[], box_sizes=[], smooth_sigma=None, flip_dims=(), crop_center=None, crop_size=None)
    if r.random() < p:
        d["noise_sigma"] = r.uniform(0.03, 0.06)
    if r.random() < p:
        n = r.randint(1, 10)
        d["box_centers"] = [tuple(r.uniform(0.2, 0.8) for _ in range(3)) for _ in range(n)]
        d["box_sizes"] = [tuple(r.uniform(0.01, 0.06) for _ in range(3)) for _ in range(n)]
    if smooth_p > 0 and r.random() < smooth_p:
        d["smooth_sigma"] = r.uniform(*smooth_sigma)
    if r.random() < p:
        d["flip_dims"] = tuple(r.sample(range(3), r.randint(1, 2)))
    if r.random() < p:
        d["crop_center"] = tuple(r.uniform(0.45, 0.55) for _ in range(3))
        d["crop_size"] = tuple(r.uniform(0.95, 1.0) for _ in range(3))
    return d


def test_train_augment_draws():
    import dataclasses
    from bodyct_dram_emph_subtype_amd.transforms import AugmentParams, TrainAugment
    assert AugmentParams().smooth_sigma is None and "smooth_sigma" not in [f for f, _ in AugmentParams().to_struct((4, 4, 4))._fields_]
    aug, r = TrainAugment(rng=random.Random(31)), random.Random(31)
    for _ in range(200):                                       # the default consumes today's stream
        ap = aug.draw()
        assert ap.smooth_sigma is None and dataclasses.asdict(ap) == replay(r, 0.5)
    assert aug.rng.random() == r.random()
    # the replay without its smooth branch is the draw as it was before the field existed
    old, r = TrainAugment(p=0.5, rng=random.Random(8), smooth_p=0.0, smooth_sigma=(1.0, 2.0)), random.Random(8)
    for _ in range(50):
        assert dataclasses.asdict(old.draw()) == replay(r, 0.5)
    aug, r = TrainAugment(rng=random.Random(32), smooth_p=1.0), random.Random(32)
    for _ in range(200):
        ap = aug.draw()
        assert 0.3 <= ap.smooth_sigma <= 0.6 and dataclasses.asdict(ap) == replay(r, 0.5, 1.0)
    aug, r = TrainAugment(p=1.0, rng=random.Random(33), smooth_p=0.4, smooth_sigma=(0.5, 2.0)), random.Random(33)
    draws = [aug.draw() for _ in range(200)]
    assert [dataclasses.asdict(ap) for ap in draws] == [replay(r, 1.0, 0.4, (0.5, 2.0)) for _ in range(200)]
    n = sum(ap.smooth_sigma is not None for ap in draws)
    assert 50 < n < 110 and all(0.5 <= ap.smooth_sigma <= 2.0 for ap in draws if ap.smooth_sigma is not None)
    for bad in ((0.6, 0.3), (-0.1, 0.3), (0.3,), (0.3, 5.0)):
        with pytest.raises(ValueError):
            TrainAugment(smooth_p=0.5, smooth_sigma=bad)
        assert TrainAugment(smooth_p=0.0, smooth_sigma=bad).draw().smooth_sigma is None    # off: the range is not looked at


def test_train_flag():
    from bodyct_dram_emph_subtype_amd import train
    p = train.build_parser()
    assert getattr(p.parse_args([]), "augment_smooth", 0.0) == 0.0                # off unless given
    assert p.parse_args(["--augment", "1", "--augment_smooth", "0.5"]).augment_smooth == 0.5
