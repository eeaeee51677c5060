"""GPU: the separable Gaussian filter of csrc/gauss.hip (dram_gauss3d through ops.gaussian_filter3d) against the numpy
float64 yardstick of tests/gauss_ref.py within B = 2 (nz + ny + nx + 3) 2^-24 max|src| (gauss_ref.bound), the three
bit-for-bit properties the fixed accumulation order gives (int16 = rint(float32), box = crop of the whole result, call =
call), the contract of the wrapper, the GaussianSmooth augmentation against the reference's recorded outputs
(tests/golden/gauss.npz) and the Gaussian in front of the scan side of the report (predict_case(scan_filter=...)).

Shapes.  The in-plane pass tiles TY = 16 rows x TX = 64 columns of one plane per workgroup (a wave filters whole rows),
the z pass has no tile (one thread per output, or per four along x where W % 4 == 0 and the output is aligned): besides
the issue's list -- single voxel, W = 2, D = 3 alone, odd W (1,7,5), W = 130 = 2 TX + 2, (5,9,67) -- the three shapes
(2,15,63), (3,16,64), (4,17,65) put the tiled axes one below, at and one above the tile, and on (4,5,3) the radii 8 and
16 overhang both sides of every axis.  W = 64 and 4 take the vector form of the z pass, every other W the scalar one.
The yardstick of a (shape, content, sigma, mode) is computed once."""
import functools
import os

import numpy as np
import pytest
import torch

import case_prep_ref as CR
import data_path_ref as R
import gauss_ref as GR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TX, TY = 64, 16                            # csrc/gauss.hip
SHAPES = [(1, 1, 1), (1, 1, 2), (3, 1, 1), (1, 7, 5), (2, 3, 130), (5, 9, 67), (2, TY - 1, TX - 1), (3, TY, TX),
          (4, TY + 1, TX + 1), (4, 5, 3)]
SIGMAS = [0.45, 0.6, 2.0, (0.0, 1.5, 1.5), (4.0, 0.3, 0.3)]                    # radii 2, 2, 8, (0, 6, 6), (16, 1, 1)
OVERHANG = (4, 5, 3)                                                           # ... and 4.0 isotropic: radius 16 on all axes
SENTINEL = 12345


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gauss.npz"))


def f32_noise(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def hu_noise(shape, seed):
    """int16 HU-like noise with a -2048 block (the fill value of a prepared case) and +-32767 planted"""
    rng = np.random.default_rng(seed)
    a = np.rint(rng.normal(-850.0, 120.0, size=shape)).astype(np.int16)
    D, H, W = shape
    a[: (D + 1) // 2, : (H + 1) // 2, : (W + 2) // 3] = -2048
    a.reshape(-1)[:: 7] = np.where(np.arange(a.size)[:: 7] % 2 == 0, 32767, -32767).astype(np.int16)
    a[-1, -1, -1] = 32767
    return a


CONTENTS = {"f32_noise": f32_noise, "hu_noise": hu_noise}


@functools.lru_cache(maxsize=None)
def volume(shape, content):
    a = CONTENTS[content](shape, 7 + len(content))
    a.setflags(write=False)
    return a


def sigma3(sigma):
    return tuple(float(s) for s in sigma) if isinstance(sigma, tuple) else (float(sigma),) * 3


@functools.lru_cache(maxsize=None)
def taps64(sigma):
    """the product's own float32 taps (held to the reference's in test_gauss_host.py), as float64, per axis"""
    from bodyct_dram_emph_subtype_amd import ops as o
    return tuple(o.gaussian_taps(s).double().numpy() for s in sigma3(sigma))


@functools.lru_cache(maxsize=None)
def reference(shape, content, sigma, mode):
    r = GR.gaussian_filter(volume(shape, content), taps64(sigma), mode)
    r.setflags(write=False)
    return r


def bound(shape, content, sigma):
    return GR.bound(taps64(sigma), np.abs(volume(shape, content).astype(np.float64)).max())


def on_device(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_within_the_bound_of_the_yardstick(ops, shape):
    worst = 0.0
    for content in CONTENTS:
        src = on_device(volume(shape, content))
        keep = src.clone()
        for sigma in SIGMAS + ([4.0] if shape == OVERHANG else []):
            B = bound(shape, content, sigma)
            for mode in GR.MODES:
                want = reference(shape, content, sigma, mode)
                out = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
                got = ops.gaussian_filter3d(src, sigma, mode=mode, out=out, out_dtype=torch.float32)
                assert got is out
                err = np.abs(got.cpu().numpy().astype(np.float64) - want)
                assert not np.isnan(err).any(), (content, sigma, mode)         # every element written
                worst = max(worst, float(err.max()) / B)
                assert err.max() <= B, (content, sigma, mode, float(err.max()) / B)
                fresh = ops.gaussian_filter3d(src, sigma, mode=mode)
                assert fresh.dtype == src.dtype and fresh.is_contiguous() and tuple(fresh.shape) == shape
                if content == "hu_noise":
                    # the int16 output is rintf of the float32 one, clamped: exactly
                    i16 = ops.gaussian_filter3d(src, sigma, mode=mode, out=torch.full(shape, SENTINEL, dtype=torch.int16,
                                                                                      device=DEV))
                    assert torch.equal(i16, fresh) and torch.equal(i16, got.round().clamp(-32768, 32767).to(torch.int16))
                    assert np.abs(i16.cpu().numpy().astype(np.float64) - want).max() <= 0.5 + B, (sigma, mode)
                else:
                    assert torch.equal(bits(fresh), bits(got)), (sigma, mode)
        assert torch.equal(src, keep), content                                # the input is only read
    print(f"[kernel/bound] {shape}: {worst:.3f}")


def test_overhanging_radii_really_overhang():
    for sigma in (2.0, 4.0):
        assert all(len(w) // 2 in (8, 16) and len(w) // 2 > max(OVERHANG) for w in taps64(sigma))
    assert [len(w) // 2 for w in taps64((0.0, 1.5, 1.5))] == [0, 6, 6] and [len(w) // 2 for w in taps64((4.0, 0.3, 0.3))] == [16, 1, 1]


def test_a_dropped_outermost_tap_would_fail():
    """the bound is tight enough to see one missing tap at radius 8 (constant volume, nearest: the result is the sum of
    the taps times the constant)"""
    w = taps64(2.0)[0]
    assert 1000.0 * 2 * w[0] > 4 * GR.bound(taps64(2.0), 1000.0)


def test_constant_extremes_come_back(ops):
    """a constant volume at +-32767 behind the replicated border: the taps sum to 1 within fp32 rounding, the result
    rounds back to the constant and the clamp holds the int16 range"""
    for v in (32767, -32767, -32768):
        src = torch.full((5, 18, 66), v, dtype=torch.int16, device=DEV)
        for sigma in (0.45, 2.0, (4.0, 0.3, 1.5)):
            assert torch.equal(ops.gaussian_filter3d(src, sigma, mode="nearest"), src), (v, sigma)
    line = torch.tensor([[[1, 2, 4, 7, 7, -3, -4, -6]]], dtype=torch.int16, device=DEV)
    got = ops.gaussian_filter3d(line, (0.0, 0.0, 0.3), mode="zero", out_dtype=torch.float32)
    w = ops.gaussian_taps(0.3).double()
    want = torch.nn.functional.conv1d(line.double().cpu().view(1, 1, -1), w.view(1, 1, -1), padding=1).view(1, 1, -1)
    assert float((got.cpu().double() - want).abs().max()) < 1e-5
    assert torch.equal(ops.gaussian_filter3d(line, (0.0, 0.0, 0.3), mode="zero"), want.round().to(torch.int16).to(DEV))


BOX_SHAPE = (9, 21, 70)
BOXES = [[[0, 3], [2, 19], [3, 66]], [[6, 9], [2, 19], [3, 66]], [[2, 7], [0, 5], [3, 66]], [[2, 7], [16, 21], [3, 66]],
         [[2, 7], [2, 19], [0, 9]], [[2, 7], [2, 19], [61, 70]], [[1, 6], [3, 18], [5, 62]], [[3, 4], [7, 8], [33, 34]],
         [[1, 8], [1, 20], [2, 70]], [[0, 9], [0, 21], [0, 70]]]                # the six faces, interior at odd offsets, ...


@pytest.mark.parametrize("mode", GR.MODES)
def test_a_box_is_the_crop_of_the_whole_result(ops, mode):
    """bit for bit, for both output types; Wo = 68 of the last-but-one box takes the vector z pass on a box"""
    for content, dtypes in (("hu_noise", (torch.int16, torch.float32)), ("f32_noise", (torch.float32,))):
        src = on_device(volume(BOX_SHAPE, content))
        for sigma in ((1.0, 0.6, 2.0), (0.0, 0.45, 0.45)):
            for dt in dtypes:
                whole = ops.gaussian_filter3d(src, sigma, mode=mode, out_dtype=dt)
                for box in BOXES:
                    (z0, z1), (y0, y1), (x0, x1) = box
                    got = ops.gaussian_filter3d(src, sigma, mode=mode, box=box, out_dtype=dt)
                    assert got.dtype == dt and got.is_contiguous() and tuple(got.shape) == (z1 - z0, y1 - y0, x1 - x0)
                    assert torch.equal(bits(got), bits(whole[z0:z1, y0:y1, x0:x1].contiguous())), (content, sigma, dt, box)
                got = ops.gaussian_filter3d(src, sigma, mode=mode, box=torch.tensor(BOXES[6]), out_dtype=dt)   # crop_slice's form
                assert torch.equal(bits(got), bits(whole[1:6, 3:18, 5:62].contiguous()))
        want = GR.gaussian_filter(volume(BOX_SHAPE, content), taps64((1.0, 0.6, 2.0)), mode, BOXES[6])
        got = ops.gaussian_filter3d(src, (1.0, 0.6, 2.0), mode=mode, box=BOXES[6], out_dtype=torch.float32)
        assert np.abs(got.cpu().numpy() - want).max() <= bound(BOX_SHAPE, content, (1.0, 0.6, 2.0))


def test_out_offsets_and_non_contiguous_input(ops):
    shape = (5, 9, 68)                                                         # W % 4 == 0: the vector z pass when aligned
    for content, dt in (("hu_noise", torch.int16), ("f32_noise", torch.float32), ("hu_noise", torch.float32)):
        src = on_device(volume(shape, content))
        want = ops.gaussian_filter3d(src, 0.6, out_dtype=dt)
        assert np.abs(want.cpu().numpy().astype(np.float64) - reference(shape, content, 0.6, "nearest")).max() \
            <= bound(shape, content, 0.6) + (0.5 if dt == torch.int16 else 0.0)
        wide = torch.zeros((5, 9, 80), dtype=src.dtype, device=DEV)
        wide[:, :, 5:73] = src
        view = wide[:, :, 5:73]
        assert not view.is_contiguous() and torch.equal(bits(ops.gaussian_filter3d(view, 0.6, out_dtype=dt)), bits(want))
        swapped = src.permute(2, 1, 0).contiguous().permute(2, 1, 0)
        assert not swapped.is_contiguous() and torch.equal(bits(ops.gaussian_filter3d(swapped, 0.6, out_dtype=dt)), bits(want))
        # an output that starts on an odd element of its storage: the vector stores fall back to single elements
        for lead in (1, 2, 3):
            flat = torch.full((src.numel() + lead,), SENTINEL, dtype=dt, device=DEV)
            out = flat[lead:].view(shape)
            assert out.data_ptr() % (4 * out.element_size()) != 0
            assert ops.gaussian_filter3d(src, 0.6, out=out, out_dtype=dt) is out
            assert torch.equal(bits(out), bits(want)) and bool((flat[:lead] == SENTINEL).all()), (content, dt, lead)
        odd_src = torch.cat([torch.zeros(1, dtype=src.dtype, device=DEV), src.reshape(-1)])[1:].view(shape)
        assert torch.equal(bits(ops.gaussian_filter3d(odd_src, 0.6, out_dtype=dt)), bits(want))


def test_two_calls_are_bit_identical(ops):
    src = on_device(volume((5, 9, 67), "f32_noise"))
    for sigma, mode in ((0.45, "zero"), (2.0, "nearest")):
        assert torch.equal(bits(ops.gaussian_filter3d(src, sigma, mode=mode)), bits(ops.gaussian_filter3d(src, sigma, mode=mode)))


def test_is_capturable(ops):
    shape = (4, TY + 1, TX + 1)
    src = on_device(volume(shape, "hu_noise"))
    eager = ops.gaussian_filter3d(src, 0.6)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.gaussian_filter3d(src, 0.6)                                        # warm-up on the side stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = ops.gaussian_filter3d(src, 0.6)
    for _ in range(2):
        captured.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
    assert np.abs(eager.cpu().numpy() - reference(shape, "hu_noise", 0.6, "nearest")).max() <= 0.5 + bound(shape, "hu_noise", 0.6)


class Spy:
    """ops._L() with the Gaussian entry points (and any others named) recorded"""

    def __init__(self, L, names=("dram_gauss3d", "dram_gauss3d_workspace")):
        self.L, self.names, self.launches = L, names, []

    def __getattr__(self, name):
        fn = getattr(self.L, name)
        if name in self.names:
            return lambda *a: self.launches.append(name) or fn(*a)
        return fn


def test_refusals_come_before_any_launch(ops, monkeypatch):
    img = torch.zeros((4, 6, 70), dtype=torch.int16, device=DEV)
    spy = Spy(ops._L())
    monkeypatch.setattr(ops, "_L", lambda: spy)
    f = ops.gaussian_filter3d
    with pytest.raises(ValueError, match="radius 17"):
        f(img, 4.2)
    with pytest.raises(ValueError, match="sigma"):
        f(img, (1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="mode"):
        f(img, 1.0, mode="reflect")
    with pytest.raises(ValueError, match="box"):
        f(img, 1.0, box=[[0, 5], [0, 6], [0, 70]])
    with pytest.raises(TypeError):
        f(img.to(torch.int32), 1.0)
    with pytest.raises(TypeError, match="out_dtype"):
        f(img.float(), 1.0, out_dtype=torch.int16)
    with pytest.raises(ValueError, match="share storage"):
        f(img, 1.0, out=img)
    with pytest.raises(ValueError, match="out"):
        f(img, 1.0, out=torch.zeros((4, 6, 71), dtype=torch.int16, device=DEV))
    with pytest.raises(TypeError, match="out"):
        f(img, 1.0, out=torch.zeros((4, 6, 70), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="device"):
        f(img, 1.0, out=torch.zeros((4, 6, 70), dtype=torch.int16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(img.cpu(), 1.0)
    assert spy.launches == []
    f(img, 1.0)
    assert spy.launches == ["dram_gauss3d_workspace", "dram_gauss3d"]


# ------------------------------------------------------------------------------------------------ the augmentation
def chain_params(gold, **keep):
    from bodyct_dram_emph_subtype_amd.transforms import AugmentParams
    full = dict(noise_sigma=float(gold["noise_sigma"]), box_centers=[tuple(c) for c in gold["box_centers"]],
                box_sizes=[tuple(c) for c in gold["box_sizes"]], smooth_sigma=float(gold["chain_sigma"]),
                flip_dims=tuple(int(d) for d in gold["flip_dims"]), crop_center=tuple(gold["crop_center"]),
                crop_size=tuple(gold["crop_size"]))
    return AugmentParams(**{k: v for k, v in full.items() if keep.get(k.split("_")[0], False)})


def test_gaussian_smooth_matches_the_recorded_reference(ops, gold):
    from bodyct_dram_emph_subtype_amd.transforms import AugmentParams, augment_image
    img = torch.from_numpy(gold["image"]).to(DEV)
    for i, sigma in enumerate(gold["smooth_sigmas"]):
        B = GR.bound(taps64(float(sigma)), np.abs(gold["image"]).max())
        got = augment_image(img, AugmentParams(smooth_sigma=float(sigma)))
        assert got.dtype == torch.float32 and got.data_ptr() != img.data_ptr()
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - gold[f"smooth_{i}"]).max())
        print(f"[kernel vs recorded GaussianSmooth] sigma {float(sigma)}: {err / B:.3f} B")
        assert err <= 2 * B, (float(sigma), err / B)
    assert torch.equal(augment_image(img, AugmentParams(smooth_sigma=0.0)), img)           # radius 0: a copy


def test_teacher_forced_chain(ops, gold):
    """each stage from the recorded output of the one before it: smooth of after_box against after_smooth within 2 B;
    flip + crop of after_smooth against after_crop through the fp64 reference and its element-wise bound"""
    from bodyct_dram_emph_subtype_amd.transforms import augment_image
    sigma = float(gold["chain_sigma"])
    box = torch.from_numpy(gold["after_box"]).to(DEV)
    B = GR.bound(taps64(sigma), np.abs(gold["after_box"]).max())
    got = augment_image(box, chain_params(gold, smooth=True))
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - gold["after_smooth"]).max())
    print(f"[kernel vs recorded after_smooth] {err / B:.3f} B")
    assert err <= 2 * B
    smooth = torch.from_numpy(gold["after_smooth"]).to(DEV)
    tail = chain_params(gold, flip=True, crop=True)
    ref = R.augment_image64(smooth, None, tail.to_struct(smooth.shape))
    for what, t in (("kernel", augment_image(smooth, tail)), ("recorded after_crop", torch.from_numpy(gold["after_crop"]).to(DEV))):
        r = R.ratio(t, ref)
        print(f"[{what}/bound] flip + crop of after_smooth: {r:.3f}")
        assert t.dtype == torch.float32 and t.shape == ref.val.shape and r <= 1.0, what
    flip = R.augment_image64(smooth, None, chain_params(gold, flip=True).to_struct(smooth.shape))
    assert R.ratio(torch.from_numpy(gold["after_flip"]).to(DEV), flip) == 0.0            # a flip is exact


def test_all_five_equal_the_three_calls(ops, gold, monkeypatch):
    from bodyct_dram_emph_subtype_amd import transforms as TR
    img = torch.from_numpy(gold["image"]).to(DEV)
    torch.manual_seed(int(gold["noise_seed"]))
    noise = torch.randn(gold["image"].shape).to(DEV)
    spy = Spy(ops._L(), ("dram_gauss3d", "dram_augment_image"))
    monkeypatch.setattr(ops, "_L", lambda: spy)
    monkeypatch.setattr(TR, "_L", lambda: spy)
    got = TR.augment_image(img, chain_params(gold, noise=True, box=True, smooth=True, flip=True, crop=True), noise)
    assert spy.launches == ["dram_augment_image", "dram_gauss3d", "dram_augment_image"]
    a = TR.augment_image(img, chain_params(gold, noise=True, box=True), noise)
    assert float(np.abs(a.cpu().numpy() - gold["after_box"]).max()) < 2e-6          # the bound of the existing fixture test
    b = ops.gaussian_filter3d(a, float(gold["chain_sigma"]), mode="zero")
    c = TR.augment_image(b, chain_params(gold, flip=True, crop=True))
    assert torch.equal(bits(got), bits(c))
    assert float(np.abs(got.cpu().numpy() - gold["after_crop"]).max()) < 2e-5       # ... and of its crop stage
    # a call whose transforms are all off is skipped
    for keep, want in (({"smooth": True}, ["dram_gauss3d"]), ({"noise": True, "smooth": True}, ["dram_augment_image", "dram_gauss3d"]),
                       ({"smooth": True, "flip": True}, ["dram_gauss3d", "dram_augment_image"])):
        spy.launches.clear()
        TR.augment_image(img, chain_params(gold, **keep), noise)
        assert spy.launches == want, keep
    # without smooth_sigma: the single fused call of before, and the same bits as the two halves composed
    spy.launches.clear()
    fused = TR.augment_image(img, chain_params(gold, noise=True, box=True, flip=True, crop=True), noise)
    assert spy.launches == ["dram_augment_image"]
    assert torch.equal(bits(fused), bits(TR.augment_image(a, chain_params(gold, flip=True, crop=True))))
    # masks ignore the smoothing
    mask = (torch.from_numpy(gold["image"]) > 0.3).to(DEV)
    spy.launches.clear()
    with_s = TR.augment_mask(mask, chain_params(gold, smooth=True, flip=True, crop=True))
    assert torch.equal(with_s, TR.augment_mask(mask, chain_params(gold, flip=True, crop=True))) and spy.launches == []
    assert TR.augment_mask(mask, chain_params(gold, smooth=True)) is mask


def test_train_augment_with_smoothing(ops):
    import random
    from bodyct_dram_emph_subtype_amd import transforms as TR
    g = torch.Generator().manual_seed(5)
    img = torch.randn(9, 11, 13, generator=g).to(DEV)
    lung = (torch.rand(9, 11, 13, generator=g) > 0.5).to(DEV)
    ap = TR.TrainAugment(p=1.0, rng=random.Random(3), smooth_p=1.0).draw()
    assert ap.smooth_sigma is not None
    torch.manual_seed(21)
    out = TR.TrainAugment(p=1.0, rng=random.Random(3), smooth_p=1.0)({"image": img, "lung_mask": lung})
    torch.manual_seed(21)
    assert torch.equal(bits(out["image"]), bits(TR.augment_image(img, ap)))
    assert torch.equal(out["lung_mask"], TR.augment_mask(lung, ap))


# ------------------------------------------------------------------------------------------------ predict_case
def _scan_side(processor, key):
    if processor._DENSITO_KEY.fullmatch(key) or processor._CLUSTER_KEY.fullmatch(key):
        return True
    return bool(processor._CORE_PEEL_KEY.fullmatch(key)) and key != "peel_mm" and \
        not key.startswith(("cle_", "pse_", "region_voxels"))


def test_predict_case_with_gaussian_scan_filter(ops, monkeypatch):
    from bodyct_dram_emph_subtype_amd import models, processor, transforms as TR
    _, lobes, spacing, _ = CR.fixture_cases()["blobs_u8"]
    rng = np.random.default_rng(3)
    hu = np.clip(np.rint(rng.normal(-900.0, 12.0, size=tuple(lobes.shape))), -940, -860).astype(np.int16)
    hu[1::3, 2::4, 1::4] = -1000                       # isolated voxels below -950 HU, none next to another
    scan = torch.from_numpy(hu)
    target, n, peel = (16, 32, 32), 5, 3.0
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    calls, medians = [], []
    real, real_median = ops.gaussian_filter3d, ops.median_filter3d
    monkeypatch.setattr(ops, "gaussian_filter3d", lambda *a, **k: calls.append((a[1:], k)) or real(*a, **k))
    monkeypatch.setattr(ops, "median_filter3d", lambda *a, **k: medians.append(a[1:]) or real_median(*a, **k))
    run = lambda **kw: processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, uid="u", region_names=names,
                                              regions=True, densitometry=True, core_peel=True, peel_mm=peel, clusters=True,
                                              **kw)
    raw = run()
    assert calls == [] and medians == [] and "scan_filter" not in raw["metrics"]
    got = run(scan_filter=("gaussian", 1.0))
    assert len(calls) == 1 and medians == []                                  # once, for three sections
    sig = tuple(1.0 / s for s in spacing)
    assert calls[0][0] == (sig,) and calls[0][1]["mode"] == "nearest"
    calls.clear()
    assert list(got["metrics"])[-1] == "scan_filter" and got["metrics"]["scan_filter"] == "gaussian1.00mm"
    assert list(got["metrics"])[:-1] == list(raw["metrics"]) and set(got) == set(raw)
    for k in ("full_cle", "full_pse"):
        assert torch.equal(got[k], raw[k]), k
    net = [k for k in raw["metrics"] if not _scan_side(processor, k)]
    assert set(processor.REGION_KEYS) <= set(net) and "cle_lesion_percentage_per_region_peel" in net
    assert {k: got["metrics"][k] for k in net} == {k: raw["metrics"][k] for k in net}

    # the scan side: the sections' own functions on gaussian_image, which is the yardstick's crop up to the rint rule
    case = TR.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid="u", want_lobes=True)
    smooth = processor.gaussian_image(scan.to(DEV), case["crop_slice"], spacing, 1.0)
    calls.clear()
    assert smooth.dtype == torch.int16 and smooth.shape == case["image"].shape
    taps = tuple(ops.gaussian_taps(s).double().numpy() for s in sig)
    assert [len(w) // 2 for w in taps] == [2, 6, 6]
    want64 = GR.gaussian_filter(hu, taps, "nearest", case["crop_slice"].tolist())
    assert np.abs(smooth.cpu().numpy() - want64).max() <= 0.5 + GR.bound(taps, np.abs(hu.astype(np.float64)).max())
    whole = real(scan.to(DEV), sig, mode="nearest")
    (z0, z1), (y0, y1), (x0, x1) = case["crop_slice"].tolist()
    assert torch.equal(smooth, whole[z0:z1, y0:y1, x0:x1])                    # the crop of the filtered scan
    labels = case["lobe_labels"]
    want = processor.densitometry_metrics(processor.densitometry(smooth, labels, spacing), names)
    want.update(processor.laa_cluster_metrics(processor.laa_clusters(smooth, labels, spacing), names))
    cp = processor.core_peel_metrics(processor.core_peel(smooth, labels, spacing, peel_mm=peel, n_regions=n), names)
    want.update({k: v for k, v in cp.items() if k != "peel_mm"})
    assert set(want) == {k for k in raw["metrics"] if _scan_side(processor, k)}
    assert {k: got["metrics"][k] for k in want} == want
    # direction: the isolated voxels are gone
    before, after = int(raw["metrics"]["laa950_clusters_per_lung"]), int(got["metrics"]["laa950_clusters_per_lung"])
    print(f"laa950 clusters per lung: {before} unfiltered, {after} behind the 1 mm Gaussian")
    assert before > 50 and after < before
    assert got["metrics"]["laa950_fraction_per_lung"] != raw["metrics"]["laa950_fraction_per_lung"]

    # only the clusters named: densitometry and core / peel are the raw scan's
    part = run(scan_filter=("gaussian", 1.0), scan_filter_sections=("clusters",))
    assert len(calls) == 1 and part["metrics"]["scan_filter"] == "gaussian1.00mm"
    for k, v in raw["metrics"].items():
        assert part["metrics"][k] == (got if processor._CLUSTER_KEY.fullmatch(k) else raw)["metrics"][k], k
    # the median's precondition does not apply
    calls.clear()
    flat = run(scan_filter=("gaussian", 1.0), dilate_iterations=0)
    assert len(calls) == 1 and flat["metrics"]["scan_filter"] == "gaussian1.00mm"
    assert {k: flat["metrics"][k] for k in want if processor._CLUSTER_KEY.fullmatch(k)} == \
        {k: v for k, v in want.items() if processor._CLUSTER_KEY.fullmatch(k)}      # the scan itself: no fill value in it
    # the median runs give what they gave
    calls.clear()
    med = run(scan_filter=(3, 3, 3))
    assert calls == [] and medians == [((3, 3, 3),)] and med["metrics"]["scan_filter"] == "median3x3x3"
    m3 = real_median(case["image"], (3, 3, 3))
    want_m = processor.densitometry_metrics(processor.densitometry(m3, labels, spacing), names)
    want_m.update(processor.laa_cluster_metrics(processor.laa_clusters(m3, labels, spacing), names))
    assert {k: med["metrics"][k] for k in want_m} == want_m
    assert torch.equal(med["full_cle"], raw["full_cle"])
