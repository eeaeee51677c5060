"""GPU: the five kernels of csrc/prep.hip between a CT scan and the network, and between the network and the written
result -- prep_image, prep_mask, resample_paste, augment_image, augment_mask -- element by element against the fp64
references of tests/data_path_ref.py, in the form production runs (above the 4096 x 256 grid cap every thread strides)
and at the edges of their parameter space: extents and source axes of length 1, identity, crops on the far faces,
every subset of the augmentation chain, every flip set, clipped / empty / overlapping boxes, d_range == 0, and the
zero-padding branches only a caller of the C entry points reaches.

Every case runs with torch.empty / torch.empty_like poisoned (floats NaN, uint8 0xFF): an unwritten voxel fails.
Floating outputs are held to the element-wise bounds derived in data_path_ref.py (rounding term + coordinate term; the
CPU tests hold ATen fp32 within half of each), masks exactly, but for the near-tie rule of the nearest crop.
Every test prints its largest kernel-to-bound ratio (pytest -s).
"""
import ctypes
import math
import random

import pytest
import torch

import data_path_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    """torch.empty / torch.empty_like return poisoned memory for the duration of a test: floating tensors NaN, uint8
    tensors 0xFF."""
    e0, el0 = torch.empty, torch.empty_like

    def fill(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(255)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(e0(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(el0(*a, **k)))
    yield
    torch.cuda.synchronize()


def T():
    return R.transforms()


def within(got, ref, what):
    assert got.dtype == torch.float32 and got.shape == ref.val.shape, what
    r = R.ratio(got, ref)
    print(f"[kernel/bound] {what}: {r:.3f}")
    assert r <= 1.0, f"{what}: {r:.3f} of the element-wise bound"
    return r


def over_cap(shape):
    assert math.prod(shape) > 4096 * 256          # above the grid cap: the grid-stride loop runs, ragged second stride


# ------------------------------------------------------------------------------------------------ prepare
@pytest.mark.parametrize("case", R.PREP_CASES, ids=[c[0] for c in R.PREP_CASES])
def test_prepare_image(ops, case):
    """window + z-score + bilinear align_corners=True in-plane + depth selection against prep_image64: per element
    inv (18 u (sum |w_k x_k| + mean) + 2 u (H G_y + W G_x)) + the propagated fp32 statistics + 2 u |result|
    (data_path_ref.prep_image64).  ATen fp32 stays at <= 0.45 of this bound (tests/test_data_path_ref.py)."""
    cid, src, tgt = case
    if cid == "over":
        over_cap(tgt)
    scan = R.scan_volume(src, 11).to(DEV)
    within(T().prepare_image(scan, tgt), R.prep_image64(scan, tgt), f"prepare_image {cid}")


@pytest.mark.parametrize("case", R.PREP_CASES, ids=[c[0] for c in R.PREP_CASES])
def test_prepare_mask(ops, case):
    """nearest in-plane by ATen's fp32 index rule + depth selection: exact, dtype preserved (bool, uint8, int16 with
    negative labels and +-32767)."""
    cid, src, tgt = case
    if cid == "over":
        over_cap(tgt)
    for k, dt in enumerate((torch.bool, torch.uint8, torch.int16)):
        m = R.mask_volume(src, 20 + k, dt)
        got = T().prepare_mask(m.to(DEV), tgt)
        assert got.dtype == dt and torch.equal(got.cpu(), R.prep_mask_ref(m, tgt)), (cid, dt)


# ------------------------------------------------------------------------------------------------ resample + paste
@pytest.mark.parametrize("case", R.PASTE_CASES, ids=[c[0] for c in R.PASTE_CASES])
def test_resample_paste(ops, case):
    """trilinear align_corners=True to the crop extent, pasted into zeros, against paste64: inside the crop
    16 u sum |w_k x_k| + 2 u (D G_z + H G_y + W G_x) per element (ATen fp32: <= 0.49 of it, reached at the 17x250x250
    up-sampling); outside the crop bit-pattern +0.0 / 0; uint8 within floor(255 clamp01(v -+ bound)); the u8-only and
    f32-only forms bit-identical to the combined one; a whole-grid crop of a same-size volume returns its input."""
    from bodyct_dram_emph_subtype_amd import processor
    cid, shape, crop, original = case
    if cid == "over":
        over_cap(original)
    inside = torch.zeros(original, dtype=torch.bool, device=DEV)
    inside[tuple(slice(a, b) for a, b in crop)] = True
    for name, dense in R.dense_volumes(shape, 31):
        dense = dense.to(DEV)
        ref = R.paste64(dense, crop, original)
        f32, u8 = processor.resample_paste(dense, crop, original, True, True)
        within(f32, ref, f"resample_paste {cid} {name}")
        assert bool((f32.view(torch.int32)[~inside] == 0).all()) and bool((u8[~inside] == 0).all())
        lo, hi = R.u8_range(ref)
        assert u8.dtype == torch.uint8 and int(((u8.double() < lo) | (u8.double() > hi)).sum()) == 0
        f_only, none = processor.resample_paste(dense, torch.tensor(crop), torch.tensor(original), True, False)
        assert none is None and torch.equal(f_only.view(torch.int32), f32.view(torch.int32))
        none, u_only = processor.resample_paste(dense, crop, original, False, True)
        assert none is None and torch.equal(u_only, u8)
        if cid == "whole":
            assert torch.equal(f32.view(torch.int32), dense.view(torch.int32))


# ------------------------------------------------------------------------------------------------ augmentations
def check_image(got, img, noise, a, what):
    return within(got, R.augment_image64(img, noise, a), what)


def check_mask(got, m, a, what, expect_no_ties=False):
    ref = R.augment_mask_ref(m, a)
    assert got.dtype == m.dtype and got.shape == m.shape, what
    if expect_no_ties:
        assert not bool(ref.near.any()), what
        assert torch.equal(got, ref.val), what
    bad = R.mask_rule_violations(got, ref)
    assert bad == 0, f"{what}: {bad} voxels equal none of their candidates"


def check_chain(shape, ap, what, seed=41, expect_no_ties=False):
    """augment_image against augment_image64 (noise stage 2 u (d_range (3 |q| + 2 |s| + |r|) + |v|), boxes and flip
    exact, crop stage 16 u sum |w_k x_k| + 7 u sum_a N_a G_a + the interpolated source bounds); augment_mask (bool and
    int16) by the mask rule: equal to augment_mask_ref outside the near-tie set, one of the candidates inside it."""
    img, noise = (t.to(DEV) for t in R.image_volume(shape, seed))
    a = ap.to_struct(shape)
    check_image(T().augment_image(img, ap, noise if a.flags & 1 else None), img, noise, a, what)
    for k, dt in enumerate((torch.bool, torch.int16)):
        m = R.mask_volume(shape, 50 + k, dt).to(DEV)
        got = T().augment_mask(m, ap)
        if not a.flags & 12:
            assert got is m
        else:
            check_mask(got, m, a, f"{what} mask {dt}", expect_no_ties)


@pytest.mark.parametrize("subset", R.SUBSETS, ids=["+".join(s) for s in R.SUBSETS])
def test_augment_every_subset(ops, subset):
    """9x11x13, every non-empty subset of {noise, boxes, flip (x, z), crop}; the crop is the near-tie case (19 % of
    the voxels within 1e-4 of a rounding tie).  ATen fp32: <= 0.31 of the image bound."""
    check_chain(R.SMALL, R.subset_params(R.SMALL, subset), "augment " + "+".join(subset))


@pytest.mark.parametrize("flip", R.FLIPS, ids=["".join(map(str, f)) for f in R.FLIPS])
def test_augment_every_flip_set(ops, flip):
    """each of the 7 flip sets alone (exact) and in the full chain"""
    check_chain(R.SMALL, R.subset_params(R.SMALL, ("flip",), flip), f"flip {flip}")
    check_chain(R.SMALL, R.subset_params(R.SMALL, ("noise", "boxes", "flip", "crop"), flip), f"chain, flip {flip}")


def test_augment_ten_boxes(ops):
    """16x32x32, ten boxes: clipped by the near and far faces (centres 0.02, 0.99), one empty (int(0.01 * 16) == 0),
    two overlapping; full chain.  No near ties (CPU census): masks exact.  ATen fp32: 0.03 of the image bound."""
    check_chain(R.MID, R.params(R.MID, True, R.TEN_BOXES, (1, 2), R.CROP_MID), "ten boxes 16x32x32", expect_no_ties=True)
    check_chain(R.MID, R.params(R.MID, False, R.TEN_BOXES), "ten boxes alone")


def test_augment_image_over_cap(ops):
    """17x250x250, noise + boxes + y flip + crop through the grid-stride loop.  ATen fp32: 0.16 of the bound."""
    over_cap(R.OVER)
    ap = R.params(R.OVER, True, R.OVER_BOXES, (1,), R.CROP_OVER)
    img, noise = (t.to(DEV) for t in R.image_volume(R.OVER, 41))
    check_image(T().augment_image(img, ap, noise), img, noise, ap.to_struct(R.OVER), "augment_image 17x250x250")


def test_augment_mask_over_cap(ops):
    """17x250x250, y flip + crop through the grid-stride loop; no near ties (CPU census): exact."""
    over_cap(R.OVER)
    ap = R.params(R.OVER, True, R.OVER_BOXES, (1,), R.CROP_OVER)
    for k, dt in enumerate((torch.bool, torch.int16)):
        m = R.mask_volume(R.OVER, 50 + k, dt).to(DEV)
        check_mask(T().augment_mask(m, ap), m, ap.to_struct(R.OVER), f"augment_mask 17x250x250 {dt}", expect_no_ties=True)


def test_constant_volume_with_noise_is_that_constant(ops):
    """d_range == 0: (v - d_min) / 1e-7 = 0, the clipped noise times a zero range, plus d_min"""
    img = torch.full(R.SMALL, 3.25, device=DEV)
    noise = R.image_volume(R.SMALL, 3)[1].to(DEV)
    for ap in (R.params(R.SMALL, True), R.params(R.SMALL, True, flip=(1,))):
        assert torch.equal(T().augment_image(img, ap, noise), img)


@pytest.mark.parametrize("flags", [8, 15])
def test_c_entry_points_zero_padding(ops, flags):
    """dram_augment_image / dram_augment_mask with a hand-filled DramAugment whose box leaves [0, 1] (box_lo
    (-0.2, 0.1, -0.05), box_hi (0.9, 1.3, 1.1)): the padding_mode='zeros' branches, alone and behind noise, boxes and all
    three flips; same bounds and mask rule.  ATen fp32: <= 0.10 of the image bound."""
    L = ops._L()
    D, H, W = R.SMALL
    a = R.direct_struct(flags)
    img, noise = (t.to(DEV) for t in R.image_volume(R.SMALL, 43))
    mm = torch.stack([img.min(), img.max()]).contiguous()
    out = torch.empty_like(img)
    rc = L.dram_augment_image(ops._p(img), ops._p(noise), ops._p(mm), ops._p(out), D, H, W, ctypes.byref(a), ops._stream())
    assert rc == 0
    ref = R.augment_image64(img, noise, a)
    assert bool((ref.coords[0] < -1).any()) and bool((ref.coords[1] > H).any())       # whole rows of padding
    within(out, ref, f"dram_augment_image flags={flags}")
    for k, dt in enumerate((torch.bool, torch.int16)):
        m = R.mask_volume(R.SMALL, 50 + k, dt).to(DEV)
        mf = m.float().contiguous()
        mo = torch.empty_like(mf)
        assert L.dram_augment_mask(ops._p(mf), ops._p(mo), D, H, W, ctypes.byref(a), ops._stream()) == 0
        check_mask(mo.to(dt), m, a, f"dram_augment_mask flags={flags} {dt}")


def test_c_entry_point_exact_ties_round_half_to_even(ops):
    """dram_augment_mask at coordinates that are EXACTLY k + 1/2 in fp64 and in fp32 (data_path_ref.exact_tie_struct):
    nearest means round-half-to-even there, as ATen's nearbyint (tests/test_data_path_ref.py) -- the one place the mask
    rule's tolerance for either side of a NEAR tie does not apply."""
    L = ops._L()
    D, H, W = R.MID
    a = R.exact_tie_struct()
    m = torch.arange(1, 1 + D * H * W, dtype=torch.float32, device=DEV).view(R.MID)
    out = torch.empty_like(m)
    assert L.dram_augment_mask(ops._p(m), ops._p(out), D, H, W, ctypes.byref(a), ops._stream()) == 0
    ref = R.augment_mask_ref(m, a)
    assert torch.equal(ref.coords[2], torch.arange(W, dtype=torch.float64, device=DEV) + 0.5)
    assert torch.equal(out, ref.val)


def test_c_entry_points_refuse_bad_arguments(ops):
    """return codes only (nothing is launched): n_boxes = 11 and out == x are DRAM_ERR_BAD_ARG"""
    L, lib = ops._L(), ops._lib
    D, H, W = R.SMALL
    img = torch.zeros(R.SMALL, device=DEV)
    out = torch.zeros(R.SMALL, device=DEV)
    mm = torch.zeros(2, device=DEV)
    good, bad = R.direct_struct(8), R.direct_struct(8)
    bad.n_boxes = 11
    st = ops._stream()
    assert lib.DRAM_ERR_BAD_ARG == -1
    assert L.dram_augment_image(ops._p(img), ops._p(img), ops._p(mm), ops._p(out), D, H, W, ctypes.byref(bad), st) == -1
    assert L.dram_augment_mask(ops._p(img), ops._p(out), D, H, W, ctypes.byref(bad), st) == -1
    assert L.dram_augment_image(ops._p(img), ops._p(out), ops._p(mm), ops._p(img), D, H, W, ctypes.byref(good), st) == -1
    assert L.dram_augment_mask(ops._p(img), ops._p(img), D, H, W, ctypes.byref(good), st) == -1
    torch.cuda.synchronize()
    assert not bool(out.any())


def test_train_augment_applies_one_draw_to_image_and_masks(ops):
    """TrainAugment(p=1.0, rng=random.Random(0)) on a sample dict equals augment_image / augment_mask with the
    parameters a twin generator draws and the noise drawn after the same torch.manual_seed; image and both masks carry
    the same flip and crop (held against the references with those parameters)."""
    tr = T()
    ap = tr.TrainAugment(p=1.0, rng=random.Random(0)).draw()
    assert ap.noise_sigma is not None and ap.box_centers and ap.flip_dims and ap.crop_center is not None
    img = R.image_volume(R.MID, 61)[0].to(DEV)
    lung = R.mask_volume(R.MID, 62, torch.bool).to(DEV)
    lesion = R.mask_volume(R.MID, 63, torch.int16).to(DEV)
    torch.manual_seed(5)
    out = tr.TrainAugment(p=1.0, rng=random.Random(0))({"image": img, "lung_mask": lung, "lesion_mask": lesion, "label": 2})
    torch.manual_seed(5)
    noise = torch.randn(img.shape, device=img.device)
    assert out["label"] == 2
    assert torch.equal(out["image"], tr.augment_image(img, ap, noise))
    a = ap.to_struct(R.MID)
    check_image(out["image"], img, noise, a, "TrainAugment image")
    for key, m in (("lung_mask", lung), ("lesion_mask", lesion)):
        assert torch.equal(out[key], tr.augment_mask(m, ap))
        check_mask(out[key], m, a, f"TrainAugment {key}")
