"""CPU: the fp64 references and element-wise bounds of tests/data_path_ref.py, validated WITHOUT the code under test.

The committed ATen fp32 oracle (oracle/med3d_oracle.py: prepare_image, prepare_mask, paste_resampled, window_u8,
gaussian_additive, box_mask_out, flip, crop_and_resize) and the fixtures recorded from the reference's own classes
(transforms.npz, processor.npz, augment.npz) must stay within HALF of every bound, at every shape
tests/test_data_path_gpu.py runs: that fixes the constants of the bounds.  Masks are exact, but for the near-tie rule
of the nearest crop, whose census per crop case is asserted here from the fp64 coordinates alone.

Measured ATen-to-bound ratios (max over elements of |aten - ref64| / bound; printed by this file under pytest -s):
prepare_image 0.45 at 9x130x97 -> 17x250x250 (coordinate term), <= 0.06 at the small shapes, transforms.npz 0.30;
paste 0.48 (8x56x72 -> 15x247x249), 0.36 (down-sampling), <= 0.14 at the edge shapes, processor.npz 0.23;
augment 0.30 (noise stage alone), <= 0.09 with the crop at 9x11x13, 0.03 (16x32x32, ten boxes), 0.16 (17x250x250),
0.10 through the zero padding of a box outside [0, 1], augment.npz 0.35 (noise) / 0.13 (crop).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import data_path_ref as R
from conftest import GOLDEN
from oracle import med3d_oracle as orc

params, subset_params, direct_struct, SUBSETS, FLIPS = R.params, R.subset_params, R.direct_struct, R.SUBSETS, R.FLIPS

HALF = 0.5
DTYPES = (torch.bool, torch.uint8, torch.int16)


def within_half(got, ref, what):
    r = R.ratio(got, ref)
    print(f"[aten/bound] {what}: {r:.3f}")
    assert r <= HALF, f"{what}: ATen fp32 at {r:.3f} of the bound (must stay within {HALF})"
    return r


# ------------------------------------------------------------------------------------------------ prepare
@pytest.mark.parametrize("case", R.PREP_CASES, ids=[c[0] for c in R.PREP_CASES])
def test_prepare_references_agree_with_aten(case):
    cid, src, tgt = case
    scan = R.scan_volume(src, 11)
    within_half(orc.prepare_image(scan, tgt), R.prep_image64(scan, tgt), f"prepare_image {cid}")
    for k, dt in enumerate(DTYPES):
        m = R.mask_volume(src, 20 + k, dt)
        ref = R.prep_mask_ref(m, tgt)
        assert ref.dtype == dt and torch.equal(orc.prepare_mask(m, tgt), ref), (cid, dt)


def test_prepare_references_agree_with_transforms_fixture():
    z = np.load(os.path.join(GOLDEN, "transforms.npz"))
    tgt = tuple(int(v) for v in z["target"])
    within_half(torch.from_numpy(z["image_out"]), R.prep_image64(torch.from_numpy(z["scan"]), tgt), "transforms.npz")
    assert torch.equal(R.prep_mask_ref(torch.from_numpy(z["mask"]), tgt), torch.from_numpy(z["mask_out"]))


# ------------------------------------------------------------------------------------------------ paste
def check_u8(u8, ref, what):
    lo, hi = R.u8_range(ref)
    bad = int(((u8.double() < lo) | (u8.double() > hi)).sum())
    assert bad == 0, f"{what}: {bad} uint8 voxels outside floor(255 clamp01(v -+ b))"


@pytest.mark.parametrize("case", R.PASTE_CASES, ids=[c[0] for c in R.PASTE_CASES])
def test_paste_reference_agrees_with_aten(case):
    cid, shape, crop, original = case
    for name, dense in R.dense_volumes(shape, 31):
        ref = R.paste64(dense, crop, original)
        full = orc.paste_resampled(dense, crop, original)
        within_half(full, ref, f"paste {cid} {name}")
        check_u8(orc.window_u8(full), ref, f"paste {cid} {name}")
        if cid == "whole":
            assert torch.equal(ref.val, dense.double()) and torch.equal(full, dense)


def test_paste_reference_agrees_with_processor_fixture():
    g = np.load(os.path.join(GOLDEN, "processor.npz"))
    ref = R.paste64(torch.from_numpy(g["dense"][0]), g["crop"], g["original"])
    within_half(torch.from_numpy(g["full"]), ref, "processor.npz")
    check_u8(torch.from_numpy(g["full_u8"]), ref, "processor.npz")


# ------------------------------------------------------------------------------------------------ augmentations
def aten_image(img, noise, ap):
    x = img
    if ap.noise_sigma is not None:
        x = orc.gaussian_additive(x, ap.noise_sigma, noise)
    if ap.box_centers:
        x = orc.box_mask_out(x, ap.box_centers, ap.box_sizes)
    if ap.flip_dims:
        x = orc.flip(x, ap.flip_dims)
    if ap.crop_center is not None:
        x = orc.crop_and_resize(x, ap.crop_center, ap.crop_size)
    return x


def aten_mask(mask, ap):
    m = mask
    if ap.flip_dims:
        m = orc.flip(m, ap.flip_dims)
    if ap.crop_center is not None:
        m = orc.crop_and_resize(m, ap.crop_center, ap.crop_size, mask=True)
    return m


def check_chain(shape, ap, what, seed=41):
    img, noise = R.image_volume(shape, seed)
    a = ap.to_struct(shape)
    r = within_half(aten_image(img, noise, ap), R.augment_image64(img, noise, a), what)
    for k, dt in enumerate((torch.bool, torch.int16)):
        m = R.mask_volume(shape, 50 + k, dt)
        ref = R.augment_mask_ref(m, a)
        assert ref.val.dtype == dt
        assert R.mask_rule_violations(aten_mask(m, ap), ref) == 0, (what, dt)
    return r


@pytest.mark.parametrize("subset", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_augment_references_agree_with_aten_every_subset(subset):
    check_chain(R.SMALL, subset_params(R.SMALL, subset), "augment " + "+".join(subset))


@pytest.mark.parametrize("flip", FLIPS, ids=["".join(map(str, f)) for f in FLIPS])
def test_augment_references_agree_with_aten_every_flip(flip):
    check_chain(R.SMALL, subset_params(R.SMALL, ("flip",), flip), f"flip {flip}")
    check_chain(R.SMALL, subset_params(R.SMALL, ("noise", "boxes", "flip", "crop"), flip), f"chain, flip {flip}")


def test_augment_references_agree_with_aten_ten_boxes_and_over_cap():
    ap = params(R.MID, True, R.TEN_BOXES, (1, 2), R.CROP_MID)
    boxes = [tuple(ap.to_struct(R.MID).boxes[b]) for b in range(10)]
    assert any(b[0] == 0 for b in boxes) and any(b[1] == 16 for b in boxes)            # clipped by the faces
    assert any(b[0] == b[1] for b in boxes)                                            # int(ms * ds) == 0: empty
    check_chain(R.MID, ap, "ten boxes 16x32x32")
    check_chain(R.OVER, params(R.OVER, True, R.OVER_BOXES, (1,), R.CROP_OVER), "chain 17x250x250")


def test_constant_volume_reference():
    img = torch.full(R.SMALL, 3.25)
    ref = R.augment_image64(img, R.image_volume(R.SMALL, 3)[1], params(R.SMALL, True).to_struct(R.SMALL))
    assert torch.equal(ref.val, img.double())


def aten_grid(t, a, mask):
    """functional.roi_align on the struct's normalised box"""
    box = torch.tensor([[a.box_lo[k], a.box_hi[k]] for k in range(3)], dtype=torch.float32).flip(0)
    theta = torch.cat([torch.diag(box[:, 1] - box[:, 0]), (-1.0 + box.sum(-1))[:, None]], dim=-1)[None]
    grid = F.affine_grid(theta, (1, 1) + tuple(t.shape), align_corners=False)
    out = F.grid_sample(t[None, None].float(), grid, mode="nearest" if mask else "bilinear", padding_mode="zeros",
                        align_corners=not mask)
    return out[0, 0].to(t.dtype)


@pytest.mark.parametrize("flags", [8, 15])
def test_zero_padding_references_agree_with_aten(flags):
    """a box outside [0, 1]: samples beyond every face, the padding_mode='zeros' branches"""
    img, noise = R.image_volume(R.SMALL, 43)
    a = direct_struct(flags)
    ap = params(R.SMALL, True, R.SMALL_BOXES, (0, 1, 2))
    pre = aten_image(img, noise, ap) if flags == 15 else img
    ref = R.augment_image64(img, noise, a)
    assert float((ref.coords[0] < -1).sum()) > 0 and float((ref.coords[1] > R.SMALL[1]).sum()) > 0
    within_half(aten_grid(pre, a, False), ref, f"zero padding flags={flags}")
    for k, dt in enumerate((torch.bool, torch.int16)):
        m = R.mask_volume(R.SMALL, 50 + k, dt)
        got = aten_grid(orc.flip(m, (0, 1, 2)) if flags == 15 else m, a, True)
        assert R.mask_rule_violations(got, R.augment_mask_ref(m, a)) == 0


def test_exact_ties_round_half_to_even():
    """the exact-tie box of data_path_ref.exact_tie_struct: frac(pix64) is exactly 1/2 along x and 0 along z and y, and
    ATen's nearbyint picks the even neighbour, as augment_mask_ref does"""
    a = R.exact_tie_struct()
    m = torch.arange(1, 1 + 16 * 32 * 32, dtype=torch.float32).view(R.MID)
    ref = R.augment_mask_ref(m, a)
    k = torch.arange(32, dtype=torch.float64)
    assert torch.equal(ref.coords[2], k + 0.5) and torch.equal(ref.coords[1], k) and torch.equal(ref.coords[0], k[:16])
    want = torch.where(k % 2 == 0, k, k + 1).long()
    assert torch.equal(ref.cands[1][2][0], want)
    assert torch.equal(aten_grid(m, a, True), ref.val)
    assert bool((ref.val[..., 31] == 0).all()) and torch.equal(ref.val[..., 1], m[..., 2])


def test_augment_references_agree_with_augment_fixture():
    g = np.load(os.path.join(GOLDEN, "augment.npz"))
    img, mask = torch.from_numpy(g["image"]), torch.from_numpy(g["mask"])
    torch.manual_seed(int(g["noise_seed"]))
    noise = torch.randn(img.shape)
    cen, siz = [tuple(c) for c in g["box_centers"]], [tuple(c) for c in g["box_sizes"]]
    fl = tuple(int(v) for v in g["flip_dims"])
    kw = dict(noise_sigma=float(g["noise_sigma"]))
    steps = [("after_noise", dict(kw)), ("after_box", dict(kw, box_centers=cen, box_sizes=siz)),
             ("after_flip", dict(kw, box_centers=cen, box_sizes=siz, flip_dims=fl)),
             ("after_crop", dict(kw, box_centers=cen, box_sizes=siz, flip_dims=fl, crop_center=tuple(g["crop_center"]),
                                 crop_size=tuple(g["crop_size"])))]
    for key, k in steps:
        a = R.transforms().AugmentParams(**k).to_struct(img.shape)
        within_half(torch.from_numpy(g[key]), R.augment_image64(img, noise, a), f"augment.npz {key}")
    a = R.transforms().AugmentParams(**steps[2][1]).to_struct(img.shape)
    assert torch.equal(R.augment_mask_ref(mask, a).val, torch.from_numpy(g["mask_after_flip"]))
    a = R.transforms().AugmentParams(**steps[3][1]).to_struct(img.shape)
    assert R.mask_rule_violations(torch.from_numpy(g["mask_after_crop"]), R.augment_mask_ref(mask, a)) == 0


# ------------------------------------------------------------------------------------------------ near-tie census
def test_near_tie_census_of_the_mask_crop_cases():
    """from the fp64 coordinates alone: the crops at 17x250x250 and 16x32x32 have NO voxel within 1e-4 of a rounding
    tie (every mask comparison there is exact); the 9x11x13 crop is the tie case: 19 % of its voxels are near ties, and
    ATen's own fp32 coordinates round 9.6 % of all voxels to the other side of rint(pix64)."""
    frac = {}
    for shape, crop in ((R.OVER, R.CROP_OVER), (R.MID, R.CROP_MID), (R.SMALL, R.CROP_TIE)):
        ap = params(shape, crop=crop)
        m = R.mask_volume(shape, 7, torch.int16)
        ref = R.augment_mask_ref(m, ap.to_struct(shape))
        frac[shape] = float(ref.near.float().mean())
        if shape == R.SMALL:
            idx = torch.arange(m.numel(), dtype=torch.float32).view(shape)           # which source voxel, not its label
            ref_i = R.augment_mask_ref(idx, ap.to_struct(shape))
            got = aten_mask(idx, ap)
            differs = float((got != ref_i.val).float().mean())
            assert bool(((got == ref_i.val) | ref_i.near).all())
            assert R.mask_rule_violations(got, ref_i) == 0
    print(f"[census] {frac}, ATen differs from rint(pix64) on {differs:.3f}")
    assert frac[R.OVER] == 0.0 and frac[R.MID] == 0.0
    assert round(frac[R.SMALL], 2) == 0.19
    assert 0.05 < differs < 0.19
