"""CPU restatement, in torch, of the reference's SubtypingInference.get_data (dataset.py:57-92) + utils.find_crops
(utils.py:53-63), so that the GPU tests of transforms.prepare_case need neither scipy nor the reference.

`iterations` rounds of binary_dilation with the full 3x3x3 structure and zero border are one (2*iterations+1)^3 box
dilation clipped to the volume = max_pool3d(lung, 2r+1, stride 1, padding r) > 0 (max_pool3d pads with -inf).
tests/test_case_prep_host.py holds this file to the fixture recorded from the reference and to scipy."""
import math

import torch
import torch.nn.functional as F


def dilate(lung: torch.Tensor, iterations: int) -> torch.Tensor:
    """lung bool [D,H,W] -> bool [D,H,W]"""
    if iterations == 0:
        return lung.clone()
    k = 2 * iterations + 1
    return F.max_pool3d(lung[None, None].float(), k, 1, iterations)[0, 0] > 0


def find_crops(lung: torch.Tensor, spacing, border):
    nz = lung.nonzero()
    if nz.numel() == 0:
        raise IndexError("no lung voxel")                # find_objects(...)[0] on an empty mask
    lo, hi = nz.min(0).values.tolist(), (nz.max(0).values + 1).tolist()
    if border > 0:
        pads = [int(math.ceil(border / sp)) for sp in spacing]
        return [(max(0, a - p), min(s, b + p)) for a, b, p, s in zip(lo, hi, pads, lung.shape)]
    return list(zip(lo, hi))


def prepare_case_ref(scan, lobes, spacing, crop_border=5, dilate_iterations=2, fill_value=-2048, ess_threshold=-910):
    """CPU tensors in, the reference's dict (tensors; both int16 images always) out."""
    scan = torch.as_tensor(scan).cpu().to(torch.int16)
    lobes = torch.as_tensor(lobes).cpu()
    assert scan.shape == lobes.shape
    lung = lobes > 0
    masked = torch.where(dilate(lung, dilate_iterations), scan, torch.tensor(fill_value, dtype=torch.int16))
    sl = find_crops(lung, spacing, crop_border)
    idx = tuple(slice(a, b) for a, b in sl)
    image, lung_c = masked[idx].contiguous(), lung[idx].contiguous()
    return {"image": image, "original_image": scan[idx].contiguous(), "lung_mask": lung_c,
            "ess_mask": (image < ess_threshold) & lung_c, "crop_slice": torch.tensor(sl, dtype=torch.int64),
            "original_size": torch.tensor(list(scan.shape), dtype=torch.int64)}


# ----------------------------------------------------------------------------------------------- synthetic cases
SPECIAL_HU = (-910, -911, -2048, 32767)


def synth_scan(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1100, -700, shape, generator=g, dtype=torch.int16)


def fixture_cases():
    """name -> (scan int16, lobes, spacing, crop_border): the inputs of tests/golden/case_prep.npz, rebuilt from seeds by
    make_golden_case.py and by the tests (the fixture stores them too; the tests check that they agree)."""
    shape = (20, 44, 52)
    cases = {}
    # labels 1-5 in two blobs, anisotropic spacing
    lobes = torch.zeros(shape, dtype=torch.uint8)
    lobes[4:15, 8:30, 6:22] = 1
    lobes[4:9, 8:30, 6:22] = 2
    lobes[9:15, 20:30, 6:22] = 3
    lobes[5:16, 10:34, 29:47] = 4
    lobes[11:16, 10:34, 29:47] = 5
    scan = synth_scan(shape, 1)
    for k, hu in enumerate(SPECIAL_HU):                 # the edge values of threshold, fill and int16, inside the lung
        scan[6, 12, 8 + k] = hu
        scan[12, 25, 31 + k] = hu
    cases["blobs_u8"] = (scan, lobes, (2.5, 0.7, 0.7), 5)
    # lung voxels in two opposite corners: box, padding and dilation all clip at the volume
    lobes = torch.zeros(shape, dtype=torch.uint8)
    lobes[0, 0, 0] = 1
    lobes[-1, -1, -1] = 5
    lobes[8:12, 20:24, 24:30] = 3
    cases["corners"] = (synth_scan(shape, 2), lobes, (1.0, 1.0, 1.0), 5)
    # one interior voxel, border 5, spacing 1
    lobes = torch.zeros(shape, dtype=torch.uint8)
    lobes[10, 22, 26] = 2
    cases["single_voxel"] = (synth_scan(shape, 3), lobes, (1.0, 1.0, 1.0), 5)
    # int16 lobes (one label above 255), tight box
    lobes = torch.zeros(shape, dtype=torch.int16)
    lobes[3:17, 5:40, 4:20] = 300
    lobes[6:14, 9:33, 30:50] = 4
    scan = synth_scan(shape, 4)
    for k, hu in enumerate(SPECIAL_HU):
        scan[7, 11, 6 + k] = hu
    cases["lobes_i16"] = (scan, lobes, (0.8, 1.4, 0.6), 0)
    return cases


KEYS = ("image", "original_image", "lung_mask", "ess_mask", "crop_slice", "original_size")
