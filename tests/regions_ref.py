"""fp64 yardstick, in torch on the CPU, of the regional predict tail (csrc/regions.hip).  The reference has no regional
code; the definition is the project's own, chosen so that it reduces to the reference's per-lung number:

  o      = F.interpolate(dense -> size, trilinear, align_corners=True) * (ess != 0)
  T[b,r] = (sum o_cle, sum o_pse, #(ess != 0), #voxels) over labels == r, r = 0..n; row 0 also takes labels above n
  pct    = T.sum / T.#voxels per sample and region (NaN for a region without voxels)

and the label resize is the masks' nearest rule: depth through linspace(0, D-1, Do).long(), min(floor(dst * in/out),
in - 1) in plane (fp32 scale: fp32 IS the specification there, as in data_path_ref.nearest_index), clamped to a byte.
A plain helper module; tests/test_regions_host.py holds the resize to the oracle's mask resize."""
import torch
import torch.nn.functional as F

import data_path_ref as R

U = 2.0 ** -24
F64 = torch.float64


def upproject64(dense, ess, size):
    """dense [B,D,H,W], ess [B,*size] (any dtype, non-zero = 1) -> float64 [B,*size]"""
    up = F.interpolate(dense.to(F64)[:, None], size=tuple(size), mode="trilinear", align_corners=True)[:, 0]
    return up * (ess != 0).to(F64)


def element_bound(dense, ess):
    """test_upproject_grid_stride's bound on one stored element: the fp32 source-position error on each axis
    (<= 2 u (n - 1) + u) times the spread of dense, plus 8 u max |dense|; 0 where ess is 0 (the product is exact)."""
    D, H, W = dense.shape[-3:]
    spread = float(dense.max() - dense.min())
    pos = sum(2 * U * (n - 1) + U for n in (D, H, W))
    return (pos * spread + 8 * U * float(dense.abs().max())) * (ess != 0).to(F64)


def rows_of(labels, n):
    """the table row of each voxel: the label, 0 for labels above n"""
    lab = labels.long()
    return torch.where(lab > n, torch.zeros_like(lab), lab)


def label_sums(vol, labels, n):
    """vol [B,...] -> [B, n+1] float64 sums of vol over the voxels of each row"""
    B = vol.shape[0]
    out = torch.zeros((B, n + 1), dtype=F64)
    return out.scatter_add_(1, rows_of(labels, n).reshape(B, -1), vol.to(F64).reshape(B, -1))


def table64(o_cle, o_pse, ess, labels, n):
    """-> [B, n+1, 4] float64: sums of the two given volumes, #(ess != 0), #voxels per row"""
    e = (ess != 0).to(F64)
    return torch.stack([label_sums(o_cle, labels, n), label_sums(o_pse, labels, n), label_sums(e, labels, n),
                        label_sums(torch.ones_like(e), labels, n)], -1)


def percentages(table):
    """[B, n+1, 4] -> (cle, pse) [B, n]: sum / #voxels of the regions 1..n, NaN where a region has no voxel"""
    vox = table[:, 1:, 3]
    return table[:, 1:, 0] / vox, table[:, 1:, 1] / vox


def resize_labels(labels, target):
    """labels [D,H,W] integer -> uint8 [Do,Ho,Wo]: nearest resize (depth indices + floor rule), clamped to 0..255"""
    return R.prep_mask_ref(labels, target).clamp(0, 255).to(torch.uint8)
