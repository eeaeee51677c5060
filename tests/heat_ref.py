"""fp64 restatement of the activation-map volumes (csrc/heat.hip), written from the operation's definition, with the
element-wise bound an fp32 implementation has to meet.  A plain helper module in the manner of data_path_ref.py:
tests/test_heat_host.py validates it on the CPU against the recorded reference outputs (tests/golden/heat.npz) and
the ATen fp32 composition (which has to stay within HALF the bound), tests/test_heat_gpu.py holds the HIP kernels to
it.  Every function works on the device of its inputs.

Definition.  dense [B,C,d,h,w], lung [B,D,H,W] (non-zero = lung), (D,H,W) = (2d,2h,2w).
  up_c = F.interpolate(dense[:, c], size=(D,H,W), mode='trilinear') (align_corners=False): output k of an axis samples
         the source at max(k/2 - 0.25, 0) -- weights {0.25, 0.75} ({1, 0} at k = 0), the far tap clamped to n - 1.
  "classsum"  dp = sum_{c>=1} max(up_c, 0);  v = dp / (max over the sample's volume of dp + 1e-7) * lung
  "plain"     v = up_0 * lung
  u8 = floor(255 clamp(v, 0, 1)).

Bounds (u = 2^-24).  At exactly x2 the coordinates and weights are exact in fp32, so there is no coordinate term.
  b_dp = ROUND u sum_c sum_k |w_k x_k|  (data_path_ref's rounding term of an 8-term weighted sum, per channel; max(., 0)
         is 1-Lipschitz) + u dp per channel ADDED to the sum (C - 2 additions round; C - 1 is counted).
  classsum  with m = peak + 1e-7: the peak is off by at most B = max over the volume of b_dp (|max f - max g| <=
            max |f - g|), so v is off by b_dp / m + v B / m, and the fp32 sum peak + 1e-7 and the quotient round once
            each: + 2 u v.  Times lung (exact).
  plain     b_v = b_dp + u |v| (the product with the mask is exact; u |v| is slack for a different nesting).
"""
import numpy as np
import torch
import torch.nn.functional as F

from data_path_ref import F64, ROUND, U, Ref, u8_range  # noqa: F401  (u8_range: re-exported for the tests)

MODES = ("classsum", "plain")


def taps(n_in):
    """(i0, i1, w0, w1) of the 2 n_in outputs of one axis"""
    k = torch.arange(2 * n_in, dtype=F64)
    src = (k / 2.0 - 0.25).clamp(min=0.0)
    i0 = src.floor()
    w1 = src - i0
    i0 = i0.long()
    return i0, (i0 + 1).clamp(max=n_in - 1), 1.0 - w1, w1


def up2(x):
    """x [..., d, h, w] fp64 -> its x2 trilinear up-sampling (align_corners=False)"""
    for a in (-3, -2, -1):
        i0, i1, w0, w1 = (t.to(x.device) for t in taps(x.shape[a]))
        shape = [1, 1, 1]
        shape[a] = -1
        x = x.index_select(a, i0) * w0.view(shape) + x.index_select(a, i1) * w1.view(shape)
    return x


def heat64(dense, lung, mode):
    """-> Ref(val, bound, None) [B,D,H,W] fp64 of v; u8_range(ref) gives the admissible bytes"""
    assert mode in MODES
    x = dense.to(F64)
    L = (lung != 0).to(F64)
    if mode == "plain":
        assert x.shape[1] == 1
        v = up2(x[:, 0]) * L
        return Ref(v, (ROUND * U * up2(x[:, 0].abs()) + U * v.abs()) * L, None)
    assert x.shape[1] >= 2
    dp = up2(x[:, 1:]).clamp(min=0.0).sum(1)
    b_dp = ROUND * U * up2(x[:, 1:].abs()).sum(1) + (x.shape[1] - 1) * U * dp
    m = dp.amax(dim=(1, 2, 3), keepdim=True) + 1e-7
    v = dp / m * L
    return Ref(v, (b_dp / m + v * b_dp.amax(dim=(1, 2, 3), keepdim=True) / m + 2.0 * U * v) * L, None)


def aten_heat(dense, lung, mode):
    """The reference's own composition in float32 (models.py:201-229 / :464-488) -> (v float32, u8) numpy [B,D,H,W]"""
    lung_np = (lung != 0).float().cpu().numpy()
    up = F.interpolate(dense.float().cpu(), size=lung_np.shape[-3:], mode="trilinear")
    vs = []
    for b in range(up.shape[0]):
        if mode == "classsum":
            dp = F.relu(up[b, 1:]).numpy().sum(0)
            dp = dp / (dp.max() + 1e-7)
        else:
            dp = up[b, 0].numpy()
        vs.append(dp * lung_np[b])
    v = np.stack(vs)
    assert v.dtype == np.float32
    return v, window01_u8(v)


def window01_u8(v):
    """utils.windowing(v, from_span=(0, 1)).astype(np.uint8) for a float32 array"""
    return (((np.clip(v, 0, 1) - 0) / float(1 - 0)) * (255 - 0) + 0).astype(np.uint8)


def unsure_share(ref):
    """share of voxels whose byte the bound leaves open (lo != hi)"""
    lo, hi = u8_range(ref)
    return float((lo != hi).double().mean())


def check_u8(got, ref, cap=0.005):
    """got uint8 [B,D,H,W] against the fp64 value: every byte within u8_range, bytes equal where lo == hi (the same
    statement), and at most `cap` of the voxels with lo != hi.  Returns the figures for printing."""
    lo, hi = u8_range(ref)
    g = torch.as_tensor(got).to(lo.device).to(F64)
    outside = int(((g < lo) | (g > hi)).sum())
    share = float((lo != hi).double().mean())
    return outside, share, outside == 0 and share <= cap
