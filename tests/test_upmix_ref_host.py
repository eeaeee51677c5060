"""Host (no GPU): the fp64 yardstick of csrc/upmix.hip, tests/upmix_ref.py, against what it stands for.

  * its 1-D weights (the kernel's fp32 recipe, and the fused form of the forward kernels) against the exact rational
    align-corners operator, Ni = 1 .. 64;
  * its three-pass composite against the definition in float64: the sum over the 27 taps of
    F.interpolate(b_t, scale_factor=2, mode="trilinear", align_corners=True) shifted by the tap with zero fill, on the
    geometries of test_kernels_gpu.UPMIX_CASES, element by element within the weight bound carried through the passes;
  * its backward composite as the transpose of its forward one."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import upmix_ref as UR
from test_kernels_gpu import UPMIX_CASES

F64 = torch.float64
CO = 4


def weight_bound(Ni):
    """|A - exact| per entry: s = fl32(scale * u) carries the two roundings of scale and of the product, each at most
    2^-24 relative to s <= Ni (the subtraction s - i0 is exact, 1 - w1 rounds once more at 2^-24 at most); a floor that
    falls on the other side of an integer moves both weights by the same distance.  The fused form has one rounding
    fewer in s and one of at most 2^-24 in scale u - i0 instead: the same bound."""
    return 2.0 * Ni * 2.0 ** -24


def exact_weights(Ni):
    """the align-corners x2 operator [2 Ni, Ni] in rational arithmetic"""
    E = [[Fraction(0)] * Ni for _ in range(2 * Ni)]
    for u in range(2 * Ni):
        s = Fraction(u * (Ni - 1), 2 * Ni - 1)
        i0 = min(s.numerator // s.denominator, Ni - 1)
        i1 = i0 + (1 if i0 < Ni - 1 else 0)
        E[u][i0] += 1 - (s - i0)
        E[u][i1] += s - i0
    return E


@pytest.mark.parametrize("fused", [False, True], ids=["recipe", "fused"])
@pytest.mark.parametrize("Ni", range(1, 65))
def test_weights_against_exact_rational_weights(Ni, fused):
    A = UR.lin_weights(Ni, fused)
    assert A.shape == (2 * Ni, Ni) and A.dtype == np.float64
    E = exact_weights(Ni)
    assert all(sum(row) == 1 for row in E)
    worst = max(abs(Fraction(float(A[u, i])) - E[u][i]) for u in range(2 * Ni) for i in range(Ni))
    assert worst <= Fraction(weight_bound(Ni)), f"Ni={Ni}: {float(worst) / (Ni * 2.0 ** -24):.3f} Ni 2^-24"
    i0, i1, w0, w1 = UR.lin_terms(Ni, fused)
    assert i0.min() >= 0 and i1.max() <= Ni - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()
    # the recipe's weights lie in [0, 1]; the fused w1 is slightly negative (w0 slightly above 1) in a last row whose
    # rounded product reached Ni - 1 from below
    slack = (Ni + 1) * 2.0 ** -24 if fused else 0.0
    assert (w0 >= 0).all() and (w1 >= -slack).all() and (w0 <= 1 + slack).all()
    r = UR.lin_terms(Ni)                                          # the two forms: the same indices, weights <= (Ni + 1) 2^-24 apart
    assert (i0 == r[0]).all() and (i1 == r[1]).all()
    assert np.abs(w1.astype(np.float64) - r[3]).max() <= (Ni + 1) * 2.0 ** -24
    assert (A[0] == np.eye(Ni)[0]).all()                          # u = 0 reads element 0 alone


def shifted(M):
    """[2N, N] -> [3, 2N, N]: row v of plane k is row v + k - 1 of M, zero outside"""
    S = torch.zeros((3,) + tuple(M.shape), dtype=F64)
    S[0, 1:] = M[:-1]
    S[1] = M
    S[2, :-1] = M[1:]
    return S


def dense_gather(b, Mz, My, Mx):
    """b [B,Ds,Hs,Ws,27 CO] through dense per-axis operators with the tap shifts"""
    B, Ds, Hs, Ws, _ = b.shape
    return torch.einsum("kzd,lye,mxf,bdefklmc->bzyxc", shifted(Mz), shifted(My), shifted(Mx),
                        b.view(B, Ds, Hs, Ws, 3, 3, 3, CO))


def draw(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


GEOMS = sorted({c[:4] for c in UPMIX_CASES})


@pytest.mark.parametrize("fused", [False, True], ids=["recipe", "fused"])
@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_composite_forward_against_interpolate_in_float64(geom, fused):
    B, Ds, Hs, Ws = geom
    b = draw((B, Ds, Hs, Ws, 27 * CO), 1)
    y, mag = UR.gather_fwd_ref(b, CO, fused)
    assert y.shape == (B, 2 * Ds, 2 * Hs, 2 * Ws, CO) and y.dtype == F64
    want = torch.zeros_like(y)
    for t in range(27):
        kz, ky, kx = t // 9, (t // 3) % 3, t % 3
        bt = b[..., t * CO:(t + 1) * CO].permute(0, 4, 1, 2, 3)
        up = F.interpolate(bt, scale_factor=2, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1)
        pad = F.pad(up, (0, 0, 1, 1, 1, 1, 1, 1))                   # zero outside the volume
        want += pad[:, kz:kz + 2 * Ds, ky:ky + 2 * Hs, kx:kx + 2 * Ws]
    # the weight bound through the three passes: d = weight_bound on the joint support of A and the exact operator,
    # W = max(|A|, |exact|):  |y - want| <= (Dz Wy Wx + Wz Dy Wx + Wz Wy Dx) |b|, plus the float64 roundings of both sides
    ops = []
    for Ni in (Ds, Hs, Ws):
        A = torch.from_numpy(UR.lin_weights(Ni, fused))
        E = torch.tensor([[float(v) for v in row] for row in exact_weights(Ni)], dtype=F64)
        ops.append((torch.maximum(A.abs(), E.abs()), ((A != 0) | (E != 0)).double() * weight_bound(Ni)))
    (Wz, Dz), (Wy, Dy), (Wx, Dx) = ops
    a = b.abs()
    bound = dense_gather(a, Dz, Wy, Wx) + dense_gather(a, Wz, Dy, Wx) + dense_gather(a, Wz, Wy, Dx)
    bound = bound + 1e-13 * dense_gather(a, Wz, Wy, Wx)
    err = (y - want).abs()
    assert bool((err <= bound).all()), f"{geom}: exceeds the weight bound by {float((err - bound).max()):.3e}"
    # the absolute sum is the same composite of |b| (all weights of the recipe are >= 0)
    assert bool((mag >= y.abs() * (1 - 1e-14)).all())
    if not fused:
        assert torch.allclose(mag, UR.gather_fwd_ref(a, CO)[0], rtol=1e-14, atol=0.0)
    # ... and the yardstick's own dense operators give the same result to float64 rounding
    A3 = [torch.from_numpy(UR.lin_weights(Ni, fused)) for Ni in (Ds, Hs, Ws)]
    assert bool(((y - dense_gather(b, *A3)).abs() <= 1e-13 * mag).all())


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_backward_composite_is_the_transpose(geom):
    B, Ds, Hs, Ws = geom
    b = draw((B, Ds, Hs, Ws, 27 * CO), 2)
    g = draw((B, 2 * Ds, 2 * Hs, 2 * Ws, CO), 3)
    y, _ = UR.gather_fwd_ref(b, CO)
    h, hm = UR.gather_bwd_ref(g, CO)
    assert h.shape == b.shape and bool((h.abs() <= hm * (1 + 1e-14)).all())
    lhs, rhs = float((y * g).sum()), float((b * h).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


def test_per_pass_layouts_and_absent_terms():
    """one pass by hand at Ni = 1 (scale 0: both rows read element 0; row 0 has no k = 0 term, row 1 no k = 2 term) and
    the IEEE rule: a zero weight inside the range times Inf is NaN, a term outside the range is absent"""
    In = torch.tensor([1.0, 10.0, 100.0], dtype=F64).view(1, 1, 1, 3, 1)
    out, mag = UR.axis_fwd_ref(In, 1, 1, 1)
    assert out.flatten().tolist() == [110.0, 11.0] and mag.flatten().tolist() == [110.0, 11.0]
    H, _ = UR.axis_bwd_ref(torch.tensor([2.0, 3.0], dtype=F64).view(1, 2, 1, 1), 1, 1, 1)
    assert H.flatten().tolist() == [3.0, 5.0, 2.0]
    In = In.clone()
    In[0, 0, 0, 0, 0] = float("inf")                                # k = 0: absent from row 0; in row 1 with w0 = 1, w1 = 0
    out, _ = UR.axis_fwd_ref(In, 1, 1, 1)
    assert float(out[0, 0, 0, 0]) == 110.0 and torch.isnan(out[0, 1, 0, 0])           # 1 * Inf + 0 * Inf
    In2 = torch.ones((1, 2, 1, 3, 1), dtype=F64)
    In2[0, 1, 0, 1, 0] = float("inf")                               # element 1, centre tap: weight 0 in row u = 0
    out, _ = UR.axis_fwd_ref(In2, 2, 1, 1)
    assert torch.isnan(out[0, 0, 0, 0]) and float(out[0, 1, 0, 0]) == float("inf")     # u = 0: 1 * 1 + 0 * Inf; u = 1: 1/3 Inf
