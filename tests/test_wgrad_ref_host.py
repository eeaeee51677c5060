"""Host: the fp64 weight-gradient references of tests/wgrad_ref.py (which tests/test_wgrad_forms_gpu.py holds the HIP
kernels to) against torch.autograd.grad of F.conv3d in float64 -- bit for bit on integer operands, where every sum is
exact in any order, and within 1e-12 A_w on normal operands."""
import pytest
import torch
import torch.nn.functional as F

from wgrad_ref import gt_abs, out_extent, wgrad_reference, wino_reference

F64 = torch.float64

GEOMS = [
    # B, D, H, W, Cin, Cout, k, stride, pad, dil     (every extent ragged against 2, 8 and 32)
    (2, 5, 11, 13, 3, 4, 3, 1, 1, 1),
    (1, 1, 9, 1, 2, 3, 3, 1, 1, 1),                 # extents of one: most taps are padding
    (2, 5, 9, 7, 3, 2, 3, 1, 2, 2),
    (1, 6, 10, 9, 2, 3, 3, 1, 4, 4),
    (1, 2, 5, 3, 2, 2, 3, 1, 4, 4),                 # dilation beyond the extents: whole taps are padding
    (1, 9, 11, 13, 3, 2, 3, 2, 1, 1),               # stride 2 on odd extents
    (2, 4, 6, 35, 2, 3, 3, 2, 1, 1),                # stride 2 on even extents (the last input row / column is unused)
    (2, 3, 7, 5, 4, 3, 1, 1, 0, 1),
]


def operands(geom, integer):
    B, D, H, W, Ci, Co, k, s, pad, dil = geom
    oshape = tuple(out_extent(n, k, s, pad, dil) for n in (D, H, W))
    g = torch.Generator().manual_seed(sum(geom))
    if integer:
        x = torch.randint(-1, 2, (B, D, H, W, Ci), generator=g).double()
        dy = torch.randint(-1, 2, (B,) + oshape + (Co,), generator=g).double()
    else:
        x = torch.randn((B, D, H, W, Ci), generator=g, dtype=F64)
        dy = torch.randn((B,) + oshape + (Co,), generator=g, dtype=F64)
    return x, dy


def autograd_dw(x, dy, geom):
    B, D, H, W, Ci, Co, k, s, pad, dil = geom
    w = torch.zeros((Co, Ci, k, k, k), dtype=F64, requires_grad=True)
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w, None, s, pad, dil)
    (dw,) = torch.autograd.grad(y, [w], dy.permute(0, 4, 1, 2, 3))
    return dw


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_tap_loop_equals_autograd_exactly_on_integer_data(geom):
    x, dy = operands(geom, True)
    dw, none = wgrad_reference(x, dy, *geom[6:])
    assert none is None and dw.dtype == F64
    want = autograd_dw(x, dy, geom)
    assert float(want.abs().max()) > 0
    assert torch.equal(dw, want)


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_tap_loop_equals_autograd_on_normal_data(geom):
    x, dy = operands(geom, False)
    dw, Aw = wgrad_reference(x, dy, *geom[6:], want_mag=True)
    want = autograd_dw(x, dy, geom)
    assert bool(((dw - want).abs() <= 1e-12 * Aw).all())
    # A_w is the gradient of the magnitudes, and bounds the gradient
    assert torch.equal(Aw, wgrad_reference(x.abs(), dy.abs(), *geom[6:])[0])
    assert bool((dw.abs() <= Aw).all())


def test_magnitude_sum_counts_every_live_product_once():
    """all-ones operands: A_w is the number of (output voxel, tap) pairs inside the volume, which has a closed form per
    axis -- a tap loop that drops an edge row or counts one twice fails here whatever autograd does"""
    for geom in GEOMS:
        B, D, H, W, Ci, Co, k, s, pad, dil = geom
        x = torch.ones((B, D, H, W, Ci), dtype=F64)
        oshape = tuple(out_extent(n, k, s, pad, dil) for n in (D, H, W))
        dy = torch.ones((B,) + oshape + (Co,), dtype=F64)
        dw, Aw = wgrad_reference(x, dy, k, s, pad, dil, want_mag=True)
        live = lambda n, no, t: sum(1 for o in range(no) if 0 <= o * s - pad + t * dil < n)
        for tap in range(k ** 3):
            kz, ky, kx = tap // (k * k), (tap // k) % k, tap % k
            n = B * live(D, oshape[0], kz) * live(H, oshape[1], ky) * live(W, oshape[2], kx)
            assert bool((dw[:, :, kz, ky, kx] == n).all()) and bool((Aw[:, :, kz, ky, kx] == n).all()), (geom, tap)


WINO_SHAPES = [(2, 5, 11, 13, 3, 4), (1, 1, 9, 12, 2, 2), (2, 3, 1, 9, 2, 3), (1, 2, 9, 1, 3, 2), (1, 4, 8, 8, 2, 2)]


@pytest.mark.parametrize("shape", WINO_SHAPES, ids=str)
def test_winograd_domain_reference(shape):
    """G^T (sum (A dy A^T) .* (B^T x B)) G is the weight gradient: exactly on integer data (every intermediate is a
    dyadic rational), within 1e-12 of the magnitude sums on normal data; M <= M_abs"""
    geom = shape + (3, 1, 1, 1)
    x, dy = operands(geom, True)
    r = wino_reference(x, dy)
    dw, _ = wgrad_reference(x, dy, 3, 1, 1, 1)
    assert torch.equal(r["dw"], dw)
    assert torch.equal(r["U"], r["U"].round())                      # integers in the Winograd domain,
    assert torch.equal(r["dw"] * 4, (r["dw"] * 4).round())          # quarters after G^T . G
    x, dy = operands(geom, False)
    r = wino_reference(x, dy)
    dw, Aw = wgrad_reference(x, dy, 3, 1, 1, 1, want_mag=True)
    assert bool(((r["dw"] - dw).abs() <= 1e-12 * gt_abs(r["M_abs"])).all())
    assert bool((r["U"].abs() <= r["M"]).all()) and bool((r["M"] <= r["M_abs"] * (1 + 1e-12)).all())
    assert float(r["M"].max()) > 0
