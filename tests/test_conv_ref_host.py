"""Host: the fp64 forward / data-gradient references of tests/conv_ref.py (which tests/test_conv_bf16_forms_gpu.py holds
the bf16 kernels to) against F.conv3d in float64 and its autograd input gradient -- bit for bit on integer operands,
where every sum is exact in any order, and within 1e-12 A on normal operands -- and to_bf16_rne's rounding."""
import pytest
import torch
import torch.nn.functional as F

from conv_ref import conv_reference, dgrad_reference, out_extent, to_bf16_rne

F64 = torch.float64

GEOMS = [
    # B, D, H, W, Cin, Cout, k, stride, pad, dil: every (k, stride, dil) class of the GPU module
    (2, 5, 11, 13, 3, 4, 3, 1, 1, 1),
    (1, 1, 9, 1, 2, 3, 3, 1, 1, 1),                 # extents of one: most taps are padding
    (2, 5, 9, 7, 3, 2, 3, 1, 2, 2),
    (1, 1, 3, 9, 2, 2, 3, 1, 2, 2),                 # an extent smaller than the dilation
    (1, 6, 10, 9, 2, 3, 3, 1, 4, 4),
    (1, 2, 5, 3, 2, 2, 3, 1, 4, 4),                 # dilation beyond the extents: whole taps are padding
    (1, 4, 6, 8, 3, 2, 3, 2, 1, 1),                 # stride 2 on even extents (the last input row / column is unused)
    (2, 2, 2, 2, 2, 3, 3, 2, 1, 1),                 # ... down to one output voxel
    (1, 9, 11, 13, 3, 2, 3, 2, 1, 1),               # stride 2 on odd extents
    (2, 3, 7, 5, 4, 3, 1, 1, 0, 1),
]


def operands(geom, integer):
    B, D, H, W, Ci, Co, k, s, pad, dil = geom
    oshape = tuple(out_extent(n, k, s, pad, dil) for n in (D, H, W))
    g = torch.Generator().manual_seed(sum(geom))
    if integer:
        draw = lambda shape, a: torch.randint(-a, a + 1, shape, generator=g).double()
        return (draw((B, D, H, W, Ci), 1), draw((Co, Ci, k, k, k), 8), draw((Co,), 3), draw((B,) + oshape + (Co,), 1))
    draw = lambda shape: torch.randn(shape, generator=g, dtype=F64)
    return draw((B, D, H, W, Ci)), draw((Co, Ci, k, k, k)), draw((Co,)), draw((B,) + oshape + (Co,))


def torch_conv(x, w, bias, dy, geom):
    """F.conv3d in float64 and its autograd input gradient, as NDHWC"""
    s, pad, dil = geom[7:]
    xc = x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    y = F.conv3d(xc, w, bias, s, pad, dil)
    (dx,) = torch.autograd.grad(y, [xc], dy.permute(0, 4, 1, 2, 3))
    return y.detach().permute(0, 2, 3, 4, 1), dx.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_tap_loops_equal_torch_exactly_on_integer_data(geom):
    x, w, bias, dy = operands(geom, True)
    for b in (bias, None):
        y, none = conv_reference(x, w, b, *geom[6:])
        want_y, want_dx = torch_conv(x, w, b, dy, geom)
        assert none is None and y.dtype == F64 and float(want_y.abs().max()) > 0
        assert torch.equal(y, want_y)
    dx, none = dgrad_reference(dy, w, x.shape, *geom[6:])
    assert none is None and dx.dtype == F64 and float(want_dx.abs().max()) > 0
    assert torch.equal(dx, want_dx)
    # the magnitudes are the same loops on absolute values: exactly, where every sum is an integer
    assert torch.equal(conv_reference(x, w, bias, *geom[6:], want_mag=True)[1],
                       conv_reference(x.abs(), w.abs(), bias.abs(), *geom[6:])[0])
    assert torch.equal(dgrad_reference(dy, w, x.shape, *geom[6:], want_mag=True)[1],
                       dgrad_reference(dy.abs(), w.abs(), x.shape, *geom[6:])[0])


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_tap_loops_equal_torch_on_normal_data_and_magnitudes_are_the_loops_on_absolute_values(geom):
    x, w, bias, dy = operands(geom, False)
    y, A = conv_reference(x, w, bias, *geom[6:], want_mag=True)
    dx, Ad = dgrad_reference(dy, w, x.shape, *geom[6:], want_mag=True)
    want_y, want_dx = torch_conv(x, w, bias, dy, geom)
    assert bool(((y - want_y).abs() <= 1e-12 * A).all())
    assert bool(((dx - want_dx).abs() <= 1e-12 * Ad).all())
    # (the same sums; the BLAS behind the matmul may order them differently for the two operand layouts)
    assert bool(((A - conv_reference(x.abs(), w.abs(), bias.abs(), *geom[6:])[0]).abs() <= 1e-14 * A).all())
    assert bool(((Ad - dgrad_reference(dy.abs(), w.abs(), x.shape, *geom[6:])[0]).abs() <= 1e-14 * Ad).all())
    assert bool((y.abs() <= A).all()) and bool((dx.abs() <= Ad).all())
    # without a bias the magnitude loses exactly |bias|
    A0 = conv_reference(x, w, None, *geom[6:], want_mag=True)[1]
    assert bool(((A - A0 - bias.abs()).abs() <= 1e-12 * A).all())


def test_magnitude_sums_count_every_live_product_once():
    """all-ones operands: A is the number of (tap, input channel) pairs inside the volume, which has a closed form per
    axis -- a tap loop that drops an edge row or counts one twice fails here whatever torch does.  The data gradient
    counts the same pairs from the input voxel's side."""
    for geom in GEOMS:
        B, D, H, W, Ci, Co, k, s, pad, dil = geom
        ext, oext = (D, H, W), tuple(out_extent(n, k, s, pad, dil) for n in (D, H, W))
        x = torch.ones((B, D, H, W, Ci), dtype=F64)
        w = torch.ones((Co, Ci, k, k, k), dtype=F64)
        dy = torch.ones((B,) + oext + (Co,), dtype=F64)
        y, A = conv_reference(x, w, None, k, s, pad, dil, want_mag=True)
        dx, Ad = dgrad_reference(dy, w, x.shape, k, s, pad, dil, want_mag=True)
        fwd = [torch.tensor([sum(1 for t in range(k) if 0 <= o * s - pad + t * dil < n) for o in range(no)], dtype=F64)
               for n, no in zip(ext, oext)]
        bwd = [torch.tensor([sum(1 for t in range(k) for o in range(no) if o * s - pad + t * dil == i) for i in range(n)],
                            dtype=F64) for n, no in zip(ext, oext)]
        want = Ci * fwd[0].view(-1, 1, 1) * fwd[1].view(1, -1, 1) * fwd[2].view(1, 1, -1)
        want_d = Co * bwd[0].view(-1, 1, 1) * bwd[1].view(1, -1, 1) * bwd[2].view(1, 1, -1)
        for got in (y, A):
            assert torch.equal(got, want.view(1, *oext, 1).expand_as(got)), geom
        for got in (dx, Ad):
            assert torch.equal(got, want_d.view(1, *ext, 1).expand_as(got)), geom


def test_to_bf16_rne_rounds_ties_to_even_and_refuses_inexact_input():
    t = torch.tensor([257.0, 259.0, -257.0, -259.0, 258.0, 0.0, -0.0, 1.0, 2.0 ** 24 - 2], dtype=F64)
    r = to_bf16_rne(t)
    assert r.dtype == torch.bfloat16
    assert r.double().tolist()[:5] == [256.0, 260.0, -256.0, -260.0, 258.0]
    assert float(r[7]) == 1.0 and float(r[8]) == 2.0 ** 24
    # -0.0 is kept (and +0.0 stays positive)
    assert torch.signbit(r[5]).item() is False and torch.signbit(r[6]).item() is True and float(r[6]) == 0.0
    # above the tie goes up, below down
    assert to_bf16_rne(torch.tensor([257.0 + 2.0 ** -10, 259.0 - 2.0 ** -10], dtype=F64)).double().tolist() == [258.0, 258.0]
    for bad in (2.0 ** 24 + 1, 1.0 + 2.0 ** -30, float("nan")):
        with pytest.raises(ValueError):
            to_bf16_rne(torch.tensor([1.0, bad], dtype=F64))
    with pytest.raises(AssertionError):
        to_bf16_rne(torch.tensor([1.0]))
