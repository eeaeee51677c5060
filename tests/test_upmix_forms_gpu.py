"""GPU: the six entry points of csrc/upmix.hip (the tap / trilinear gather of the first decoder convolution) in every
pass and storage form, element by element against the fp64 yardstick tests/upmix_ref.py (held to exact rational
weights and to F.interpolate in float64 by tests/test_upmix_ref_host.py).

The entry points are called through the C ABI with the return code checked, so the per-pass forms -- bf16 input, bf16
output, a base that aliases the output, statistics on and off, the bf16 -> bf16 backward form ops.py never calls, channel
counts from 4 to 128 -- are driven directly.  Every output buffer is NaN before the call; every element is held to a
bound  n u sum |w x|  with n the kernel's own chain length (u = 2^-24; + one rounding to 8 significant bits for a bf16
store, store_bound), never to a whole-tensor norm:

    generic forward pass   6 fmas into one accumulator                                   n = 6
    last forward pass      the same + the base                                           n = 7, on sum |w x| + |base|
    statistic rows         per row, kind and channel against the fp64 sums of the STORED values read back:
                           ceil(block voxels / vpi) additions per thread + vpi in the fixed-order fold
    backward pass          a window of at most 8 fmas + the rounding of w0 + w1           n = 10
    composite              the per-pass factors multiplied: (1 + 6u)^2 (1 + 7u) - 1, (1 + 10u)^3 - 1

The weights enter the reference as exact float64 operands in the form each kernel computes them, both pinned on the host
by tests/test_upmix_ref_host.py: the forward passes' w1 = fma(scale, u, -i0) (lin_src_fused in csrc/upmix.hip;
upmix_ref fused=True), the transposed pass's w1 = fl(scale u) - i0 (lin_src as compiled; the recipe).  Held to the
recipe, the forward pass misses 6 u sum |w x| at (1, 8, 6, 128) by 3.5e-7 from the weights alone.

The non-finite cases pin the rule of the yardstick: a term outside the range is ABSENT (an Inf at the clamped address of
an out-of-range tap reaches no output), a term inside it follows IEEE arithmetic."""
import math

import pytest
import torch

import upmix_ref as UR
from test_launch_regimes_gpu import BF16, DEV, F32, F64, U, UB, Excess, ops, poison, store_bound  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
VPB = 512                      # csrc/upmix.hip UPMIX_VPB: voxels per statistics row of the last pass
DT = {"f32": F32, "bf16": BF16}

# (outer, Ni, m, C) of the generic passes
AXIS_GEOMS = [(1, 1, 1, 4), (2, 2, 9, 32), (3, 5, 7, 64), (1, 8, 6, 128), (5, 3, 18, 8)]


def consts():
    from bodyct_dram_emph_subtype_amd import _lib
    return _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED


def draw(shape, seed, dtype=F32):
    """seeded on the host (the same values on every machine), as a value of the storage type"""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def nans(shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def call_fwd(ops, x, outer, Ni, m, C):
    assert x.numel() == outer * Ni * m * 3 * C
    out = nans((outer, 2 * Ni, m, C))
    rc = ops._L().dram_upmix_axis_fwd(ops._p(x), int(x.dtype == BF16), ops._p(out), outer, Ni, m, C, ops._stream())
    assert rc == 0
    return out


def call_final(ops, x, base, out, stats, outer, Ni, m, C):
    assert x.dtype == F32 and x.numel() == outer * Ni * m * 3 * C and out.numel() == outer * 2 * Ni * m * C
    assert base is None or (base.dtype == out.dtype and base.numel() == out.numel())
    assert stats is None or stats.numel() >= ops._L().dram_upmix_stat_rows(out.numel() // C) * 2 * C
    rc = ops._L().dram_upmix_axis_fwd_final(ops._p(x), ops._p(base), ops._p(out), int(out.dtype == BF16), ops._p(stats),
                                            outer, Ni, m, C, ops._stream())
    assert rc == 0


def call_bwd(ops, g, hdt, outer, Ni, m, C):
    assert g.numel() == outer * 2 * Ni * m * C
    h = nans((outer, Ni, m, 3, C), hdt)
    rc = ops._L().dram_upmix_axis_bwd(ops._p(g), int(g.dtype == BF16), ops._p(h), int(hdt == BF16), outer, Ni, m, C,
                                      ops._stream())
    assert rc == 0
    return h


_REF = {}


def fwd_reference(geom, dtype, seed):
    """(input of the storage type on the host, fp64 result with the forward kernels' weights, absolute sum), computed
    once and never written to"""
    key = ("fwd", geom, dtype, seed)
    if key not in _REF:
        outer, Ni, m, C = geom
        x = draw((outer, Ni, m, 3, C), seed, dtype)
        _REF[key] = (x,) + UR.axis_fwd_ref(x.double(), Ni, m, C, fused=True)
    return _REF[key]


def bwd_reference(geom, dtype, seed):
    key = ("bwd", geom, dtype, seed)
    if key not in _REF:
        outer, Ni, m, C = geom
        g = draw((outer, 2 * Ni, m, C), seed, dtype)
        _REF[key] = (g,) + UR.axis_bwd_ref(g.double(), Ni, m, C)
    return _REF[key]


def check(what, got, ref, bound):
    ex = Excess(what)
    ex.add(got.cpu().reshape(ref.shape), ref, bound)
    ex.check()


# ------------------------------------------------------------------------------------------------ a. generic forward
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("geom", AXIS_GEOMS, ids=str)
def test_axis_fwd(ops, geom, dt):
    """dram_upmix_axis_fwd, fp32 and bf16 input (widened exactly for the reference): |out - ref| <= 6 u sum |w x|"""
    outer, Ni, m, C = geom
    x, ref, mag = fwd_reference(geom, DT[dt], 11)
    out = call_fwd(ops, x.to(DEV), outer, Ni, m, C)
    check(f"axis_fwd {geom} {dt}", out, ref, 6 * U * mag)


# ------------------------------------------------------------------------------------------------ b. last forward pass
# id -> (C, outer, Ni, m), statistics rows, voxels of the last row
FINAL_CASES = {
    "c64-ragged": ((64, 1, 3, 100), 2, 88),         # last block not a multiple of vpi = 16
    "c128": ((128, 2, 2, 130), 3, 16),              # vpi = 8, all 256 threads write statistics
    "c4-scale0": ((4, 1, 1, 515), 3, 6),            # vpi = 256, last block 6 voxels, scale 0
    "c32-one-block": ((32, 3, 5, 7), 1, 210),       # one partial block whose voxels cross `outer` boundaries
    "c64-exact": ((64, 2, 4, 64), 2, 512),          # exact multiple
}
BASES = ["none", "distinct", "alias"]
FINAL_PARAMS = ([(c, d, b, s) for c in ("c64-ragged", "c128") for d in DT for b in BASES for s in (True, False)]
                + [(c, d, b, True) for c in ("c4-scale0", "c32-one-block", "c64-exact")
                   for d, b in (("f32", "alias"), ("bf16", "none"), ("bf16", "distinct"))])


def run_final(ops, case, dt, base_kind, want_stats, x=None):
    """-> (out, base as given or None, stats with one guard row behind or None)"""
    (C, outer, Ni, m), rows, _ = FINAL_CASES[case]
    nvox = outer * 2 * Ni * m
    if x is None:
        x = fwd_reference((outer, Ni, m, C), F32, 12)[0]
    base0 = None if base_kind == "none" else draw((nvox, C), 13, DT[dt])
    base = None if base0 is None else base0.to(DEV)
    out = base.clone() if base_kind == "alias" else nans((nvox, C), DT[dt])
    stats = nans((rows + 1, 2, C)) if want_stats else None
    call_final(ops, x.to(DEV), out if base_kind == "alias" else base, out, stats, outer, Ni, m, C)
    if base_kind == "distinct":
        assert torch.equal(base.cpu(), base0), "the base was written to"
    return out, base0, stats


@pytest.mark.parametrize("case,dt,base_kind,want_stats", FINAL_PARAMS,
                         ids=[f"{c}-{d}-{b}-{'stats' if s else 'nostats'}" for c, d, b, s in FINAL_PARAMS])
def test_axis_fwd_final(ops, case, dt, base_kind, want_stats):
    """dram_upmix_axis_fwd_final: stored values within store_bound(ref, dtype, 7 u (sum |w x| + |base|)); every
    statistic row, kind and channel against the fp64 sum over that block of the stored values read back, within
    (ceil(block voxels / vpi) + vpi) u sum |a| (sum a^2 for the squares); the row behind the last stays untouched;
    without statistics (null pointer) the stored values are the same bits."""
    (C, outer, Ni, m), rows, last = FINAL_CASES[case]
    nvox = outer * 2 * Ni * m
    vpi = 256 // (C // 4)
    assert ops._L().dram_upmix_stat_rows(nvox) == rows == -(-nvox // VPB) and nvox - (rows - 1) * VPB == last
    _, ref, mag = fwd_reference((outer, Ni, m, C), F32, 12)
    out, base0, stats = run_final(ops, case, dt, base_kind, want_stats)
    what = f"axis_fwd_final {case} {dt} base={base_kind}"
    ref, mag = ref.reshape(nvox, C), mag.reshape(nvox, C)
    if base0 is not None:
        ref, mag = ref + base0.double(), mag + base0.double().abs()
    check(f"{what} stored values", out, ref, store_bound(ref, DT[dt], 7 * U * mag))
    if not want_stats:
        on, _, _ = run_final(ops, case, dt, base_kind, True)
        assert torch.equal(on, out), f"{what}: the stored values differ without statistics"
        return
    stored = out.cpu().double()
    assert bool(torch.isnan(stats[rows]).all()), f"{what}: wrote behind statistics row {rows - 1}"
    ex = Excess(f"{what} statistic rows")
    for r in range(rows):
        a = stored[r * VPB:(r + 1) * VPB]
        n = -(-a.shape[0] // vpi) + vpi
        ex.add(stats[r, 0].cpu(), a.sum(0), n * U * a.abs().sum(0))
        ex.add(stats[r, 1].cpu(), (a * a).sum(0), n * U * (a * a).sum(0))
    ex.check()


# ------------------------------------------------------------------------------------------------ c. backward pass
@pytest.mark.parametrize("hdt", list(DT))
@pytest.mark.parametrize("gdt", list(DT))
@pytest.mark.parametrize("geom", AXIS_GEOMS, ids=str)
def test_axis_bwd(ops, geom, gdt, hdt):
    """dram_upmix_axis_bwd in its four storage forms: store_bound(ref, h dtype, 10 u sum |w g|)"""
    outer, Ni, m, C = geom
    g, ref, mag = bwd_reference(geom, DT[gdt], 21)
    h = call_bwd(ops, g.to(DEV), DT[hdt], outer, Ni, m, C)
    check(f"axis_bwd {geom} {gdt}->{hdt}", h, ref, store_bound(ref, DT[hdt], 10 * U * mag))


def test_axis_bwd_window_sweep(ops):
    """fp32 -> fp32 at every Ni in 1 .. 64 (outer = 1, C = 4): the candidate window (ulo, uhi) itself.  m = 1 on normal
    data within 10 u sum |w g|; and m = 2 Ni with G[v][mi] = [v == mi], where element (n, mi, k) is the ONE weight
    A[mi + k - 1][n] -- a single fma with 1 onto 0, exact but for the rounding of w0 + w1: within u |A|, so a dropped
    candidate fails whatever its weight, and an element outside A's support must be exactly 0."""
    bad = []
    for Ni in range(1, 65):
        g, ref, mag = bwd_reference((1, Ni, 1, 4), F32, 100 + Ni)
        h = call_bwd(ops, g.to(DEV), F32, 1, Ni, 1, 4).cpu().double()
        e1 = float(torch.nan_to_num((h - ref).abs() - 10 * U * mag, nan=math.inf).max())
        m = 2 * Ni
        eye = torch.eye(m).view(1, m, m, 1).expand(1, m, m, 4).contiguous()
        ref, mag = UR.axis_bwd_ref(eye.double(), Ni, m, 4)
        A = torch.from_numpy(UR.lin_weights(Ni))
        for k in range(3):                      # the yardstick's own layout: H[n][mi][k] = A[mi + k - 1][n]
            lo, hi = max(0, 1 - k), min(m, m + 1 - k)
            assert torch.equal(ref[0, :, lo:hi, k, 0], A[lo + k - 1:hi + k - 1].T)
        h = call_bwd(ops, eye.to(DEV), F32, 1, Ni, m, 4).cpu().double()
        e2 = float(torch.nan_to_num((h - ref).abs() - U * mag, nan=math.inf).max())
        if e1 > 0 or e2 > 0:
            bad.append((Ni, e1, e2))
    assert not bad, f"Ni, excess on normal data, excess on the impulses: {bad}"


# ------------------------------------------------------------------------------------------------ d. the composite
COMPOSITE = [(1, 3, 5, 2, 32), (2, 2, 3, 4, 64)]



@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("case", COMPOSITE, ids=str)
def test_composite_through_ops(ops, poison, case, dt):
    """ops.upmix_gather_fwd (in place on a base, with statistics) and ops.upmix_gather_bwd against the composed
    yardstick: the (outer, Ni, m) arguments ops.py passes.  Intermediates are fp32, so with e1 = (1 + 6 u)^2:
    forward  |y - ref| <= store_bound(ref, dtype, (e1 - 1) M + 7 u (e1 M + |base|)),
    backward |h - ref| <= store_bound(ref, dtype, ((1 + 10 u)^3 - 1) M),  M the composed absolute sum."""
    B, Ds, Hs, Ws, Co = case
    b = draw((B, Ds, Hs, Ws, 27 * Co), 31, DT[dt])
    base = draw((B, 2 * Ds, 2 * Hs, 2 * Ws, Co), 32, DT[dt])
    dy = draw((B, 2 * Ds, 2 * Hs, 2 * Ws, Co), 33, DT[dt])
    ref, M = UR.gather_fwd_ref(b.double(), Co, fused=True)
    ref = ref + base.double()
    e1 = (1 + 6 * U) ** 2
    based = base.clone().to(DEV)
    y, stats = ops.upmix_gather_fwd(b.to(DEV), based, Co, True)
    assert y.data_ptr() == based.data_ptr() and y.dtype == DT[dt]
    check(f"upmix_gather_fwd {case} {dt}", y, ref,
          store_bound(ref, DT[dt], (e1 - 1) * M + 7 * U * (e1 * M + base.double().abs())))
    nvox = B * 8 * Ds * Hs * Ws
    assert stats.shape == (ops._L().dram_upmix_stat_rows(nvox), 2, Co)
    stored = y.cpu().double().reshape(nvox, Co)
    ex = Excess(f"upmix_gather_fwd {case} {dt} statistic rows")
    vpi = 256 // (Co // 4)
    for r in range(stats.shape[0]):
        a = stored[r * VPB:(r + 1) * VPB]
        n = -(-a.shape[0] // vpi) + vpi
        ex.add(stats[r, 0].cpu(), a.sum(0), n * U * a.abs().sum(0))
        ex.add(stats[r, 1].cpu(), (a * a).sum(0), n * U * (a * a).sum(0))
    ex.check()
    y0, none = ops.upmix_gather_fwd(b.to(DEV), None, Co, False)
    assert none is None and y0.dtype == DT[dt]
    ref0 = ref - base.double()
    check(f"upmix_gather_fwd {case} {dt} without base", y0, ref0,
          store_bound(ref0, DT[dt], (e1 - 1) * M + 7 * U * e1 * M))
    href, hM = UR.gather_bwd_ref(dy.double(), Co)
    h = ops.upmix_gather_bwd(dy.to(DEV))
    assert h.dtype == DT[dt]
    check(f"upmix_gather_bwd {case} {dt}", h, href, store_bound(href, DT[dt], ((1 + 10 * U) ** 3 - 1) * hM))


# ------------------------------------------------------------------------------------------------ e. non-finite borders
def planted(Ni, outer, m, C, value, seed):
    """normal data with `value` at In[outer-1][0][1][k=0][2] (the clamped address of the out-of-range tap of row v = 0)
    and at In[0][Ni-1][m-2][k=2][C-3] (that of row v = 2 Ni - 1); and the same data with zeros there"""
    x = draw((outer, Ni, m, 3, C), seed)
    zero = x.clone()
    for t, v in ((x, value), (zero, 0.0)):
        t[outer - 1, 0, 1, 0, 2] = v
        t[0, Ni - 1, m - 2, 2, C - 3] = v
    return x, zero


def check_planted(what, got, got_zero, ref, Ni):
    """the non-finite outputs are the reference's, and every other output has the bits of the run with zeros planted
    (it reads neither element).  From Ni = 3 on that is all of the rows v = 0 and v = 2 Ni - 1: at Ni = 1 element 0 is
    element Ni - 1 too, and each of the two rows reads one of the planted elements through its in-range taps."""
    got, got_zero = got.cpu().reshape(ref.shape), got_zero.cpu().reshape(ref.shape)
    fin = torch.isfinite(ref)
    assert not bool(fin.all()) and bool(torch.isfinite(got_zero).all())
    if Ni >= 3:
        assert bool(fin[:, 0].all()) and bool(fin[:, 2 * Ni - 1].all())
    leak = (~torch.isfinite(got)) & fin
    assert not bool(leak.any()), (f"{what}: {int(leak.sum())} outputs are non-finite where the reference is finite, the "
                                  f"first at (o, v, m, c) = {tuple(int(i) for i in leak.nonzero()[0])}")
    assert torch.equal(torch.isfinite(got), fin), f"{what}: the non-finite outputs are not the reference's"
    assert torch.equal(got[fin], got_zero[fin]), f"{what}: finite outputs differ from the run with zeros planted"


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("value", [INF, NAN], ids=["inf", "nan"])
@pytest.mark.parametrize("Ni", [1, 3, 8])
def test_nonfinite_border_generic_pass(ops, Ni, value, dt):
    """An Inf / NaN at the clamped address of an out-of-range tap reaches no output of the generic pass."""
    outer, m, C = 2, 5, 8
    x, zero = planted(Ni, outer, m, C, value, 41)
    ref, _ = UR.axis_fwd_ref(x.to(DT[dt]).double(), Ni, m, C, fused=True)
    got = call_fwd(ops, x.to(DT[dt]).to(DEV), outer, Ni, m, C)
    got_zero = call_fwd(ops, zero.to(DT[dt]).to(DEV), outer, Ni, m, C)
    check_planted(f"axis_fwd Ni={Ni} {value} {dt}", got, got_zero, ref, Ni)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("value", [INF, NAN], ids=["inf", "nan"])
@pytest.mark.parametrize("Ni", [1, 3, 8])
def test_nonfinite_border_final_pass(ops, Ni, value, dt):
    """... nor of the last pass (the z axis of the composite), fp32 and bf16 output"""
    outer, m, C = 2, 5, 8
    x, zero = planted(Ni, outer, m, C, value, 42)
    ref, _ = UR.axis_fwd_ref(x.double(), Ni, m, C, fused=True)
    outs = []
    for t in (x, zero):
        out = nans((outer * 2 * Ni * m, C), DT[dt])
        call_final(ops, t.to(DEV), None, out, None, outer, Ni, m, C)
        outs.append(out)
    check_planted(f"axis_fwd_final Ni={Ni} {value} {dt}", outs[0], outs[1], ref, Ni)


def test_nonfinite_border_composite(ops, poison):
    """ops.upmix_gather_fwd with an Inf at x = 0 in a tap with kx = 0 and at z = Ds - 1 in a tap with kz = 2: the
    finite mask is the reference's"""
    B, Ds, Hs, Ws, Co = 1, 3, 5, 2, 32
    b = draw((B, Ds, Hs, Ws, 27 * Co), 43)
    b[0, 1, 2, 0, ((1 * 3 + 1) * 3 + 0) * Co + 5] = INF
    b[0, Ds - 1, 3, 1, ((2 * 3 + 1) * 3 + 1) * Co + 7] = INF
    ref, _ = UR.gather_fwd_ref(b.double(), Co, fused=True)
    y, _ = ops.upmix_gather_fwd(b.to(DEV), None, Co, False)
    fin = torch.isfinite(ref)
    assert not bool(fin.all())
    leak = (~torch.isfinite(y.cpu())) & fin
    assert not bool(leak.any()), f"{int(leak.sum())} outputs are non-finite where the reference is finite"
    assert torch.equal(torch.isfinite(y.cpu()), fin)


@pytest.mark.parametrize("Ni", [1, 3, 8])
def test_nonfinite_border_backward_pass(ops, Ni):
    """the transposed pass skips its out-of-range candidates: an Inf in g at v = 0 and at v = 2 Ni - 1"""
    outer, m, C = 2, 5, 8
    g = draw((outer, 2 * Ni, m, C), 44)
    g[1, 0, 1, 2] = INF
    g[0, 2 * Ni - 1, 3, 5] = INF
    ref, _ = UR.axis_bwd_ref(g.double(), Ni, m, C)
    h = call_bwd(ops, g.to(DEV), F32, outer, Ni, m, C).cpu()
    assert not bool(torch.isfinite(ref).all())
    assert torch.equal(torch.isfinite(h), torch.isfinite(ref))


# ------------------------------------------------------------------------------------------------ f. weight split / merge
@pytest.mark.parametrize("case", [(32, 64, 32), (3, 5, 2)], ids=str)
def test_split_weight_merge_wgrad_roundtrip(ops, poison, case):
    """merge_wgrad(split_weight(w)) == w bit for bit; (3, 5, 2): 567 elements, a ragged last block"""
    Co, Cu, Cs = case
    w = draw((Co, Cu + Cs, 3, 3, 3), 51)
    wlo, ws = ops.upmix_split_weight(w.to(DEV), Cu)
    assert torch.equal(wlo.reshape(27, Co, Cu).cpu(), w[:, :Cu].reshape(Co, Cu, 27).permute(2, 0, 1))
    assert torch.equal(ws.cpu(), w[:, Cu:])
    assert torch.equal(ops.upmix_merge_wgrad(wlo, ws).cpu(), w)


# ------------------------------------------------------------------------------------------------ g. refusals
def test_refusals_launch_nothing(ops):
    """unsupported channel counts and null operands are refused with the output untouched (still all NaN)"""
    BAD_ARG, UNSUPPORTED = consts()
    L, s = ops._L(), ops._stream()
    src = torch.zeros(1 << 16, device=DEV)
    outs = {dt: nans((1 << 16,), dt) for dt in (F32, BF16)}
    stats = nans((64, 2, 256))
    p = ops._p
    got = []
    for C in (6, 0, 12, 132):
        for bf in (0, 1):
            got.append((f"final C={C} bf16={bf}", UNSUPPORTED,
                        L.dram_upmix_axis_fwd_final(p(src), None, p(outs[BF16 if bf else F32]), bf, p(stats), 1, 2, 3, C, s)))
        if C in (6, 0):
            for bf in (0, 1):
                got.append((f"fwd C={C} in_bf16={bf}", UNSUPPORTED,
                            L.dram_upmix_axis_fwd(p(src), bf, p(outs[F32]), 1, 2, 3, C, s)))
                for hbf in (0, 1):
                    got.append((f"bwd C={C} g_bf16={bf} h_bf16={hbf}", UNSUPPORTED,
                                L.dram_upmix_axis_bwd(p(src), bf, p(outs[BF16 if hbf else F32]), hbf, 1, 2, 3, C, s)))
    o = p(outs[F32])
    got += [("fwd null in", BAD_ARG, L.dram_upmix_axis_fwd(None, 0, o, 1, 2, 3, 8, s)),
            ("fwd null out", BAD_ARG, L.dram_upmix_axis_fwd(p(src), 0, None, 1, 2, 3, 8, s)),
            ("final null in", BAD_ARG, L.dram_upmix_axis_fwd_final(None, None, o, 0, p(stats), 1, 2, 3, 8, s)),
            ("final null out", BAD_ARG, L.dram_upmix_axis_fwd_final(p(src), None, None, 0, p(stats), 1, 2, 3, 8, s)),
            ("bwd null g", BAD_ARG, L.dram_upmix_axis_bwd(None, 0, o, 0, 1, 2, 3, 8, s)),
            ("bwd null h", BAD_ARG, L.dram_upmix_axis_bwd(p(src), 0, None, 0, 1, 2, 3, 8, s))]
    wrong = [(what, want, rc) for what, want, rc in got if rc != want]
    assert not wrong, f"(call, expected, returned): {wrong}"
    torch.cuda.synchronize()
    for t in list(outs.values()) + [stats]:
        assert bool(torch.isnan(t).all()), "a refused call wrote to its output"
