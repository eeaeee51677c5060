"""GPU: the six launch forms of the stem convolution Conv3d(1, 64, k=7, s=2, p=3) -- forward and weight gradient, fp32
(csrc/stem.hip), bf16 store / bf16 dy on the fp32 matrix cores (stem.hip, DRAM_STEM_BF16=0) and on the bf16 matrix cores
(csrc/stem_bf16.hip) -- element by element against a plain fp64 tap loop on the device, at the shapes that enter the
persistent loops (a second trip of a workgroup, the prefetch guard, the stale LDS tile), the boundary slab counts of
the ordered slab reduce, and ragged / one-voxel extents.

Part A (test_exact_*): operands in {-1, 0, 1} with at most 255 live taps per filter.  Every product and every partial
sum is then an integer that fp32 and bf16 hold exactly (|y| <= 255, a tile's sum of y^2 < 2^24, |dw| < 2^24 -- asserted
from the reference itself), so the result does not depend on summation order or arithmetic path and every form must
equal the reference BIT FOR BIT: y, every raw per-tile statistic row, the folded statistics, dw.

Part B (test_rounding_*): normal random operands, every element held to a bound derived from the kernels' arithmetic
(see the test's docstring); the measured worst ratios are printed.

Every case asserts the form it claims -- forward tiles, workgroups, trips -- from the library's own sizing exports
(dram_stem_num_tiles, dram_stem_fwd_blocks, dram_stem_bwd_weight_workspace), and which kernel ran from the library's
kernel timeline (family "stem": variants 0 / 1 are stem.hip's forward / weight gradient, 2 / 3 stem_bf16.hip's).
All allocations of the wrappers are poisoned (test_launch_regimes_gpu.poison): an unwritten element is NaN.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_launch_regimes_gpu import BF16, DEV, F32, F64, U, UB, Excess, ops, poison, store_bound  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SLAB_BYTES = 64 * 352 * 4        # one workgroup's slab of the weight gradient: [64 co][352 taps] float (dram_hip.h)

# form -> (storage type of y / dy, DRAM_STEM_BF16, timeline variant of the forward, of the weight gradient)
FORMS = {"f32": (F32, None, 0, 1), "bf16-store": (BF16, "0", 0, 1), "bf16-mm": (BF16, None, 2, 3)}

# case -> (B, D, H, W) and the form it claims: forward tiles, trips of the busiest workgroup of the persistent bf16
# forward, weight-gradient sub-tiles (= B Do ceil(Ho/8) ceil(Wo/8)), trips of the busiest weight-gradient workgroup,
# workgroups that make one trip more than the idlest (0: all make the same number)
CASES = {
    # 48 forward workgroups make a second trip (in batch 1); weight-gradient workgroups make 3 or 4; every output extent
    # ragged against 4 / 8 / 8, every input extent odd
    "persist-ragged": ((2, 33, 119, 103), dict(tiles=560, fwd_trips=2, fwd_extra=48, total=1904, wg_trips=4, wg_extra=368)),
    # exactly one weight-gradient workgroup makes a second trip; 512 slabs
    "one-over": ((1, 38, 34, 130), dict(tiles=135, fwd_trips=1, fwd_extra=0, total=513, wg_trips=2, wg_extra=1)),
    # exactly at the cap: no second trip
    "at-cap": ((1, 64, 64, 64), dict(tiles=128, fwd_trips=1, fwd_extra=0, total=512, wg_trips=1, wg_extra=0)),
    # one output voxel: everything but the centre tap is padding
    "one-voxel": ((1, 1, 1, 1), dict(tiles=1, fwd_trips=1, fwd_extra=0, total=1, wg_trips=1, wg_extra=0)),
    # one output voxel over an 8-wide tile in x
    "one-voxel-over": ((1, 2, 15, 17), dict(tiles=2, fwd_trips=1, fwd_extra=0, total=2, wg_trips=1, wg_extra=0)),
    # the ragged shape of test_bf16_gpu.py::test_stem_bf16_matrix_core_kernels
    "even-odd": ((2, 9, 20, 35), dict(tiles=24, fwd_trips=1, fwd_extra=0, total=60, wg_trips=1, wg_extra=0)),
}
# slab counts at the main-loop / tail boundary of the slab reduce (k + 28 < nslab; k += 32, four slab groups)
NSLAB = [1, 4, 5, 29, 32, 33, 61, 64]
for _k in NSLAB:
    CASES[f"nslab-{_k}"] = ((1, 2 * _k, 16, 16), dict(tiles=-(-_k // 4), fwd_trips=1, fwd_extra=0, total=_k, wg_trips=1,
                                                      wg_extra=0))
ROUNDING_CASES = ["persist-ragged", "even-odd"]


def out_extents(ops, shape):
    return tuple(ops.stem_out(n) for n in shape[1:])


def launch_form(ops, shape):
    """The form the library gives `shape`, from its sizing exports alone."""
    L = ops._L()
    B, D, H, W = shape
    Do, Ho, Wo = out_extents(ops, shape)
    tiles = L.dram_stem_num_tiles(B, Do, Ho, Wo)
    fblk = L.dram_stem_fwd_blocks(tiles)
    total = B * Do * -(-Ho // 8) * -(-Wo // 8)
    nbytes = L.dram_stem_bwd_weight_workspace(B, D, H, W)
    assert nbytes % SLAB_BYTES == 0
    wblk = nbytes // SLAB_BYTES
    assert 1 <= fblk <= tiles and 1 <= wblk <= total
    return dict(tiles=tiles, fwd_blocks=fblk, fwd_trips=-(-tiles // fblk), fwd_extra=tiles % fblk, total=total,
                wg_blocks=wblk, wg_trips=-(-total // wblk), wg_extra=total % wblk)


def assert_form(ops, case):
    shape, claim = CASES[case]
    form = launch_form(ops, shape)
    got = {k: form[k] for k in claim}
    assert got == claim, f"{case}: the library gives this shape the form {form}, the case claims {claim}"
    return form


# ------------------------------------------------------------------------------------------------ reference
def tap_reference(x, w, dy, want_mag):
    """The fp64 tap loop: x [B,D,H,W], w [64,343], dy [B,Do,Ho,Wo,64], all float64 on one device ->
    y [B,Do,Ho,Wo,64], dw [64,343] and, with want_mag, A = conv(|x|, |w|) and A_w = sum |dy| |x| (else None)."""
    B, D, H, W = x.shape
    Do, Ho, Wo = dy.shape[1:4]
    xp = torch.zeros((B, D + 6, H + 6, W + 6), dtype=F64, device=x.device)
    xp[:, 3:3 + D, 3:3 + H, 3:3 + W] = x
    y = torch.zeros((B, Do, Ho, Wo, 64), dtype=F64, device=x.device)
    dw = torch.zeros((64, 343), dtype=F64, device=x.device)
    A = torch.zeros_like(y) if want_mag else None
    Aw = torch.zeros_like(dw) if want_mag else None
    dyt = dy.reshape(-1, 64).T.contiguous()
    dyt_abs = dyt.abs() if want_mag else None
    for tap in range(343):
        kz, ky, kx = tap // 49, (tap // 7) % 7, tap % 7
        xs = xp[:, kz::2, ky::2, kx::2][:, :Do, :Ho, :Wo].contiguous()
        y.addcmul_(xs[..., None], w[:, tap])
        dw[:, tap] = dyt @ xs.reshape(-1)
        if want_mag:
            A.addcmul_(xs.abs()[..., None], w[:, tap].abs())
            Aw[:, tap] = dyt_abs @ xs.abs().reshape(-1)
    return y, dw, A, Aw


def tile_sums(v):
    """[B,Do,Ho,Wo,C] -> [tiles, C]: sums over the 4 x 8 x 8 output tiles clipped to the extents, tiles in the order
    (b, tz, ty, tx) of the statistic rows."""
    B, Do, Ho, Wo, C = v.shape
    p = F.pad(v, (0, 0, 0, -Wo % 8, 0, -Ho % 8, 0, -Do % 4))
    nz, ny, nx = p.shape[1] // 4, p.shape[2] // 8, p.shape[3] // 8
    return p.view(B, nz, 4, ny, 8, nx, 8, C).sum((2, 4, 6)).reshape(B * nz * ny * nx, C)


def cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


def integer_operands(shape, oshape):
    """x, dy i.i.d. in {-1, 0, 1}; w +-1 on 255 taps per filter, the other 88 (chosen per filter) zero.  Drawn on the
    host: the same values on every machine."""
    g = cpu_gen(sum(shape) + 1000 * shape[3])
    x = torch.randint(-1, 2, shape, generator=g).double()
    dy = torch.randint(-1, 2, oshape + (64,), generator=g).double()
    w = (torch.randint(0, 2, (64, 343), generator=g) * 2 - 1).double()
    dead = torch.rand((64, 343), generator=g).argsort(1)[:, :88]
    w.scatter_(1, dead, 0.0)
    assert int((w != 0).sum(1).max()) == 255 and bool((w != 0).any(0).all())      # all 343 taps live in some filter
    if x.numel() == 1:
        x.fill_(-1.0)                                   # the one input voxel must not be the draw's zero
    assert float(x.abs().sum()) > 0 and float(dy.abs().sum()) > 0
    return x, w, dy


def real_operands(shape, oshape, rounded):
    """normal random x, 0.1 w, dy; `rounded`: to bf16 first (the bf16 forms round x and w on their way in, dy is stored
    in bf16: the reference sees the same operands)"""
    g = cpu_gen(7 + sum(shape))
    x = torch.randn(shape, generator=g)
    dy = torch.randn(oshape + (64,), generator=g)
    w = 0.1 * torch.randn((64, 343), generator=g)
    if rounded:
        x, dy, w = (t.to(BF16).float() for t in (x, dy, w))
    return x.double(), w.double(), dy.double()


_REF = {}


def reference(ops, case, kind):
    """dict(x, w [64,1,7,7,7], dy: float32 device operands; y, dw, A, Aw: float64), computed once per (case, kind) and
    shared, never written to.  kind: "int" | "real" | "real-bf16"."""
    key = (case, kind)
    if key not in _REF:
        shape = CASES[case][0]
        oshape = (shape[0],) + out_extents(ops, shape)
        if kind == "int":
            x, w, dy = integer_operands(shape, oshape)
        else:
            x, w, dy = real_operands(shape, oshape, kind == "real-bf16")
        x, w, dy = x.to(DEV), w.to(DEV), dy.to(DEV)
        y, dw, A, Aw = tap_reference(x, w, dy, kind != "int")
        if kind == "int":               # the exact regime, from the reference itself
            assert float(y.abs().max()) <= 255
            assert float(tile_sums(y * y).max()) < 2 ** 24
            assert float(dw.abs().max()) < 2 ** 24
            assert float(y.abs().max()) > 0 and float(dw.abs().max()) > 0
        assert bool((x.float().double() == x).all() and (w.float().double() == w).all() and (dy.float().double() == dy).all())
        _REF[key] = dict(x=x.float(), w=w.float().view(64, 1, 7, 7, 7).contiguous(), dy=dy.float(), y=y,
                         dw=dw.view(64, 1, 7, 7, 7), A=A, Aw=None if Aw is None else Aw.view(64, 1, 7, 7, 7))
    return _REF[key]


# ------------------------------------------------------------------------------------------------ running a form
def run_form(ops, monkeypatch, form, ref):
    """forward with and without statistics, the weight gradient twice, under the kernel timeline: the launches must be
    of the form's own kernels."""
    dt, env, v_fwd, v_wg = FORMS[form]
    if env is None:
        monkeypatch.delenv("DRAM_STEM_BF16", raising=False)
    else:
        monkeypatch.setenv("DRAM_STEM_BF16", env)
    dy = ref["dy"].to(dt)
    assert torch.equal(dy.double(), ref["dy"].double())              # dy is a bf16 value already
    tl = ops.KernelTimeline()
    tl.start()
    try:
        y, stats = ops.stem_fwd(ref["x"], ref["w"], True, dt)
        y0, none = ops.stem_fwd(ref["x"], ref["w"], False, dt)
        dw = ops.stem_bwd_weight(ref["x"], dy)
        dw2 = ops.stem_bwd_weight(ref["x"], dy)
        fam = tl.families()
    finally:
        tl.stop()
    variants = {v: n for v, (n, _) in fam["stem"]["variants"].items()}
    assert variants == {v_fwd: 2, v_wg: 2}, f"{form}: stem launches by variant {variants}"
    assert none is None and y.dtype == dt and y0.dtype == dt and dw.dtype == F32
    return y, stats, y0, dw, dw2


def assert_same(got, want, what):
    """bit-for-bit (as values: got and want widened to float64); NaN -- an unwritten element -- differs"""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, the first at {i}: "
                             f"{float(got[i])} for {float(want[i])}")


def check_exact(ops, monkeypatch, case, form):
    lf = assert_form(ops, case)
    ref = reference(ops, case, "int")
    dt = FORMS[form][0]
    y, stats, y0, dw, dw2 = run_form(ops, monkeypatch, form, ref)
    what = f"{case} {form}"
    yr = ref["y"]
    assert torch.equal(yr.to(dt).double(), yr)                       # the reference is a value of the storage type
    assert_same(y, yr, f"{what} y")
    assert_same(y0, yr, f"{what} y (want_stats=False)")
    assert stats.shape == (lf["tiles"], 2, 64) and stats.dtype == F32
    assert_same(stats[:, 0], tile_sums(yr), f"{what} statistic rows, sum y")
    assert_same(stats[:, 1], tile_sums(yr * yr), f"{what} statistic rows, sum y^2")
    fold = ops.reduce_partials(stats)
    assert fold.dtype == F64
    assert_same(fold, torch.stack([yr.sum((0, 1, 2, 3)), (yr * yr).sum((0, 1, 2, 3))]), f"{what} folded statistics")
    assert_same(dw, ref["dw"], f"{what} dw")
    assert torch.equal(dw2, dw), f"{what}: the weight gradient is not deterministic"


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", [c for c in CASES if not c.startswith("nslab-")])
def test_exact_on_integer_data(ops, poison, monkeypatch, case, form):
    """Part A: y, the raw statistic rows, their fold and dw equal the fp64 tap loop bit for bit, in the claimed form."""
    check_exact(ops, monkeypatch, case, form)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k", NSLAB)
def test_exact_slab_reduce_boundaries(ops, poison, monkeypatch, k, form):
    """Part A at (1, 2k, 16, 16): k weight-gradient workgroups, so the ordered reduce folds nslab = k slabs -- each
    boundary of its unrolled main loop and its tail."""
    lf = assert_form(ops, f"nslab-{k}")
    assert lf["wg_blocks"] == k
    check_exact(ops, monkeypatch, f"nslab-{k}", form)


def test_persistent_cases_are_persistent(ops):
    """what the persistent cases are for, from the sizing exports: a second trip of the bf16 forward in the last batch
    element, 3 and 4 trips of the weight gradient; one weight-gradient workgroup one over; none at the cap"""
    f = assert_form(ops, "persist-ragged")
    assert f["fwd_blocks"] < f["tiles"] and f["fwd_blocks"] >= f["tiles"] // 2       # second trips start in batch 1
    assert f["wg_trips"] == 4 and 0 < f["wg_extra"] < f["wg_blocks"]                # 3 or 4 trips
    f = assert_form(ops, "one-over")
    assert f["total"] == f["wg_blocks"] + 1
    f = assert_form(ops, "at-cap")
    assert f["total"] == f["wg_blocks"]
    shape = CASES["at-cap"][0]
    more = (shape[0], shape[1] + 2) + shape[2:]                       # one more output plane: the cap holds
    assert ops._L().dram_stem_bwd_weight_workspace(*more) // SLAB_BYTES == f["wg_blocks"]


# ------------------------------------------------------------------------------------------------ Part B
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", ROUNDING_CASES)
def test_rounding_on_real_data(ops, poison, monkeypatch, capsys, case, form):
    """Part B: normal random x, 0.1 w, dy (rounded to bf16 first for the bf16 forms), u = 2^-24:
      y:  |y - ref| <= store_bound(ref, dtype, 2 * 343 u A), A = conv(|x|, |w|): 343 terms in one accumulator chain (a
          padded tap adds an exact zero), the 2 for the unknown order of the partial sums inside an MFMA;
      dw: |dw - ref| <= 2 (64 trips + 21) u A_w, A_w = sum |dy| |x|: a workgroup accumulates 64 voxels per trip, the slab
          reduce is 16 + 3 + 2 additions deep;
      statistic rows: stem_bf16.hip sums its own stored (rounded) values -- against the fp64 tile sums of the kernel's y,
          within 256 u sum |y| and 256 u sum y^2 (256 voxels per tile, y^2 of a bf16 value is exact in fp32); stem.hip
          sums its fp32 accumulators -- against the reference's tile sums, within the sum of the element bounds
          e = 2 * 343 u A (2 |ref| e + e^2 for the squares) plus the same summation term.
    The measured worst ratios are printed."""
    lf = assert_form(ops, case)
    dt = FORMS[form][0]
    ref = reference(ops, case, "real" if form == "f32" else "real-bf16")
    y, stats, y0, dw, dw2 = run_form(ops, monkeypatch, form, ref)
    what = f"{case} {form}"
    yr, A = ref["y"], ref["A"]
    e = 2 * 343 * U * A
    yb = store_bound(yr, dt, e)
    checks = [Excess(f"{what} y"), Excess(f"{what} dw"), Excess(f"{what} statistic rows")]
    checks[0].add(y, yr, yb)
    kw = 2 * (64 * lf["wg_trips"] + 21)
    checks[1].add(dw, ref["dw"], kw * U * ref["Aw"])
    assert stats.shape == (lf["tiles"], 2, 64)
    if form == "bf16-mm":
        yk = y.double()
        s_ref = [tile_sums(yk), tile_sums(yk * yk)]
        s_bnd = [256 * U * tile_sums(yk.abs()), 256 * U * s_ref[1]]
    else:
        e2 = 2 * yr.abs() * e + e * e
        s_ref = [tile_sums(yr), tile_sums(yr * yr)]
        s_bnd = [(1 + 256 * U) * tile_sums(e) + 256 * U * tile_sums(yr.abs()),
                 (1 + 256 * U) * tile_sums(e2) + 256 * U * s_ref[1]]
    for r in range(2):
        checks[2].add(stats[:, r], s_ref[r], s_bnd[r])
    worst = lambda got, want, den: float(torch.nan_to_num((got.double() - want).abs() / den, nan=math.inf).max())
    # y beyond the one rounding of a bf16 store (2^-8 |ref|), in units of u A; fp32 storage: the whole error
    y_arith = float(torch.nan_to_num(((y.double() - yr).abs() - (0.0 if dt == F32 else UB * yr.abs())) / (U * A),
                                     nan=math.inf).max())
    with capsys.disabled():
        print(f"\n[stem {what}] tiles {lf['tiles']} fwd workgroups {lf['fwd_blocks']} trips {lf['fwd_trips']}; wgrad "
              f"sub-tiles {lf['total']} workgroups {lf['wg_blocks']} trips {lf['wg_trips']}: "
              f"y |err| / (u A) {y_arith:.1f} (allowed {2 * 343}; |err| / bound {worst(y, yr, yb):.3f}); "
              f"dw |err| / (u A_w) {worst(dw, ref['dw'], U * ref['Aw']):.1f} (allowed {kw}); "
              f"statistic rows |err| / bound {worst(stats[:, 0], s_ref[0], s_bnd[0]):.3f}, "
              f"{worst(stats[:, 1], s_ref[1], s_bnd[1]):.3f}")
    for ex in checks:
        ex.check()
    assert torch.equal(y0, y), f"{what}: y differs without statistics"
    assert torch.equal(dw2, dw), f"{what}: the weight gradient is not deterministic"
