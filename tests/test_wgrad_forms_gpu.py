"""GPU: the convolution weight gradients outside the 3-D Winograd pipeline -- the direct fp32 kernels of
csrc/conv_wgrad.hip (conv_wgrad2_kernel, the five geometry variants of conv_wgrad_kernel in their wide and narrow
tiles, wgrad_reduce_kernel), the in-plane Winograd z-walking kernel of csrc/conv_wgrad_w2d.hip with its reduce, and
the bf16 weight gradient of csrc/conv_bf16.hip in its tile and z-walking forms -- element by element against the fp64
tap loop of tests/wgrad_ref.py on the device, at the smallest shapes that select each form: one and several channel
pairs, extents ragged against the 8 x 8 column / the 32-voxel row chunk / the 2 x 2 tile, one- and two-plane volumes
(rings never full), several columns per workgroup with a ragged last slab (the ring is re-primed between columns),
uneven chunk splits, and the slab counts 1, 7, 8, 9, 15, 16, 17 around the 8-way main loop of every ordered reduce.

Part A (test_exact_*): operands in {-1, 0, 1}.  Every product and every partial sum is an integer below 2^24 (asserted
from the reference itself); the in-plane Winograd transforms have entries 0, +-1 and 1/2, so there every intermediate
is an integer and dw a multiple of 1/4.  The result then does not depend on summation order or arithmetic path: every
form must equal the reference BIT FOR BIT, and a second call the first.

Part B (test_rounding_*): normal random operands, every element held to a bound derived from the kernel's arithmetic
(the test's docstring); the measured worst ratios are printed.

Every case asserts the form it claims before it looks at a value: the slab count from the library's workspace exports
(dram_conv3d_bwd_weight_workspace, dram_wgrad_w2d_workspace, dram_conv3d_bwd_weight_bf16_workspace: bytes / one slab),
columns, columns per workgroup and the ragged last slab from it, the plan's routing from dram_conv_wgrad_algo, and
which kernel ran from the library's kernel timeline (family conv_wgrad: variant 2 is conv_wgrad2_kernel, 10 + v
conv_wgrad_kernel's geometry variant v; conv_wgrad_w2d; wgrad_bf16: 0 / 1 tile kernel / reduce, 2 / 3 z-walk / reduce).
A case whose shape the library gives another form fails with both printed: change the shape, not the assertion.
All allocations of the wrapper are poisoned (test_launch_regimes_gpu.poison), the slab workspace included (the
wrapper's cached scratch is dropped before every call): an unwritten element is NaN.
"""
import ctypes
import math

import pytest
import torch

from test_launch_regimes_gpu import BF16, DEV, F32, F64, U, Excess, ops, poison  # noqa: F401 (fixtures)
from wgrad_ref import gt_abs, wgrad_reference, wino_reference

pytestmark = pytest.mark.gpu

NSLAB = [1, 7, 8, 9, 15, 16, 17]       # around the `k + 8 <= nslab` main loop and the tail of the ordered reduces

# kind -> (DRAM_CONV_ALGO, operand type, timeline family)
KINDS = {"wgrad2": ("1", F32, "conv_wgrad"), "direct": ("1", F32, "conv_wgrad"), "w2d": ("3", F32, "conv_wgrad_w2d"),
         "bf16-tile": (None, BF16, "wgrad_bf16"), "bf16-zwalk": (None, BF16, "wgrad_bf16")}


def case(kind, B, D, H, W, Cin, Cout, k=3, stride=1, dil=1, v0=False, **claim):
    return dict(kind=kind, geom=(B, D, H, W, Cin, Cout, k, stride, dil), v0=v0, claim=claim)


# The claims are what the case is for, in the terms of launch_form() below.
CASES = {
    # ---- conv_wgrad2_kernel: stride 1, dilation 1, fp32, 8 x 8 columns walked through z
    "z-one-pair": case("wgrad2", 1, 6, 8, 10, 32, 32, nslab=2, cpw=1),
    "z-96-32": case("wgrad2", 1, 4, 16, 16, 96, 32, nslab=4, cpw=1),
    "z-ragged": case("wgrad2", 2, 5, 11, 13, 64, 64, nslab=8, cpw=1),
    "z-D1": case("wgrad2", 1, 1, 9, 12, 32, 32, nslab=4, cpw=1),
    "z-D2": case("wgrad2", 1, 2, 9, 12, 64, 32, nslab=4, cpw=1),
    # 16 pairs x 35 columns > 512 slots: two columns per workgroup, the last slab has one
    "z-cpw2": case("wgrad2", 1, 3, 40, 56, 128, 128, ncols=35, nslab=18, cpw=2, rag=1),
    "z-cpw2-ragged": case("wgrad2", 1, 3, 37, 53, 128, 128, ncols=35, nslab=18, cpw=2, rag=1),
    # ---- conv_wgrad_kernel: variants 1 .. 4 (dilation 2, dilation 4, stride 2, 1x1x1), wide (Cout % 64 == 0) and narrow
    "v1-wide": case("direct", 1, 5, 9, 7, 64, 64, dil=2, variant=1, cps=1),
    "v1-narrow": case("direct", 1, 5, 9, 7, 64, 32, dil=2, variant=1, cps=1),
    "v2-wide": case("direct", 1, 6, 10, 9, 64, 64, dil=4, variant=2, cps=1),
    "v2-narrow": case("direct", 1, 6, 10, 9, 64, 96, dil=4, variant=2, cps=1),
    "v3-wide": case("direct", 1, 9, 11, 13, 64, 64, stride=2, variant=3, cps=1),         # stride 2 on odd extents
    "v3-narrow": case("direct", 1, 9, 11, 13, 64, 32, stride=2, variant=3, cps=1),
    "v4-wide": case("direct", 2, 3, 7, 5, 64, 64, k=1, variant=4, cps=1),                # 210 voxels: not a multiple of 256
    "v4-narrow": case("direct", 2, 3, 7, 5, 64, 96, k=1, variant=4, cps=1),
    # variant 0 (stride 1, dilation 1: DRAM_WGRAD_V=1 takes the z-walking kernel away) on two of the shapes above
    "v0-ragged": case("direct", 2, 5, 11, 13, 64, 64, v0=True, variant=0, cps=1),
    "v0-D2": case("direct", 1, 2, 9, 12, 64, 32, v0=True, variant=0, cps=1),
    # more than one 32-voxel chunk per output row, the last one ragged
    "Wo33": case("direct", 1, 2, 5, 33, 64, 64, dil=2, variant=1, XC=2),
    "Wo70": case("direct", 1, 2, 3, 70, 64, 32, dil=2, variant=1, XC=3),
    "s2-Wo34": case("direct", 1, 3, 5, 67, 64, 64, stride=2, variant=3, XC=2),
    # dilation beyond every extent but one: whole taps are padding
    "dil-over": case("direct", 1, 2, 5, 3, 64, 64, dil=4, variant=2, cps=1),
    # uneven splits: 130 chunks in slabs of 3 (the last has 1), 131 in slabs of 2
    "uneven": case("direct", 1, 2, 65, 20, 128, 128, dil=2, variant=1, NC=130, nslab=44, cps=3, rag=1),
    "uneven-k1": case("direct", 1, 1, 131, 19, 128, 128, k=1, variant=4, NC=131, nslab=66, cps=2, rag=1),
    # ---- conv_wgrad_w2d_kernel
    "w-32-32": case("w2d", 1, 5, 8, 8, 32, 32, nslab=1, cpw=1),
    "w-96-96": case("w2d", 1, 4, 9, 10, 96, 96, nslab=4, cpw=1),
    "w-ragged": case("w2d", 2, 5, 11, 13, 32, 64, nslab=8, cpw=1),
    "w-D1": case("w2d", 1, 1, 9, 12, 32, 32, nslab=4, cpw=1),
    "w-D2": case("w2d", 1, 2, 9, 12, 32, 32, nslab=4, cpw=1),
    "w-H1": case("w2d", 2, 3, 1, 9, 32, 32, nslab=4, cpw=1),                              # half-empty 2 x 2 tiles
    "w-W1": case("w2d", 2, 3, 9, 1, 32, 32, nslab=4, cpw=1),
    # 4 pairs x 81 columns > 256 slots: two columns per workgroup, the last slab has one
    "w-cpw2": case("w2d", 1, 3, 72, 72, 64, 64, ncols=81, nslab=41, cpw=2, rag=1),
    "w-cpw2-ragged": case("w2d", 1, 3, 69, 69, 64, 64, ncols=81, nslab=41, cpw=2, rag=1),
    "w-cpw6": case("w2d", 1, 2, 67, 70, 128, 128, ncols=81, nslab=14, cpw=6, rag=3),
    # ---- bf16: tile form (4 x 8 x 8 lattice tiles, strided over the slabs, two in flight)
    "t-ragged": case("bf16-tile", 2, 5, 11, 13, 64, 64, units=16, nslab=8, cpw=2, rag=0),
    "t-narrow": case("bf16-tile", 2, 5, 11, 13, 64, 32, units=16, nslab=8, cpw=2, rag=0),   # half a 64-wide co block
    "t-multi": case("bf16-tile", 1, 9, 17, 24, 64, 64, units=27, nslab=13, cpw=3, rag=1),   # 3 tiles, or 2: an odd trip
    "t-dil2": case("bf16-tile", 1, 6, 10, 9, 64, 32, dil=2, units=8, nslab=4, cpw=2, rag=0),
    # ---- bf16: z-walking form (8 x 8 lattice columns, strided over the slabs)
    "zw-ragged": case("bf16-zwalk", 2, 5, 11, 13, 64, 64, units=8, nslab=8, cpw=1, rag=0),
    "zw-narrow": case("bf16-zwalk", 2, 5, 11, 13, 64, 32, units=8, nslab=8, cpw=1, rag=0),  # the one-co-half kernel
    "zw-zseg": case("bf16-zwalk", 1, 9, 17, 24, 64, 64, units=18, nslab=18, cpw=1, rag=0),   # two z segments (5 + 4 planes)
    # 384 columns of the dilation-4 lattice on 256 slabs: two columns, or one; residue classes of 3 and 2 planes
    "zw-multi": case("bf16-zwalk", 1, 9, 40, 68, 64, 64, dil=4, units=384, nslab=256, cpw=2, rag=128),
    "zw-dil2": case("bf16-zwalk", 1, 6, 10, 9, 64, 32, dil=2, units=8, nslab=8, cpw=1, rag=0),
}
# ---- the ordered reduces at their boundary slab counts
for _n in NSLAB:
    # wgrad_reduce_kernel behind conv_wgrad_kernel: one chunk per output row, one slab per chunk
    CASES[f"r-direct-{_n}"] = case("direct", 1, 1, _n, 20, 64, 32, dil=2, variant=1, NC=_n, nslab=_n, cps=1)
    # ... and behind conv_wgrad2_kernel; wgrad_w2d_reduce_kernel: _n columns of one 8 x 8 tile
    CASES[f"r-z-{_n}"] = case("wgrad2", _n, 2, 8, 8, 32, 32, ncols=_n, nslab=_n, cpw=1)
    CASES[f"r-w-{_n}"] = case("w2d", _n, 2, 8, 8, 32, 32, ncols=_n, nslab=_n, cpw=1)
    CASES[f"r-t-{_n}"] = case("bf16-tile", 2 * _n, 3, 8, 8, 64, 64, units=2 * _n, nslab=_n, cpw=2, rag=0)
    CASES[f"r-zw-{_n}"] = case("bf16-zwalk", _n, 3, 8, 8, 64, 64, units=_n, nslab=_n, cpw=1, rag=0)

BF16_CASES = [c for c, v in CASES.items() if v["kind"].startswith("bf16")]
F32_CASES = [c for c in CASES if c not in BF16_CASES]
# Part B: one ragged and one several-columns (chunks, tiles) case per kernel
ROUNDING_CASES = ["z-ragged", "z-cpw2-ragged", "v3-wide", "uneven", "w-ragged", "w-cpw2-ragged", "t-ragged", "t-multi",
                  "zw-ragged", "zw-multi"]


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the form of a case
def set_env(monkeypatch, name, nw=None):
    c = CASES[name]
    algo = KINDS[c["kind"]][0]
    for key, val in (("DRAM_CONV_ALGO", algo), ("DRAM_WGRAD_V", "1" if c["v0"] else None),
                     ("DRAM_BF16_WGRAD", c["kind"][5:] if c["kind"].startswith("bf16") else None), ("DRAM_BF16_NW", nw)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)


def geom_of(ops, name):
    B, D, H, W, Cin, Cout, k, stride, dil = CASES[name]["geom"]
    return ops.ConvGeom(B, D, H, W, Cin, Cout, k, stride, dil * (k - 1) // 2, dil)


def launch_form(ops, name):
    """The form the library gives the case's shape under the environment set_env() set, from its sizing exports alone."""
    L = ops._L()
    kind = CASES[name]["kind"]
    g = geom_of(ops, name)
    d = ctypes.byref(g.desc())
    form = dict(walgo=int(L.dram_conv_wgrad_algo(d)))
    if kind in ("wgrad2", "direct"):
        nbytes, slab = int(L.dram_conv3d_bwd_weight_workspace(d)), g.taps * g.Cout * g.Cin * 4
    elif kind == "w2d":
        nbytes, slab = int(L.dram_wgrad_w2d_workspace(d)), 48 * g.Cout * g.Cin * 4
    else:                       # slabs are whole 64-wide blocks of output channels
        assert L.dram_conv_bf16_supported(d) == 1
        nbytes, slab = int(L.dram_conv3d_bwd_weight_bf16_workspace(d)), 27 * cdiv(g.Cout, 64) * 64 * g.Cin * 4
    assert nbytes > 0 and nbytes % slab == 0, f"{name}: workspace {nbytes} bytes, one slab {slab}"
    form["nslab"] = ns = nbytes // slab
    if kind in ("wgrad2", "w2d"):
        form["ncols"] = nc = g.B * cdiv(g.H, 8) * cdiv(g.W, 8)
        form["cpw"] = cdiv(nc, ns)
        form["rag"] = nc % form["cpw"]
        assert ns == cdiv(nc, form["cpw"])
        # voxels (w2d: 2 x 2 tiles) one workgroup folds into an accumulator
        form["n"] = form["cpw"] * g.D * (64 if kind == "wgrad2" else 16)
    elif kind == "direct":
        make_plan2 = g.k == 3 and g.stride == 1 and g.dil == 1 and not CASES[name]["v0"]
        form["variant"] = -1 if make_plan2 else {(3, 1, 1): 0, (3, 1, 2): 1, (3, 1, 4): 2, (3, 2, 1): 3,
                                                 (1, 1, 1): 4}[(g.k, g.stride, g.dil)]
        form["XC"] = cdiv(g.Wo, 32)
        form["NC"] = nc = g.B * g.Do * g.Ho * form["XC"]
        form["cps"] = cdiv(nc, ns)
        form["rag"] = nc % form["cps"]
        assert ns == cdiv(nc, form["cps"])
        form["n"] = form["cps"] * 32
    else:
        lat = lambda n, per: cdiv(cdiv(n, g.dil), per)
        cols = g.B * g.dil ** 3 * lat(g.H, 8) * lat(g.W, 8)
        if kind == "bf16-tile":
            units, vox = cols * lat(g.D, 4), 256
        else:
            # z segments per column (plan_zwalk): doubled while the launch is under 512 workgroups and a segment keeps
            # 4 planes; mirrored here, and checked against the slab count the library reports
            Lz, npairs, nzs = cdiv(g.D, g.dil), (g.Cin // 64) * cdiv(g.Cout, 64), 1
            while cols * nzs * npairs < 512 and Lz // (nzs * 2) >= 4:
                nzs *= 2
            units, vox = cols * nzs, 64 * cdiv(Lz, nzs)
            assert ns == min(cdiv(1024, npairs), units, 256), f"{name}: {ns} slabs for {units} column segments"
        form["units"] = units
        form["cpw"] = cdiv(units, ns)          # the busiest workgroup's share (units are dealt out round-robin)
        form["rag"] = units % ns               # workgroups that fold one more than the idlest (0: all the same)
        form["n"] = form["cpw"] * vox
    return form


def assert_form(ops, name):
    c = CASES[name]
    form = launch_form(ops, name)
    want_algo = {"wgrad2": 0, "direct": 0, "w2d": 2}.get(c["kind"])
    if want_algo is not None:
        assert form["walgo"] == want_algo, f"{name}: dram_conv_wgrad_algo plans {form['walgo']}, the case is for {want_algo}"
    got ={k: form.get(k) for k in c["claim"]}
    assert got == c["claim"], f"{name}: the library gives this shape the form {form}, the case claims {c['claim']}"
    return form


# ------------------------------------------------------------------------------------------------ reference
_REF = {}


def operands(name, kind):
    """host draws (the same values on every machine): "int" i.i.d. in {-1, 0, 1}; "real" normal, rounded to bf16 first
    for the bf16 kernels (the reference sees the operands the kernel sees)"""
    c = CASES[name]
    B, D, H, W, Cin, Cout, k, stride, dil = c["geom"]
    pad = dil * (k - 1) // 2
    oshape = tuple((n + 2 * pad - (dil * (k - 1) + 1)) // stride + 1 for n in (D, H, W))
    gen = torch.Generator().manual_seed(sum(c["geom"]) + 1000 * W + (0 if kind == "int" else 7))
    if kind == "int":
        x = torch.randint(-1, 2, (B, D, H, W, Cin), generator=gen).float()
        dy = torch.randint(-1, 2, (B,) + oshape + (Cout,), generator=gen).float()
    else:
        x = torch.randn((B, D, H, W, Cin), generator=gen)
        dy = torch.randn((B,) + oshape + (Cout,), generator=gen)
    dt = KINDS[c["kind"]][1]
    return x.to(dt).to(DEV), dy.to(dt).to(DEV)


def reference(ops, name, kind):
    """dict(x, dy: device operands in the kernel's type; dw, Aw: float64; wino: wino_reference() for the real-data
    in-plane Winograd cases), computed once per (case, kind), shared, never written to"""
    key = (name, kind)
    if key not in _REF:
        c = CASES[name]
        B, D, H, W, Cin, Cout, k, stride, dil = c["geom"]
        x, dy = operands(name, kind)
        if kind == "int":
            assert torch.equal(x.double(), x.double().round()) and float(x.abs().max()) == 1.0     # exact in bf16 too
        dw, Aw = wgrad_reference(x, dy, k, stride, dil * (k - 1) // 2, dil, want_mag=True)
        wino = None
        if kind == "int":       # the exact regime, from the reference itself
            assert float(Aw.max()) < 2 ** 24 and float(dw.abs().max()) > 0
            if c["kind"] == "w2d":
                assert 16 * B * D * H * W < 2 ** 24         # |A dy A^T| <= 4, |B^T x B| <= 4, one product per voxel and point
        elif c["kind"] == "w2d":
            wino = wino_reference(x, dy)
            assert bool(((wino["dw"] - dw).abs() <= 1e-12 * gt_abs(wino["M_abs"])).all())
        _REF[key] = dict(x=x, dy=dy, dw=dw, Aw=Aw, wino=wino)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ running a case
def timeline_claim(name, form):
    kind = CASES[name]["kind"]
    if kind == "wgrad2":
        return {2: 2}
    if kind == "direct":
        return {10 + form["variant"]: 2}
    if kind == "w2d":
        return {0: 2}
    return {0: 2, 1: 2} if kind == "bf16-tile" else {2: 2, 3: 2}


def run_case(ops, name, form, ref):
    """the weight gradient twice through ops.conv3d_bwd_weight, with a fresh (poisoned) slab workspace each time, under
    the kernel timeline: the launches must be the claimed kernel's and nothing else"""
    g = geom_of(ops, name)
    family = KINDS[CASES[name]["kind"]][2]
    tl = ops.KernelTimeline(64)
    tl.start()
    try:
        ops._WORKSPACE.clear()
        dw = ops.conv3d_bwd_weight(ref["x"], ref["dy"], g)
        ops._WORKSPACE.clear()
        dw2 = ops.conv3d_bwd_weight(ref["x"], ref["dy"], g)
        fam = tl.families()
    finally:
        tl.stop()
    ran = {f: {v: n for v, (n, _) in r["variants"].items()} for f, r in fam.items()}
    assert ran == {family: timeline_claim(name, form)}, f"{name}: launches by family and variant {ran}"
    assert dw.dtype == F32 and dw.shape == (g.Cout, g.Cin, g.k, g.k, g.k)
    return dw, dw2


def assert_same(got, want, what):
    """bit-for-bit (as values: got widened to float64); NaN -- an unwritten element -- differs"""
    got = got.double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, the first at (co, ci, kz, ky, kx) = "
                             f"{i}: {float(got[i])} for {float(want[i])}")


def check_exact(ops, monkeypatch, capsys, name, nw=None):
    set_env(monkeypatch, name, nw)
    form = assert_form(ops, name)
    ref = reference(ops, name, "int")
    dw, dw2 = run_case(ops, name, form, ref)
    with capsys.disabled():
        print(f"\n[wgrad exact {name}{'' if nw is None else ' NW=' + nw}] {CASES[name]['kind']} {CASES[name]['geom']}: {form}")
    assert_same(dw, ref["dw"], name)
    assert torch.equal(dw2, dw), f"{name}: the weight gradient is not deterministic"
    return form


@pytest.mark.parametrize("name", [c for c in F32_CASES if not c.startswith("r-")])
def test_exact_fp32(ops, poison, monkeypatch, capsys, name):
    """Part A: dw equals the fp64 tap loop bit for bit, in the claimed form, twice."""
    check_exact(ops, monkeypatch, capsys, name)


@pytest.mark.parametrize("n", NSLAB)
@pytest.mark.parametrize("behind", ["direct", "z", "w"])
def test_exact_slab_reduce_boundaries_fp32(ops, poison, monkeypatch, capsys, behind, n):
    """Part A with exactly n slabs: wgrad_reduce_kernel behind conv_wgrad_kernel (n one-chunk rows) and behind
    conv_wgrad2_kernel (n columns), wgrad_w2d_reduce_kernel (n columns) -- each boundary of the 8-way main loop and tail"""
    form = check_exact(ops, monkeypatch, capsys, f"r-{behind}-{n}")
    assert form["nslab"] == n


@pytest.mark.parametrize("nw", ["4", "8"])
@pytest.mark.parametrize("name", [c for c in BF16_CASES if not c.startswith("r-")])
def test_exact_bf16(ops, poison, monkeypatch, capsys, name, nw):
    """Part A for the bf16 weight gradient (bf16 x and dy, fp32 dw): DRAM_BF16_WGRAD = tile | zwalk x DRAM_BF16_NW
    (which sizes the forward's tiles: the weight gradient's form and bits must not depend on it)"""
    check_exact(ops, monkeypatch, capsys, name, nw)


@pytest.mark.parametrize("nw", ["4", "8"])
@pytest.mark.parametrize("n", NSLAB)
@pytest.mark.parametrize("wform", ["t", "zw"])
def test_exact_slab_reduce_boundaries_bf16(ops, poison, monkeypatch, capsys, wform, n, nw):
    """Part A with exactly n slabs behind the bf16 tile and z-walking kernels (wgrad3_bf16_reduce_kernel, per-result form)"""
    form = check_exact(ops, monkeypatch, capsys, f"r-{wform}-{n}", nw)
    assert form["nslab"] == n


def test_multi_column_cases_are_multi_column(ops, monkeypatch):
    """what the several-columns cases are for, from the sizing exports: every z-walking kernel has a case whose workgroups
    own two or more columns with a ragged last slab, conv_wgrad_kernel an uneven chunk split"""
    for name, cpw in (("z-cpw2", 2), ("z-cpw2-ragged", 2), ("w-cpw2", 2), ("w-cpw2-ragged", 2), ("w-cpw6", 3)):
        set_env(monkeypatch, name)
        f = assert_form(ops, name)
        assert f["cpw"] >= cpw and f["rag"] != 0 and f["nslab"] * f["cpw"] > f["ncols"]
    for name in ("uneven", "uneven-k1"):
        set_env(monkeypatch, name)
        f = assert_form(ops, name)
        assert f["cps"] >= 2 and f["rag"] != 0 and f["nslab"] * f["cps"] > f["NC"]
    for name in ("t-multi", "zw-multi"):
        set_env(monkeypatch, name)
        f = assert_form(ops, name)
        assert f["cpw"] >= 2 and f["rag"] != 0


# ------------------------------------------------------------------------------------------------ Part B
def worst_ratio(got, want, bound):
    """max |got - want| / bound; an element whose bound is 0 (every product in the padding) must be exact"""
    err = (got.double() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf))
    return float(torch.nan_to_num(r, nan=math.inf).max())


@pytest.mark.parametrize("name", ROUNDING_CASES)
def test_rounding_on_real_data(ops, poison, monkeypatch, capsys, name):
    """Part B: normal random x and dy (rounded to bf16 first for the bf16 kernels), u = 2^-24, every element of dw.

    Direct fp32 and bf16 kernels: an element is a chain of at most n additions of products into one accumulator --
    n the voxels one workgroup folds (columns per workgroup x planes x 64; chunks per slab x 32; tiles x 256), each
    product rounded once (fp32 operands) or exact (bf16 operands) -- and then the reduce's at most nslab + 8 additions:
        |dw - ref| <= (n + nslab + 8) u A_w,    A_w = sum |dy| |x|.

    In-plane Winograd kernel, to first order in u.  With U the sum in the Winograd domain (per z tap and point),
    M = sum |A dy A^T| |B^T x B| and M_abs = sum (|A| |dy| |A^T|) (|B^T| |x| |B|) >= M, n = 16 cpw D the 2 x 2 tiles a
    workgroup folds:
      * B^T x B is one multiplication by +-1 (exact) and three FMAs: 3 roundings, each relative to the running sum of
        |x| terms -- 3 u (|B^T| |x| |B|) per factor; A dy A^T likewise 3 u (|A| |dy| |A^T|).  Together 6 u M_abs.
      * the accumulation: n products and additions in one chain, then the reduce's nslab + 8: (n + nslab + 8) u M.
      * gt3w rounds twice per output (0.5 * is exact) and is applied twice: 4 u |G^T| |U| |G| <= 4 u |G^T| M |G|.
        |dw - ref| <= |G^T| (6 u M_abs + (n + nslab + 12) u M) |G|.
    The constant differs from a bound on M alone because the transforms round relative to the magnitudes of their
    terms, not of their (cancelling) sum.  The measured worst ratio error / bound is printed."""
    set_env(monkeypatch, name)
    form = assert_form(ops, name)
    ref = reference(ops, name, "real")
    dw, dw2 = run_case(ops, name, form, ref)
    n, ns = form["n"], form["nslab"]
    if CASES[name]["kind"] == "w2d":
        w = ref["wino"]
        bound = gt_abs(6 * U * w["M_abs"] + (n + ns + 12) * U * w["M"])
        told = f"|err| / bound {worst_ratio(dw, ref['dw'], bound):.4f} (6 u M_abs + {n + ns + 12} u M through |G^T| . |G|)"
    else:
        bound = (n + ns + 8) * U * ref["Aw"]
        told = (f"|err| / (u A_w) {worst_ratio(dw, ref['dw'], U * ref['Aw']):.2f} (allowed {n + ns + 8}); |err| / bound "
                f"{worst_ratio(dw, ref['dw'], bound):.4f}")
    with capsys.disabled():
        print(f"\n[wgrad rounding {name}] {CASES[name]['kind']} {CASES[name]['geom']}: {form}: {told}")
    ex = Excess(f"{name} dw")
    ex.add(dw, ref["dw"], bound)
    ex.check()
    assert torch.equal(dw2, dw), f"{name}: the weight gradient is not deterministic"
