"""GPU: the forward and data-gradient convolutions of the bf16-storage path (csrc/conv_bf16.hip) -- conv3_bf16_kernel
<NB, EPI, NW> in its eight instantiations, gemm1_bf16_kernel<NB, EPI> in its four, the stride-2 route through
s2d_bf16_kernel / dram_s2_embed_weight / d2s_bf16_kernel, and the two cast kernels -- element by element against the
fp64 tap loops of tests/conv_ref.py on the device, at the smallest shapes that select each form: one workgroup and one
channel chunk (`last` on the first chunk), 2, 3 and 18 chunks (the 3-slot weight ring across chunk boundaries), 32- and
64-column tiles in either pass, extents of one voxel, lattices ragged against the 4- / 8-plane x 8 x 8 tile, dilations
2 and 4 down to residue classes without a voxel, a workgroup count that is no multiple of 8 (xcd_remap's remainder),
one and several 256-row tiles of the 1x1x1 GEMM with an odd and an even number of K chunks, its 128-column tiles just
above and just below the 512-workgroup threshold.  tests/test_bf16_gpu.py stays the network-sized, coarse layer
(relative L2 of whole tensors); a wrong halo voxel, a dropped tap or a stale ring slot passes there and fails here.

Part A (test_exact_*): operands are small integers, exact in bf16 (x, dy, add in {-1, 0, 1}; weights in {-1, 0, 1}, in
one case per kernel from a wider set so that results pass 256 and are rounded; gate in {-1, -0.0, 0, 1}).  Every
product and every partial sum is an integer below 2^24 (asserted from the reference itself: max A < 2^24), so neither
the summation order nor the MFMA grouping can change a bit: the output must equal the reference, rounded ONCE to
nearest even, BIT FOR BIT, a second call the first, and the BatchNorm sums (per-channel sum of the rounded y^2 < 2^24,
asserted) the fp64 sums of the rounded output exactly, row by row and in total.

test_exact_conv3_under_memory_load repeats Part A for five conv3 cases while a second stream saturates HBM: the LDS-DMA of
the weight ring then lands late enough for a missing wait to show.

Part B (test_rounding_*): normal random operands (rounded to bf16 first: the reference sees what the kernel sees),
every element held to a bound derived from the kernel's arithmetic (the tests' docstrings); the measured worst ratios
are printed.

Every case asserts the form it claims before it looks at a value: the only launches on the library's kernel timeline
are of family conv_bf16 with the claimed variant (conv3_bf16_kernel: epi * 4 + (NW == 8 ? 2 : 0) + (NB - 1);
gemm1_bf16_kernel: 8 + epi * 2 + (NB == 4); the stride-2 route adds the bn_elementwise variants 9 and 10 of its
space-to-depth and depth-to-space launches), and the derived counts (lattice tiles per axis, channel chunks, workgroups,
workgroups % 8) are recomputed here from the geometry exactly as fill_tiles / launch_conv / launch_gemm1 compute them and
checked against ops.conv_plan(g).bf16_stat_rows.  A case whose shape the library gives another form fails with both
printed: change the shape, not the assertion.  All allocations of the wrappers are poisoned
(test_launch_regimes_gpu.poison): an unwritten output element or statistic row is NaN.

Not covered: tensors beyond 4 GB (the 64-bit descriptor bases of conv3_bf16_kernel) -- they cannot be tested in seconds.
"""
import math
import zlib

import pytest
import torch

from test_launch_regimes_gpu import BF16, DEV, F32, F64, U, Excess, check_sums, ops, poison  # noqa: F401 (fixtures)
from conv_ref import conv_reference, dgrad_reference, to_bf16_rne

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -8             # bf16 unit roundoff: half an ulp, relative
NWS = ["4", "8"]            # DRAM_BF16_NW: z-slices (waves) per conv3_bf16_kernel tile


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the cases
# name -> (pass kinds, geometry (B, D, H, W, Cin, Cout, k, stride, dil), claim).  The claim is what the case is for, in
# the terms of pass_form() below: per pass the 32-column blocks NB of a tile and the K chunks, and whatever else the case
# exercises.  `wide`: weights drawn from {-wide .. wide} (results pass 256: RNE ties), thinned to the fraction `keep`.
def c3(B, D, H, W, Cin, Cout, dil, fwd, dgrad, **more):
    """conv3_bf16_kernel: k = 3, stride 1, pad = dil; fwd / dgrad = (NB, chunks)"""
    return (("fwd", "dgrad"), (B, D, H, W, Cin, Cout, 3, 1, dil),
            dict(fwd=dict(nb=fwd[0], chunks=fwd[1]), dgrad=dict(nb=dgrad[0], chunks=dgrad[1]), **more))


def g1(kinds, B, D, H, W, Cin, Cout, **more):
    """gemm1_bf16_kernel: k = 1; more: per pass dict(nb, chunks, ...)"""
    return (kinds, (B, D, H, W, Cin, Cout, 1, 1, 1), more)


def s2(B, D, H, W, Cin, Cout, fwd, dgrad, **more):
    """the stride-2 route: k = 3, stride 2, pad 1; the claims are those of the stride-1 launch on (D/2, H/2, W/2, 8 Cin)"""
    return (("fwd", "dgrad"), (B, D, H, W, Cin, Cout, 3, 2, 1),
            dict(fwd=dict(nb=fwd[0], chunks=fwd[1]), dgrad=dict(nb=dgrad[0], chunks=dgrad[1]), **more))


CASES = {
    # ---- conv3_bf16_kernel.  The forward takes NB from Cout and its chunks from Cin; the data gradient swaps them.
    "one-tile": c3(1, 4, 8, 8, 32, 32, 1, (1, 1), (1, 1), nblk=1, wide=8),      # `last` is true on the first chunk
    "ragged": c3(1, 5, 9, 7, 64, 64, 1, (2, 2), (2, 2)),                # ragged on all three axes
    "three-chunks": c3(2, 3, 10, 17, 96, 32, 1, (1, 3), (1, 1)),        # dgrad: 3 channel tiles
    "nb-mixed": c3(1, 6, 9, 11, 64, 32, 1, (1, 2), (2, 1)),
    "18-chunks": c3(1, 4, 8, 8, 576, 64, 1, (2, 18), (2, 2), wide=8),   # the weight ring across 18 chunk boundaries
    "D1": c3(1, 1, 9, 12, 64, 64, 1, (2, 2), (2, 2)),                   # every neighbour along the axis is padding
    "H1": c3(2, 3, 1, 9, 32, 64, 1, (2, 1), (1, 2)),
    "W1": c3(2, 3, 9, 1, 32, 64, 1, (2, 1), (1, 2)),
    "z9": c3(1, 9, 8, 8, 64, 64, 1, (2, 2), (2, 2), tz={"4": 3, "8": 2}),      # the last z tile has one plane
    "z16": c3(1, 16, 8, 8, 64, 64, 1, (2, 2), (2, 2), tz={"4": 4, "8": 2}),    # full 8-plane tiles
    "d2": c3(1, 9, 12, 10, 128, 64, 2, (2, 4), (2, 2)),
    "d2-small": c3(1, 5, 9, 7, 64, 64, 2, (2, 2), (2, 2)),
    "d4": c3(1, 6, 10, 9, 64, 32, 4, (1, 2), (2, 1)),
    "dil-over": c3(1, 2, 5, 3, 64, 64, 4, (2, 2), (2, 2), empty_rows=40),      # residue classes with no voxel at all
    "wg-18": c3(3, 4, 9, 17, 64, 64, 1, (2, 2), (2, 2), nblk=18, rem=2),       # xcd_remap's remainder
    # ---- gemm1_bf16_kernel
    "g-210": g1(("fwd", "dgrad"), 2, 3, 7, 5, 64, 64, fwd=dict(nb=2, chunks=1, rows=1), dgrad=dict(nb=2, chunks=1),
                wide=32),                                                      # one ragged row tile, one K chunk
    "g-315": g1(("fwd", "dgrad"), 1, 5, 9, 7, 256, 128, fwd=dict(nb=2, chunks=4, rows=2), dgrad=dict(nb=2, chunks=2)),
    # 3 chunks forward and 5 backward: the double buffer ends on either stage; 320 is not a multiple of 128
    "g-odd": g1(("fwd", "dgrad"), 1, 8, 8, 9, 192, 320, fwd=dict(nb=2, chunks=3, rows=3, n_tiles=5),
                dgrad=dict(nb=2, chunks=5, n_tiles=3)),
    # 257 row tiles, the last with 60 rows; 514 workgroups: 128-column tiles
    "g-nb4-fwd": g1(("fwd",), 1, 31, 46, 46, 64, 256, fwd=dict(nb=4, chunks=1, rows=257, tail=60, nblk=514)),
    "g-nb4-dgrad": g1(("dgrad",), 1, 31, 46, 46, 256, 64, dgrad=dict(nb=4, chunks=1, rows=257, tail=60, nblk=514)),
    "g-nb4-k2": g1(("fwd",), 1, 31, 46, 46, 128, 256, fwd=dict(nb=4, chunks=2, nblk=514)),     # both stages, 128 columns
    # 251 row tiles x 2 = 502 < 512 tiles of 128 columns: must still be 64-column tiles
    "g-nb4-under": g1(("fwd",), 1, 31, 46, 45, 64, 256, fwd=dict(nb=2, chunks=1, rows=251, nblk=1004)),
    # ---- the stride-2 route
    "s2-222": s2(1, 2, 2, 2, 8, 32, (1, 2), (2, 1), cmin=True),                # every non-central parity is padding
    # (wide: the gradient of the space-to-depth tensor passes 256, so rounding it BEFORE the epilogue shows)
    "s2-468": s2(1, 4, 6, 8, 32, 64, (2, 8), (2, 2), wide=32, keep=0.3),
    "s2-b2": s2(2, 4, 6, 8, 8, 64, (2, 2), (2, 2), cmin=True),
    "s2-b2-c32": s2(2, 4, 6, 8, 32, 32, (1, 8), (2, 1)),
}
CONV3_CASES = [n for n, c in CASES.items() if c[1][6:8] == (3, 1)]
GEMM1_CASES = [n for n, c in CASES.items() if c[1][6] == 1]
S2_CASES = [n for n, c in CASES.items() if c[1][6:8] == (3, 2)]
# Part B: one ragged and one multi-tile case per kernel and epilogue (NB 1 and 2 / 2 and 4 in either pass)
ROUNDING_CONV3 = ["ragged", "nb-mixed", "three-chunks", "wg-18", "d2-small"]
ROUNDING_GEMM1 = ["g-210", "g-315", "g-nb4-fwd", "g-nb4-dgrad"]
ROUNDING_S2 = ["s2-468", "s2-b2"]


def kernel_of(name):
    k, stride = CASES[name][1][6:8]
    return "gemm1" if k == 1 else ("conv3" if stride == 1 else "s2")


# ------------------------------------------------------------------------------------------------ the form of a case
def set_env(monkeypatch, nw):
    if nw is None:
        monkeypatch.delenv("DRAM_BF16_NW", raising=False)
    else:
        monkeypatch.setenv("DRAM_BF16_NW", nw)
    monkeypatch.delenv("DRAM_BF16_S2", raising=False)


def geoms_of(ops, name):
    """(the case's geometry, the geometry the bf16 kernel is launched with: the space-to-depth one for stride 2)"""
    B, D, H, W, Cin, Cout, k, stride, dil = CASES[name][1]
    g = ops.ConvGeom(B, D, H, W, Cin, Cout, k, stride, dil * (k - 1) // 2, dil)
    if stride == 1:
        assert ops.conv_plan(g).bf16, f"{name}: not a geometry of the bf16 kernels"
        return g, g
    gk = ops.s2_geom(g)
    assert gk is not None and not ops.conv_plan(g).bf16, f"{name}: not a geometry of the stride-2 route"
    return g, gk


def pass_form(gk, p, nw):
    """The launch of pass p ("fwd" | "dgrad") on the kernel geometry gk, as launch_conv / launch_gemm1 derive it."""
    cin, cout = (gk.Cin, gk.Cout) if p == "fwd" else (gk.Cout, gk.Cin)
    epi = 0 if p == "fwd" else 1
    if gk.k == 3:
        nwi = int(nw)
        nb = 2 if cout % 64 == 0 else 1                                  # pick_nb
        lat = lambda n, per: cdiv(cdiv(n, gk.dil), per)                  # fill_tiles
        tiles = (lat(gk.D, nwi), lat(gk.H, 8), lat(gk.W, 8))
        rows = gk.B * gk.dil ** 3 * math.prod(tiles)
        n_tiles = cout // (32 * nb)
        return dict(kernel=f"conv3_bf16_kernel<{nb}, {epi}, {nwi}>", nb=nb, chunks=cin // 32, n_tiles=n_tiles, tiles=tiles,
                    rows=rows, nblk=rows * n_tiles, rem=rows * n_tiles % 8, variant=epi * 4 + (2 if nwi == 8 else 0) + nb - 1,
                    tile_vox=64 * nwi)
    M = gk.B * gk.D * gk.H * gk.W
    rows = cdiv(M, 256)
    nb = 4 if cout % 128 == 0 else 2
    if nb == 4 and rows * (cout // 128) < 512:
        nb = 2
    n_tiles = cout // (32 * nb)
    return dict(kernel=f"gemm1_bf16_kernel<{nb}, {epi}>", nb=nb, chunks=cin // 64, n_tiles=n_tiles, rows=rows,
                tail=M - (rows - 1) * 256, nblk=rows * n_tiles, rem=rows * n_tiles % 8, variant=8 + epi * 2 + (nb == 4),
                tile_vox=256)


def claimed_forms(name, gk, nw):
    kinds, _, claim = CASES[name]
    forms = {p: pass_form(gk, p, nw) for p in kinds}
    for p, f in forms.items():
        want = dict(claim.get(p, {}))
        for key in ("nblk", "rem"):                   # case-level claims hold for every pass of a conv3 case
            if key in claim:
                want[key] = claim[key]
        if "tz" in claim:
            want["tz"], f = claim["tz"][nw], dict(f, tz=f["tiles"][0])
        got = {k: f.get(k) for k in want}
        assert got == want, f"{name} {p}: the library's rules give this shape the form {f}, the case claims {want}"
    return forms


def assert_form(ops, name, nw):
    g, gk = geoms_of(ops, name)
    forms = claimed_forms(name, gk, nw)
    rows = ops.conv_plan(gk).bf16_stat_rows
    mine = pass_form(gk, "fwd", nw)["rows"]
    assert rows == mine, f"{name}: the library plans {rows} statistic rows, the mirrored tiling has {mine}"
    claim = CASES[name][2]
    if claim.get("cmin"):
        B, D, H, W, Cin, Cout = CASES[name][1][:6]
        smallest = min(c for c in range(1, 65) if ops.s2_geom(ops.ConvGeom(B, D, H, W, c, Cout, 3, 2, 1, 1)) is not None)
        assert Cin == smallest, f"{name}: the smallest Cin ops.s2_geom accepts is {smallest}"
    if name == "wg-18":
        assert all(f["nblk"] % 8 != 0 and f["nblk"] > 8 for f in forms.values())
    if name == "g-nb4-under":
        f = forms["fwd"]
        assert 500 <= f["rows"] * (gk.Cout // 128) <= 511 and f["nb"] == 2
    return g, gk, forms


def tile_rows(gk, nw):
    """[B, D, H, W] (device, int64): the statistic row = lattice tile (decode_tile's order) or 256-row tile of a voxel"""
    B, D, H, W = gk.B, gk.D, gk.H, gk.W
    if gk.k == 1:
        return (torch.arange(B * D * H * W, device=DEV) // 256).view(B, D, H, W)
    d, nwi = gk.dil, int(nw)
    f = pass_form(gk, "fwd", nw)
    Tz, Ty, Tx = f["tiles"]
    ar = lambda n: torch.arange(n, device=DEV)
    b, z, y, x = ar(B).view(B, 1, 1, 1), ar(D).view(1, D, 1, 1), ar(H).view(1, 1, H, 1), ar(W).view(1, 1, 1, W)
    cls = ((b * d + z % d) * d + y % d) * d + x % d
    return ((cls * Tz + (z // d) // nwi) * Ty + (y // d) // 8) * Tx + (x // d) // 8


# ------------------------------------------------------------------------------------------------ operands, reference
_REF = {}
GATE_VALUES = [-1.0, -0.0, 0.0, 1.0]


def operands(name, kind):
    """host draws (the same values on every machine).  "int": x, dy, add in {-1, 0, 1}, weights in {-1, 0, 1} or, for a
    `wide` case, in {-wide .. wide} thinned so that an output's variance stays near 2^14 (results pass 256, the sum of
    their squares stays below 2^24), bias in {-2 .. 2}, gate in {-1, -0.0, 0, 1}.  "real": normal, rounded to bf16
    (weights scaled by 0.1; the bias stays fp32, as the kernel takes it)."""
    _, (B, D, H, W, Cin, Cout, k, stride, dil), claim = CASES[name]
    pad = dil * (k - 1) // 2
    oshape = (B,) + tuple((n + 2 * pad - (dil * (k - 1) + 1)) // stride + 1 for n in (D, H, W)) + (Cout,)
    ishape, wshape = (B, D, H, W, Cin), (Cout, Cin, k, k, k)
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) + (0 if kind == "int" else 7))
    if kind == "int":
        tri = lambda shape: torch.randint(-1, 2, shape, generator=gen).float()
        x, dy, add = tri(ishape), tri(oshape), tri(ishape)
        a = claim.get("wide")
        if a:
            Kmax = k ** 3 * max(Cin, Cout)
            keep = claim.get("keep", min(1.0, 2.0 ** 14 / (Kmax * (2 / 3) * a * (a + 1) / 3)))
            w = (torch.randint(-a, a + 1, wshape, generator=gen) * (torch.rand(wshape, generator=gen) < keep)).float()
        else:
            w = tri(wshape)
        bias = torch.randint(-2, 3, (Cout,), generator=gen).float()
        gate = torch.tensor(GATE_VALUES)[torch.randint(0, 4, ishape, generator=gen)]
    else:
        nrm = lambda shape: torch.randn(shape, generator=gen).to(BF16).float()
        x, dy, add, gate = nrm(ishape), nrm(oshape), nrm(ishape), nrm(ishape)
        w = (torch.randn(wshape, generator=gen) * 0.1).to(BF16).float()
        bias = torch.randn((Cout,), generator=gen)
    return dict(x=x.to(BF16).to(DEV), dy=dy.to(BF16).to(DEV), add=add.to(BF16).to(DEV), gate=gate.to(BF16).to(DEV),
                w=w.to(DEV), bias=bias.to(DEV))


def reference(name, kind):
    """operands (device, in the kernel's types) and the fp64 results -- y, Ay (no bias), dx, Adx (no epilogue) --
    computed once per (case, kind), shared, never written to"""
    key = (name, kind)
    if key not in _REF:
        kinds, (B, D, H, W, Cin, Cout, k, stride, dil), _ = CASES[name]
        r = operands(name, kind)
        if kind == "int":
            for t in (r["x"], r["dy"], r["add"], r["w"], r["bias"]):
                assert torch.equal(t.double(), t.double().round()) and float(t.abs().max()) <= 32
            assert torch.equal(r["w"], r["w"].to(BF16).float())
            gv = r["gate"].float()
            assert float(gv.abs().max()) == 1.0 and int(torch.signbit(gv[gv == 0]).sum()) > 0     # -0.0 survived
        pad = dil * (k - 1) // 2
        if "fwd" in kinds:
            r["y"], r["Ay"] = conv_reference(r["x"], r["w"], None, k, stride, pad, dil, want_mag=True)
        if "dgrad" in kinds:
            r["dx"], r["Adx"] = dgrad_reference(r["dy"], r["w"], (B, D, H, W, Cin), k, stride, pad, dil, want_mag=True)
        _REF[key] = r
    return _REF[key]


def fwd_forms(name):
    """forward epilogues: the 1x1x1 GEMM takes no bias (dram_conv3d_fwd_bf16)"""
    return ["nobias"] if kernel_of(name) == "gemm1" else ["bias", "nobias"]


DGRAD_FORMS = ["plain", "add", "add+gate"]


def expected(ref, p, form):
    """(exact value before the store rounding, magnitude A of its terms, the conv part alone)"""
    if p == "fwd":
        if form == "bias":
            b = ref["bias"].double()
            return ref["y"] + b, ref["Ay"] + b.abs(), ref["y"]
        return ref["y"], ref["Ay"], ref["y"]
    if form == "plain":
        return ref["dx"], ref["Adx"], ref["dx"]
    a = ref["add"].double()
    if form == "add+gate":
        a = a * (ref["gate"].double() > 0)           # -0.0 > 0 and 0 > 0 are false: both gate off
    return ref["dx"] + a, ref["Adx"] + a.abs(), ref["dx"]


# ------------------------------------------------------------------------------------------------ running a case
def run_case(ops, name, g, forms, ref):
    """every form of every pass of the case twice through ops.conv3d_fwd_keep / ops.conv3d_bwd_data under the kernel
    timeline: the launches must be the claimed kernels' and nothing else.  The weights are packed outside it."""
    kinds = CASES[name][0]
    wf, wb = ops.pack_conv_weight(ref["w"], True, True, g, BF16)
    assert wf.dtype == BF16 and wb.dtype == BF16
    out, want = {}, {"conv_bf16": {}}
    is_s2 = kernel_of(name) == "s2"
    tl = ops.KernelTimeline(64)
    tl.start()
    try:
        if "fwd" in kinds:
            for form in fwd_forms(name):
                b = ref["bias"] if form == "bias" else None
                out["fwd", form] = [ops.conv3d_fwd_keep(ref["x"], wf, b, g, True, False)[:2] for _ in range(2)]
            n = 2 * len(fwd_forms(name))
            want["conv_bf16"][forms["fwd"]["variant"]] = n
            if is_s2:
                want.setdefault("bn_elementwise", {})[9] = n
        if "dgrad" in kinds:
            for form in DGRAD_FORMS:
                a = None if form == "plain" else ref["add"]
                gt = ref["gate"] if form == "add+gate" else None
                out["dgrad", form] = [(ops.conv3d_bwd_data(ref["dy"], wb, g, a, gt), None) for _ in range(2)]
            want["conv_bf16"][forms["dgrad"]["variant"]] = 6
            if is_s2:
                want.setdefault("bn_elementwise", {})[10] = 6
        fam = tl.families()
    finally:
        tl.stop()
    ran = {f: {v: n for v, (n, _) in r["variants"].items()} for f, r in fam.items()}
    assert ran == want, f"{name}: launches by family and variant {ran}, the case claims {want}"
    return out


def assert_same(got, want, what):
    """bit for bit (as values, both widened to float64); NaN -- an unwritten element -- differs"""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, the first at {i}: "
                             f"{float(got[i])} for {float(want[i])}")


def row_sums(values, rows, nrows):
    """[nrows, 2, C] float64: per statistic row the sums of values [.., C] and of their squares"""
    v = values.double().reshape(-1, values.shape[-1])
    idx = rows.reshape(-1)
    out = torch.zeros((nrows, 2, v.shape[1]), dtype=F64, device=v.device)
    out[:, 0].index_add_(0, idx, v)
    out[:, 1].index_add_(0, idx, v * v)
    return out


def describe(name, nw, forms):
    f = "; ".join(f"{p}: {v['kernel']} variant {v['variant']}, " + ", ".join(f"{k} {v[k]}" for k in v if k not in
                  ("kernel", "variant", "tile_vox")) for p, v in forms.items())
    return f"{name}{'' if nw is None else ' NW=' + nw} {CASES[name][1]}: {f}"


def check_exact(ops, monkeypatch, capsys, name, nw):
    set_env(monkeypatch, nw)
    g, gk, forms = assert_form(ops, name, nw)
    ref = reference(name, "int")
    out = run_case(ops, name, g, forms, ref)
    with capsys.disabled():
        print(f"\n[conv bf16 exact {describe(name, nw, forms)}]")
    claim = CASES[name][2]
    rounded_somewhere = False
    for (p, form), calls in out.items():
        what = f"{name} {p} {form}"
        v, A, conv = expected(ref, p, form)
        # the exact regime, from the reference itself
        assert float(A.max()) < 2 ** 24 and float(conv.abs().max()) > 0, what
        if kernel_of(name) == "s2" and p == "dgrad" and form != "plain":
            # the epilogue acts on the already rounded gradient of the space-to-depth tensor
            v = to_bf16_rne(conv).double() + (v - conv)
        want = to_bf16_rne(v)
        assert float((want.double() ** 2).sum((0, 1, 2, 3)).max()) < 2 ** 24, what
        rounded_somewhere |= bool((want.double() != v).any())
        (y, st), (y2, st2) = calls
        assert y.dtype == BF16
        assert_same(y, want, what)
        assert torch.equal(y2.view(torch.int16), y.view(torch.int16)), f"{what}: a second call differs"
        if p == "fwd":
            nrows = forms["fwd"]["rows"]
            assert st.dtype == F32 and st.shape == (nrows, 2, gk.Cout)
            assert bool(torch.isfinite(st).all()), f"{what}: a statistic row was left poisoned or is not finite"
            rows = tile_rows(gk, nw)
            want_rows = row_sums(want, rows, nrows)
            empty = torch.bincount(rows.reshape(-1), minlength=nrows) == 0
            if "empty_rows" in claim:
                assert int(empty.sum()) == claim["empty_rows"], \
                    f"{what}: {int(empty.sum())} tiles without a voxel, the case claims {claim['empty_rows']}"
            assert bool((st[empty] == 0).all()), f"{what}: a tile without a voxel wrote statistics other than 0"
            assert_same(st, want_rows, f"{what} statistic rows")
            assert_same(ops.reduce_partials(st), want_rows.sum(0), f"{what} reduce_partials(stats)")
            assert torch.equal(st2, st), f"{what}: the statistics of a second call differ"
    if claim.get("wide"):
        assert rounded_somewhere, f"{name}: no element of the exact result needs rounding: RNE ties are not exercised"
    return forms


@pytest.mark.parametrize("nw", NWS)
@pytest.mark.parametrize("name", CONV3_CASES)
def test_exact_conv3(ops, poison, monkeypatch, capsys, name, nw):
    """Part A for conv3_bf16_kernel under DRAM_BF16_NW = 4 and 8: forward with and without bias (y and the BatchNorm sums,
    row by row and folded), data gradient without epilogue, with add, with add * (gate > 0) -- each equal to the fp64
    tap loop rounded once, bit for bit, in the claimed form, twice."""
    check_exact(ops, monkeypatch, capsys, name, nw)


@pytest.mark.parametrize("name", GEMM1_CASES)
def test_exact_gemm1(ops, poison, monkeypatch, capsys, name):
    """Part A for gemm1_bf16_kernel: forward (no bias: the 1x1x1 convolutions carry none) and the three data-gradient
    forms, 64- and 128-column tiles on either side of the 512-workgroup threshold."""
    check_exact(ops, monkeypatch, capsys, name, None)


@pytest.mark.parametrize("nw", NWS)
@pytest.mark.parametrize("name", S2_CASES)
def test_exact_stride2_route(ops, poison, monkeypatch, capsys, name, nw):
    """Part A for the stride-2 convolution as a stride-1 convolution over the space-to-depth tensor (s2d_bf16_kernel,
    dram_s2_embed_weight, conv3_bf16_kernel, d2s_bf16_kernel) through ops.conv3d_fwd_keep / conv3d_bwd_data /
    pack_conv_weight(..., BF16).  The shortcut epilogue is applied by the depth-to-space pass to the already rounded
    gradient: dx == rne(rne(ref) + add * (gate > 0)), with and without gate."""
    check_exact(ops, monkeypatch, capsys, name, nw)


@pytest.fixture(scope="module")
def traffic():
    """1 GiB (four times the memory-side cache) for a second stream to sweep"""
    buf = torch.zeros(1 << 28, dtype=F32, device=DEV)
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nw", NWS)
@pytest.mark.parametrize("name", ["one-tile", "three-chunks", "nb-mixed", "ragged", "wg-18"])
def test_exact_conv3_under_memory_load(ops, poison, monkeypatch, capsys, traffic, name, nw):
    """Part A while another stream keeps HBM saturated.  The weight ring is fetched by LDS-DMA two tap groups ahead; on an
    idle chip every group has landed long before its turn, whatever the kernel waits for (with the full wait in front of
    the last group of the last chunk taken out, every other case of this module still passes).  Under load the DMA lands
    late, and only the waits keep a tap group from being read before it is there."""
    reference(name, "int")
    ops.cast(torch.zeros(8, device=DEV), BF16)          # library and code objects loaded before the load starts
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(256):                             # ~0.15 s of read + write sweeps; the case takes ~0.01 s
            traffic.add_(1.0)
    try:
        check_exact(ops, monkeypatch, capsys, name, nw)
        busy = not side.query()
    finally:
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    assert busy, f"{name}: the load had ended before the case did: nothing was tested under load"


def test_every_instantiation_is_claimed():
    """the variants the cases claim (and assert from the timeline, each in its own test) are exactly the 12 instantiations
    of family conv_bf16: conv3_bf16_kernel<1|2, 0|1, 4|8> = 0 .. 7, gemm1_bf16_kernel<2|4, 0|1> = 8 .. 11"""
    from types import SimpleNamespace
    claimed = set()
    for name, (kinds, (B, D, H, W, Cin, Cout, k, stride, dil), _) in CASES.items():
        gk = SimpleNamespace(B=B, D=D, H=H, W=W, Cin=Cin, Cout=Cout, k=k, dil=dil)
        if stride == 2:
            gk = SimpleNamespace(B=B, D=D // 2, H=H // 2, W=W // 2, Cin=8 * Cin, Cout=Cout, k=3, dil=1)
        for nw in ([None] if k == 1 else NWS):
            claimed |= {f["variant"] for f in claimed_forms(name, gk, nw).values()}
    assert claimed == set(range(12)), f"variants of family conv_bf16 the cases claim: {sorted(claimed)}"


# ------------------------------------------------------------------------------------------------ Part B
def worst_ratio(got, want, bound):
    """max |got - want| / bound; an element whose bound is 0 (every product in the padding) must be exact"""
    err = (got.double() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf))
    return float(torch.nan_to_num(r, nan=math.inf).max())


def check_rounding(ops, monkeypatch, capsys, name, nw):
    set_env(monkeypatch, nw)
    g, gk, forms = assert_form(ops, name, nw)
    ref = reference(name, "real")
    out = run_case(ops, name, g, forms, ref)
    _, (B, D, H, W, Cin, Cout, k, stride, dil), _ = CASES[name]
    told = []
    ex = Excess(name)
    for (p, form), calls in out.items():
        what = f"{name} {p} {form}"
        v, A, conv = expected(ref, p, form)
        K = k ** 3 * (Cin if p == "fwd" else Cout)
        e = (K + 2) * U * A
        if kernel_of(name) == "s2" and p == "dgrad" and form != "plain":
            bound = U16 * (v.abs() + U16 * conv.abs() + e) + U16 * conv.abs() + e
        else:
            bound = U16 * (v.abs() + e) + e
        (y, st), (y2, st2) = calls
        told.append(f"{p} {form} {worst_ratio(y, v, bound):.4f}")
        ex.add(y, v, bound)
        assert torch.equal(y2.view(torch.int16), y.view(torch.int16)), f"{what}: a second call differs"
        if p == "fwd":
            f = forms["fwd"]
            assert st.shape == (f["rows"], 2, gk.Cout) and bool(torch.isfinite(st).all()), what
            own = y.double()
            rows = tile_rows(gk, nw)
            want_rows = row_sums(own, rows, f["rows"])
            mag_rows = row_sums(own.abs(), rows, f["rows"])
            mag_rows[:, 1] = want_rows[:, 1]
            sbound = (f["tile_vox"] + 2) * U * mag_rows
            told.append(f"{p} {form} statistic rows {worst_ratio(st, want_rows, sbound):.4f}")
            ex.add(st, want_rows, sbound)
            check_sums(ops.reduce_partials(st), st, f"{what} reduce_partials(stats)")
            assert torch.equal(st2, st), f"{what}: the statistics of a second call differ"
    with capsys.disabled():
        print(f"\n[conv bf16 rounding {describe(name, nw, forms)}]\n    worst |err| / bound: " + ", ".join(told))
    ex.check()


ROUNDING_DOC = """Part B: normal random operands, rounded to bf16 first; every element of every form.

    The products of bf16 operands are exact in the fp32 accumulators of the MFMA; K = taps * Cin of them (the data
    gradient: taps * Cout) are added in fp32, then the bias or the shortcut term add * (gate > 0): at most K + 1
    additions, each rounding a partial sum that A = sum |x| |w| + |bias| (+ |add| (gate > 0)) bounds.  With u = 2^-24,
    u16 = 2^-8 (half a bf16 ulp, relative) and e = (K + 2) u A the fp32 value is within e of the fp64 value v, and the
    one rounding of the store adds u16 of it:
        |y - v| <= u16 (|v| + e) + e.
    The stride-2 route rounds the gradient of the space-to-depth tensor (ref, within u16 (|ref| + e) + e) and applies the
    epilogue to the rounded value in the depth-to-space pass, which rounds again (K counts the 27 Cin products that are
    not zeros of the embedding; adding a zero rounds nothing):
        |dx - v| <= u16 (|v| + u16 |ref| + e) + u16 |ref| + e,    v = ref + add (gate > 0).
    BatchNorm sums: a statistic row is a chain of at most n = voxels of one tile (64 NW; 256 rows of the GEMM) fp32
    additions of the kernel's own rounded y (its squares: 16 significant bits, exact), so |row - sum| <= (n + 2) u sum
    |term| against the fp64 sums of the kernel's own y per tile; the fold of the rows goes through check_sums.
    The measured worst ratios error / bound are printed; the assertion is ratio <= 1."""


@pytest.mark.parametrize("nw", NWS)
@pytest.mark.parametrize("name", ROUNDING_CONV3)
def test_rounding_conv3(ops, poison, monkeypatch, capsys, name, nw):
    check_rounding(ops, monkeypatch, capsys, name, nw)


@pytest.mark.parametrize("name", ROUNDING_GEMM1)
def test_rounding_gemm1(ops, poison, monkeypatch, capsys, name):
    check_rounding(ops, monkeypatch, capsys, name, None)


@pytest.mark.parametrize("nw", NWS)
@pytest.mark.parametrize("name", ROUNDING_S2)
def test_rounding_stride2_route(ops, poison, monkeypatch, capsys, name, nw):
    check_rounding(ops, monkeypatch, capsys, name, nw)


for _t in (test_rounding_conv3, test_rounding_gemm1, test_rounding_stride2_route):
    _t.__doc__ = ROUNDING_DOC


# ------------------------------------------------------------------------------------------------ the cast kernels
def _bits(words):
    return torch.tensor(words, dtype=torch.int64).to(torch.int32).view(F32)


# RNE ties of the 16 dropped bits (even and odd kept mantissa, either sign, a carry into the exponent), just above and
# below a tie, +-0, +-inf, NaN, the largest finite fp32 (rounds to inf) and the largest that stays finite
CAST_SPECIALS = _bits([0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0x3FFF8000, 0x00000000, 0x7F800000, 0x7FC00000,
                       0x7F7FFFFF, 0x7F7F7FFF]).repeat(2) * torch.tensor([1.0] * 10 + [-1.0] * 10)


def same_bits(got, want):
    """equal bit patterns, except that a NaN only has to stay a NaN"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    it = torch.int16 if got.dtype == BF16 else torch.int32
    return bool(torch.equal(torch.isnan(got), nan) and torch.equal(got.view(it)[~nan], want.view(it)[~nan]))


@pytest.mark.parametrize("offset", [0, 1])
def test_cast_kernels_bit_equal_torch(ops, poison, offset):
    """dram_cast_f32_to_bf16 / dram_cast_bf16_to_f32 through ops.cast against torch's CPU .to(bfloat16) / .float(), bit
    for bit: n = 1, 3, 4, 5 (below, at and above one 4-element vector, every special value at every position), 1023 and
    1025 (the vector loop with a scalar tail of 3 and 1); offset 1: a view that starts one element into its allocation,
    which is not aligned for the vector form (the scalar path)."""
    assert bool(torch.isnan(CAST_SPECIALS).any()) and bool(torch.isinf(CAST_SPECIALS).any())
    assert torch.signbit(CAST_SPECIALS[CAST_SPECIALS == 0]).tolist() == [False, True]
    gen = torch.Generator().manual_seed(5)
    pool = torch.cat([CAST_SPECIALS, torch.randn(1100, generator=gen) * 3.0])
    draws = [(n, s) for n in (1, 3, 4, 5) for s in range(len(CAST_SPECIALS))] + [(1023, 0), (1025, 7)]
    for n, s in draws:
        h32 = pool.roll(-s)[:n].clone()
        h16 = h32.to(BF16)
        for src, dtype, want in ((h32, BF16, h16), (h16, F32, h16.float())):
            buf = torch.zeros(n + offset, dtype=src.dtype, device=DEV)
            buf[offset:] = src.to(DEV)
            view = buf[offset:]
            assert view.data_ptr() % 16 == offset * src.element_size() and same_bits(view, src)
            got = ops.cast(view, dtype)
            assert same_bits(got, want), f"cast to {dtype}, n = {n}, offset {offset}, specials from {s}: {got.cpu()} for {want}"
    # the largest finite fp32 rounds to inf, NaN stays NaN
    r = ops.cast(_bits([0x7F7FFFFF, 0x7FC00000, 0x7F7F7FFF]).to(DEV), BF16).float().cpu()
    assert math.isinf(float(r[0])) and math.isnan(float(r[1])) and math.isfinite(float(r[2]))
