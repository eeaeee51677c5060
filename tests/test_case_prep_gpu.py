"""GPU: transforms.prepare_case (csrc/case_prep.hip: lung bounding box + the fused dilate / fill / crop / masks pass)
and processor.predict_case.  Every comparison is on integers or booleans: the bar is exact equality -- against the
fixture recorded from the reference's SubtypingInference.get_data (tests/golden/case_prep.npz) and against its torch
restatement tests/case_prep_ref.py (held to that fixture and to scipy by tests/test_case_prep_host.py).

Every buffer the wrapper allocates is poisoned (`poison`), and masks are compared as bytes, so a voxel the kernel did not
write, or wrote as anything but 0 / 1, cannot pass.  Shapes: the x extent crosses one and two 64-voxel ballot runs
((3,4,70), (5,9,130)), the 256-voxel tile of case_prepare_kernel once and twice ((3,5,260), (10,20,530): the only
cases that read the halo runs of a neighbouring tile), its 8-plane / 8-row tile on every axis, and lung_bbox's
16 384-voxel partial rows ((40,70,200): 35 of them)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import case_prep_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I16_POISON, I32_POISON = 0x5A5A, 0x5A5A5A5A


@pytest.fixture(scope="module")
def T():
    import bodyct_dram_emph_subtype_amd as pkg
    from bodyct_dram_emph_subtype_amd import transforms
    pkg.load_library()
    return transforms


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "case_prep.npz"))


@pytest.fixture
def poison(monkeypatch):
    """torch.empty returns poisoned memory for the duration of a test (as tests/test_launch_regimes_gpu.py does):
    uint8 0xFF (not a 0 / 1 mask byte), int16 0x5A5A, int32 0x5A5A5A5A (partial rows, the box), floats NaN."""
    e0 = torch.empty

    def fill(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(255)
        elif t.dtype == torch.int16:
            t.fill_(I16_POISON)
        elif t.dtype == torch.int32:
            t.fill_(I32_POISON)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(e0(*a, **k)))
    yield
    torch.cuda.synchronize()


def check(got, want, want_original=True, what=""):
    """got: prepare_case's dict; want: the reference dict (tensors or arrays).  Exact, dtypes included."""
    for k in ("image", "original_image"):
        if k == "original_image" and not want_original:
            assert k not in got, what
            continue
        g = got[k]
        assert g.dtype == torch.int16 and g.is_cuda and g.is_contiguous(), (what, k)
        assert torch.equal(g.cpu(), torch.as_tensor(want[k])), (what, k)
    for k in ("lung_mask", "ess_mask"):
        g = got[k]
        assert g.dtype == torch.bool and g.is_cuda, (what, k)
        assert torch.equal(g.view(torch.uint8).cpu(), torch.as_tensor(want[k]).to(torch.uint8)), (what, k)   # bytes 0 / 1
    for k in ("crop_slice", "original_size"):
        g = got[k]
        assert g.dtype == torch.int64 and not g.is_cuda, (what, k)
        assert torch.equal(g, torch.as_tensor(want[k])), (what, k, g.tolist())
    assert tuple(got["crop_slice"].shape) == (3, 2) and tuple(got["original_size"].shape) == (3,)


# ------------------------------------------------------------------------------------------------ the reference fixture
@pytest.mark.parametrize("name", sorted(ref.fixture_cases()))
def test_fixture_cases(T, golden, poison, name):
    scan, lobes, spacing, border = ref.fixture_cases()[name]
    got = T.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, crop_border=border, want_original=True, uid=name)
    check(got, {k: golden[f"{name}:{k}"] for k in ref.KEYS}, what=name)
    assert got["uid"] == name
    assert set(got) == {"image", "original_image", "lung_mask", "ess_mask", "crop_slice", "original_size", "uid"}


# ------------------------------------------------------------------------------------------------ random sparse lobes
SHAPES = [(7, 9, 11), (12, 6, 17), (3, 4, 70), (5, 9, 130), (40, 70, 200), (3, 5, 260), (10, 20, 530)]
SPACING = (2.5, 0.7, 1.0)            # border 5 -> pads 2, 8, 5


def random_case(shape, p, seed, lobe_dtype=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    lobes = ((torch.rand(shape, generator=g) < p) * torch.randint(1, 6, shape, generator=g)).to(lobe_dtype)
    if not bool(lobes.any()):
        lobes[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 3
    scan = torch.randint(-1000, -800, shape, generator=g, dtype=torch.int16)     # both sides of the ess threshold
    return scan, lobes


@pytest.mark.parametrize("p", [0.002, 0.02, 0.3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_lobes_every_radius_and_border(T, poison, shape, p):
    scan, lobes = random_case(shape, p, seed=sum(shape) + int(p * 1000))
    sd, ld = scan.to(DEV), lobes.to(DEV)
    for border in (0, 5):
        for r in (0, 1, 2, 3):
            want = ref.prepare_case_ref(scan, lobes, SPACING, crop_border=border, dilate_iterations=r)
            got = T.prepare_case(sd, ld, SPACING, crop_border=border, dilate_iterations=r, want_original=True)
            check(got, want, what=f"{shape} p={p} border={border} r={r}")


def test_sizing_export_and_partial_rows(T):
    from bodyct_dram_emph_subtype_amd import ops
    L = ops._L()
    assert L.dram_lung_bbox_nblk(40 * 70 * 200) == 35 and L.dram_lung_bbox_nblk(7 * 9 * 11) == 1


@pytest.mark.parametrize("xa", [10, 58, 250])        # inside a run, across a 64-voxel run edge, across the 256-voxel tile edge
def test_dilated_blobs_touch_at_gap_4_and_not_at_gap_5(T, poison, xa):
    shape = (9, 12, 300)
    for gap in (4, 5):
        lobes = torch.zeros(shape, dtype=torch.uint8)
        lobes[3:6, 4:8, xa:xa + 4] = 1
        lobes[3:6, 4:8, xa + 4 + gap:xa + 8 + gap] = 2
        scan = torch.full(shape, -900, dtype=torch.int16)
        got = T.prepare_case(scan.to(DEV), lobes.to(DEV), (1, 1, 1), crop_border=0, dilate_iterations=2)
        check(got, ref.prepare_case_ref(scan, lobes, (1, 1, 1), crop_border=0), want_original=False, what=f"gap {gap}")
        row = got["image"][1, 1].cpu()                   # a row through both blobs; the crop starts at x = xa
        filled = (row == -2048).nonzero().flatten().tolist()
        assert filled == ([] if gap == 4 else [4 + 2]), (gap, filled)     # the one voxel 3 away from either blob


# ------------------------------------------------------------------------------------------------ types and options
def test_lobe_and_scan_types(T, poison):
    shape = (12, 6, 17)
    scan, lobes = random_case(shape, 0.05, seed=5)
    want = ref.prepare_case_ref(scan, lobes, SPACING)
    sd = scan.to(DEV)
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64, torch.int8, torch.float32):
        check(T.prepare_case(sd, lobes.to(dt).to(DEV), SPACING, want_original=True), want, what=str(dt))
    check(T.prepare_case(sd, (lobes > 0).to(DEV), SPACING, want_original=True), want, what="bool lobes")
    check(T.prepare_case(scan.float().to(DEV), lobes.to(DEV), SPACING, want_original=True), want, what="float scan")
    check(T.prepare_case(scan.to(torch.int32).to(DEV), lobes.to(DEV), SPACING, want_original=True), want, what="int32 scan")
    # negative labels are not lung (the reference tests lobe > 0), as int16 inside the kernel and as int32 through the wrapper
    neg = lobes.to(torch.int16)
    neg[0, 0, :] = -3
    neg[-1, -1, -1] = -1
    want = ref.prepare_case_ref(scan, neg, SPACING)
    assert int(want["lung_mask"].sum()) == int((neg > 0).sum())
    check(T.prepare_case(sd, neg.to(DEV), SPACING, want_original=True), want, what="negative int16 labels")
    check(T.prepare_case(sd, neg.to(torch.int32).to(DEV), SPACING, want_original=True), want, what="negative int32 labels")
    # int16 labels with a zero low byte
    hi = lobes.to(torch.int16) * 256
    check(T.prepare_case(sd, hi.to(DEV), SPACING, want_original=True), ref.prepare_case_ref(scan, hi, SPACING), what="labels * 256")


def test_views_unaligned_and_non_contiguous(T, poison):
    scan, lobes = random_case((8, 9, 11), 0.05, seed=6)
    want = ref.prepare_case_ref(scan[1:], lobes[1:], SPACING)
    sd, ld = scan.to(DEV), lobes.to(DEV)
    assert ld[1:].data_ptr() % 16 != 0                   # 99 bytes into the allocation
    check(T.prepare_case(sd[1:], ld[1:], SPACING, want_original=True), want, what="offset views")
    li = lobes.to(torch.int16).to(DEV)
    assert li[1:].data_ptr() % 16 != 0
    check(T.prepare_case(sd[1:], li[1:], SPACING, want_original=True), want, what="offset int16 view")
    st, lt = scan.permute(2, 1, 0), lobes.permute(2, 1, 0)
    check(T.prepare_case(st.to(DEV), lt.to(DEV), SPACING, want_original=True), ref.prepare_case_ref(st, lt, SPACING),
          what="permuted views")


def test_fill_threshold_and_want_original(T, poison):
    scan, lobes = random_case((12, 6, 17), 0.05, seed=7)
    sd, ld = scan.to(DEV), lobes.to(DEV)
    for fill, thr in ((-2048, -910), (-1024, -950), (32767, -32768), (-32768, 32767)):
        want = ref.prepare_case_ref(scan, lobes, SPACING, fill_value=fill, ess_threshold=thr)
        got = T.prepare_case(sd, ld, SPACING, fill_value=fill, ess_threshold=thr)
        check(got, want, want_original=False, what=f"fill {fill} thr {thr}")
    assert int(want["ess_mask"].sum()) == int(((scan < 32767) & (lobes > 0)).sum())
    # the inputs are left alone
    assert torch.equal(sd.cpu(), scan) and torch.equal(ld.cpu(), lobes)


def test_two_calls_are_bit_identical(T, poison):
    scan, lobes = random_case((40, 70, 200), 0.02, seed=8)
    sd, ld = scan.to(DEV), lobes.to(DEV)
    a = T.prepare_case(sd, ld, SPACING, want_original=True)
    b = T.prepare_case(sd, ld, SPACING, want_original=True)
    for k in ("image", "original_image", "lung_mask", "ess_mask", "crop_slice", "original_size"):
        assert torch.equal(a[k].view(torch.uint8) if a[k].dtype == torch.bool else a[k],
                           b[k].view(torch.uint8) if b[k].dtype == torch.bool else b[k]), k


# ------------------------------------------------------------------------------------------------ errors
def test_python_errors(T):
    z = torch.zeros((4, 5, 6), dtype=torch.int16, device=DEV)
    with pytest.raises(IndexError):
        T.prepare_case(z, torch.zeros((4, 5, 6), dtype=torch.uint8, device=DEV), (1, 1, 1))
    with pytest.raises(IndexError):
        T.prepare_case(z, torch.full((4, 5, 6), -1, dtype=torch.int16, device=DEV), (1, 1, 1))
    with pytest.raises(ValueError):
        T.prepare_case(z, torch.ones((4, 5, 7), dtype=torch.uint8, device=DEV), (1, 1, 1))
    with pytest.raises(ValueError):
        T.prepare_case(z, torch.ones((4, 5, 6), dtype=torch.uint8, device=DEV), (1, 1, 1), dilate_iterations=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.prepare_case(z, torch.ones((4, 5, 6), dtype=torch.uint8), (1, 1, 1))


def test_c_entry_points_refuse_bad_arguments(T, poison):
    """Each call below is refused before any launch (non-zero code) and leaves its outputs untouched."""
    from bodyct_dram_emph_subtype_amd import ops, _lib
    L, p, s = ops._L(), ops._p, ops._stream
    D, H, W = 4, 5, 16
    scan = torch.zeros((D, H, W), dtype=torch.int16, device=DEV)
    lobes = torch.ones((D, H, W), dtype=torch.uint8, device=DEV)
    part = torch.empty((1, 8), dtype=torch.int32, device=DEV)
    box = torch.empty((8,), dtype=torch.int32, device=DEV)
    bad = _lib.DRAM_ERR_BAD_ARG
    assert L.dram_lung_bbox(None, 1, p(part), p(box), D, H, W, s()) == bad
    assert L.dram_lung_bbox(p(lobes), 1, None, p(box), D, H, W, s()) == bad
    assert L.dram_lung_bbox(p(lobes), 1, p(part), None, D, H, W, s()) == bad
    assert L.dram_lung_bbox(p(lobes), 3, p(part), p(box), D, H, W, s()) == bad
    assert L.dram_lung_bbox(p(lobes), 1, p(part), p(box), 0, H, W, s()) == bad
    assert L.dram_lung_bbox(p(lobes[0, 0, 1:]), 1, p(part), p(box), 1, 1, 15, s()) == bad          # not 16-byte aligned
    assert L.dram_lung_bbox(p(lobes), 1, p(part), p(box), 2048, 1024, 1024, s()) == _lib.DRAM_ERR_UNSUPPORTED
    img = torch.empty((D, H, W), dtype=torch.int16, device=DEV)
    lung = torch.empty((D, H, W), dtype=torch.uint8, device=DEV)
    ess = torch.empty((D, H, W), dtype=torch.uint8, device=DEV)

    def prep(scan_=scan, lobes_=lobes, code=1, img_=img, lung_=lung, ess_=ess, vol=(D, H, W), off=(0, 0, 0), crop=(D, H, W),
             r=2, fill=-2048, thr=-910):
        return L.dram_case_prepare(p(scan_), p(lobes_), code, p(img_), p(lung_), p(ess_), None, *vol, *off, *crop, r, fill,
                                   thr, s())

    for kw in (dict(scan_=None), dict(lobes_=None), dict(img_=None), dict(lung_=None), dict(ess_=None), dict(code=0),
               dict(r=-1), dict(r=4), dict(fill=-32769), dict(fill=32768), dict(thr=40000), dict(off=(-1, 0, 0)),
               dict(off=(1, 0, 0)), dict(off=(0, 1, 0)), dict(off=(0, 0, 1)), dict(crop=(D + 1, H, W)),
               dict(crop=(0, H, W)), dict(crop=(D, H, -3)), dict(off=(2 ** 31 - 1, 0, 0)), dict(vol=(0, H, W))):
        assert prep(**kw) == bad, kw
    assert prep(vol=(2048, 1024, 1024)) == _lib.DRAM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((img == I16_POISON).all()) and bool((lung == 255).all()) and bool((ess == 255).all())
    assert bool((box == I32_POISON).all()) and bool((part == I32_POISON).all())
    assert prep() == 0                                                                  # and the good call runs
    torch.cuda.synchronize()
    assert bool((lung == 1).all()) and bool((img == 0).all()) and bool((ess == 0).all())


# ------------------------------------------------------------------------------------------------ predict_case
def test_predict_case_is_the_composition(T, golden):
    """scan + lobes -> report entry: bit for bit the existing functions composed by hand on the FIXTURE's prepared dict
    (recorded from the reference), and the pasted volumes are zero outside crop_slice."""
    from bodyct_dram_emph_subtype_amd import models, processor
    name = "blobs_u8"
    scan, lobes, spacing, border = ref.fixture_cases()[name]
    target = (16, 32, 32)
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()

    prepared = {k: torch.as_tensor(golden[f"{name}:{k}"]) for k in ("image", "lung_mask", "ess_mask", "crop_slice", "original_size")}
    sample = T.prepare_sample({k: (v.to(DEV) if k.endswith(("image", "_mask")) else v) for k, v in prepared.items()}, target)
    batch = {k: v.unsqueeze(0) for k, v in sample.items()}
    batch["uid"] = [name]
    want = processor.build_outputs([mod.predict_step(batch, 0)], want_u8=True)[0]

    got = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, uid=name, crop_border=border)
    assert got["entity"] == name and got["metrics"] == want["metrics"] and got["error_messages"] == []
    (z0, z1), (y0, y1), (x0, x1) = prepared["crop_slice"].tolist()
    for k in ("full_cle", "full_pse"):
        assert got[k].dtype == torch.uint8 and tuple(got[k].shape) == tuple(scan.shape)
        assert torch.equal(got[k], want[k]), k
        outside = got[k].clone()
        outside[z0:z1, y0:y1, x0:x1] = 0
        assert int(outside.count_nonzero()) == 0, k
    gf = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, uid=name, want_u8=False, crop_border=border)
    assert gf["full_cle"].dtype == torch.float32 and gf["metrics"] == want["metrics"]
