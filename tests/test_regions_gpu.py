"""GPU: the regional predict tail of csrc/regions.hip -- dram_upproject_regions (both heads' up-projection and the
per-region table in one pass) and dram_prep_labels -- against the fp64 yardstick of tests/regions_ref.py, and the path
from scan + lobes to the per-lobe report (transforms.prepare_case(want_lobes) -> predict_step -> processor).

Shapes: the smallest at which each launch form can go wrong -- (a) 385 voxels: one block with a ragged last wave;
(b) a source axis of length 1 (scale 0), 34 blocks, uncapped, ragged last block; (c) 1 105 920 voxels: the block count
capped at 1024, every thread strides, ragged last stride -- each with n_regions 1, 5 (8 accumulator rows) and 15 (16).
Every case runs with torch.empty poisoned (floats NaN, uint8 0xFF): an unwritten element fails.  Every test prints its
figures before it asserts (pytest -s).

Bounds (u = 2^-24).  A stored element: test_upproject_grid_stride's, (sum over axes of 2 u (n - 1) + u) x the spread of
dense + 8 u max |dense|.  A table sum against the fp64 sum of the kernel's OWN stored volume over the same voxels (which
isolates the summation from the interpolation): (strides + 9) u sum |o|, strides = ceil(voxels / (nblk * 256)) additions
of a thread, 6 of the wave fold, 3 of the block fold; the fold over the blocks is in double.  Counts are exact.
"""
import math

import pytest
import torch

import case_prep_ref as CR
import regions_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = RR.U


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    e0, el0 = torch.empty, torch.empty_like

    def fill(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(255)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(e0(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(el0(*a, **k)))
    yield
    torch.cuda.synchronize()


SHAPES = {"a-one-block": ((2, 3, 4), (5, 7, 11)), "b-scale0-uncapped": ((1, 4, 4), (16, 33, 65)),
          "c-capped": ((4, 16, 16), (9, 384, 320))}
B = 2
_CACHE = {}


def inputs(sid):
    """dense [B,2,D,H,W] (signed, so that sum |o| != |sum o|), ess bytes 0/1 and the fp64 volumes: computed once per
    shape, shared by its cases and left unchanged"""
    if sid not in _CACHE:
        dense_shape, size = SHAPES[sid]
        g = torch.Generator().manual_seed(len(_CACHE) + 71)
        dense = torch.randn((B, 2) + dense_shape, generator=g)
        ess = (torch.rand((B,) + size, generator=g) > 0.5).to(torch.uint8)
        ref = [RR.upproject64(dense[:, h], ess, size) for h in (0, 1)]
        _CACHE[sid] = (dense, ess, ref)
    return _CACHE[sid]


def labels_for(size, n, seed):
    """random labels 0..n; sample 1 misses label n altogether and holds no foreign label; sample 0 holds a few voxels
    above n (they belong to row 0)"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, n + 1, (B,) + size, generator=g, dtype=torch.uint8)
    lab[1][lab[1] == n] = 0
    flat = lab[0].view(-1)
    foreign = torch.tensor([n + 1, 200, 255, n + 1], dtype=torch.uint8)
    flat[torch.tensor([0, 3, flat.numel() // 2, flat.numel() - 1])] = foreign
    return lab, foreign.numel()


def check_case(ops, sid, n, ess_zero=False):
    dense, ess, ref = inputs(sid)
    (D, H, W), size = SHAPES[sid]
    vps = math.prod(size)
    if ess_zero:
        ess, ref = torch.zeros_like(ess), [torch.zeros_like(r) for r in ref]
    labels, n_foreign = labels_for(size, n, 5 + n)
    dd = dense.to(DEV)
    heads = [dd[:, 0], dd[:, 1]]                                  # two channel views, batch stride 2 D H W
    assert not heads[0].is_contiguous() and heads[1].stride(0) == 2 * D * H * W
    e_d, l_d = ess.to(DEV), labels.to(DEV)
    nblk = ops._L().dram_region_nblk(vps)
    strides = -(-vps // (nblk * 256))
    what = f"{sid} n={n}" + (" ess=0" if ess_zero else "")
    print(f"[{what}] voxels {vps}, blocks {nblk}, strides {strides}")

    up_c, up_p, table = ops.upproject_regions(heads[0], heads[1], e_d, l_d, size, n)
    assert up_c.shape == up_p.shape == (B,) + size and up_c.dtype == torch.float32
    assert table.shape == (B, n + 1, 4) and table.dtype == torch.float64
    t = table.cpu()

    # the volumes: dram_upproject's bit for bit, and each element against fp64
    ups = []
    for h, (name, up) in enumerate((("cle", up_c), ("pse", up_p))):
        want = ops.upproject(heads[h].contiguous(), e_d.float(), size)[0]
        same = torch.equal(up, want)
        u = up.cpu()
        ups.append(u)
        err = (u.double() - ref[h]).abs()
        eb = RR.element_bound(dense[:, h], ess)
        ratio = float((err / eb.clamp_min(1e-300)).max()) if not ess_zero else float(err.max())
        print(f"[{what}] {name}: equal to upproject {same}; worst element error / bound {ratio:.3f}")
        assert same, f"{what}: {name} differs from dram_upproject"
        assert not torch.isnan(u).any() and bool((err <= eb).all()), f"{what}: {name} {ratio:.3f} of the element bound"

    # the table sums against the fp64 sums of the stored volumes
    mine = RR.table64(ups[0], ups[1], ess, labels, n)
    mag = RR.table64(ups[0].abs(), ups[1].abs(), ess, labels, n)
    kappa = strides + 9
    for col, name in ((0, "cle"), (1, "pse")):
        err = (t[:, :, col] - mine[:, :, col]).abs()
        bound = kappa * U * mag[:, :, col]
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"[{what}] sum {name}: worst error / (kappa={kappa} u sum|o|) {worst:.3f}; "
              f"sum|o| / |sum o| up to {float((mag[:, :, col] / mine[:, :, col].abs().clamp_min(1e-30)).max()):.1f}")
        assert not torch.isnan(t).any() and bool((err <= bound).all()), f"{what}: sum {name} {worst:.3f} of the bound"

    # the counts
    assert torch.equal(t[:, :, 2:], mine[:, :, 2:]), f"{what}: counts"
    assert t[:, :, 3].sum(1).tolist() == [float(vps)] * B
    assert float(t[1, 1:, 3].sum()) == float((labels[1] > 0).sum())            # no foreign label in sample 1
    assert float(t[1, n, 3]) == 0.0                                            # ... and no label n
    assert float(t[0, 0, 3]) == float((labels[0] == 0).sum()) + n_foreign      # foreign labels land in row 0
    assert float(t[0, 1:, 3].sum()) == float((labels[0] > 0).sum()) - n_foreign
    if ess_zero:
        assert float(t[:, :, :3].abs().sum()) == 0.0

    # table only, and a second call
    none_c, none_p, only = ops.upproject_regions(heads[0], heads[1], e_d, l_d, size, n, want_volumes=False)
    assert none_c is None and none_p is None and torch.equal(only, table), f"{what}: table-only differs"
    again = ops.upproject_regions(heads[0], heads[1], e_d, l_d, size, n)
    assert torch.equal(again[2], table) and torch.equal(again[0], up_c) and torch.equal(again[1], up_p), f"{what}: second call"


@pytest.mark.parametrize("n", [1, 5, 15])
@pytest.mark.parametrize("sid", sorted(SHAPES))
def test_volumes_table_counts(ops, sid, n):
    check_case(ops, sid, n)


def test_all_zero_ess(ops):
    check_case(ops, "a-one-block", 5, ess_zero=True)


def test_launch_forms_are_the_intended_ones(ops):
    L = ops._L()
    assert [L.dram_region_nblk(math.prod(SHAPES[s][1])) for s in sorted(SHAPES)] == [1, 34, 1024]
    assert math.prod(SHAPES["a-one-block"][1]) % 64 and math.prod(SHAPES["b-scale0-uncapped"][1]) % 1024
    assert math.prod(SHAPES["c-capped"][1]) % (1024 * 256) and math.prod(SHAPES["c-capped"][1]) > 1024 * 256


def test_bool_masks_and_rejections(ops):
    dense, ess, _ = inputs("a-one-block")
    size = SHAPES["a-one-block"][1]
    labels, _ = labels_for(size, 5, 3)
    dd, e_d, l_d = dense.to(DEV), ess.to(DEV), labels.to(DEV)
    a, b = dd[:, 0], dd[:, 1]
    want = ops.upproject_regions(a, b, e_d, l_d, size)
    got = ops.upproject_regions(a, b, e_d.bool(), l_d, size)
    assert torch.equal(got[2], want[2]) and torch.equal(got[0], want[0])
    with pytest.raises(RuntimeError):
        ops.upproject_regions(a, b, e_d.cpu(), l_d, size)
    with pytest.raises(TypeError):
        ops.upproject_regions(a, b, e_d.float(), l_d, size)
    with pytest.raises(TypeError):
        ops.upproject_regions(a.double(), b, e_d, l_d, size)
    with pytest.raises(ValueError):
        ops.upproject_regions(a, b, e_d[:1], l_d, size)
    with pytest.raises(ValueError):
        ops.upproject_regions(a, b, e_d, l_d[..., :8], size)
    with pytest.raises(ValueError):
        ops.upproject_regions(a, b[:, :1], e_d, l_d, size)
    with pytest.raises(ValueError):
        ops.upproject_regions(a, b.contiguous(), e_d, l_d, size)            # two batch strides
    with pytest.raises(ValueError):
        ops.upproject_regions(a[..., ::2], b[..., ::2], e_d, l_d, size)     # a sample that is not contiguous


# ------------------------------------------------------------------------------------------------ prepare_labels
TARGETS = [(10, 9, 16), (7, 30, 11), (3, 14, 40), (1, 1, 1)]       # Do > D (repeated planes), Ho < H, Wo == W; Ho > H; ...


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.bool], ids=["u8", "i16", "bool"])
def test_prepare_labels_reads_a_strided_crop(ops, dtype):
    from bodyct_dram_emph_subtype_amd import transforms as T
    g = torch.Generator().manual_seed(9)
    vol = torch.randint(0, 2 if dtype == torch.bool else 7, (12, 20, 24), generator=g).to(dtype)
    if dtype == torch.int16:
        vol[2, 3, 5], vol[2, 3, 6], vol[8, 16, 20] = 300, -7, 256
    vd = vol.to(DEV)
    crop_d, crop = vd[2:9, 3:17, 5:21], vol[2:9, 3:17, 5:21]
    assert not crop_d.is_contiguous() and tuple(crop_d.shape) == (7, 14, 16)
    for size in TARGETS:
        got = T.prepare_labels(crop_d, size)
        assert got.dtype == torch.uint8 and tuple(got.shape) == size and got.is_contiguous()
        via_mask = T.prepare_mask(crop_d.contiguous().float(), size).clamp(0, 255).to(torch.uint8)
        assert torch.equal(got, via_mask), (dtype, size)
        assert torch.equal(got.cpu(), RR.resize_labels(crop.to(torch.int16), size)), (dtype, size)
        assert torch.equal(got > 0, T.prepare_mask(crop_d > 0, size)), (dtype, size)
    if dtype == torch.int16:
        full = T.prepare_labels(crop_d, tuple(crop_d.shape)).cpu()
        assert int(full[0, 0, 0]) == 255 and int(full[0, 0, 1]) == 0 and int(full[6, 13, 15]) == 255    # 300, -7, 256
    # a source whose x stride is not 1 is copied, not misread
    tr = vd.transpose(1, 2)[2:9, 5:21, 3:17]
    assert torch.equal(T.prepare_labels(tr, (7, 16, 14)), tr.to(torch.int16).clamp(0, 255).to(torch.uint8))


# ------------------------------------------------------------------------------------------------ scan + lobes -> report
PLAIN_KEYS = {"cle_dense_outs", "cle_precentages", "pse_dense_outs", "pse_precentages", "crop_slices", "original_size", "uids"}
REGION_OUT_KEYS = {"region_table", "cle_region_percentages", "pse_region_percentages", "region_voxels", "region_ess_fraction"}
LUNG_METRICS = ("cle_severity_score", "cle_lesion_percentage_per_lung", "pse_severity_score", "pse_lesion_percentage_per_lung")


@pytest.mark.parametrize("name", ["blobs_u8", "lobes_i16"])
def test_predict_case_with_regions(ops, name):
    from bodyct_dram_emph_subtype_amd import models, processor, transforms as T
    scan, lobes, spacing, border = CR.fixture_cases()[name]
    target, n = (16, 32, 32), 5
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()

    case = T.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid=name, crop_border=border, want_lobes=True)
    crop = tuple(slice(int(a), int(b)) for a, b in case["crop_slice"].tolist())
    assert case["lobe_labels"].dtype == lobes.dtype and torch.equal(case["lobe_labels"].cpu(), lobes[crop])
    assert case["lobe_labels"].untyped_storage().data_ptr() != case["lung_mask"].untyped_storage().data_ptr()
    sample = T.prepare_sample(case, target)
    labels = sample["lobe_labels"]
    assert labels.dtype == torch.uint8 and torch.equal(labels.cpu(), RR.resize_labels(lobes[crop], target))
    assert torch.equal(labels > 0, sample["lung_mask"])
    keys = ("image", "lung_mask", "ess_mask", "crop_slice", "original_size")
    batch = {k: sample[k].unsqueeze(0) for k in keys}
    batch["uid"] = [name]
    plain = mod.predict_step(batch, 0)
    assert set(plain) == PLAIN_KEYS                                            # without the key: today's keys
    reg = mod.predict_step(dict(batch, lobe_labels=labels.unsqueeze(0)), 0)
    assert set(reg) == PLAIN_KEYS | REGION_OUT_KEYS
    for h in ("cle", "pse"):
        assert torch.equal(reg[f"{h}_dense_outs"], plain[f"{h}_dense_outs"]), h
        a, b = float(reg[f"{h}_precentages"][0]), float(plain[f"{h}_precentages"][0])
        print(f"[{name}] {h} per lung: fused {a:.9g}, two passes {b:.9g}")
        assert reg[f"{h}_precentages"].dtype == plain[f"{h}_precentages"].dtype and abs(a - b) <= 1e-5 * abs(b), h

    # the regional numbers against the yardstick on the returned volumes and the resized labels
    t = reg["region_table"].cpu()
    assert tuple(t.shape) == (1, n + 1, 4) and t.dtype == torch.float64
    oc, op = (reg[f"{h}_dense_outs"][:, 0].cpu() for h in ("cle", "pse"))
    ess, lab = sample["ess_mask"].cpu()[None], labels.cpu()[None]
    want = RR.table64(oc, op, ess, lab, n)
    mag = RR.table64(oc.abs(), op.abs(), ess, lab, n)
    vps = math.prod(target)
    kappa = -(-vps // (ops._L().dram_region_nblk(vps) * 256)) + 9
    assert torch.equal(t[:, :, 2:], want[:, :, 2:])
    vox = want[:, 1:, 3]
    for col, h in ((0, "cle"), (1, "pse")):
        got, ref = reg[f"{h}_region_percentages"].cpu(), RR.percentages(want)[col]
        assert tuple(got.shape) == (1, n) and torch.equal(got.isnan(), vox == 0), h
        err = (got - ref).abs()[vox > 0]
        bound = (kappa * U * mag[:, 1:, col] / vox)[vox > 0]
        print(f"[{name}] {h} regions {[round(v, 6) for v in got[0].tolist()]}; worst error / bound "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), h
    assert torch.equal(reg["region_voxels"].cpu(), vox.long())
    assert torch.equal(reg["region_ess_fraction"].cpu().nan_to_num(-1.0), (want[:, 1:, 2] / vox).nan_to_num(-1.0))

    if name == "blobs_u8":                                                     # every lung label is <= n
        assert float(t[0, 0, 2]) == 0.0 and float(vox.sum()) == float(sample["lung_mask"].sum())
        for col, h in ((0, "cle"), (1, "pse")):
            pct = reg[f"{h}_region_percentages"][0].cpu()
            mean = float((pct * vox[0]).nansum() / vox.sum())
            lung = float(plain[f"{h}_precentages"][0])
            print(f"[{name}] {h}: voxel-weighted mean of the regions {mean:.9g}, per lung {lung:.9g}")
            assert abs(mean - lung) <= 1e-5 * abs(lung), h
    else:                                                                      # label 300 -> 255 -> row 0
        assert float(t[0, 0, 2]) > 0 and vox[0].tolist()[:3] == [0.0, 0.0, 0.0] and float(vox[0, 3]) > 0

    # the report entry
    kw = dict(uid=name, crop_border=border)
    e_plain = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, **kw)
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    e_reg = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, regions=True, region_names=names, **kw)
    assert set(e_plain["metrics"]) == set(LUNG_METRICS) and e_plain["error_messages"] == []
    assert {k: e_reg["metrics"][k] for k in LUNG_METRICS} == e_plain["metrics"]
    for k in ("full_cle", "full_pse"):
        assert torch.equal(e_reg[k], e_plain[k]), k
    assert {k: e_reg["metrics"][k] for k in processor.REGION_KEYS} == processor.region_metrics(t[0], names)
    if name == "blobs_u8":
        assert e_reg["error_messages"] == []
        assert all(v is not None for v in e_reg["metrics"]["cle_severity_score_per_region"].values())
    else:
        assert len(e_reg["error_messages"]) == 1 and "outside 1..5" in e_reg["error_messages"][0]
        assert str(int(t[0, 0, 2])) in e_reg["error_messages"][0]
        assert e_reg["metrics"]["cle_lesion_percentage_per_region"]["RUL"] is None
        assert e_reg["metrics"]["cle_lesion_percentage_per_region"]["LUL"] is not None
