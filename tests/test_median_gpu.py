"""GPU: the median noise filter of csrc/median.hip (dram_median3d through ops.median_filter3d) against the numpy yardstick
of tests/median_ref.py, exactly (torch.equal), for all seven window sizes, and the filter in front of the scan side of the
report (predict_case(scan_filter=...)).

Shapes.  The kernel's constants are TX = 64, TY = 8, TZ = 8 (outputs per workgroup along x, y, z; a thread owns an x-pair
and walks the TZ planes; the staged row is TX + 2 wide): besides the issue's list -- single voxel, W = 2, D = 3 alone, odd
W (1,7,5), W = 130 = 2 TX + 2, (5,9,67), (7,33,129) with 129 = 2 TX + 1 and 33 = 4 TY + 1 -- the three shapes
(7,7,63), (8,8,64), (9,9,65) put every axis one below, at and one above its tile extent, so that a last tile holds
one plane / one row / one voxel (a pair with no right half).  Contents: the whole int16 range with -32768 / 32767 planted
at the corners and inside, three values only (ties everywhere), a constant, HU-like noise with a -2048 block.  The
yardstick of a (shape, content, size) is computed once."""
import functools

import numpy as np
import pytest
import torch

import case_prep_ref as CR
import median_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TX, TY, TZ = 64, 8, 8                      # csrc/median.hip
SHAPES = [(1, 1, 1), (1, 1, 2), (3, 1, 1), (1, 7, 5), (2, 3, 130), (5, 9, 67), (7, 33, 129),
          (TZ - 1, TY - 1, TX - 1), (TZ, TY, TX), (TZ + 1, TY + 1, TX + 1)]
SENTINEL = 12345


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


@functools.lru_cache(maxsize=None)
def volume(shape, content):
    a = MR.CONTENTS[content](shape, 7 + len(content))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(shape, content, size):
    r = MR.median_filter(volume(shape, content), size)
    r.setflags(write=False)
    return r


def on_device(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_yardstick(ops, shape):
    for content in MR.CONTENTS:
        src = on_device(volume(shape, content))
        keep = src.clone()
        for size in MR.SIZES:
            out = torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV)
            got = ops.median_filter3d(src, size, out=out)
            assert got is out
            want = torch.from_numpy(np.array(reference(shape, content, size)))
            assert torch.equal(got.cpu(), want), (content, size)              # every element written, none a sentinel left
            fresh = ops.median_filter3d(src, size)
            assert fresh.dtype == torch.int16 and fresh.is_contiguous() and torch.equal(fresh, got), (content, size)
        assert torch.equal(src, keep), content                                # the input is only read


def test_sentinel_is_no_value_of_the_cases():
    for shape in SHAPES:
        for content in MR.CONTENTS:
            if content != "full_range":
                assert not (volume(shape, content) == SENTINEL).any()


def test_extremes_survive_the_packed_comparison(ops):
    """-32768 and 32767 side by side in both halves of a pair: a median that compared unsigned, or across the halves of a
    register, would order them wrongly"""
    a = np.empty((1, 1, 8), dtype=np.int16)
    a[0, 0] = [-32768, 32767, -32768, -1, 0, 32767, 32767, -32768]
    for size in ((1, 1, 3), (3, 3, 3)):
        got = ops.median_filter3d(on_device(a), size).cpu().numpy()
        assert got.tolist() == [[[-32768, -32768, -1, -1, 0, 32767, 32767, -32768]]] == MR.median_filter(a, size).tolist()


def test_non_contiguous_input_and_offset_output(ops):
    shape = (5, 9, 67)
    base = volume(shape, "full_range")
    src = on_device(base)
    want = torch.from_numpy(np.array(reference(shape, "full_range", (3, 3, 3))))
    wide = torch.zeros((5, 9, 80), dtype=torch.int16, device=DEV)
    wide[:, :, 5:72] = src
    view = wide[:, :, 5:72]
    assert not view.is_contiguous() and torch.equal(ops.median_filter3d(view).cpu(), want)
    swapped = src.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    assert not swapped.is_contiguous() and torch.equal(ops.median_filter3d(swapped).cpu(), want)
    # an output that starts on an odd element of its storage: the pair stores fall back to halves where they must
    flat = torch.full((src.numel() + 1,), SENTINEL, dtype=torch.int16, device=DEV)
    out = flat[1:].view(shape)
    assert out.data_ptr() % 4 == 2 and ops.median_filter3d(src, out=out) is out
    assert torch.equal(out.cpu(), want) and int(flat[0]) == SENTINEL
    odd_src = torch.cat([torch.zeros(1, dtype=torch.int16, device=DEV), src.reshape(-1)])[1:].view(shape)
    assert odd_src.data_ptr() % 4 == 2 and torch.equal(ops.median_filter3d(odd_src).cpu(), want)


def test_two_calls_are_bit_identical(ops):
    src = on_device(volume((7, 33, 129), "three_values"))
    for size in ((3, 3, 3), (1, 3, 3)):
        assert torch.equal(ops.median_filter3d(src, size), ops.median_filter3d(src, size))


def test_is_capturable(ops):
    shape = (7, 33, 129)
    src = on_device(volume(shape, "hu_noise"))
    eager = ops.median_filter3d(src)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.median_filter3d(src)                                              # warm-up on the side stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = ops.median_filter3d(src)
    for _ in range(2):
        captured.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
    assert torch.equal(eager.cpu(), torch.from_numpy(np.array(reference(shape, "hu_noise", (3, 3, 3)))))


def test_refusals_come_before_any_launch(ops, monkeypatch):
    img = torch.zeros((4, 6, 70), dtype=torch.int16, device=DEV)
    L = ops._L()
    launches = []

    class Spy:
        def __getattr__(self, name):
            if name == "dram_median3d":
                return lambda *a: launches.append(name) or L.dram_median3d(*a)
            return getattr(L, name)

    monkeypatch.setattr(ops, "_L", lambda: Spy())
    with pytest.raises(ValueError, match="size"):
        ops.median_filter3d(img, (1, 1, 1))
    with pytest.raises(ValueError, match="size"):
        ops.median_filter3d(img, (5, 3, 3))
    with pytest.raises(TypeError):
        ops.median_filter3d(img.float())
    with pytest.raises(ValueError, match="share storage"):
        ops.median_filter3d(img, out=img)
    with pytest.raises(ValueError, match="out"):
        ops.median_filter3d(img, out=torch.zeros((4, 6, 71), dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError, match="device"):
        ops.median_filter3d(img, out=torch.zeros((4, 6, 70), dtype=torch.int16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.median_filter3d(img.cpu())
    assert launches == []
    ops.median_filter3d(img)
    assert launches == ["dram_median3d"]


# ------------------------------------------------------------------------------------------------ predict_case
def _scan_side(processor, key):
    if processor._DENSITO_KEY.fullmatch(key) or processor._CLUSTER_KEY.fullmatch(key):
        return True
    return bool(processor._CORE_PEEL_KEY.fullmatch(key)) and key != "peel_mm" and \
        not key.startswith(("cle_", "pse_", "region_voxels"))


def test_predict_case_with_scan_filter(ops, monkeypatch):
    from bodyct_dram_emph_subtype_amd import models, processor, transforms as TR
    _, lobes, spacing, _ = CR.fixture_cases()["blobs_u8"]
    rng = np.random.default_rng(3)
    hu = np.clip(np.rint(rng.normal(-900.0, 12.0, size=tuple(lobes.shape))), -940, -860).astype(np.int16)
    hu[1::3, 2::4, 1::4] = -1000                       # isolated voxels below -950 HU, none next to another
    scan = torch.from_numpy(hu)
    target, n, peel = (16, 32, 32), 5, 3.0
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    calls = []
    real = ops.median_filter3d
    monkeypatch.setattr(ops, "median_filter3d", lambda *a, **k: calls.append(a[1:]) or real(*a, **k))
    run = lambda **kw: processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, uid="u", region_names=names,
                                              regions=True, densitometry=True, core_peel=True, peel_mm=peel, clusters=True,
                                              **kw)
    raw = run()
    assert calls == [] and "scan_filter" not in raw["metrics"]
    got = run(scan_filter=(3, 3, 3))
    assert calls == [((3, 3, 3),)]                                            # once, for three sections
    calls.clear()
    assert list(got["metrics"])[-1] == "scan_filter" and got["metrics"]["scan_filter"] == "median3x3x3"
    assert list(got["metrics"])[:-1] == list(raw["metrics"]) and set(got) == set(raw)
    for k in ("full_cle", "full_pse"):
        assert torch.equal(got[k], raw[k]), k
    net = [k for k in raw["metrics"] if not _scan_side(processor, k)]
    assert set(processor.REGION_KEYS) <= set(net) and "cle_lesion_percentage_per_region_peel" in net
    assert {k: got["metrics"][k] for k in net} == {k: raw["metrics"][k] for k in net}

    # the scan side: the sections' own functions on the filtered crop, and the filter is the yardstick's
    case = TR.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid="u", want_lobes=True)
    smooth = ops.median_filter3d(case["image"])
    calls.clear()
    assert torch.equal(smooth.cpu(), torch.from_numpy(MR.median_filter(case["image"].cpu().numpy(), (3, 3, 3))))
    assert torch.equal(processor.filtered_image(case["image"], (3, 3, 3)), smooth)
    labels = case["lobe_labels"]
    want = processor.densitometry_metrics(processor.densitometry(smooth, labels, spacing), names)
    want.update(processor.laa_cluster_metrics(processor.laa_clusters(smooth, labels, spacing), names))
    cp = processor.core_peel_metrics(processor.core_peel(smooth, labels, spacing, peel_mm=peel, n_regions=n), names)
    want.update({k: v for k, v in cp.items() if k != "peel_mm"})
    assert set(want) == {k for k in raw["metrics"] if _scan_side(processor, k)}
    assert {k: got["metrics"][k] for k in want} == want
    # direction: the isolated voxels are gone
    before, after = int(raw["metrics"]["laa950_clusters_per_lung"]), int(got["metrics"]["laa950_clusters_per_lung"])
    print(f"laa950 clusters per lung: {before} unfiltered, {after} behind the 3x3x3 median")
    assert before > 50 and after < before
    assert got["metrics"]["laa950_fraction_per_lung"] != raw["metrics"]["laa950_fraction_per_lung"]

    # only the clusters named: densitometry and core / peel are the raw scan's
    calls.clear()
    part = run(scan_filter=(3, 3, 3), scan_filter_sections=("clusters",))
    assert len(calls) == 1 and part["metrics"]["scan_filter"] == "median3x3x3"
    for k, v in raw["metrics"].items():
        assert part["metrics"][k] == (got if processor._CLUSTER_KEY.fullmatch(k) else raw)["metrics"][k], k
    calls.clear()
    flat = run(scan_filter=(1, 3, 3), scan_filter_sections=("densitometry",))
    assert calls == [((1, 3, 3),)] and flat["metrics"]["scan_filter"] == "median1x3x3"
    want13 = processor.densitometry_metrics(processor.densitometry(real(case["image"], (1, 3, 3)), labels, spacing), names)
    assert {k: flat["metrics"][k] for k in want13} == want13
    assert torch.equal(flat["full_cle"], raw["full_cle"])
