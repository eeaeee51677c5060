"""GPU: the fixed-point bilateral filter of csrc/bilateral.hip (dram_bilateral3d through ops.bilateral_filter3d) against
the numpy int64 yardstick of tests/bilateral_ref.py, exactly (torch.equal), and the filter in front of the scan side of
the report (processor.bilateral_image, predict_case(scan_filter=("bilateral", sigma_mm, sigma_hu))).

Shapes.  The kernel's constants are TX = 32, TY = 8, TZ = 8 (outputs per workgroup along x, y, z; a thread owns an
(x, y) column and walks the TZ planes; the staged tile has the halo of the radii on every side): besides the issue's list
-- single voxel, W = 2, D = 3 alone, odd W (1,7,5), (2,3,4) smaller than the radius on every axis, (5,9,67),
(7,33,129) -- the three shapes (7,7,31), (8,8,32), (9,9,33) put every axis one below, at and one above its tile extent.
Contents: the four of median_ref (the whole int16 range: the |d| clamp and the wide sum; three values; HU noise with a
-2048 block; a constant).  Parameters: radius 1 with a three-entry range table, radii (0,3,3) at 60 HU, radius 5 at
the 289 HU cap (on the shapes up to (5,9,67)).  Masks: none, labels 0..5 with holes as uint8 and as int16 (negative
labels among them: non-zero is inside), a strided view, all zero, all non-zero.  The yardstick of a (shape, content,
parameters, mask) is computed once."""
import functools

import numpy as np
import pytest
import torch

import bilateral_ref as BR
import case_prep_ref as CR
import median_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TX, TY, TZ = 32, 8, 8                      # csrc/bilateral.hip
SHAPES = [(1, 1, 1), (1, 1, 2), (3, 1, 1), (1, 7, 5), (2, 3, 4), (5, 9, 67), (7, 33, 129),
          (TZ - 1, TY - 1, TX - 1), (TZ, TY, TX), (TZ + 1, TY + 1, TX + 1)]
PARAMS = [((0.5, 0.5, 0.5), 0.5), ((0.2, 1.4, 1.4), 60.0), ((2.5, 2.5, 2.5), 289.0)]      # radii 1, (0,3,3), 5
RADIUS5_SHAPES = SHAPES[:6]                # radius 5 on the shapes up to (5,9,67): the yardstick stays within seconds
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
def labels(shape):
    """labels 0..5, a sixth of them 0, with a block hole and the first voxel inside"""
    rng = np.random.default_rng(sum(shape))
    lab = rng.integers(0, 6, size=shape).astype(np.uint8)
    D, H, W = shape
    lab[D // 2:, H // 3: H // 3 + 2, W // 4: W // 4 + 5] = 0
    lab[0, 0, 0] = 4
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def reference(shape, content, param, mask):
    """mask: None | 'labels' | 'zero'"""
    within = None if mask is None else (labels(shape) if mask == "labels" else np.zeros(shape, dtype=np.uint8))
    r = BR.bilateral_filter(volume(shape, content), param[0], param[1], within=within)
    r.setflags(write=False)
    return r


def on_device(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def params_of(shape):
    return [p for p in PARAMS if p[0][0] < 2.5 or shape in RADIUS5_SHAPES]


def test_the_parameters_take_the_radii_and_tables_they_are_meant_to(ops):
    assert [tuple(ops.bilateral_radius(s) for s in p[0]) for p in PARAMS] == [(1, 1, 1), (0, 3, 3), (5, 5, 5)]
    assert [len(ops.bilateral_tables(*p)[3]) for p in PARAMS] == [3, 213, 1022]
    assert all(len(params_of(s)) == (3 if s in RADIUS5_SHAPES else 2) for s in SHAPES) and (2, 3, 4) in RADIUS5_SHAPES


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_yardstick(ops, shape):
    D, H, W = shape
    lab = on_device(labels(shape))
    signed = lab.to(torch.int16) * torch.where(torch.arange(W, device=DEV) % 2 == 0, -1, 1).to(torch.int16)
    wide = torch.zeros((D, H + 2, W + 3), dtype=torch.uint8, device=DEV)
    wide[:, 1:H + 1, 2:W + 2] = lab
    view = wide[:, 1:H + 1, 2:W + 2]                                          # z / y strides of its own, x stride 1
    sparse = torch.zeros((D, H, 2 * W), dtype=torch.int16, device=DEV)
    sparse[:, :, ::2] = signed                                                # x stride 2: made contiguous by the wrapper
    masks = [(None, None), ("labels", lab), ("labels", signed), ("labels", view), ("labels", sparse[:, :, ::2]),
             ("labels", lab != 0), ("zero", torch.zeros(shape, dtype=torch.uint8, device=DEV)),
             (None, torch.full(shape, 7, dtype=torch.uint8, device=DEV)), (None, torch.full(shape, -3, dtype=torch.int16, device=DEV))]
    assert view.stride() == ((H + 2) * (W + 3), W + 3, 1) and signed.dtype == torch.int16 and bool((signed < 0).any())
    for content in MR.CONTENTS:
        src = on_device(volume(shape, content))
        keep = src.clone()
        for param in params_of(shape):
            for k, (mask, within) in enumerate(masks):
                out = torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV)
                got = ops.bilateral_filter3d(src, param[0], param[1], within=within, out=out)
                assert got is out
                want = torch.from_numpy(np.array(reference(shape, content, param, mask)))
                assert torch.equal(got.cpu(), want), (content, param, k)      # every element written, no sentinel left
                if mask == "zero":
                    assert torch.equal(got, src)
            fresh = ops.bilateral_filter3d(src, *param)
            assert fresh.dtype == torch.int16 and fresh.is_contiguous()
            assert torch.equal(fresh.cpu(), torch.from_numpy(np.array(reference(shape, content, param, None))))
        assert torch.equal(src, keep), content                                # the input is only read
    assert torch.equal(lab.cpu(), torch.from_numpy(np.array(labels(shape))))  # ... and so is the mask


def test_the_filter_does_something_on_the_cases():
    """the yardsticks differ from their inputs and from one another, so equality above is no equality of identities;
    three_values (-32768, -950, 32767) is the exception that has to be one: every difference lies beyond the range table"""
    shape = (5, 9, 67)
    for content in ("full_range", "hu_noise"):
        src = volume(shape, content)
        plain, masked = reference(shape, content, PARAMS[2], None), reference(shape, content, PARAMS[2], "labels")
        assert not np.array_equal(plain, src) and not np.array_equal(plain, masked), content
        assert np.array_equal(masked[labels(shape) == 0], src[labels(shape) == 0])
    for param in PARAMS:
        assert np.array_equal(reference(shape, "three_values", param, None), volume(shape, "three_values"))
        assert np.array_equal(reference(shape, "constant", param, "labels"), volume(shape, "constant"))


def test_exact_ties_round_half_up(ops):
    """sigma_x = sqrt(1 / (2 ln 2)) makes T_x[1] = 128 and S = 128, sigma_hu = 289 makes R[1] = 256: between two
    neighbours one unit away the centre's num / den is exactly +-65536 / 131072 = +-0.5, and the quotient is rounded up"""
    sigma = (0.0, 0.0, (1.0 / (2.0 * np.log(2.0))) ** 0.5)
    tz, ty, tx, R = ops.bilateral_tables(sigma, 289.0)
    assert (tz, ty, tx[:2], R[:2]) == ([256], [256], [256, 128], [256, 256])
    for sign, middle in ((1, 1), (-1, 0)):
        a = np.array([[[sign, 0, sign]]], dtype=np.int16) * np.ones((3, 4, 1), dtype=np.int16)
        want = BR.bilateral_filter(a, sigma, 289.0)
        assert (want[:, :, 1] == middle).all()
        assert torch.equal(ops.bilateral_filter3d(on_device(a), sigma, 289.0).cpu(), torch.from_numpy(want))


def test_scalar_sigma_and_truncate(ops):
    shape = (5, 9, 67)
    src = on_device(volume(shape, "hu_noise"))
    assert torch.equal(ops.bilateral_filter3d(src, 0.5, 0.5), ops.bilateral_filter3d(src, (0.5, 0.5, 0.5), 0.5))
    want = BR.bilateral_filter(volume(shape, "hu_noise"), (1.0, 0.6, 1.2), 45.0, truncate=3.0)    # radii (3, 2, 4)
    assert torch.equal(ops.bilateral_filter3d(src, (1.0, 0.6, 1.2), 45.0, truncate=3.0).cpu(), torch.from_numpy(want))
    assert torch.equal(ops.bilateral_filter3d(src, (0.2, 0.1, 0.0), 60.0), src)                   # all radii 0: the identity


def test_non_contiguous_input_and_odd_offsets(ops):
    shape = (5, 9, 67)
    param = PARAMS[1]
    src = on_device(volume(shape, "full_range"))
    want = torch.from_numpy(np.array(reference(shape, "full_range", param, None)))
    wide = torch.zeros((5, 9, 80), dtype=torch.int16, device=DEV)
    wide[:, :, 5:72] = src
    view = wide[:, :, 5:72]
    assert not view.is_contiguous() and torch.equal(ops.bilateral_filter3d(view, *param).cpu(), want)
    swapped = src.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    assert not swapped.is_contiguous() and torch.equal(ops.bilateral_filter3d(swapped, *param).cpu(), want)
    # an output and an input that start on an odd element of their storage
    flat = torch.full((src.numel() + 2,), SENTINEL, dtype=torch.int16, device=DEV)
    out = flat[1:-1].view(shape)
    assert out.data_ptr() % 4 == 2 and ops.bilateral_filter3d(src, *param, out=out) is out
    assert torch.equal(out.cpu(), want) and int(flat[0]) == SENTINEL and int(flat[-1]) == SENTINEL
    odd_src = torch.cat([torch.zeros(1, dtype=torch.int16, device=DEV), src.reshape(-1)])[1:].view(shape)
    assert odd_src.data_ptr() % 4 == 2 and torch.equal(ops.bilateral_filter3d(odd_src, *param).cpu(), want)
    lab = on_device(labels(shape))
    odd_lab = torch.cat([torch.zeros(1, dtype=torch.uint8, device=DEV), lab.reshape(-1)])[1:].view(shape)
    masked = torch.from_numpy(np.array(reference(shape, "full_range", param, "labels")))
    assert torch.equal(ops.bilateral_filter3d(odd_src, *param, within=odd_lab, out=out).cpu(), masked)


def test_two_calls_are_bit_identical(ops):
    src = on_device(volume((7, 33, 129), "three_values"))
    lab = on_device(labels((7, 33, 129)))
    for param in PARAMS:
        assert torch.equal(ops.bilateral_filter3d(src, *param), ops.bilateral_filter3d(src, *param))
        assert torch.equal(ops.bilateral_filter3d(src, *param, within=lab), ops.bilateral_filter3d(src, *param, within=lab))


def test_is_capturable(ops):
    shape = (7, 33, 129)
    param = PARAMS[1]
    src = on_device(volume(shape, "hu_noise"))
    lab = on_device(labels(shape))
    eager = ops.bilateral_filter3d(src, *param, within=lab)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.bilateral_filter3d(src, *param, within=lab)                       # warm-up on the side stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = ops.bilateral_filter3d(src, *param, within=lab)
    for _ in range(2):
        captured.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
    assert torch.equal(eager.cpu(), torch.from_numpy(np.array(reference(shape, "hu_noise", param, "labels"))))


def test_refusals_come_before_any_launch(ops, monkeypatch):
    img = torch.zeros((4, 6, 70), dtype=torch.int16, device=DEV)
    L = ops._L()
    launches = []

    class Spy:
        def __getattr__(self, name):
            if name == "dram_bilateral3d":
                return lambda *a: launches.append(name) or L.dram_bilateral3d(*a)
            return getattr(L, name)

    monkeypatch.setattr(ops, "_L", lambda: Spy())
    f = ops.bilateral_filter3d
    with pytest.raises(ValueError, match="radius 6"):
        f(img, 3.0, 60.0)
    with pytest.raises(ValueError, match="sigma"):
        f(img, (1.0, 1.0), 60.0)
    with pytest.raises(ValueError, match="sigma_hu"):
        f(img, 1.0, 0.0)
    with pytest.raises(ValueError, match="1024"):
        f(img, 1.0, 290.0)
    with pytest.raises(TypeError):
        f(img.float(), 1.0, 60.0)
    with pytest.raises(ValueError, match="share storage"):
        f(img, 1.0, 60.0, out=img)
    with pytest.raises(ValueError, match="out"):
        f(img, 1.0, 60.0, out=torch.zeros((4, 6, 71), dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError, match="device"):
        f(img, 1.0, 60.0, out=torch.zeros((4, 6, 70), dtype=torch.int16))
    with pytest.raises(ValueError, match="within"):
        f(img, 1.0, 60.0, within=torch.zeros((4, 6, 71), dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError, match="within"):
        f(img, 1.0, 60.0, within=torch.zeros((4, 6, 70), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(img, 1.0, 60.0, within=torch.zeros((4, 6, 70), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(img.cpu(), 1.0, 60.0)
    assert launches == []
    f(img, 1.0, 289.0)
    assert launches == ["dram_bilateral3d"]


# ------------------------------------------------------------------------------------------------ the report
def _scan_side(processor, key):
    if processor._DENSITO_KEY.fullmatch(key) or processor._CLUSTER_KEY.fullmatch(key):
        return True
    return bool(processor._CORE_PEEL_KEY.fullmatch(key)) and key != "peel_mm" and \
        not key.startswith(("cle_", "pse_", "region_voxels"))


def _noisy_scan(lobes):
    rng = np.random.default_rng(3)
    hu = np.clip(np.rint(rng.normal(-900.0, 12.0, size=tuple(lobes.shape))), -940, -860).astype(np.int16)
    hu[1::3, 2::4, 1::4] = -1000                       # isolated voxels below -950 HU, none next to another
    hu[lobes.numpy() == 0] += 900                      # the chest wall and the mediastinum: what a Gaussian would mix in
    return hu


def test_bilateral_image_is_the_crop_of_the_filtered_scan_at_lung_voxels(ops):
    from bodyct_dram_emph_subtype_amd import processor, transforms as TR
    _, lobes, spacing, _ = CR.fixture_cases()["blobs_u8"]
    hu = _noisy_scan(lobes)
    scan = torch.from_numpy(hu).to(DEV)
    sig = processor.bilateral_sigma_voxels("t", spacing, 1.0)
    assert max(ops.bilateral_radius(s) for s in sig) >= 2
    whole = ops.bilateral_filter3d(scan, sig, 60.0, within=lobes.to(DEV))
    assert torch.equal(whole.cpu(), torch.from_numpy(BR.bilateral_filter(hu, sig, 60.0, within=lobes.numpy())))
    for kw in ({}, {"dilate_iterations": 0}, {"dilate_iterations": 0, "crop_border": 0}):
        case = TR.prepare_case(scan, lobes.to(DEV), spacing, uid="u", want_lobes=True, **kw)
        got = processor.bilateral_image(case["image"], case["lobe_labels"], spacing, 1.0, 60.0)
        (z0, z1), (y0, y1), (x0, x1) = case["crop_slice"].tolist()
        lung = case["lobe_labels"] != 0
        assert got.dtype == torch.int16 and got.shape == case["image"].shape and int(lung.sum()) > 1000
        assert torch.equal(got[lung], whole[z0:z1, y0:y1, x0:x1][lung]), kw
        assert torch.equal(got[~lung], case["image"][~lung]), kw              # a voxel outside the lung keeps the case's value
        assert not torch.equal(got[lung], case["image"][lung])


def test_predict_case_with_bilateral_scan_filter(ops, monkeypatch):
    from bodyct_dram_emph_subtype_amd import models, processor, transforms as TR
    _, lobes, spacing, _ = CR.fixture_cases()["blobs_u8"]
    scan = torch.from_numpy(_noisy_scan(lobes))
    target, n, peel = (16, 32, 32), 5, 3.0
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    calls, others = [], []
    real = ops.bilateral_filter3d
    real_median, real_gauss = ops.median_filter3d, ops.gaussian_filter3d
    monkeypatch.setattr(ops, "bilateral_filter3d", lambda *a, **k: calls.append((a[1:], sorted(k))) or real(*a, **k))
    monkeypatch.setattr(ops, "median_filter3d", lambda *a, **k: others.append("median") or real_median(*a, **k))
    monkeypatch.setattr(ops, "gaussian_filter3d", lambda *a, **k: others.append("gaussian") or real_gauss(*a, **k))
    run = lambda **kw: processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, uid="u", region_names=names,
                                              regions=True, densitometry=True, core_peel=True, peel_mm=peel, clusters=True,
                                              **kw)
    raw = run()
    assert calls == [] and others == [] and "scan_filter" not in raw["metrics"]
    got = run(scan_filter=("bilateral", 1.0, 60.0))
    sig = tuple(1.0 / s for s in spacing)
    assert calls == [((sig, 60.0), ["within"])] and others == []               # once, for three sections
    calls.clear()
    assert list(got["metrics"])[-1] == "scan_filter" and got["metrics"]["scan_filter"] == "bilateral1.00mm60.0hu"
    assert list(got["metrics"])[:-1] == list(raw["metrics"]) and set(got) == set(raw)
    for k in ("full_cle", "full_pse"):
        assert torch.equal(got[k], raw[k]), k
    net = [k for k in raw["metrics"] if not _scan_side(processor, k)]
    assert set(processor.REGION_KEYS) <= set(net) and "cle_lesion_percentage_per_region_peel" in net
    assert {k: got["metrics"][k] for k in net} == {k: raw["metrics"][k] for k in net}

    # the scan side: the sections' own functions on bilateral_image, which is the yardstick's
    case = TR.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid="u", want_lobes=True)
    labels_ = case["lobe_labels"]
    smooth = processor.bilateral_image(case["image"], labels_, spacing, 1.0, 60.0)
    calls.clear()
    assert torch.equal(smooth.cpu(), torch.from_numpy(BR.bilateral_filter(case["image"].cpu().numpy(), sig, 60.0,
                                                                          within=labels_.cpu().numpy())))
    want = processor.densitometry_metrics(processor.densitometry(smooth, labels_, spacing), names)
    want.update(processor.laa_cluster_metrics(processor.laa_clusters(smooth, labels_, spacing), names))
    cp = processor.core_peel_metrics(processor.core_peel(smooth, labels_, spacing, peel_mm=peel, n_regions=n), names)
    want.update({k: v for k, v in cp.items() if k != "peel_mm"})
    assert set(want) == {k for k in raw["metrics"] if _scan_side(processor, k)}
    assert {k: got["metrics"][k] for k in want} == want
    assert {k: raw["metrics"][k] for k in want} != want                       # ... and they are not the raw scan's
    print("laa950 fraction per lung:", raw["metrics"]["laa950_fraction_per_lung"], "unfiltered,",
          got["metrics"]["laa950_fraction_per_lung"], "behind the bilateral filter")

    # only the clusters named: densitometry and core / peel are the raw scan's
    part = run(scan_filter=("bilateral", 1.0, 60.0), scan_filter_sections=("clusters",))
    assert len(calls) == 1 and part["metrics"]["scan_filter"] == "bilateral1.00mm60.0hu"
    for k, v in raw["metrics"].items():
        assert part["metrics"][k] == (got if processor._CLUSTER_KEY.fullmatch(k) else raw)["metrics"][k], k
    # no section named that is on: nothing is filtered and the key is absent
    calls.clear()
    assert "scan_filter" not in processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, uid="u",
                                                       region_names=names, densitometry=True,
                                                       scan_filter=("bilateral", 1.0, 60.0),
                                                       scan_filter_sections=("clusters",))["metrics"] and calls == []
    # the median's precondition does not apply: taps never leave the lung, so the fill value is never a tap
    flat = run(scan_filter=["bilateral", 1, 60], dilate_iterations=0)
    assert len(calls) == 1 and flat["metrics"]["scan_filter"] == "bilateral1.00mm60.0hu" and others == []
    lung_only = [k for k in want if processor._CLUSTER_KEY.fullmatch(k) or processor._DENSITO_KEY.fullmatch(k)]
    assert lung_only and {k: flat["metrics"][k] for k in lung_only} == {k: want[k] for k in lung_only}
