"""GPU: the per-lobe histogram of csrc/densito.hip (dram_lobe_hist through ops.lobe_histogram) against the numpy
yardstick of tests/densito_ref.py -- hist and sums EXACTLY, every case -- and the path from scan + lobes to the
densitometry entries of the report (transforms.prepare_case(want_lobes) -> processor.densitometry -> predict_case).

Shapes, from dram_lobe_hist_nblk's own rule (1024 threads x 8 voxels = 8192 voxels per workgroup and step, at most 256
workgroups): (a) 5 x 7 x 11 = 385 voxels: one workgroup, 49 groups of 8 in one ragged wave, the last group ragged, W no
multiple of any vector width (most groups cross a row end); (b) 6 x 37 x 123 = 27 306 voxels, the labels a crop view
big[1:, 2:, 3:] of a 7 x 39 x 126 volume (rows start at element 5169 + 126 k: odd for every other row, strides above
the shape): 4 workgroups, uncapped, the last one ragged; (c) 9 x 512 x 457 = 2 105 856 voxels, the smallest kind of
size that puts the workgroup count at its cap of 256 (9 x 384 x 320 gives 135 workgroups): 8704 voxels more than one full
stride of the grid, so the second stride is ragged (workgroup 0 full, workgroup 1 partly, the rest idle) and rows of
457 start at odd offsets.
Every case runs with torch.empty / empty_like poisoned (floats NaN, bytes 0xFF, integers a large negative number): an
unwritten element fails.  Every case prints its launch figures before it asserts (pytest -s)."""
import math

import numpy as np
import pytest
import torch

import case_prep_ref as CR
import densito_ref as DR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -1234567891


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
        elif t.dtype in (torch.int32, torch.int64):
            t.fill_(POISON)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(e0(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(el0(*a, **k)))
    yield
    torch.cuda.synchronize()


SHAPES = {"a-one-group": (5, 7, 11), "b-crop-view": (6, 37, 123), "c-capped": (9, 512, 457)}
OFFSET = (1, 2, 3)                      # (b): the labels are big[1:, 2:, 3:]
WG_VOXELS, WG_CAP = 8192, 256
_SCANS = {}


def scan_of(sid):
    """lung-like HU (peak near -850, every third y-row quantised to multiples of 32 so that equal x-neighbours are
    common), with the edge values of bins and int16 sprinkled in: computed once per shape, shared, left unchanged"""
    if sid not in _SCANS:
        shape = SHAPES[sid]
        scan, _ = DR.lung_like(shape, 5, seed=len(_SCANS) + 31)
        scan[:, ::3, :] = (scan[:, ::3, :] // 32) * 32
        flat = scan.reshape(-1)
        edge = np.array([-32768, -1101, -1100, -1099, -1025, -1024, -1023, -951, -950, -949, -1, 0, 947, 948, 32767], dtype=np.int16)
        pos = np.linspace(0, flat.size - 1, edge.size * 3).astype(np.int64)
        flat[pos] = np.tile(edge, 3)
        scan.setflags(write=False)
        _SCANS[sid] = (scan, torch.from_numpy(scan.copy()).to(DEV))
    return _SCANS[sid]


def labels_of(shape, n, kind, seed):
    """'u8': labels 0..n in x-runs of random length, a few voxels above n (-> row 0), region n absent when n > 1;
    'i16': the same as int16 with negatives (not lung) and 300 (-> row 0)"""
    rng = np.random.default_rng(seed)
    total = math.prod(shape)
    runs = rng.integers(1, 40, size=total // 8 + 2)
    lab = np.repeat(rng.integers(0, n + 1, size=runs.size), runs)[:total].astype(np.int16)
    assert lab.size == total
    if n > 1:
        lab[lab == n] = 0
    pos = rng.choice(total, size=min(12, total // 8), replace=False)
    if kind == "u8":
        lab[pos] = np.resize(np.array([n + 1, 200, 255]), pos.size)
        lab = lab.astype(np.uint8)
    else:
        lab[pos] = np.resize(np.array([300, -1, -32768, n + 1, 32767, -7]), pos.size)
    return lab.reshape(shape)


def on_device(sid, lab):
    """the label operand: contiguous, or for (b) a crop view of a larger volume filled with a foreign label"""
    t = torch.from_numpy(lab)
    if sid != "b-crop-view":
        return t.to(DEV)
    big = torch.full(tuple(s + o for s, o in zip(lab.shape, OFFSET)), 3, dtype=t.dtype)
    big[OFFSET[0]:, OFFSET[1]:, OFFSET[2]:] = t
    view = big.to(DEV)[OFFSET[0]:, OFFSET[1]:, OFFSET[2]:]
    assert not view.is_contiguous() and view.stride(2) == 1 and view.storage_offset() % 2 == 1
    assert view.stride(1) > lab.shape[2] and view.stride(0) > lab.shape[1] * view.stride(1)
    return view


def figures(ops, shape, n, nbins):
    vox = math.prod(shape)
    nblk = ops._L().dram_lobe_hist_nblk(vox)
    groups = -(-vox // 8)
    counters = (n + 1) * nbins
    lds = 4 * (8192 if counters <= 8192 else 16384 if counters <= 16384 else 32768)
    return (f"voxels {vox}, workgroups {nblk}, groups of 8: {groups}, strides {-(-groups // (nblk * 1024))}, "
            f"counters {counters} in {lds // 1024} KiB LDS")


def check(ops, what, scan_np, scan_d, lab_np, lab_d, n, hu_lo=-1024, nbins=1024):
    print(f"[{what}] {figures(ops, scan_np.shape, n, nbins)}")
    want_h, want_s = DR.histogram(scan_np, lab_np, n, hu_lo, nbins)
    hist, sums = ops.lobe_histogram(scan_d, lab_d, n, hu_lo, nbins)
    assert hist.dtype == sums.dtype == torch.int64 and tuple(hist.shape) == (n + 1, nbins) and tuple(sums.shape) == (n + 1, 2)
    h, s = hist.cpu().numpy(), sums.cpu().numpy()
    print(f"[{what}] rows {s[:, 0].tolist()}; differing bins {int((h != want_h).sum())}, differing sums {int((s != want_s).sum())}")
    assert np.array_equal(h, want_h), what
    assert np.array_equal(s, want_s), what
    assert int(s[:, 0].sum()) == int((lab_np > 0).sum())                      # the rows add up to the lung
    again = ops.lobe_histogram(scan_d, lab_d, n, hu_lo, nbins)
    assert torch.equal(again[0], hist) and torch.equal(again[1], sums), f"{what}: second call"
    return h, s


@pytest.mark.parametrize("kind", ["u8", "i16"])
@pytest.mark.parametrize("n", [1, 5, 15])
@pytest.mark.parametrize("sid", sorted(SHAPES))
def test_hist_and_sums_are_exact(ops, sid, n, kind):
    scan_np, scan_d = scan_of(sid)
    lab = labels_of(SHAPES[sid], n, kind, seed=7 * n + len(kind))
    h, s = check(ops, f"{sid} n={n} {kind}", scan_np, scan_d, lab, on_device(sid, lab), n)
    if n > 1:
        assert int(s[n, 0]) == 0 and int(h[n].sum()) == 0                     # the absent region
    assert int(s[0, 0]) > 0                                                   # labels above n are in row 0


@pytest.mark.parametrize("n", [5, 15])
@pytest.mark.parametrize("sid", sorted(SHAPES))
def test_other_bins(ops, sid, n):
    """hu_lo = -1100, nbins = 2048: 6 x 2048 counters take the 64 KiB image, 16 x 2048 the 128 KiB one (supported)"""
    scan_np, scan_d = scan_of(sid)
    lab = labels_of(SHAPES[sid], n, "u8", seed=n)
    check(ops, f"{sid} n={n} bins -1100..947", scan_np, scan_d, lab, on_device(sid, lab), n, hu_lo=-1100, nbins=2048)


def test_unsupported_layouts_are_refused(ops):
    scan_np, scan_d = scan_of("a-one-group")
    lab = torch.from_numpy(labels_of(SHAPES["a-one-group"], 5, "u8", 1)).to(DEV)
    for kw in (dict(nbins=1000), dict(nbins=4096), dict(n_regions=15, nbins=2048, hu_lo=30800), dict(hu_lo=-40000)):
        with pytest.raises(RuntimeError, match="code -2"):
            ops.lobe_histogram(scan_d, lab, **kw)


def test_one_label_one_value_everywhere(ops):
    """maximal contention: every voxel of (c) hits ONE counter, which ends at 2 105 856 -- far above 2^16, and one
    workgroup alone sees 8192 or 16384 of them"""
    shape = SHAPES["c-capped"]
    scan = np.full(shape, -873, dtype=np.int16)
    lab = np.full(shape, 4, dtype=np.uint8)
    h, s = check(ops, "one counter", scan, torch.from_numpy(scan).to(DEV), lab, torch.from_numpy(lab).to(DEV), 5)
    assert int(h[4, -873 + 1024]) == math.prod(shape) == int(h.sum()) and s[4].tolist() == [math.prod(shape), -873 * math.prod(shape)]


def test_edge_values_only(ops):
    """both end bins, the threshold edges and the raw int64 sum: HU drawn from ten edge values only"""
    shape = SHAPES["c-capped"]
    values = np.array([-32768, -1025, -1024, -1023, -951, -950, -949, -1, 0, 32767], dtype=np.int16)
    rng = np.random.default_rng(5)
    scan = values[rng.integers(0, values.size, size=shape)]
    lab = labels_of(shape, 5, "i16", seed=3)
    h, s = check(ops, "edge values", scan, torch.from_numpy(scan).to(DEV), lab, torch.from_numpy(lab).to(DEV), 5)
    assert int(h[:, 1:-1].sum()) == int(((scan > -1024) & (scan < -1) & (lab > 0)).sum())
    assert int(s[:, 1].sum()) == int(scan.astype(np.int64)[lab > 0].sum())


def test_launch_forms_are_the_intended_ones(ops):
    L = ops._L()
    vox = {k: math.prod(v) for k, v in SHAPES.items()}
    assert [L.dram_lobe_hist_nblk(vox[s]) for s in sorted(SHAPES)] == [1, 4, WG_CAP]
    assert vox["a-one-group"] % 8 and vox["a-one-group"] < 64 * 8 and SHAPES["a-one-group"][2] % 2
    assert vox["b-crop-view"] % WG_VOXELS and vox["b-crop-view"] % 8 and SHAPES["b-crop-view"][2] % 8
    assert L.dram_lobe_hist_nblk(WG_CAP * WG_VOXELS - WG_VOXELS) == WG_CAP - 1              # (c) is just above the cap ...
    assert WG_CAP * WG_VOXELS < vox["c-capped"] < WG_CAP * WG_VOXELS + 2 * WG_VOXELS          # ... and its 2nd stride ragged
    assert (vox["c-capped"] - WG_CAP * WG_VOXELS) % WG_VOXELS and SHAPES["c-capped"][2] % 2


def test_label_views_and_types(ops):
    scan_np, scan_d = scan_of("b-crop-view")
    shape = SHAPES["b-crop-view"]
    lab = labels_of(shape, 5, "u8", seed=2)
    want_h, want_s = DR.histogram(scan_np, lab, 5)
    ld = torch.from_numpy(lab).to(DEV)
    tr = ld.transpose(1, 2).contiguous().transpose(1, 2)                      # x stride != 1: copied, not misread
    assert tr.stride(2) != 1
    hist, sums = ops.lobe_histogram(scan_d, tr, 5)
    assert np.array_equal(hist.cpu().numpy(), want_h) and np.array_equal(sums.cpu().numpy(), want_s)
    lung = lab > 0                                                            # bool labels: one region
    hb, sb = ops.lobe_histogram(scan_d, torch.from_numpy(lung).to(DEV), 1)
    wh, ws = DR.histogram(scan_np, lung.astype(np.uint8), 1)
    assert np.array_equal(hb.cpu().numpy(), wh) and np.array_equal(sb.cpu().numpy(), ws)
    odd = torch.empty(scan_d.numel() + 1, dtype=torch.int16, device=DEV)[1:].view(shape)      # image base not 16-byte aligned
    odd.copy_(scan_d)
    assert odd.data_ptr() % 16 and odd.is_contiguous()
    ho, so = ops.lobe_histogram(odd, ld, 5)
    assert np.array_equal(ho.cpu().numpy(), want_h) and np.array_equal(so.cpu().numpy(), want_s)
    with pytest.raises(TypeError):
        ops.lobe_histogram(scan_d, ld.to(torch.int32))
    with pytest.raises(TypeError):
        ops.lobe_histogram(scan_d.float(), ld)
    with pytest.raises(ValueError):
        ops.lobe_histogram(scan_d, ld[:, :, :100])
    with pytest.raises(ValueError):
        ops.lobe_histogram(scan_d[:, :, ::2], ld[:, :, ::2])                  # the image must be contiguous


# ------------------------------------------------------------------------------------------------ densitometry
def test_densitometry_equals_the_yardstick(ops):
    from bodyct_dram_emph_subtype_amd import processor
    shape, spacing = (12, 64, 83), (1.25, 0.7, 0.65)
    scan, lab = DR.lung_like(shape, 5, seed=17)
    lab[lab == 2] = 0                                                         # an absent lobe
    lab[3, 5, 20:24] = 9                                                      # lung outside 1..5
    want = DR.densitometry(scan, lab, spacing)
    p15 = want["perc"][0]
    print(f"[densitometry] yardstick Perc15 {p15.tolist()}, LAA-950 {want['laa'][0].round(4).tolist()}, "
          f"volumes {want['volume_ml'].round(2).tolist()} ml")
    assert np.all((p15[[1, 3, 4, 5]] > -1024 + 1) & (p15[[1, 3, 4, 5]] < -2))      # strictly inside the bins (yardstick alone)
    got = processor.densitometry(torch.from_numpy(scan).to(DEV), torch.from_numpy(lab).to(DEV), spacing)
    assert all(v.is_cuda for v in got.values() if torch.is_tensor(v))
    DR.assert_matches(got, want, "device")
    assert int(got["voxels"][0]) == 4 and int(got["voxels"][2]) == 0
    kw = dict(n_regions=5, thresholds=(-856, -700), percentiles=(10, 50), hu_lo=-1100, nbins=2048)
    got = processor.densitometry(torch.from_numpy(scan).to(DEV), torch.from_numpy(lab).to(DEV), spacing, **kw)
    DR.assert_matches(got, DR.densitometry(scan, lab, spacing, 5, (-856, -700), (10, 50), -1100, 2048), "other bins")
    with pytest.raises(ValueError, match="threshold"):
        processor.densitometry(torch.from_numpy(scan).to(DEV), torch.from_numpy(lab).to(DEV), spacing, thresholds=(-1024,))


def test_densitometry_is_capturable(ops):
    from bodyct_dram_emph_subtype_amd import processor
    shape, spacing = SHAPES["b-crop-view"], (1.0, 0.8, 0.8)
    scan_np, scan_d = scan_of("b-crop-view")
    lab = on_device("b-crop-view", labels_of(shape, 5, "u8", seed=4))
    eager = processor.densitometry(scan_d, lab, spacing)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        processor.densitometry(scan_d, lab, spacing)                          # warm-up on the side stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = processor.densitometry(scan_d, lab, spacing)
    keys = ("voxels", "volume_ml", "mean_density", "laa", "laa_counts", "perc")
    for _ in range(2):
        for k in keys:
            captured[k].fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(captured[k].nan_to_num(-1.0), eager[k].nan_to_num(-1.0)), k
            assert torch.equal(captured["whole_lung"][k].nan_to_num(-1.0), eager["whole_lung"][k].nan_to_num(-1.0)), k


@pytest.mark.parametrize("name", ["blobs_u8", "lobes_i16"])
def test_crop_loses_nothing(ops, name):
    """prepare_case's crop against the UNCROPPED scan and lobes: the whole-lung count is lung_mask.sum(), the count
    below -910 is ess_mask.sum() (the reference's ess rule), and both are the yardstick's on the full volumes"""
    from bodyct_dram_emph_subtype_amd import processor, transforms as T
    scan, lobes, spacing, border = CR.fixture_cases()[name]
    case = T.prepare_case(scan.to(DEV), lobes.to(DEV), spacing, uid=name, crop_border=border, want_lobes=True)
    got = processor.densitometry(case["image"], case["lobe_labels"], spacing)
    want = DR.densitometry(scan.numpy(), lobes.numpy(), spacing)
    DR.assert_matches(got, want, name)
    whole = got["whole_lung"]
    i910 = got["thresholds"].index(-910)
    print(f"[{name}] lung voxels {int(whole['voxels'])}, below -910: {int(whole['laa_counts'][i910])}")
    assert int(whole["voxels"]) == int(case["lung_mask"].sum()) == int((lobes > 0).sum())
    assert int(whole["laa_counts"][i910]) == int(case["ess_mask"].sum()) == int(((scan < -910) & (lobes > 0)).sum())


@pytest.mark.parametrize("name", ["blobs_u8", "lobes_i16"])
def test_predict_case_with_densitometry(ops, name, monkeypatch):
    from bodyct_dram_emph_subtype_amd import models, processor
    scan, lobes, spacing, border = CR.fixture_cases()[name]
    target = (16, 32, 32)
    torch.manual_seed(11)
    mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    kw = dict(uid=name, crop_border=border, region_names=names)
    calls = []
    fused = ops.upproject_regions
    monkeypatch.setattr(ops, "upproject_regions", lambda *a, **k: calls.append(1) or fused(*a, **k))

    e_plain = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, **kw)
    e_dens = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, densitometry=True, **kw)
    assert calls == []                                                          # regions=False: the two-pass tail
    want = processor.densitometry_metrics(DR.densitometry(scan.numpy(), lobes.numpy(), spacing), names)
    new = set(e_dens["metrics"]) - set(e_plain["metrics"])
    assert new == set(want) and len(want) == 10
    assert {k: e_dens["metrics"][k] for k in want} == want
    print(f"[{name}] {({k: e_dens['metrics'][k] for k in sorted(want) if k.endswith('_per_lung')})}")
    assert {k: e_dens["metrics"][k] for k in e_plain["metrics"]} == e_plain["metrics"]
    assert set(e_dens) == set(e_plain) and e_dens["entity"] == e_plain["entity"]
    for k in ("full_cle", "full_pse"):
        assert torch.equal(e_dens[k], e_plain[k]), k
    if name == "blobs_u8":
        assert e_dens["error_messages"] == e_plain["error_messages"] == []
        assert e_dens["metrics"]["volume_ml_per_region"]["RUL"] is not None
    else:                                                                       # label 300: lung in no region
        outside = int((lobes > 5).sum())
        assert len(e_dens["error_messages"]) == 1 and str(outside) in e_dens["error_messages"][0]
        assert "1..5" in e_dens["error_messages"][0] and e_dens["metrics"]["mean_lung_density_per_region"]["RUL"] is None

    # both switches: the regional keys are those of regions=True alone, the densitometry keys those above
    e_reg = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, regions=True, **kw)
    n_fused = len(calls)
    e_both = processor.predict_case(mod, scan.to(DEV), lobes.to(DEV), spacing, target, regions=True, densitometry=True,
                                    densitometry_kw=dict(thresholds=(-950, -910), percentiles=(15,)), **kw)
    assert n_fused == 1 and len(calls) == 2
    assert {k: e_both["metrics"][k] for k in e_reg["metrics"]} == e_reg["metrics"]
    assert {k: e_both["metrics"][k] for k in want} == want
    assert e_both["error_messages"][:len(e_reg["error_messages"])] == e_reg["error_messages"]
    for k in ("full_cle", "full_pse"):
        assert torch.equal(e_both[k], e_plain[k]), k
