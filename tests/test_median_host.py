"""Host side of the median noise filter (no GPU): the numpy yardstick of tests/median_ref.py against
scipy.ndimage.median_filter(mode='nearest') (where scipy is present) and against a triple loop over the definition; the
header's entry point and the launcher's refusals through ctypes with dummy pointers (no launch); the refusals of
ops.median_filter3d and of predict_case(scan_filter=...) on CPU tensors; predict_case with every kernel wrapper replaced by
its yardstick (the stubs of tests/golden/make_golden_report.py) for the 16 switch combinations; and the property the
option rests on: at lung voxels the filtered prepared crop is the crop of the filtered scan."""
import ctypes
import importlib.util
import itertools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import case_prep_ref as CP
import median_ref as MR
from conftest import GOLDEN


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("size", MR.SIZES)
def test_yardstick_equals_scipy(size):
    ndi = pytest.importorskip("scipy.ndimage")
    for shape, seed in (((5, 9, 67), 1), ((1, 7, 5), 2), ((3, 1, 1), 3), ((2, 3, 130), 4)):
        for name, make in MR.CONTENTS.items():
            a = make(shape, seed)
            assert np.array_equal(MR.median_filter(a, size), ndi.median_filter(a, size=size, mode="nearest")), (shape, name)


def test_yardstick_equals_the_definition():
    assert len(MR.SIZES) == 7 and (3, 3, 3) in MR.SIZES and (1, 3, 3) in MR.SIZES and (1, 1, 1) not in MR.SIZES
    a = MR.full_range((3, 4, 5), 11)
    b = MR.three_values((3, 4, 5), 12)
    for size in MR.SIZES:
        for v in (a, b):
            got = MR.median_filter(v, size)
            assert got.dtype == np.int16 and got.flags.c_contiguous and np.array_equal(got, MR.brute_force(v, size)), size
    one = np.array([[[7]]], dtype=np.int16)
    assert MR.median_filter(one, (3, 3, 3)).tolist() == [[[7]]]
    line = np.array([[[5, -32768, 32767, 0]]], dtype=np.int16)                  # windows: 5 5 -32768 | ... | 32767 0 0
    assert MR.median_filter(line, (1, 1, 3)).tolist() == [[[5, 5, 0, 0]]]
    assert MR.median_filter(line, (3, 3, 1)).tolist() == line.tolist()          # replication alone changes nothing


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_point_is_declared_and_exported():
    from ctypes import c_int as I, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _build, _lib
    res, args = _lib.SIGNATURES["dram_median3d"]
    assert res is I and list(args) == [P, P, I, I, I, I, I, I, P]
    out = subprocess.run(["nm", "-D", "--defined-only", _build.build_library()], capture_output=True, text=True,
                         check=True).stdout
    assert "dram_median3d" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_median3d_refuses_bad_and_unsupported_arguments_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    one, two = ctypes.c_void_p(256), ctypes.c_void_p(512)       # never dereferenced: the argument checks come first

    def call(src=one, dst=two, size=(5, 7, 11), r=(1, 1, 1)):
        return lib.dram_median3d(src, dst, *size, *r, None)

    assert call(src=None) == BAD and call(dst=None) == BAD and call(src=None, dst=None) == BAD
    assert call(dst=one) == BAD                                                   # out == in
    for axis in range(3):
        for v in (0, -1):
            assert call(size=tuple(v if a == axis else s for a, s in enumerate((5, 7, 11)))) == BAD, (axis, v)
        for v in (2, -1, 3, 100):
            assert call(r=tuple(v if a == axis else 1 for a in range(3))) == BAD, (axis, v)
            assert call(r=tuple(v if a == axis else 0 for a in range(3))) == BAD, (axis, v)
    assert call(r=(0, 0, 0)) == BAD
    for r in itertools.product((0, 1), repeat=3):
        if max(r):
            assert call(size=(2048, 1024, 1024), r=r) == UNS, r                    # 2^31 voxels
            assert call(size=(2 ** 31 - 1, 2, 1), r=r) == UNS, r
    assert call(size=(2048, 1024, 1024), r=(0, 0, 0)) == BAD                       # a bad argument is named first
    assert call(size=(2048, 1024, 1024), dst=one) == BAD


def test_python_wrapper_refuses_before_the_device_is_touched():
    from bodyct_dram_emph_subtype_amd import ops
    img = torch.zeros(2, 3, 4, dtype=torch.int16)
    for size in ((3, 3), (3, 3, 3, 3), (1, 1, 1), (5, 3, 3), (3, 2, 3), (0, 3, 3), (-3, 3, 3), 3, None, "333", (True, 3, 3)):
        with pytest.raises(ValueError, match="size"):
            ops.median_filter3d(img, size)
    for bad in (img[0], img[:, :, :0], torch.zeros(1, 2, 3, 4, dtype=torch.int16), img.numpy()):
        with pytest.raises(ValueError, match="image"):
            ops.median_filter3d(bad)
    for bad in (img.float(), img.to(torch.int32), img.to(torch.uint8), img.bool()):
        with pytest.raises(TypeError, match="int16"):
            ops.median_filter3d(bad)
    with pytest.raises(TypeError, match="out"):
        ops.median_filter3d(img, out=torch.zeros(2, 3, 4, dtype=torch.int32))
    with pytest.raises(TypeError, match="out"):
        ops.median_filter3d(img, out=np.zeros((2, 3, 4), dtype=np.int16))
    with pytest.raises(ValueError, match="out"):
        ops.median_filter3d(img, out=torch.zeros(2, 3, 5, dtype=torch.int16))
    with pytest.raises(ValueError, match="out"):
        ops.median_filter3d(img, out=torch.zeros(2, 4, 3, dtype=torch.int16).transpose(1, 2))
    big = torch.zeros(2, 2, 3, 4, dtype=torch.int16)
    for image, out in ((img, img), (big[0], big[1]), (img, img.view(-1).view(2, 3, 4))):
        with pytest.raises(ValueError, match="share storage"):
            ops.median_filter3d(image, out=out)
    for size in ((3, 3, 3), (1, 3, 3), [3, 1, 1], np.array([1, 1, 3])):           # all in order: only the device is missing
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.median_filter3d(img, size)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.median_filter3d(img.transpose(0, 2), out=torch.zeros(4, 3, 2, dtype=torch.int16))
    assert ops.median_size("f", [3, 1, 3]) == (3, 1, 3)


# ------------------------------------------------------------------------------------------------ the report
@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_report", os.path.join(GOLDEN, "make_golden_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_predict_case_refuses_before_any_device_work(gen):
    from bodyct_dram_emph_subtype_amd import processor
    scan = torch.zeros(gen.ORIGINAL, dtype=torch.int16)                          # CPU tensors: prepare_case would refuse them
    run = lambda **kw: processor.predict_case(gen.Module(), scan, scan.to(torch.uint8), gen.SPACING, gen.SHAPE, **kw)
    for names in (("regions",), ("densitometry", "regions"), ("cluster",), ("densitometry", "full_cle"), ("",)):
        for size in (None, (3, 3, 3)):
            with pytest.raises(ValueError, match="scan_filter_sections"):
                run(scan_filter=size, scan_filter_sections=names, densitometry=True)
    for size in ((1, 1, 1), (3, 3), (5, 3, 3), (3, 3, 2), 3, "median3x3x3"):
        with pytest.raises(ValueError, match="scan_filter"):
            run(scan_filter=size, clusters=True)
        with pytest.raises(ValueError, match="scan_filter"):
            run(scan_filter=size)                                                # also with every section off
    for kw in ({"dilate_iterations": 0}, {"crop_border": 0}, {"crop_border": -1.0}, {"dilate_iterations": 0, "crop_border": 5}):
        with pytest.raises(ValueError, match="dilate_iterations >= 1 and crop_border > 0"):
            run(scan_filter=(1, 3, 3), densitometry=True, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):                   # without the filter they are prepare_case's
            run(densitometry=True, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):                       # all in order: only the device is missing
        run(scan_filter=(3, 3, 3), scan_filter_sections=("clusters",), clusters=True, dilate_iterations=1, crop_border=0.5)
    assert processor.filter_name((3, 3, 3)) == "median3x3x3" and processor.filter_name([1, 3, 3]) == "median1x3x3"
    assert list(processor._SECTIONS) == ["regions", "densitometry", "core_peel", "clusters"]      # no fifth record


def _scan_side(processor, key):
    """the metric keys that are computed from the scan's HU values"""
    if processor._DENSITO_KEY.fullmatch(key) or processor._CLUSTER_KEY.fullmatch(key):
        return True
    return bool(processor._CORE_PEEL_KEY.fullmatch(key)) and key != "peel_mm" and \
        not key.startswith(("cle_", "pse_", "region_voxels"))


def _counts_laa(line):
    return "low-attenuation voxels" in line


def test_predict_case_filters_once_and_only_the_named_sections(gen, monkeypatch):
    from bodyct_dram_emph_subtype_amd import ops, processor, transforms
    size = (3, 3, 3)
    img, lab = gen.fixture()
    smooth = MR.median_filter(img, size)
    assert not np.array_equal(smooth, img)
    calls = []

    def median_stub(image, size=(3, 3, 3), out=None):
        calls.append((tuple(size), image.numpy().copy()))
        return torch.from_numpy(MR.median_filter(image.numpy(), tuple(size)))

    def run(fixture, **kw):
        with monkeypatch.context() as m:
            m.setattr(gen, "fixture", lambda: fixture)
            for owner, name, new in gen.stubs(processor, ops, transforms):
                m.setattr(owner, name, new)
            m.setattr(ops, "median_filter3d", median_stub)
            scan = torch.zeros(gen.ORIGINAL, dtype=torch.int16)
            return processor.predict_case(gen.Module(), scan, scan.to(torch.uint8), gen.SPACING, gen.SHAPE, uid="case",
                                          peel_mm=gen.PEEL_MM, **kw)

    def same_volumes(a, b):
        return torch.equal(a["full_cle"], b["full_cle"]) and torch.equal(a["full_pse"], b["full_pse"])

    differed = set()
    for bits in itertools.product((False, True), repeat=4):
        sw = dict(zip(gen.SWITCHES, bits))
        tag = "".join(str(int(b)) for b in bits)
        scan_sections = [s for s in gen.SWITCHES[1:] if sw[s]]
        raw = run((img, lab), **sw)
        assert not calls, tag
        assert run((img, lab), scan_filter=None, **sw)["metrics"] == raw["metrics"] and not calls, tag
        ref = run((smooth, lab), **sw)                       # the same combination, unfiltered, on the filtered fixture
        assert not calls and "scan_filter" not in raw["metrics"] and "scan_filter" not in ref["metrics"], tag
        got = run((img, lab), scan_filter=size, **sw)
        # filtered exactly once, and the case's own image, when a named section is on; never otherwise
        assert len(calls) == (1 if scan_sections else 0), tag
        if scan_sections:
            assert calls[0][0] == size and np.array_equal(calls[0][1], img), tag
            assert list(got["metrics"])[-1] == "scan_filter" and got["metrics"]["scan_filter"] == "median3x3x3", tag
            assert list(got["metrics"])[:-1] == list(raw["metrics"]), tag            # the same keys in the same order
        else:
            assert got["metrics"] == raw["metrics"] and list(got["metrics"]) == list(raw["metrics"]), tag
        calls.clear()
        for k, v in got["metrics"].items():
            if k == "scan_filter":
                continue
            want = ref if _scan_side(processor, k) else raw
            assert v == want["metrics"][k], (tag, k)
            if _scan_side(processor, k) and v != raw["metrics"][k]:
                differed.add(k)
        assert [e for e in got["error_messages"] if not _counts_laa(e)] == \
            [e for e in raw["error_messages"] if not _counts_laa(e)], tag
        assert [e for e in got["error_messages"] if _counts_laa(e)] == [e for e in ref["error_messages"] if _counts_laa(e)], tag
        assert same_volumes(got, raw) and got["entity"] == raw["entity"] == "case", tag
        json.dumps({"metrics": got["metrics"], "error_messages": got["error_messages"]})

        # only the clusters named: densitometry and core / peel read the raw image
        part = run((img, lab), scan_filter=size, scan_filter_sections=("clusters",), **sw)
        assert len(calls) == (1 if sw["clusters"] else 0), tag
        calls.clear()
        assert ("scan_filter" in part["metrics"]) == sw["clusters"], tag
        for k, v in part["metrics"].items():
            if k == "scan_filter":
                continue
            want = ref if processor._CLUSTER_KEY.fullmatch(k) else raw
            assert v == want["metrics"][k], (tag, k)
        # no section named: nothing is filtered, nothing is added
        none = run((img, lab), scan_filter=size, scan_filter_sections=(), **sw)
        assert not calls and none["metrics"] == raw["metrics"] and none["error_messages"] == raw["error_messages"], tag
    # the comparison above has teeth: the filter moves numbers of all three scan-side sections on this fixture
    assert {"laa950_fraction_per_lung", "laa950_clusters_per_lung", "mean_lung_density_per_lung_peel"} <= differed, differed


def test_in_plane_filter_is_named_in_the_report(gen, monkeypatch):
    from bodyct_dram_emph_subtype_amd import ops, processor, transforms
    for owner, name, new in gen.stubs(processor, ops, transforms):
        monkeypatch.setattr(owner, name, new)
    seen = []
    monkeypatch.setattr(ops, "median_filter3d", lambda image, size=(3, 3, 3), out=None: (
        seen.append(tuple(size)), torch.from_numpy(MR.median_filter(image.numpy(), tuple(size))))[1])
    scan = torch.zeros(gen.ORIGINAL, dtype=torch.int16)
    entry = processor.predict_case(gen.Module(), scan, scan.to(torch.uint8), gen.SPACING, gen.SHAPE, densitometry=True,
                                   scan_filter=[1, 3, 3], dilate_iterations=1, crop_border=0.1)
    assert seen == [(1, 3, 3)] and entry["metrics"]["scan_filter"] == "median1x3x3"
    want = processor.densitometry_metrics(processor.densitometry(
        torch.from_numpy(MR.median_filter(gen.fixture()[0], (1, 3, 3))), torch.from_numpy(gen.fixture()[1]), gen.SPACING))
    assert {k: entry["metrics"][k] for k in want} == want
    assert processor.filtered_image(torch.from_numpy(gen.fixture()[0]), (1, 3, 3)).dtype == torch.int16 and len(seen) == 2


# ------------------------------------------------------------------------------------------------ filter, then crop
@pytest.mark.parametrize("size", [(3, 3, 3), (1, 3, 3)])
def test_filtered_crop_equals_crop_of_filtered_scan_at_lung_voxels(size):
    """prepare_case's defaults (two dilations, 5 mm of padding): every window centred on a lung voxel holds the scan's own
    values, and the crop is clipped only where the scan ends"""
    cases = CP.fixture_cases()
    shape = (20, 44, 52)
    lobes = torch.zeros(shape, dtype=torch.uint8)                # a lung along three faces of the scan, and one inside
    lobes[0:6, 0:20, 40:52] = 2
    lobes[9:14, 25:40, 5:30] = 1
    cases["faces"] = (CP.synth_scan(shape, 9), lobes, (2.5, 0.7, 0.7), 5)
    touched_edge = False
    for name in ("blobs_u8", "corners", "single_voxel", "faces"):
        scan, lobes, spacing, border = cases[name]
        case = CP.prepare_case_ref(scan, lobes, spacing)                     # dilate_iterations=2, crop_border=5
        lung = case["lung_mask"].numpy()
        idx = tuple(slice(int(a), int(b)) for a, b in case["crop_slice"].tolist())
        whole = MR.median_filter(scan.numpy(), size)[idx]
        crop = MR.median_filter(case["image"].numpy(), size)
        assert lung.any() and np.array_equal(crop[lung], whole[lung]), name
        full_lung = (lobes > 0).numpy()
        touched_edge |= bool(full_lung[0].any() or full_lung[:, 0].any() or full_lung[:, :, -1].any())
        # and it is a property of the preparation, not of the data: without dilation the fill value leaks in
        bare = CP.prepare_case_ref(scan, lobes, spacing, dilate_iterations=0)
        if name != "single_voxel":
            assert not np.array_equal(MR.median_filter(bare["image"].numpy(), size)[lung], whole[lung]), name
    assert touched_edge
