"""CPU: the scan + lobes -> prepared-case step (transforms.prepare_case, processor.predict_case) -- the torch
restatement the GPU tests compare against (tests/case_prep_ref.py) is held to the fixture recorded from the reference's
SubtypingInference.get_data and to scipy's iterated dilation; the C ABI declares and binds the new entry points; the
public functions refuse CPU tensors like the rest of the package."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import case_prep_ref as ref


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "case_prep.npz"))


def test_fixture_holds_the_cases_the_tests_rebuild(golden):
    """The synthetic inputs are rebuilt from seeds; the fixture's copies must be those very arrays, and carry what the
    cases are there for: labels 1-5, corner voxels, a single voxel, int16 lobes, the edge HU values inside the lung."""
    cases = ref.fixture_cases()
    assert {k.split(":")[0] for k in golden.files} == set(cases)
    for name, (scan, lobes, spacing, border) in cases.items():
        assert np.array_equal(golden[f"{name}:scan"], scan.numpy()) and golden[f"{name}:scan"].dtype == np.int16
        assert np.array_equal(golden[f"{name}:lobes"], lobes.numpy()) and golden[f"{name}:lobes"].dtype == lobes.numpy().dtype
        assert tuple(golden[f"{name}:spacing"]) == tuple(spacing) and int(golden[f"{name}:border"]) == border
    scan, lobes, _, _ = cases["blobs_u8"]
    assert set(lobes.unique().tolist()) == {0, 1, 2, 3, 4, 5}
    for hu in ref.SPECIAL_HU:
        assert bool(((scan == hu) & (lobes > 0)).any())
    lobes = cases["corners"][1]
    assert lobes[0, 0, 0] > 0 and lobes[-1, -1, -1] > 0
    assert int((cases["single_voxel"][1] > 0).sum()) == 1
    assert cases["lobes_i16"][1].dtype == torch.int16 and int(cases["lobes_i16"][1].max()) > 255
    assert golden["blobs_u8:image"].dtype == np.int16 and golden["blobs_u8:lung_mask"].dtype == np.bool_
    assert golden["blobs_u8:crop_slice"].shape == (3, 2) and golden["blobs_u8:original_size"].tolist() == [20, 44, 52]
    # the strict `<` of the ess threshold is visible in the recorded data: -910 inside the lung is not ess, -911 is
    z0, y0, x0 = golden["blobs_u8:crop_slice"][:, 0]
    assert not golden["blobs_u8:ess_mask"][6 - z0, 12 - y0, 8 - x0] and golden["blobs_u8:ess_mask"][6 - z0, 12 - y0, 9 - x0]


@pytest.mark.parametrize("name", sorted(ref.fixture_cases()))
def test_restatement_equals_the_reference_fixture(golden, name):
    scan, lobes, spacing, border = ref.fixture_cases()[name]
    out = ref.prepare_case_ref(scan, lobes, spacing, crop_border=border)
    for k in ref.KEYS:
        want = golden[f"{name}:{k}"]
        assert out[k].numpy().dtype == want.dtype, (k, out[k].dtype, want.dtype)
        assert np.array_equal(out[k].numpy(), want), k


@pytest.mark.parametrize("iterations", [0, 1, 2, 3])
def test_restatement_equals_scipy_iterated_dilation(iterations):
    ndimage = pytest.importorskip("scipy.ndimage")
    g = torch.Generator().manual_seed(10 + iterations)
    for shape, p in (((7, 9, 11), 0.02), ((12, 6, 17), 0.3), ((5, 9, 130), 0.002)):
        lung = torch.rand(shape, generator=g) < p
        lung[0, 0, 0] = lung[-1, -1, -1] = True           # dilation clipped at the volume's corners
        got = ref.dilate(lung, iterations).numpy()
        if iterations == 0:
            want = lung.numpy()                          # scipy reads iterations=0 as "until nothing changes"
        else:
            want = ndimage.binary_dilation(lung.numpy(), ndimage.generate_binary_structure(3, 3), iterations=iterations)
        assert np.array_equal(got, want), (shape, p)


def test_restatement_errors():
    with pytest.raises(IndexError):
        ref.prepare_case_ref(torch.zeros(3, 4, 5, dtype=torch.int16), torch.zeros(3, 4, 5, dtype=torch.uint8), (1, 1, 1))


def test_header_declares_and_lib_binds_the_case_entry_points():
    from ctypes import c_int, c_longlong, c_void_p
    from bodyct_dram_emph_subtype_amd import _lib
    header = open(os.path.join(ROOT, "include", "dram_hip.h")).read()
    P, I = c_void_p, c_int
    expect = {"dram_lung_bbox_nblk": (I, [c_longlong]),
              "dram_lung_bbox": (I, [P, I, P, P, I, I, I, P]),
              "dram_case_prepare": (I, [P, P, I, P, P, P, P] + [I] * 12 + [P])}
    for name, (res, args) in expect.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res and list(got_args) == args, (name, got_res, got_args)
    lib = _lib.load()                                   # dlopen needs no GPU; the sizing export launches nothing
    for name in expect:
        assert getattr(lib, name).argtypes == expect[name][1]
    assert lib.dram_lung_bbox_nblk(1) == 1 and lib.dram_lung_bbox_nblk(16385) == 2
    assert lib.dram_lung_bbox_nblk(300 * 512 * 512) == 1024


def test_prepare_case_has_no_cpu_path():
    from bodyct_dram_emph_subtype_amd import transforms
    scan, lobes, spacing, _ = ref.fixture_cases()["single_voxel"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        transforms.prepare_case(scan, lobes, spacing)


def test_predict_case_has_no_cpu_path():
    from bodyct_dram_emph_subtype_amd import processor
    scan, lobes, spacing, _ = ref.fixture_cases()["single_voxel"]

    class Module:
        def predict_step(self, batch, batch_idx):
            raise AssertionError("predict_step reached with CPU tensors")

    with pytest.raises(RuntimeError, match="no CPU path"):
        processor.predict_case(Module(), scan, lobes, spacing, target_size=(16, 32, 32))
