"""Host side of the validation / test activation-map panels (no GPU): the fp64 yardstick of tests/heat_ref.py against
what the reference's own _draw_predictions recorded (tests/golden/heat.npz) and against the ATen fp32 composition,
the slice rule, the colour table, the sheet assembly, and the library's argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import data_path_ref as R
import heat_ref as HR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heat.npz")
FIXTURES = (("cls", "classsum"), ("reg", "plain"))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def models():
    from bodyct_dram_emph_subtype_amd import models as m
    return m


def _refs(golden, kind, mode):
    lung = torch.from_numpy(golden[f"{kind}:lungs"])
    return [HR.heat64(torch.from_numpy(golden[f"{kind}:dense{i}"]), lung, mode) for i in (0, 1)]


@pytest.mark.parametrize("kind,mode", FIXTURES)
def test_fp64_yardstick_holds_the_recorded_reference_bytes(golden, kind, mode):
    """every uint8 voxel the reference fed its drawing function lies in u8_range of the fp64 value (equal bytes where
    the range is one byte), and the bound leaves at most 0.5 % of the voxels open"""
    for ref, row in zip(_refs(golden, kind, mode), (2, 3)):
        outside, share, ok = HR.check_u8(golden[f"{kind}:volumes"][:, row], ref)
        print(f"[golden {kind} row {row}] outside {outside}, open {100 * share:.3f} %")
        assert ok, (outside, share)


@pytest.mark.parametrize("kind,mode", FIXTURES)
def test_golden_mask_rows_are_the_inputs(golden, kind, mode):
    vol = golden[f"{kind}:volumes"]
    assert (vol[:, 1] == golden[f"{kind}:lungs"] * 255).all() and (vol[:, 4] == golden[f"{kind}:ems"] * 255).all()
    s = golden[f"{kind}:scans"]
    for b in range(s.shape[0]):          # utils.windowing(scan, from_span=None) in float32
        q = (s[b] - s[b].min()) / float(s[b].max() - s[b].min()) * 255
        assert q.dtype == np.float32 and (vol[b, 0] == q.astype(np.uint8)).all()


@pytest.mark.parametrize("mode,shape", [("classsum", (2, 6, 4, 6, 8)), ("classsum", (2, 3, 8, 16, 16)),
                                        ("plain", (2, 1, 8, 16, 16))])
def test_aten_fp32_stays_within_half_the_bound(mode, shape):
    g = R.gen(5)
    dense = torch.randn(shape, generator=g) if mode == "classsum" else 3.0 * torch.rand(shape, generator=g) - 1.0
    lung = torch.rand((shape[0],) + tuple(2 * n for n in shape[2:]), generator=g) > 0.3
    ref = HR.heat64(dense, lung, mode)
    v, u8 = HR.aten_heat(dense, lung, mode)
    r = R.ratio(torch.from_numpy(v), ref)
    outside, share, ok = HR.check_u8(u8, ref)
    print(f"[aten/bound] {mode} {shape}: {r:.3f}; u8 outside {outside}, open {100 * share:.3f} %")
    assert r <= 0.5 and ok


def test_yardstick_edges():
    """the far tap is clamped, output 0 copies source 0, an all-negative class sum is all zeros without a NaN"""
    i0, i1, w0, w1 = HR.taps(3)
    assert i0.tolist() == [0, 0, 0, 1, 1, 2] and i1.tolist() == [1, 1, 1, 2, 2, 2]
    assert w1.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25] and (w0 + w1 == 1).all()
    x = torch.randn(1, 1, 2, 2, 4, dtype=torch.float64)
    want = torch.nn.functional.interpolate(x, scale_factor=2, mode="trilinear")
    assert torch.allclose(HR.up2(x), want, rtol=0, atol=1e-14)
    ref = HR.heat64(-torch.rand(1, 3, 2, 2, 4), torch.ones(1, 4, 4, 8, dtype=torch.bool), "classsum")
    assert (ref.val == 0).all() and torch.isfinite(ref.bound).all()


def test_panel_slices(models):
    ps = models.panel_slices
    # mid-volume lung [10, 30) of 40: flipped frame 10..30, stride 4 -> flipped ids 10, 14, 18, 22, 26
    assert ps(10, 30, 40) == [29, 25, 21, 17, 13]
    # the order is the flipped frame's: descending original indices, starting at the lung's last slice
    assert ps(0, 8, 8) == [7, 6, 5, 4, 3]
    assert ps(3, 16, 16, num_slices=3) == [15, 11, 7]
    # lung thinner than num_slices: the whole volume, (D - 1) // num apart
    assert ps(20, 23, 40) == [39, 32, 25, 18, 11]
    # ... and a volume too short for that raises like range(s, e, 0)
    with pytest.raises(ValueError):
        ps(1, 3, 5)
    assert ps(1, 3, 6) == [5, 4, 3, 2, 1]
    # empty lung (dram_lung_bbox gives an all-zero box)
    assert ps(0, 0, 40) is None


def test_panel_slices_match_the_flipped_reference_rule(models):
    """against a direct restatement on a flipped mask: find the extent, stride, take num, flip back"""
    rng = np.random.default_rng(0)
    for _ in range(50):
        D = int(rng.integers(6, 40))
        z0 = int(rng.integers(0, D))
        z1 = int(rng.integers(z0 + 1, D + 1))
        m = np.zeros(D, dtype=bool)
        m[z0:z1] = True
        f = np.flatnonzero(m[::-1])
        s, e = int(f[0]), int(f[-1]) + 1
        st = (e - s) // 5
        if st == 0:
            s, e = 0, D - 1
            st = (e - s) // 5
        assert models.panel_slices(z0, z1, D) == [D - 1 - k for k in list(range(s, e, st))[:5]]


def test_jet_table_is_pinned(models):
    jet = models.JET
    assert jet.shape == (256, 3) and jet.dtype == np.uint8
    assert jet[0].tolist() == [0, 0, 128] and jet[128].tolist() == [130, 255, 126] and jet[255].tolist() == [128, 0, 0]
    assert jet[:, 1].argmax() == 96 and (jet[96:160, 1] == 255).all()      # green plateau around the middle


def test_sheet_assembly(models):
    rng = np.random.default_rng(1)
    panels = rng.integers(0, 256, size=(5, 3, 4, 8), dtype=np.uint8)
    sheet = models.sheet_from_panels(panels)
    assert sheet.shape == (5 * 4, 3 * 8, 3) and sheet.dtype == np.uint8
    for r in range(5):
        for k in range(3):
            grey = panels[0, k].astype(np.int64)[..., None]
            want = np.repeat(grey, 3, -1) if r == 0 else (models.JET[panels[r, k]].astype(np.int64) + grey + 1) >> 1
            assert (sheet[4 * r:4 * r + 4, 8 * k:8 * k + 8] == want).all(), (r, k)
    with pytest.raises(ValueError):
        models.sheet_from_panels(panels.astype(np.float32))


def test_entry_points_and_argument_checks():
    """the header's prototypes, the block count, and every rejection of the C entry points that precedes a launch"""
    from ctypes import c_int as I, c_longlong as LL, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _lib
    assert _lib.SIGNATURES["dram_heat_nblk"] == (I, [LL])
    assert _lib.SIGNATURES["dram_heat_peak"] == (I, [P, LL, LL, I, P, I, I, I, I, I, I, I, P])
    assert _lib.SIGNATURES["dram_heat_volume"] == (I, [P, LL, LL, I, P, P, P, I, P, P, I, I, I, I, I, I, I, I, P])
    assert (_lib.DRAM_HEAT_CLASSSUM, _lib.DRAM_HEAT_PLAIN) == (0, 1)
    lib = _lib.load()                        # dlopen works without a GPU; only argument checks run
    assert [lib.dram_heat_nblk(v) for v in (1, 512, 2048, 2049, 32 * 64 * 64, 1 << 30)] == [1, 1, 1, 2, 64, 512]
    one, BAD, UNS = ctypes.c_void_p(64), _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    CS, PL = _lib.DRAM_HEAT_CLASSSUM, _lib.DRAM_HEAT_PLAIN

    def vol(mode=CS, C=6, zsel=None, nz=0, grid=(4, 4, 4), out=(8, 8, 8), dense=one, lung=one, peak=one, f32=one, u8=one):
        return lib.dram_heat_volume(dense, 1024, 64, C, lung, peak, zsel, nz, f32, u8, mode, 1, *grid, *out, None)

    assert vol(out=(8, 8, 9)) == BAD and vol(out=(4, 4, 4)) == BAD          # not exactly twice the dense grid
    assert vol(C=1) == BAD and vol(peak=None) == BAD                        # classsum: >= 2 channels, and the peak
    assert vol(mode=PL, C=2) == BAD and vol(mode=7) == BAD
    assert vol(zsel=one, nz=0) == BAD and vol(zsel=one, nz=-3) == BAD
    assert vol(dense=None) == BAD and vol(lung=None) == BAD and vol(f32=None, u8=None) == BAD
    assert vol(grid=(4, 4, 6), out=(8, 8, 12)) == BAD                       # w % 4
    assert vol(grid=(512, 1024, 512), out=(1024, 2048, 1024)) == UNS        # D H W = 2^31
    assert lib.dram_heat_peak(one, 1024, 64, 1, one, 1, 4, 4, 4, 8, 8, 8, None) == BAD
    assert lib.dram_heat_peak(one, 1024, 64, 6, one, 1, 4, 4, 4, 8, 8, 7, None) == BAD
    assert lib.dram_heat_peak(one, 1024, 64, 6, one, 1, 512, 1024, 512, 1024, 2048, 1024, None) == UNS


def test_wrappers_reject_host_tensors_before_any_launch():
    from bodyct_dram_emph_subtype_amd import ops
    dense, lung = torch.zeros(1, 6, 4, 4, 4), torch.ones(1, 8, 8, 8, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.heat_peak(dense)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.heat_volume(dense, lung, "classsum", torch.zeros(1))
    with pytest.raises(ValueError):
        ops.heat_volume(dense, lung, "sum")
