"""Host side of the class-activation maps (no GPU): the library exports the new entry points with the header's
prototypes, the binding parsed from the header carries them, and every argument check of activation_map /
target_activations that precedes the first launch raises without a device."""
import ctypes
import os
import subprocess

import pytest
import torch

CAM_ENTRY_POINTS = ("dram_cam_nblk", "dram_cam_point", "dram_cam_sum", "dram_cam_combine", "dram_cam_point_bf16",
                    "dram_cam_sum_bf16", "dram_cam_combine_bf16")


def test_cam_entry_points_are_exported_with_the_headers_prototypes():
    from ctypes import c_int as I, c_longlong as LL, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _build, _lib
    head = [P, P, P, P, P, P, I, I, I, P, I, I, I, I, I, I]      # x w bias gdense gpool lungs Dl Hl Wl out B D H W NO sigmoid
    expect = {"dram_cam_nblk": [LL], "dram_cam_point": head + [I, I, P], "dram_cam_sum": head + [P],
              "dram_cam_combine": [P, P, P, P, I, I, I, I, I, I, P]}
    for name in CAM_ENTRY_POINTS:
        res, args = _lib.SIGNATURES[name]
        assert res is I and list(args) == expect[name.replace("_bf16", "")], name
    assert (_lib.DRAM_CAM_GRADCAM, _lib.DRAM_CAM_HIRESCAM, _lib.DRAM_CAM_LAYERCAM) == (0, 1, 2)
    path = _build.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(CAM_ENTRY_POINTS) <= exported, set(CAM_ENTRY_POINTS) - exported
    lib = _lib.load()                       # dlopen works without a GPU; only host-side entry points are called
    assert lib.dram_cam_nblk.argtypes == [ctypes.c_longlong]
    assert [lib.dram_cam_nblk(v) for v in (1, 2048, 2049, 16 * 32 * 32, 64 * 128 * 128, 1 << 26)] == [1, 1, 2, 8, 512, 512]
    # the gradcam sum pass's partials are folded by ONE block of dram_fold_partials: no ticket word, no memset
    assert lib.dram_fold_partials_stages(lib.dram_cam_nblk(1 << 26)) == 1
    # rejected before any launch: NULL operands, an unknown method, more than 2^31 - 1 elements
    assert lib.dram_cam_point(None, None, None, None, None, None, 0, 0, 0, None, 1, 1, 1, 1, 2, 1, 1, 1, None) == _lib.DRAM_ERR_BAD_ARG
    one = ctypes.c_void_p(16)               # (never dereferenced: the argument checks come first)
    assert lib.dram_cam_point(one, one, one, None, one, None, 0, 0, 0, one, 1, 1, 1, 1, 2, 1, _lib.DRAM_CAM_GRADCAM, 1, None) \
        == _lib.DRAM_ERR_BAD_ARG
    for fn, tail in ((lib.dram_cam_point, (2, 1, _lib.DRAM_CAM_HIRESCAM, 1, None)), (lib.dram_cam_sum, (2, 1, None))):
        assert fn(one, one, one, None, one, None, 0, 0, 0, one, 2, 256, 512, 512, *tail) == _lib.DRAM_ERR_UNSUPPORTED
    assert lib.dram_cam_combine(one, one, one, one, 2, 256, 512, 512, 2, 1, None) == _lib.DRAM_ERR_UNSUPPORTED


def test_the_documents_name_the_cam_entry_points():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read() + open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("dram_cam_point", "dram_cam_sum", "dram_cam_combine", "activation_map", "target_activations"):
        assert name in text, name


def test_activation_map_argument_checks_raise_without_a_device():
    from bodyct_dram_emph_subtype_amd import med3d, ops
    torch.manual_seed(0)
    m, c = med3d.resnet18segreg().eval(), med3d.resnet18segcls().eval()
    x = torch.zeros(1, 1, 16, 32, 32)
    one = torch.ones(1)
    for mod, kw in [(m, dict(score=(0, 0), method="scorecam")),
                    (m, dict(score=(0, 0), out_grads=(one, None))),
                    (m, dict()),
                    (m, dict(out_grads=(None, None), dense_grads=(None, None))),
                    (m, dict(out_grads=(one,))),
                    (m, dict(score=(0, 1))),
                    (m, dict(score=(2, 0))),
                    (c, dict(score=(0, 6))),
                    (c, dict(score=(1, None))),
                    (c, dict(score=(0, -1))),
                    (m, dict(out_grads=(torch.ones(2), None))),
                    (c, dict(out_grads=(torch.ones(1, 3), None))),
                    (m, dict(dense_grads=(torch.ones(1, 1, 8, 16, 15), None))),
                    (m, dict(score=(0, 0), upsample_mask=torch.ones(2, 16, 32, 32)))]:
        with pytest.raises(ValueError):
            mod.activation_map(x, **kw)
    # well-formed arguments on the CPU: refused as forward refuses them
    for mod, kw in [(m, dict(score=(0, None))), (c, dict(score=(1, 2))), (m, dict(out_grads=(one, None)))]:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod.activation_map(x, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.target_activations(x)
    with pytest.raises(ValueError):
        ops.cam(torch.zeros(1, 2, 2, 2, 32), torch.zeros(2, 32), torch.zeros(2), None, torch.zeros(1, 2), None, True, "scorecam")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cam(torch.zeros(1, 2, 2, 2, 32), torch.zeros(2, 32), torch.zeros(2), None, torch.zeros(1, 2), None, True)
    assert all(p.grad is None for p in m.parameters())
