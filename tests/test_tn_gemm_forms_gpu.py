"""GPU: the streaming and the persistent form of the fp32 TN batched GEMM (Winograd-domain and 1x1x1 weight gradients)
against the one-tile kernels they replace -- bit for bit -- and against fp64.

DRAM_NN_STREAM, the switch of the streaming GEMMs, as wino_gemm.hip's run_tn reads it: 0 = the one-tile kernels (wino_gemm_tn_kernel, wino_gemm_tn64_kernel), 2 = the
new forms wherever they are legal, on 8 workgroups: a case of a few hundred (point, split) chains or items then runs
several of them per workgroup, wraps the stage ring and ends on tails shorter than the ring.  (The 64 x 64 launches of
the pipeline keep wino_gemm_tn64_kernel under every value: a streaming form in its order measured no faster.)
The bar against fp64 is the one of test_conv3d_winograd_path (test_kernels_gpu.py): rel. L2 < 2 tol, tol = 3e-5 for F(4,3)^3 and 1e-5 otherwise.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


def to_ndhwc(t):  # NCDHW cpu -> NDHWC gpu
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


TN_CASES = [
    # B, D, H, W, Cin, Cout, dil   (the smallest shapes that reach each path; F(4,3)^3 figures)
    (2, 32, 32, 32, 64, 64, 1),         # 64 x 64 sums (k halves): stays on the 64 x 64 kernel whatever the switch says
    (2, 32, 32, 32, 128, 64, 1),        # 64 x 128 streaming form: 8 steps of 32 rows = 16 stages a chain
    (1, 8, 16, 16, 256, 256, 4),        # 256 x 256 tiles, Tpad 256, 2 splits of 4 k steps: the short-K regime of the workload
    (1, 16, 16, 16, 128, 256, 2),       # 128-column tiles split over t
    (2, 4, 8, 8, 192, 320, 1),          # ragged N: the clamped DMA column
    (1, 5, 7, 6, 64, 256, 1),           # a chain shorter than the ring
]

_REF = {}


def wgrad_ref(case, k):
    """fp64 weight gradient of F.conv3d (autograd), computed once per case"""
    if (case, k) not in _REF:
        B, D, H, W, Cin, Cout, dil = case
        x = rnd(B, Cin, D, H, W, seed=1).double()
        w = (rnd(Cout, Cin, k, k, k, seed=2) * 0.1).double().requires_grad_(True)
        gy = rnd(B, Cout, D, H, W, seed=4).double()
        pad = dil * (k - 1) // 2
        _REF[(case, k)] = torch.autograd.grad(F.conv3d(x, w, None, 1, pad, dil), w, gy)[0]
    return _REF[(case, k)]


@pytest.mark.parametrize("case", TN_CASES, ids=[str(c) for c in TN_CASES])
def test_winograd_weight_gradient_forms_equal_one_tile_kernels(ops, monkeypatch, case):
    """conv3d_bwd_weight on the Winograd pipeline, tilings F(2,3)^3 and F(4,3)^3: the new TN forms give the bits of the
    one-tile kernels, from the input itself and from the forward's cached image, and both agree with fp64."""
    monkeypatch.setenv("DRAM_CONV_ALGO", "2")
    B, D, H, W, Cin, Cout, dil = case
    x = to_ndhwc(rnd(B, Cin, D, H, W, seed=1))
    gy = to_ndhwc(rnd(B, Cout, D, H, W, seed=4))
    w = (rnd(Cout, Cin, 3, 3, 3, seed=2) * 0.1).to(DEV)
    g = ops.ConvGeom(B, D, H, W, Cin, Cout, 3, 1, dil, dil)
    assert ops.conv_use_wino(g)
    ref = wgrad_ref(case, 3)
    for tiling in ("2,2,2", "4,4,4"):
        monkeypatch.setenv("DRAM_WINO_TILING", tiling)
        tol = 3e-5 if tiling == "4,4,4" else 1e-5
        wf, _ = ops.pack_conv_weight(w, True, False, g)
        _, _, v = ops.conv3d_fwd_keep(x, wf, None, g, False, True)
        assert v is not None
        res = {}
        for mode in ("0", "2"):
            monkeypatch.setenv("DRAM_NN_STREAM", mode)
            res[mode] = (ops.conv3d_bwd_weight(x, gy, g), ops.conv3d_bwd_weight(x, gy, g, v_cache=v))
        monkeypatch.delenv("DRAM_NN_STREAM")
        dflt = ops.conv3d_bwd_weight(x, gy, g)                 # ... and whatever the default picks at this size
        assert torch.equal(res["0"][0], res["2"][0]), tiling
        assert torch.equal(res["0"][1], res["2"][1]), tiling
        assert torch.equal(res["0"][0], res["0"][1]) and torch.equal(res["0"][0], dflt), tiling
        for mode in ("0", "2"):
            err = rel_l2(res[mode][0].cpu().double(), ref)
            print(f"{case} F({tiling}) DRAM_NN_STREAM={mode}: rel. L2 vs fp64 {err:.3e} (bar {2 * tol:.0e})")
            assert err < 2 * tol, (tiling, mode, err)


C1_CASE = (1, 8, 16, 16, 128, 192, 1)       # 1x1x1: one point, 16 splits of 4 k steps, 64 x 128 tiles


def test_conv1x1_weight_gradient_forms_equal_one_tile_kernel(ops, monkeypatch):
    """The 1x1x1 weight gradient goes through the same launcher with one point: by default it stays on the one-tile
    kernel, DRAM_NN_STREAM=2 sends it through the persistent form -- same bits, and fp64 within 2e-5."""
    monkeypatch.delenv("DRAM_CONV_ALGO", raising=False)
    B, D, H, W, Cin, Cout, _ = C1_CASE
    x = to_ndhwc(rnd(B, Cin, D, H, W, seed=1))
    gy = to_ndhwc(rnd(B, Cout, D, H, W, seed=4))
    g = ops.ConvGeom(B, D, H, W, Cin, Cout, 1, 1, 0, 1)
    assert ops.conv_algo(g) == 3
    res = {}
    for mode in ("0", "2"):
        monkeypatch.setenv("DRAM_NN_STREAM", mode)
        res[mode] = ops.conv3d_bwd_weight(x, gy, g)
    monkeypatch.delenv("DRAM_NN_STREAM")
    assert torch.equal(res["0"], res["2"]) and torch.equal(res["0"], ops.conv3d_bwd_weight(x, gy, g))
    ref = wgrad_ref(C1_CASE, 1)
    for mode in ("0", "2"):
        err = rel_l2(res[mode].cpu().double(), ref)
        print(f"1x1x1 {C1_CASE} DRAM_NN_STREAM={mode}: rel. L2 vs fp64 {err:.3e} (bar 2e-05)")
        assert err < 2e-5, (mode, err)


def test_resnet18_train_step_gradients_do_not_depend_on_the_tn_form(monkeypatch):
    """One small ResNet-18 train step (1 x 1 x 16 x 32 x 32, the shape of test_survey_anchor): every parameter gradient
    with the one-tile TN kernels (DRAM_NN_STREAM=0, which also puts the NN side on its tiled kernels: bit-identical,
    test_winograd_streaming_gemm_equals_tiled_gemm) and with the forms run_tn picks by default is the same bits -- the
    dispatch sends real layer shapes the right way."""
    from bodyct_dram_emph_subtype_amd import med3d

    def grads():
        torch.manual_seed(0)
        m = med3d.resnet18segreg()
        gen = torch.Generator().manual_seed(1)
        x = torch.randn(1, 1, 16, 32, 32, generator=gen)
        lungs = (torch.rand(1, 1, 16, 32, 32, generator=gen) > 0.3).float()
        m = m.to(DEV).train()
        dense, outs = m(x.to(DEV), lungs.to(DEV))
        (outs[0].sum() + 2.0 * outs[1].sum() + 0.1 * (dense[0] * dense[1]).mean()).backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}

    monkeypatch.setenv("DRAM_NN_STREAM", "0")
    g0 = grads()
    monkeypatch.delenv("DRAM_NN_STREAM")
    g1 = grads()
    assert g0.keys() == g1.keys() and len(g0) > 20
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
