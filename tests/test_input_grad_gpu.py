"""GPU: gradients with respect to the input volume, and backward through eval-mode BatchNorm.

  a. kernel: ops.stem_bwd_data vs torch's float64 transposed convolution on the CPU, relative L2 <= 5e-6 (the bar
     test_stem holds the stem weight gradient to: the same fp32 MFMA arithmetic over far shorter sums; torch's own fp32
     transposed convolution sits at 3.7e-7 - 4.7e-7 on these inputs), fp32 and bf16 dy, two calls bit-identical.
  b. network, fp32: x.grad and every parameter gradient vs the float64 oracle on the HIP forward's own decisions, train
     mode and eval mode (seeded running statistics); bar = test_network_gpu.grad_tol, computed here.
  c. a training step is unchanged: same parameter gradients bit for bit with and without x.requires_grad, no
     stem-data-gradient launch in a plain step, no weight-gradient launch in an attribution call.
  d. model.input_gradient == the requires_grad_ + backward route, bit for bit; no .grad touched.
  e. bf16 storage: x.grad vs the fp64 oracle pinned to the bf16 forward's decisions, bar max(1e-1, 2 x the reference
     autocast arithmetic's own distance from its fp32 self).
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_loss, head_weights, make_inputs, rel_l2
from oracle import med3d_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
STEM_DGRAD_TOL = 5e-6
GRAD_TOL = 1e-4

# timeline families that only weight-gradient kernels record under (include/dram_hip.h)
WGRAD_FAMILIES = ("wino_gemm_tn", "wino_wgrad_out", "conv_wgrad_w2d", "conv_wgrad", "wgrad_bf16")
STEM_WGRAD_VARIANTS, STEM_DGRAD_VARIANTS = (1, 3), (4, 5)


def grad_tol(e_cpu32):
    """The rule of tests/test_network_gpu.py::grad_tol."""
    return min(max(GRAD_TOL, 3.0 * e_cpu32), 5e-4)


def is_noise_param(name):
    """conv bias directly followed by a BATCH-statistics BatchNorm: analytically zero gradient (train mode only)."""
    return name.endswith(".0.bias") and name.startswith("us")


def build(factory, seed, stats_seed=None):
    from bodyct_dram_emph_subtype_amd import med3d
    torch.manual_seed(seed)
    kw = dict(n_classes=[6, 3]) if factory.endswith("cls") else {}
    m = getattr(med3d, factory)(**kw)
    if stats_seed is not None:          # non-trivial running statistics: mean ~ 0.1 N(0,1), var in [0.5, 1.5]
        g = torch.Generator().manual_seed(stats_seed)
        for name, b in m.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return m


def pinned_decisions(out):
    from bodyct_dram_emph_subtype_amd.engine import forward_decisions
    return {k: v.cpu() for k, v in forward_decisions(out.grad_fn.saved_state).items()}


# ------------------------------------------------------------------------------------------------ a. kernel
# (2,64,128,128): 1 024 tiles, so the persistent workgroups (at most 512) walk more than one tile
@pytest.mark.parametrize("shape", [(1, 8, 8, 8), (2, 9, 14, 11), (2, 16, 24, 40), (1, 64, 128, 128), (2, 64, 128, 128),
                                   (1, 1, 1, 1), (1, 5, 37, 18)], ids=str)
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
def test_stem_bwd_data_vs_float64(dram, shape, dt):
    ops = dram.ops
    dram.load_library()
    g = torch.Generator().manual_seed(5)
    B, D, H, W = shape
    w = 0.1 * torch.randn(64, 1, 7, 7, 7, generator=g)
    x = torch.randn(B, 1, D, H, W, generator=g, dtype=torch.float64).requires_grad_()
    y = F.conv3d(x, w.double(), None, 2, 3)
    gy = torch.randn(y.shape, generator=g).to(dt)                    # (the yardstick gets the same rounded dy, widened)
    ref, = torch.autograd.grad(y, x, gy.double())
    dyd = gy.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    with ops.launch_scope(DEV):
        dx = ops.stem_bwd_data(dyd, w.to(DEV), shape)
        dx2 = ops.stem_bwd_data(dyd, w.to(DEV), shape)
    assert dx.dtype == torch.float32 and tuple(dx.shape) == shape
    e = rel_l2(dx.cpu(), ref[:, 0])
    print(f"[stem_bwd_data {shape} {dt}] rel-L2 vs float64 {e:.2e}")
    assert e <= STEM_DGRAD_TOL, e
    assert torch.equal(dx, dx2)


def test_bn_bwd_apply_eval_kernel(dram):
    """dy = scale * dz * mask: mask from z (y not read) == mask re-derived from y, fp32 and bf16, with column sums."""
    ops = dram.ops
    dram.load_library()
    g = torch.Generator().manual_seed(9)
    for shape in ((2, 5, 6, 7, 64), (1, 3, 4, 5, 32), (1, 2, 3, 3, 96), (1, 17, 32, 32, 64)):
        C = shape[-1]
        y = torch.randn(shape, generator=g)
        dz = torch.randn(shape, generator=g)
        scale, shift = torch.rand(C, generator=g) + 0.5, 0.3 * torch.randn(C, generator=g)
        for dt in (torch.float32, BF):
            yd, dzd = y.to(DEV).to(dt), dz.to(DEV).to(dt)
            sc, sh = scale.to(DEV), shift.to(DEV)
            with ops.launch_scope(DEV):
                z = ops.bn_apply(yd, sc, sh, None, 1, True)
                a = ops.bn_bwd_apply_eval(dzd, z, None, sc, None, True)
                b, cp = ops.bn_bwd_apply_eval(dzd, None, yd, sc, sh, True, want_colsum=True)
                lin = ops.bn_bwd_apply_eval(dzd, None, None, sc, None, False)
            assert torch.equal(a, b)
            ref = dzd.double().cpu() * scale.double() * (z.double().cpu() > 0)
            tol = 1e-6 if dt == torch.float32 else 2 ** -8
            assert rel_l2(a.double().cpu(), ref) <= tol
            assert rel_l2(lin.double().cpu(), dzd.double().cpu() * scale.double()) <= tol
            if 256 % (C // 4) == 0:
                assert cp is not None
                assert rel_l2(cp.double().sum((0, 1)).cpu(), ref.reshape(-1, C).sum(0)) <= (1e-5 if dt == torch.float32 else 1e-2)
            else:
                assert cp is None


# ------------------------------------------------------------------------------------------------ b. network, fp32
def oracle_grads(sd0, names, x, lungs, factory, hw, train, pins, dt):
    lv = {k: (v.clone().to(dt).requires_grad_(True) if k in names
              else (v.clone().to(dt) if v.is_floating_point() else v.clone())) for k, v in sd0.items()}
    xo = x.detach().clone().to(dt).requires_grad_()
    od, oo = orc.forward(lv, xo, None if lungs is None else lungs.to(dt), factory, train=train, pins=pins)
    golden_loss(factory, od, oo, [t.to(dt) for t in hw]).backward()
    out = {n: lv[n].grad for n in names}
    out["x"] = xo.grad
    return out


def network_case(factory, shape, train, seed=3):
    m = build(factory, seed, stats_seed=seed + 100)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    names = [n for n, _ in m.named_parameters()]
    x, lungs = make_inputs(seed + 1, shape)
    hw = head_weights(seed + 1, shape[0])
    m = m.to(DEV).train(train)
    xd, ld = x.to(DEV).requires_grad_(), lungs.to(DEV)
    dense, outs = m(xd, ld)
    pins = pinned_decisions(dense[0])
    golden_loss(factory, dense, outs, [t.to(DEV) for t in hw]).backward()
    assert xd.grad is not None and xd.grad.dtype == torch.float32 and xd.grad.shape == xd.shape
    if not train:
        with torch.no_grad():
            de, oe = m(xd.detach(), ld)
        for a, b in zip(dense + outs, de + oe):
            assert torch.equal(a.detach(), b), "eval forward of the gradient path differs from the no_grad eval forward"
        for k, v in m.state_dict().items():
            if k not in names:
                assert torch.equal(v.cpu(), sd0[k]), f"buffer {k} changed in eval mode"
    g64 = oracle_grads(sd0, names, x, lungs, factory, hw, train, pins, torch.float64)
    g32 = oracle_grads(sd0, names, x, lungs, factory, hw, train, pins, torch.float32)
    got = {n: p.grad for n, p in m.named_parameters()}
    got["x"] = xd.grad
    worst = (0.0, 0.0, "")
    for n in ["x"] + names:
        assert got[n] is not None, n
        gh = got[n].double().cpu()
        if train and is_noise_param(n):
            assert float(gh.norm()) < 1e-4, n
            continue
        e_hip, e_cpu = rel_l2(gh, g64[n]), rel_l2(g32[n], g64[n])
        worst = max(worst, (e_hip, e_cpu, n))
        if n == "x":
            print(f"[{factory} {shape} {'train' if train else 'eval'}] x.grad vs decision-pinned fp64 oracle {e_hip:.2e} "
                  f"(CPU fp32 oracle: {e_cpu:.2e}, bar {grad_tol(e_cpu):.1e})")
        assert e_hip <= grad_tol(e_cpu), f"{n}: hip vs decision-pinned fp64 oracle {e_hip:.2e} (CPU fp32: {e_cpu:.2e})"
    print(f"[{factory} {shape} {'train' if train else 'eval'}] worst (hip, cpu-fp32, tensor): {worst}")


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("factory,shape", [("resnet18segreg", (1, 1, 16, 32, 32)), ("resnet18segcls", (1, 1, 16, 32, 32)),
                                           ("resnet50segreg", (1, 1, 16, 32, 32)), ("resnet18segreg", (2, 1, 16, 32, 48))],
                         ids=["r18reg", "r18cls", "r50reg", "r18reg-B2"])
def test_network_input_and_parameter_gradients(dram, factory, shape, train):
    dram.load_library()
    network_case(factory, shape, train)


def test_network_mid_size_eval(dram):
    """1x1x64x128x128, ResNet-18, eval: the large-grid launch forms on the path."""
    dram.load_library()
    network_case("resnet18segreg", (1, 1, 64, 128, 128), False)


# ------------------------------------------------------------------------------------------------ c. nothing moved
def _families(dram, fn):
    tl = dram.ops.KernelTimeline()
    tl.start()
    try:
        fn()
        return tl.families()
    finally:
        tl.stop()


def _stem_launches(fams, variants):
    return sum(fams.get("stem", {"variants": {}})["variants"].get(v, [0, 0.0])[0] for v in variants)


def test_training_step_is_unchanged_and_attribution_launches_no_weight_gradient(dram):
    dram.load_library()
    factory, shape = "resnet18segreg", (1, 1, 16, 32, 32)
    m = build(factory, 3).to(DEV).train()
    x, lungs = make_inputs(4, shape)
    hw = [t.to(DEV) for t in head_weights(4, 1)]
    ld = lungs.to(DEV)

    def step(req):
        m.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_(req)
        dense, outs = m(xd, ld)
        golden_loss(factory, dense, outs, hw).backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in m.named_parameters()}, xd.grad

    step(False)                                        # (first step of a shape: weights packed in place)
    fam_plain = _families(dram, lambda: step(False))
    g0, gx0 = step(False)
    g1, gx1 = step(True)
    assert gx0 is None and gx1 is not None
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert _stem_launches(fam_plain, STEM_DGRAD_VARIANTS) == 0
    assert _stem_launches(fam_plain, STEM_WGRAD_VARIANTS) == 1
    assert any(f in fam_plain for f in WGRAD_FAMILIES)

    for train in (False, True):
        m.train(train)
        fam = _families(dram, lambda: m.input_gradient(x.to(DEV), ld, out_grads=(hw[2], hw[3])))
        assert _stem_launches(fam, STEM_DGRAD_VARIANTS) == 2      # scatter GEMM + fold
        assert _stem_launches(fam, STEM_WGRAD_VARIANTS) == 0
        assert not [f for f in WGRAD_FAMILIES if f in fam], fam.keys()


# ------------------------------------------------------------------------------------------------ d. attribution helper
@pytest.mark.parametrize("recompute", [False, True], ids=["keep", "recompute"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_input_gradient_equals_autograd_route(dram, recompute, train):
    dram.load_library()
    factory, shape = "resnet18segreg", (2, 1, 16, 32, 48)
    m = build(factory, 3, stats_seed=8).to(DEV).train(train)
    x, lungs = make_inputs(4, shape)
    hw = [t.to(DEV) for t in head_weights(4, shape[0])]
    ld = lungs.to(DEV)

    def autograd_route():
        xd = x.to(DEV).requires_grad_()
        dense, outs = m(xd, ld)
        gd = torch.autograd.grad(golden_loss(factory, dense, outs, hw), xd)[0]
        return gd, [d.detach() for d in dense]

    m.activation_recompute = False
    ref, dense = autograd_route()
    # the cotangents autograd handed to the network in that route, taken the same way on the detached outputs
    with torch.no_grad():
        outs = m(x.to(DEV), ld)[1]
    leaves = [t.detach().clone().requires_grad_() for t in dense + outs]
    cot = torch.autograd.grad(golden_loss(factory, leaves[:2], leaves[2:], hw), leaves)
    assert all(p.grad is None for p in m.parameters())           # autograd.grad: nothing accumulated
    m.activation_recompute = recompute
    if recompute:
        assert torch.equal(autograd_route()[0], ref)
    got = m.input_gradient(x.to(DEV), ld, out_grads=cot[2:], dense_grads=cot[:2])
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert torch.equal(got, ref)
    assert all(p.grad is None for p in m.parameters())
    # existing .grad tensors stay as they are
    for p in m.parameters():
        p.grad = torch.full_like(p, 0.25)
    m.input_gradient(x.to(DEV), ld, out_grads=(hw[2], None))
    assert all(bool((p.grad == 0.25).all()) for p in m.parameters())


def test_frozen_parameters_eval_mode_gradient_flows_to_input_only(dram):
    """requires_grad_(False) on every parameter + x.requires_grad_(): the autograd route takes the attribution path."""
    dram.load_library()
    factory, shape = "resnet18segcls", (1, 1, 16, 32, 32)
    m = build(factory, 3, stats_seed=8).to(DEV).eval()
    x, lungs = make_inputs(4, shape)
    hw = [t.to(DEV) for t in head_weights(4, 1)]
    xd = x.to(DEV).requires_grad_()
    dense, outs = m(xd, lungs.to(DEV))
    ref = torch.autograd.grad(golden_loss(factory, dense, outs, hw), xd)[0]
    for p in m.parameters():
        p.requires_grad_(False)
    fam = _families(dram, lambda: golden_loss(factory, *m(xd, lungs.to(DEV)), hw).backward())
    assert torch.equal(xd.grad, ref)
    assert not [f for f in WGRAD_FAMILIES if f in fam] and _stem_launches(fam, STEM_WGRAD_VARIANTS) == 0


# ------------------------------------------------------------------------------------------------ e. bf16 storage
def _loss(dense, outs):
    return outs[0].float().sum() * 0.7 - outs[1].float().sum() * 1.3 + 0.1 * (dense[0].float() * dense[1].float()).mean()


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_input_gradient_bf16_storage(dram, train):
    """x.grad with bf16 activations (2x1x32x64x64, ResNet-18) vs the fp64 oracle pinned to the bf16 forward's decisions.
    Bar: max(1e-1, 2 x e_ref), e_ref = distance of the reference arithmetic's CPU autocast(bfloat16) x.grad from its
    fp32 x.grad (decisions free)."""
    from bodyct_dram_emph_subtype_amd.engine import forward_decisions
    dram.load_library()
    factory, shape = "resnet18segreg", (2, 1, 32, 64, 64)
    m = build(factory, 3, stats_seed=None if train else 8)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    x = torch.randn(*shape, generator=g)
    lungs = (torch.rand(*shape, generator=g) > 0.3).float()
    m = m.to(DEV).train(train)
    m.storage_dtype = BF
    xd = x.to(DEV).requires_grad_()
    dense, outs = m(xd, lungs.to(DEV))
    saved = dense[0].grad_fn.saved_state
    assert saved["xs"].dtype == BF and saved["xup3"].dtype == BF
    pins = {k: v.cpu() for k, v in forward_decisions(saved).items()}
    _loss(dense, outs).backward()
    assert xd.grad.dtype == torch.float32

    def oracle_xgrad(dt, pins=None, autocast=False):
        lv = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
        xo = x.detach().clone().to(dt).requires_grad_()
        if autocast:
            with torch.autocast("cpu", dtype=BF):
                d, o = orc.forward(lv, xo, lungs.to(dt), factory, train=train, pins=pins)
        else:
            d, o = orc.forward(lv, xo, lungs.to(dt), factory, train=train, pins=pins)
        _loss(d, o).backward()
        return xo.grad

    e = rel_l2(xd.grad.cpu(), oracle_xgrad(torch.float64, pins))
    e_ref = rel_l2(oracle_xgrad(torch.float32, autocast=True), oracle_xgrad(torch.float32))
    if e_ref != e_ref:          # the reference's autocast backward overflowed: the 1e-1 floor alone holds
        e_ref = 0.0
    print(f"[{factory} bf16 {'train' if train else 'eval'}] x.grad vs decision-pinned fp64 oracle (hip, reference-autocast-vs-fp32): "
          f"({e:.3e}, {e_ref:.3e})")
    assert e <= max(1e-1, 2.0 * e_ref), f"x.grad: {e:.2e} (reference autocast vs its fp32 self: {e_ref:.2e})"


# ------------------------------------------------------------------------------------------------ f. host checks on the GPU box
def test_cpu_operands_are_rejected_before_launch(dram):
    dram.load_library()
    ops = dram.ops
    m = build("resnet18segreg", 3).to(DEV).eval()
    x, _ = make_inputs(4, (1, 1, 16, 32, 32), with_lungs=False)
    with pytest.raises(RuntimeError):
        m.input_gradient(x, out_grads=(torch.ones(1), None))
    with pytest.raises(ValueError):
        m.input_gradient(x.to(DEV), out_grads=(torch.ones(1), None))          # cotangent on the CPU
    with pytest.raises(ValueError):
        m.input_gradient(x.to(DEV), out_grads=(None, None))
    w = torch.zeros(64, 1, 7, 7, 7)
    with ops.launch_scope(DEV):
        with pytest.raises(RuntimeError):
            ops.stem_bwd_data(torch.zeros(1, 4, 4, 4, 64), w.to(DEV), (1, 8, 8, 8))
        with pytest.raises(RuntimeError):
            ops.stem_bwd_data(torch.zeros(1, 4, 4, 4, 64, device=DEV), w, (1, 8, 8, 8))
        with pytest.raises(ValueError):
            ops.stem_bwd_data(torch.zeros(1, 4, 4, 4, 64, device=DEV), w.to(DEV), (1, 9, 9, 9))
        with pytest.raises(TypeError):
            ops.stem_bwd_data(torch.zeros(1, 4, 4, 4, 64, device=DEV, dtype=torch.float16), w.to(DEV), (1, 8, 8, 8))
