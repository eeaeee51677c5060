"""GPU: class-activation maps at get_target_layer() (the us3 output A the heads read) through the HIP engine.

  a. kernel: ops.cam vs plain torch in float64 on the CPU (A requires grad, G = autograd.grad(s, A), then the formulas),
     every method, relu on and off, fp32 and bf16 A (the yardstick gets the same rounded A, widened); and vs the same
     formulas in float64 on the G that ops.head_bwd returns for the same operands.  Bar: relative L2 <= 1e-5, the bar
     test_head holds head_bwd's dx to (the same dpre, the same 32-term sums; alpha is a double fold).  Two calls are
     bit-identical.
     The yardstick's pre-ReLU map must be >= 10 % positive and >= 10 % negative for gradcam and hirescam on every shape
     of 100 voxels or more, so that relu=True compares something.  Two cases cannot meet that by construction and are
     excluded from that assertion only: (1,1,1,1) has a single value, and layercam's pre-ReLU map, sum_c max(G,0) A with
     A = relu(.) >= 0, is never negative (there relu on and off must agree, which is asserted instead).
  b. target_activations is the tensor the heads read: fed back through ops.head_fwd with the module's head weights it
     reproduces forward's dense maps bit for bit.
  c. activation_map end to end vs the float64 formulas on target_activations' own output and the state_dict head
     weights, pooled-score denominator included; score= == its one-hot out_grads; upsample_mask == ops.upproject.
  d. nothing else moves: parameters, buffers, .grad, a later training step, launches, peak memory.
  e. errors raise before anything is launched.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_loss, head_weights, make_inputs, rel_l2
from test_input_grad_gpu import build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
TOL = 1e-5
METHODS = ("gradcam", "hirescam", "layercam")


def maps_from(G, A, method, relu):
    """The issue's formulas: G, A [B,V,32] float64 -> [B,V]."""
    if method == "gradcam":
        m = (G.mean(1, keepdim=True) * A).sum(-1)
    elif method == "hirescam":
        m = (G * A).sum(-1)
    else:
        m = (G.clamp_min(0) * A).sum(-1)
    return m.clamp_min(0) if relu else m


# ------------------------------------------------------------------------------------------------ a. kernel
# (shape, NO, sigmoid, lungs grid or None, gdense given)
KERNEL_CASES = [
    ((1, 1, 1, 1), 2, True, None, True),
    ((2, 3, 5, 7), 2, True, (7, 9, 5), True),            # odd everywhere, mask at non-integer ratios 7/3, 9/5, 5/7
    ((2, 3, 5, 7), 9, False, None, False),
    ((1, 5, 37, 18), 2, True, None, False),
    ((1, 5, 37, 18), 9, False, None, True),
    ((2, 16, 32, 32), 2, True, (32, 64, 64), False),     # 8 partial blocks per sample, two samples
    ((2, 16, 32, 32), 2, True, (32, 64, 64), True),
    ((2, 16, 32, 32), 9, False, None, True),
]


def kernel_operands(case):
    shape, NO, sig, lg, with_gd = case
    B, D, H, W = shape
    g = torch.Generator().manual_seed(11)
    A = torch.randn(B, D, H, W, 32, generator=g).relu()
    w = 0.3 * torch.randn(NO, 32, generator=g)
    b = 0.2 * torch.randn(NO, generator=g)
    gpool = torch.randn(B, NO, generator=g) / (D * H * W)
    gd = torch.randn(B, NO, D, H, W, generator=g) / (D * H * W) if with_gd else None
    lungs = (torch.rand(B, *lg, generator=g) > 0.3).float() if lg else None
    return A, w, b, gpool, gd, lungs


def kernel_reference(A, w, b, gpool, gd, lungs, sig):
    """-> (G [B,V,32], A [B,V,32]) float64 by autograd on the CPU."""
    B, D, H, W, _ = A.shape
    A64 = A.double().requires_grad_()
    pre = torch.einsum("bdhwk,ok->bodhw", A64, w.double()) + b.double()[None, :, None, None, None]
    dense = torch.sigmoid(pre) if sig else pre
    L = F.interpolate(lungs.double()[:, None], (D, H, W), mode="nearest") if lungs is not None else torch.ones(B, 1, D, H, W).double()
    s = (gpool.double() * (dense * L).sum((2, 3, 4))).sum()
    if gd is not None:
        s = s + (gd.double() * dense).sum()
    G, = torch.autograd.grad(s, A64)
    return G.reshape(B, -1, 32), A64.detach().reshape(B, -1, 32)


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: f"{c[0]}-NO{c[1]}-{'sig' if c[2] else 'lin'}-L{c[3]}-gd{int(c[4])}")
def test_cam_kernel_vs_float64(dram, case, dt):
    ops = dram.ops
    dram.load_library()
    shape, NO, sig, lg, with_gd = case
    B, D, H, W = shape
    A, w, b, gpool, gd, lungs = kernel_operands(case)
    A = A.to(dt)                                          # (the yardstick gets the same rounded A, widened)
    G, A64 = kernel_reference(A.float(), w, b, gpool, gd, lungs, sig)
    dev = lambda t: None if t is None else t.to(DEV)
    Ad, wd, bd, gpd, gdd, ld = map(dev, (A, w, b, gpool, gd, lungs))
    with ops.launch_scope(DEV):
        # second yardstick: the layer gradient ops.head_bwd returns for the same operands (fp32 storage of the same values)
        dense = ops.head_fwd(Ad.float(), wd, bd, ld, sig)[0] if sig else None
        G2 = ops.head_bwd(Ad.float(), wd, dense, gdd, gpd, ld, sig)[0]
    G2 = G2.double().cpu().reshape(B, -1, 32)
    assert rel_l2(G2, G) <= TOL
    for method in METHODS:
        pre = maps_from(G, A64, method, False)
        if method != "layercam" and pre.numel() >= 100:
            pos, neg = float((pre > 0).double().mean()), float((pre < 0).double().mean())
            assert pos >= 0.1 and neg >= 0.1, (method, pos, neg)
        got = {}
        for relu in (False, True):
            with ops.launch_scope(DEV):
                m = ops.cam(Ad, wd, bd, gdd, gpd, ld, sig, method, relu)
                m2 = ops.cam(Ad, wd, bd, gdd, gpd, ld, sig, method, relu)
            assert m.dtype == torch.float32 and tuple(m.shape) == shape
            assert torch.equal(m, m2)
            got[relu] = m
            e = rel_l2(m.cpu().reshape(B, -1), maps_from(G, A64, method, relu))
            e2 = rel_l2(m.cpu().reshape(B, -1), maps_from(G2, A64, method, relu))
            print(f"[cam {shape} NO={NO} {dt} {method} relu={relu}] rel-L2 vs fp64 {e:.2e}, vs head_bwd's G {e2:.2e}")
            assert e <= TOL, (method, relu, e)
            assert e2 <= TOL, (method, relu, e2)
        if method == "layercam":
            assert torch.equal(got[True], got[False].clamp_min(0))
            assert float(pre.min()) >= 0.0


def test_cam_wrapper_rejects_bad_operands(dram):
    ops = dram.ops
    dram.load_library()
    A, w, b, gpool, gd, lungs = (t.to(DEV) if t is not None else None for t in kernel_operands(KERNEL_CASES[1]))
    with ops.launch_scope(DEV):
        with pytest.raises(ValueError):
            ops.cam(A, w, b, gd, gpool, lungs, True, "scorecam")
        with pytest.raises(ValueError):
            ops.cam(A, w, b, gd, gpool[:1].contiguous(), lungs, True)
        with pytest.raises(ValueError):
            ops.cam(A[..., :16].contiguous(), w, b, gd, gpool, lungs, True)
        with pytest.raises(RuntimeError):
            ops.cam(A.cpu(), w, b, gd, gpool, lungs, True)
        with pytest.raises(TypeError):
            ops.cam(A.half(), w, b, gd, gpool, lungs, True)


# ------------------------------------------------------------------------------------------------ b, c. network
SHAPE = (2, 1, 16, 32, 32)
NETS = [("resnet18segreg", True), ("resnet18segreg", False), ("resnet18segcls", True)]     # (factory, with lungs)


def net(factory, train, dt, seed=3):
    m = build(factory, seed, stats_seed=seed + 100).to(DEV).train(train)
    m.storage_dtype = dt
    return m


def stacked_heads(m):
    sd = m.state_dict()
    w = torch.cat([sd["fcs.0.weight"].flatten(1), sd["fcs.1.weight"].flatten(1)], 0).contiguous()
    return w, torch.cat([sd["fcs.0.bias"], sd["fcs.1.bias"]], 0).contiguous()


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("factory", ["resnet18segreg", "resnet18segcls"])
def test_target_activations_is_what_the_heads_read(dram, factory, train, dt):
    ops = dram.ops
    dram.load_library()
    m = net(factory, train, dt)
    x, lungs = make_inputs(4, SHAPE)
    xd, ld = x.to(DEV), lungs.to(DEV)
    A = m.target_activations(xd, ld)
    assert A.dtype == torch.float32 and tuple(A.shape) == (2, 32, 8, 16, 16)
    assert float(A.min()) >= 0.0
    with torch.no_grad():
        dense, _ = m(xd, ld)
    w, b = stacked_heads(m)
    sig = factory.endswith("reg")
    with ops.launch_scope(DEV):
        again = ops.head_fwd(A.permute(0, 2, 3, 4, 1).contiguous().to(dt), w, b, ld[:, 0].contiguous() if sig else None, sig)[0]
    assert torch.equal(again, torch.cat(dense, 1))


def network_reference(m, A, lungs, og, dg):
    """float64 on the CPU from target_activations' output and the state_dict heads: (G, A) [B,V,32]."""
    reg = m.HEAD == "reg"
    n0 = m.n_classes[0]
    w, b = (t.double().cpu() for t in stacked_heads(m))
    A64 = A.double().cpu().requires_grad_()
    B, grid = A64.shape[0], tuple(A64.shape[2:])
    pre = torch.einsum("bkdhw,ok->bodhw", A64, w) + b[None, :, None, None, None]
    if reg:
        dense = torch.sigmoid(pre)
        L = F.interpolate(lungs.double().cpu(), grid, mode="nearest") if lungs is not None else torch.ones(B, 1, *grid).double()
        pooled = (dense * L).sum((2, 3, 4)) / L.sum((2, 3, 4))            # [B,2]
        outs = [pooled[:, 0], pooled[:, 1]]
    else:
        dense = pre
        pooled = pre.mean((2, 3, 4))
        outs = [pooled[:, :n0], pooled[:, n0:]]
    denses = [dense[:, :n0], dense[:, n0:]]
    s = sum((g.double().cpu() * y).sum() for g, y in zip(list(og) + list(dg), outs + denses) if g is not None)
    G, = torch.autograd.grad(s, A64)
    flat = lambda t: t.detach().permute(0, 2, 3, 4, 1).reshape(B, -1, 32)
    return flat(G), flat(A64)


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("factory,with_lungs", NETS, ids=["reg-lungs", "reg-nolungs", "cls"])
def test_activation_map_end_to_end(dram, factory, with_lungs, train, dt):
    ops = dram.ops
    dram.load_library()
    m = net(factory, train, dt)
    reg = factory.endswith("reg")
    x, lungs = make_inputs(4, SHAPE)
    xd, ld = x.to(DEV), (lungs.to(DEV) if with_lungs else None)
    A = m.target_activations(xd, ld)
    B, grid = SHAPE[0], tuple(A.shape[2:])
    g = torch.Generator().manual_seed(21)
    hw = head_weights(4, B)
    nvox = grid[0] * grid[1] * grid[2]
    dcot = torch.randn(B, m.n_classes[1], *grid, generator=g) / nvox
    score = (1, 0) if reg else (0, 4)
    onehot = torch.ones(B) if reg else F.one_hot(torch.full((B,), 4), 6).float()
    targets = [                                           # (keyword arguments, (out_grads, dense_grads) for the yardstick)
        (dict(score=score), ([None, onehot] if reg else [onehot, None], [None, None])),
        (dict(out_grads=(hw[2], hw[3]) if reg else (hw[0], hw[1])), (list(hw[2:]) if reg else list(hw[:2]), [None, None])),
        (dict(out_grads=(hw[2], None) if reg else (None, hw[1]), dense_grads=(None, dcot)),
         ([hw[2], None] if reg else [None, hw[1]], [None, dcot])),
    ]
    todev = lambda kw: {k: (tuple(None if t is None else t.to(DEV) for t in v) if k != "score" else v) for k, v in kw.items()}
    for kw, (og, dg) in targets:
        G, A64 = network_reference(m, A, lungs if with_lungs else None, og, dg)
        for method in METHODS:
            got = m.activation_map(xd, ld, method=method, relu=False, **todev(kw))
            assert got.dtype == torch.float32 and tuple(got.shape) == (B, 1) + grid
            e = rel_l2(got.cpu().reshape(B, -1), maps_from(G, A64, method, False))
            print(f"[activation_map {factory} lungs={with_lungs} train={train} {dt} {sorted(kw)} {method}] rel-L2 {e:.2e}")
            assert e <= TOL, (sorted(kw), method, e)
            rl = m.activation_map(xd, ld, method=method, relu=True, **todev(kw))
            assert torch.equal(rl, got.clamp_min(0))
    # score= is its one-hot out_grads; upsample_mask is ops.upproject of the low-resolution map
    og = [None if t is None else t.to(DEV) for t in targets[0][1][0]]
    mask = (torch.rand(B, *SHAPE[2:], generator=g) > 0.3).float().to(DEV)
    for method in METHODS:
        a = m.activation_map(xd, ld, score=score, method=method)
        assert torch.equal(a, m.activation_map(xd, ld, out_grads=og, method=method))
        up = m.activation_map(xd, ld, score=score, method=method, upsample_mask=mask)
        assert tuple(up.shape) == (B, 1) + SHAPE[2:]
        with ops.launch_scope(DEV):
            assert torch.equal(up[:, 0], ops.upproject(a[:, 0].contiguous(), mask, SHAPE[2:])[0])


# ------------------------------------------------------------------------------------------------ d. nothing else moves
def _families(dram, fn):
    tl = dram.ops.KernelTimeline()
    tl.start()
    try:
        fn()
        return tl.families()
    finally:
        tl.stop()


def test_nothing_else_moves(dram):
    dram.load_library()
    factory = "resnet18segreg"
    m = net(factory, False, torch.float32)
    x, lungs = make_inputs(4, SHAPE)
    xd, ld = x.to(DEV), lungs.to(DEV)
    hw = [t.to(DEV) for t in head_weights(4, SHAPE[0])]
    mask = torch.ones(SHAPE[0], *SHAPE[2:], device=DEV)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for method in METHODS:
        m.activation_map(xd, ld, score=(0, None), method=method, upsample_mask=mask)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in m.parameters())

    # launches: the matrix-pipe families record a no-grad forward's launches, the whole call at most 4 more
    def fwd():
        with torch.no_grad():
            m(xd, ld)

    for train in (False, True):
        m.train(train)
        fwd()                                             # (warm: the first forward of a mode may pack weights)
        fam_fwd = _families(dram, fwd)
        for method in METHODS:
            fam = _families(dram, lambda: m.activation_map(xd, ld, out_grads=(hw[2], hw[3]), method=method, upsample_mask=mask))
            mfma = lambda f: {k: v["launches"] for k, v in f.items() if v["bound"] == "mfma"}
            assert mfma(fam) == mfma(fam_fwd), method
            extra = sum(v["launches"] for v in fam.values()) - sum(v["launches"] for v in fam_fwd.values())
            assert 0 < extra <= 4, (method, extra)

    # a training step after a CAM call == the same step without one
    def step(mm):
        mm.zero_grad(set_to_none=True)
        dense, outs = mm(xd, ld)
        golden_loss(factory, dense, outs, hw).backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in mm.named_parameters()}

    m0, m1 = net(factory, True, torch.float32), net(factory, True, torch.float32)
    m1.eval()
    m1.activation_map(xd, ld, score=(0, 0))
    m1.train()
    g0, g1 = step(m0), step(m1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_peak_memory_is_a_no_grad_forward_plus_the_results(dram):
    dram.load_library()
    m = net("resnet18segreg", False, torch.float32)
    x, lungs = make_inputs(4, SHAPE)
    xd, ld = x.to(DEV), lungs.to(DEV)

    def peak(fn):
        fn()                                              # (warm: workspaces, packed weights)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    def fwd():
        with torch.no_grad():
            return m(xd, ld)

    p_fwd, (dense, _) = peak(fwd)
    nbytes = lambda t: t.numel() * t.element_size()
    dense_bytes = sum(nbytes(d) for d in dense)
    us3_bytes = SHAPE[0] * 32 * 8 * 16 * 16 * 4
    del dense
    for method in METHODS:
        p_cam, out = peak(lambda: m.activation_map(xd, ld, score=(0, 0), method=method))
        assert p_cam <= p_fwd + us3_bytes + dense_bytes + nbytes(out) + (1 << 20), (method, p_cam, p_fwd)
        del out


# ------------------------------------------------------------------------------------------------ e. errors
def test_errors_raise_before_anything_is_launched(dram):
    dram.load_library()
    m = net("resnet18segreg", True, torch.float32)        # train(): a forward would update the running statistics
    c = net("resnet18segcls", True, torch.float32)
    x, lungs = make_inputs(4, SHAPE)
    xd, ld = x.to(DEV), lungs.to(DEV)
    one = torch.ones(SHAPE[0], device=DEV)
    before = {k: v.clone() for k, v in list(m.state_dict().items()) + [("c." + k, v) for k, v in c.state_dict().items()]}

    def bad():
        for exc, mod, a, kw in [
                (ValueError, m, (xd, ld), dict(score=(0, 0), method="scorecam")),
                (ValueError, m, (xd, ld), dict(score=(0, 0), out_grads=(one, None))),
                (ValueError, m, (xd, ld), dict()),
                (ValueError, m, (xd, ld), dict(out_grads=(None, None), dense_grads=None)),
                (ValueError, m, (xd, ld), dict(score=(0, 1))),
                (ValueError, m, (xd, ld), dict(score=(2, 0))),
                (ValueError, c, (xd, ld), dict(score=(0, 6))),
                (ValueError, c, (xd, ld), dict(score=(1, None))),
                (ValueError, m, (xd, ld), dict(out_grads=(torch.ones(SHAPE[0], 1, device=DEV), None))),
                (ValueError, m, (xd, ld), dict(dense_grads=(torch.ones(SHAPE[0], 1, 8, 16, 15, device=DEV), None))),
                (ValueError, m, (xd, ld), dict(out_grads=(one.cpu(), None))),
                (RuntimeError, m, (x, lungs), dict(score=(0, 0)))]:
            with pytest.raises(exc):
                mod.activation_map(*a, **kw)
        with pytest.raises(RuntimeError):
            m.target_activations(x, lungs)

    fam = _families(dram, bad)
    assert not fam, fam
    after = list(m.state_dict().items()) + [("c." + k, v) for k, v in c.state_dict().items()]
    for k, v in after:
        assert torch.equal(v, before[k]), k
