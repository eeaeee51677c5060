"""GPU: fused global-norm / value gradient clipping of the fused optimizers (csrc/optim.hip: dram_grad_norm_multi,
dram_*_clip, dram_grad_scale_multi), the drop-in clip_grad_norm_ / clip_grad_value_, and the harness flags
--gradient_clip_val / --gradient_clip_algorithm / --accumulate_grad_batches.

The gradient set of the kernel tests: chunk tails (16383 / 16384 / 16385 around DRAM_OPT_CHUNK = 16384), tensors smaller
than one float4, a multi-chunk tensor with a tail (70001), one network-shaped weight, and -- where the fold of the
per-chunk partial sums matters -- a 20 000 000-element tensor (1 221 chunks: more partials than the 1 024 lanes of the
folding workgroup take in one sweep)."""
import logging
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1,), (3,), (16383,), (16384,), (16385,), (70001,), (64, 1, 7, 7, 7)]
BIG = 20_000_000
ULP = 1.2e-7                     # one fp32 ulp, relative


@pytest.fixture(scope="module")
def grad_set():
    """(small gradients, the big one) on the device + the fp64 sum of squares of each, computed once on the CPU."""
    g = torch.Generator().manual_seed(1234)
    small = [torch.randn(s, generator=g) for s in SHAPES]
    big = torch.randn(BIG, generator=g)
    sq = [float(t.double().square().sum()) for t in small + [big]]
    return [t.to(DEV) for t in small], big.to(DEV), sq


def _bits(t):
    return t.detach().cpu().view(torch.int32).clone()


def _norm_opt(grads, max_norm, grad_scale=1.0):
    """An optimizer whose step is the norm launch and nothing else of interest: SGD with lr 0 on zero parameters."""
    from bodyct_dram_emph_subtype_amd.optim import FusedSGD
    params = [torch.zeros_like(t).requires_grad_(True) for t in grads]
    for p, t in zip(params, grads):
        p.grad = t
    opt = FusedSGD(params, lr=0.0, max_grad_norm=max_norm)
    opt.grad_scale = grad_scale
    return opt, params


def _coef_ref(max_norm, n):
    """torch.nn.utils.clip_grad_norm_'s coefficient, in fp32 on the CPU, from the norm `n` (a float32 value)."""
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(n, dtype=torch.float32) + 1e-6), max=1.0)


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_norm_matches_fp64(grad_set, grad_scale):
    """last_grad_norm == float32(|grad_scale| sqrt(sum g^2)) of an fp64 CPU evaluation within one fp32 ulp (1.2e-7
    relative): squares and sums are taken in double, so the only rounding that can show is the final cast."""
    small, big, sq = grad_set
    opt, _ = _norm_opt(small + [big], 1.0, grad_scale)
    assert opt.last_grad_norm is None
    opt.step()
    n = opt.last_grad_norm
    assert n.dim() == 0 and n.is_cuda and n.dtype == torch.float32
    ref = float(np.float32(grad_scale * math.sqrt(sum(sq))))
    rel = abs(float(n) - ref) / ref
    print(f"grad_scale {grad_scale}: norm {float(n)!r} fp64 reference {ref!r} rel {rel:.3e}")
    assert rel <= ULP
    # ... and without the big tensor (one sweep of the fold, every chunk-tail form)
    opt, _ = _norm_opt(small, 1.0, grad_scale)
    opt.step()
    ref = float(np.float32(grad_scale * math.sqrt(sum(sq[:-1]))))
    rel = abs(float(opt.last_grad_norm) - ref) / ref
    print(f"grad_scale {grad_scale} (small set): norm {float(opt.last_grad_norm)!r} reference {ref!r} rel {rel:.3e}")
    assert rel <= ULP


def test_norm_is_deterministic(grad_set):
    small, big, _ = grad_set
    runs = []
    for _ in range(2):
        opt, _ = _norm_opt(small + [big], 100.0)
        opt.step()
        runs.append((_bits(opt.last_grad_norm), _bits(opt.last_clip_coef)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].view(torch.float32)) < 1.0            # (the clip was active: the coefficient carries bits)


def test_norm_does_not_depend_on_alignment(grad_set):
    """The same values as separate (256-byte aligned) tensors and as views at ODD element offsets into one flat buffer
    (4-byte aligned: what the data-parallel step's small-gradient bucket hands over): bit-identical norm."""
    small, _, _ = grad_set
    opt, _ = _norm_opt(small, 1.0)
    opt.step()
    flat = torch.zeros(sum(t.numel() + 2 for t in small) + 1, device=DEV)
    views, off = [], 1
    for t in small:
        v = flat[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and v.data_ptr() % 4 == 0
        views.append(v)
        off += t.numel() + (2 if t.numel() % 2 == 0 else 1)      # the next offset is odd again
    opt_v, _ = _norm_opt(views, 1.0)
    opt_v.step()
    assert torch.equal(_bits(opt.last_grad_norm), _bits(opt_v.last_grad_norm))
    assert torch.equal(_bits(opt.last_clip_coef), _bits(opt_v.last_clip_coef))


@pytest.mark.parametrize("with_big", [False, True])
def test_coefficient_is_torchs(grad_set, with_big):
    """clip[3] is bit-identical to clamp(max_norm / (n + 1e-6), max=1) in fp32 from the kernel's own n, for max_norm
    below, above and equal to the norm (changed between steps of ONE optimizer: the attribute is live)."""
    small, big, sq = grad_set
    grads = small + ([big] if with_big else [])
    total = math.sqrt(sum(sq if with_big else sq[:-1]))
    opt, _ = _norm_opt(grads, 0.37 * total)
    opt.step()
    n = float(opt.last_grad_norm)
    for max_norm in (0.37 * total, 3.0 * total, n):
        opt.max_grad_norm = max_norm
        opt.step()
        assert float(opt.last_grad_norm) == n
        got, ref = opt.last_clip_coef.cpu(), _coef_ref(max_norm, n)
        print(f"big {with_big} max_norm {max_norm!r} norm {n!r} coef {float(got)!r} reference {float(ref)!r}")
        assert torch.equal(_bits(got), _bits(ref))
    assert float(_coef_ref(0.37 * total, n)) < 1.0 and float(_coef_ref(3.0 * total, n)) == 1.0


def _steps(make_opt, grads_per_step, transform=None, observe=None):
    """4 steps with ExponentialLR on fresh parameters (seeded); transform(step, g) -> the gradient handed over."""
    g = torch.Generator().manual_seed(7)
    params = [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in SHAPES]
    opt = make_opt(params)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.95)
    for k, gs in enumerate(grads_per_step):
        for p, t in zip(params, gs):
            p.grad = transform(k, t) if transform else t.clone()
        opt.step()
        if observe:
            observe(k, opt)
        sched.step()
    torch.cuda.synchronize()
    state = [{k: v.cpu() for k, v in opt.state[p].items() if torch.is_tensor(v) and v.dim()} for p in params]
    return [p.detach().cpu() for p in params], state


@pytest.fixture(scope="module")
def step_grads():
    g = torch.Generator().manual_seed(99)
    return [[torch.randn(s, generator=g).to(DEV) for s in SHAPES] for _ in range(4)]


def _same(a, b):
    (pa, sa), (pb, sb) = a, b
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    for x, y in zip(sa, sb):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("which", ["adam", "sgd"])
def test_clipped_update_is_the_plain_update_on_clipped_gradients(step_grads, which):
    """FusedAdam(max_grad_norm) on g == FusedAdam() on g.mul(coef), coef read back from the first optimizer: parameters,
    exp_avg, exp_avg_sq bit-identical after 4 steps; likewise FusedSGD with momentum, clip_grad_value against
    g.clamp(-v, v), and max_grad_norm = 1e30 against no clipping at all."""
    from bodyct_dram_emph_subtype_amd.optim import FusedAdam, FusedSGD
    cls, kw = ((FusedAdam, dict(lr=1e-2, weight_decay=0.01)) if which == "adam"
               else (FusedSGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-4)))
    coefs = []
    clipped = _steps(lambda ps: cls(ps, max_grad_norm=25.0, **kw), step_grads,
                     observe=lambda k, o: coefs.append(o.last_clip_coef.clone()))
    assert all(0.0 < float(c) < 1.0 for c in coefs), [float(c) for c in coefs]
    _same(clipped, _steps(lambda ps: cls(ps, **kw), step_grads, transform=lambda k, t: t.mul(coefs[k])))
    v = 0.75
    _same(_steps(lambda ps: cls(ps, clip_grad_value=v, **kw), step_grads),
          _steps(lambda ps: cls(ps, **kw), step_grads, transform=lambda k, t: t.clamp(-v, v)))
    _same(_steps(lambda ps: cls(ps, max_grad_norm=1e30, **kw), step_grads), _steps(lambda ps: cls(ps, **kw), step_grads))


def test_clipped_update_spans_parameter_groups(step_grads):
    """One norm over ALL parameters of the optimizer, across parameter groups: two groups with their own lr give the
    single-group coefficient, and each group's update uses it."""
    from bodyct_dram_emph_subtype_amd.optim import FusedAdam
    coefs, coefs2 = [], []
    one = _steps(lambda ps: FusedAdam(ps, lr=1e-2, max_grad_norm=25.0), step_grads,
                 observe=lambda k, o: coefs.append(_bits(o.last_clip_coef)))
    two = _steps(lambda ps: FusedAdam([dict(params=ps[:3]), dict(params=ps[3:])], lr=1e-2, max_grad_norm=25.0), step_grads,
                 observe=lambda k, o: coefs2.append(_bits(o.last_clip_coef)))
    for a, b in zip(coefs, coefs2):
        assert torch.equal(a, b)
    _same(one, two)


def test_clipped_optimizers_match_torch(step_grads):
    """torch.nn.utils.clip_grad_norm_ / clip_grad_value_ + torch.optim.Adam / SGD on the CPU, 4 steps, at the bar
    test_fused_adam_and_sgd_match_torch uses for the same arithmetic."""
    from bodyct_dram_emph_subtype_amd.optim import FusedAdam, FusedSGD
    for cls_f, cls_r, kw in ((FusedAdam, torch.optim.Adam, dict(lr=1e-2, weight_decay=0.01)),
                             (FusedSGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-4))):
        for clip in (dict(max_grad_norm=25.0), dict(clip_grad_value=0.75)):
            g = torch.Generator().manual_seed(7)
            ref = [torch.randn(s, generator=g).requires_grad_(True) for s in SHAPES]
            o_r = cls_r(ref, **kw)
            sched_r = torch.optim.lr_scheduler.ExponentialLR(o_r, gamma=0.95)
            for gs in step_grads:
                for r, t in zip(ref, gs):
                    r.grad = t.cpu()
                if "max_grad_norm" in clip:
                    torch.nn.utils.clip_grad_norm_(ref, clip["max_grad_norm"])
                else:
                    torch.nn.utils.clip_grad_value_(ref, clip["clip_grad_value"])
                o_r.step()
                sched_r.step()
            got, _ = _steps(lambda ps: cls_f(ps, **kw, **clip), step_grads)
            for r, d in zip(ref, got):
                assert torch.allclose(d, r.detach(), rtol=2e-5, atol=2e-6), (cls_f.__name__, clip)


def test_drop_in_clip_functions_match_torch(step_grads):
    """optim.clip_grad_norm_ / clip_grad_value_ (in place) against torch.nn.utils' on the CPU.  The torch side runs on
    float64 copies of the gradients: the bar on the returned norm is one fp32 ulp, which torch's own fp32 summation of
    1e5 squares does not promise to keep, and the bar is about this kernel's rounding, not torch's."""
    from bodyct_dram_emph_subtype_amd import optim
    gs = step_grads[0]
    for max_norm in (25.0, 1e6):
        ref = [torch.zeros(t.shape, dtype=torch.float64).requires_grad_(True) for t in gs]
        dev = [torch.zeros_like(t).requires_grad_(True) for t in gs]
        for r, d, t in zip(ref, dev, gs):
            r.grad, d.grad = t.cpu().double(), t.clone()
        n_ref = float(np.float32(float(torch.nn.utils.clip_grad_norm_(ref, max_norm))))
        n = optim.clip_grad_norm_(dev, max_norm)
        assert n.is_cuda and n.dim() == 0
        rel = abs(float(n) - n_ref) / n_ref
        print(f"clip_grad_norm_({max_norm}): norm {float(n)!r} torch {n_ref!r} rel {rel:.3e}")
        assert rel <= ULP
        for r, d, t in zip(ref, dev, gs):
            assert torch.allclose(d.grad.cpu(), r.grad.float(), rtol=1e-6, atol=0.0)
            if max_norm == 1e6:
                assert torch.equal(d.grad, t)                  # coefficient 1: nothing moved
    ref = [torch.zeros(t.shape).requires_grad_(True) for t in gs]
    dev = [torch.zeros_like(t).requires_grad_(True) for t in gs]
    for r, d, t in zip(ref, dev, gs):
        r.grad, d.grad = t.cpu(), t.clone()
    dev[1].grad[1] = float("nan")                              # a NaN stays a NaN, as in torch.clamp
    ref[1].grad[1] = float("nan")
    torch.nn.utils.clip_grad_value_(ref, 0.75)
    optim.clip_grad_value_(dev, 0.75)
    for r, d in zip(ref, dev):
        assert torch.equal(_bits(d.grad), _bits(r.grad))
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(dev, 1.0, norm_type=1)
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(dev, 1.0, norm_type=float("inf"))


def test_graphed_train_step_with_clipping_equals_eager_steps():
    """FusedAdam(capturable=True, max_grad_norm) inside graph.GraphedTrainStep: norm and clipped update are kernel nodes
    of the captured step.  Replays equal the same number of eager steps bit for bit, and a max_grad_norm changed between
    replays reaches the captured launches (sync_hyper): norm and coefficient equal the eager ones after the change."""
    from bodyct_dram_emph_subtype_amd import med3d
    from bodyct_dram_emph_subtype_amd.graph import GraphedTrainStep
    from bodyct_dram_emph_subtype_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(1, 1, 16, 32, 32, generator=g).to(DEV),
                (torch.rand(1, 1, 16, 32, 32, generator=g) > 0.3).float().to(DEV)) for _ in range(4)]

    def run(mode):
        torch.manual_seed(11)
        m = med3d.resnet18segreg().to(DEV).train()
        opt = FusedAdam(m.parameters(), lr=1e-3, capturable=True, max_grad_norm=0.5)
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)

        def loss_fn(image, lung):
            dense, outs = m(image, lung)
            return outs[0].sum() + 2.0 * outs[1].sum() + 0.1 * (dense[0] * dense[1]).mean()

        def eager(*b):
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(*b)
            loss.backward()
            opt.step()
            return loss.detach().clone()
        if mode == "graph":
            step = GraphedTrainStep(m, opt, loss_fn, batches[0], warmup=2)
            assert step.graph is not None
        else:
            eager(*batches[0]); eager(*batches[0])
            step = eager
        seen = []
        for i, b in enumerate(batches[1:]):
            loss = step(*b).clone()
            seen.append((loss, _bits(opt.last_grad_norm), _bits(opt.last_clip_coef)))
            if i == 0:
                sched.step()
                opt.max_grad_norm = 0.05               # must reach the captured norm launch
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        st = {i: {k: v.cpu() for k, v in s.items()} for i, s in opt.state_dict()["state"].items()}
        return seen, sd, st

    s_g, sd_g, st_g = run("graph")
    s_e, sd_e, st_e = run("eager")
    for (la, na, ca), (lb, nb, cb) in zip(s_g, s_e):
        print("loss", float(la), float(lb), "norm", float(na.view(torch.float32)), "coef", float(ca.view(torch.float32)),
              float(cb.view(torch.float32)))
        assert torch.equal(la, lb) and torch.equal(na, nb) and torch.equal(ca, cb)
    # the clip was active throughout, and the changed bound changed the coefficient
    assert all(float(c.view(torch.float32)) < 1.0 for _, _, c in s_g)
    assert torch.equal(_bits(_coef_ref(0.5, float(s_g[0][1].view(torch.float32)))), s_g[0][2])
    for _, n, c in s_g[1:]:
        assert torch.equal(_bits(_coef_ref(0.05, float(n.view(torch.float32)))), c)
    for k in sd_e:
        assert torch.equal(sd_g[k], sd_e[k]), k
    for i in st_e:
        assert float(st_g[i]["step"]) == float(st_e[i]["step"]) == 5.0
        assert torch.equal(st_g[i]["exp_avg"], st_e[i]["exp_avg"]) and torch.equal(st_g[i]["exp_avg_sq"], st_e[i]["exp_avg_sq"])


def _world1_clipped(port, outdir):
    """One rank under RCCL with the collectives forced on (as tests/test_distributed_gpu.py::_nccl_world1), eager:
    3 clipped data-parallel steps against 3 clipped plain steps."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from bodyct_dram_emph_subtype_amd import distributed as ddist, med3d
        from bodyct_dram_emph_subtype_amd.optim import FusedAdam
        g = torch.Generator().manual_seed(501)
        x = torch.randn(2, 1, 16, 32, 32, generator=g).cuda()
        lungs = (torch.rand(2, 1, 16, 32, 32, generator=g) > 0.3).float().cuda()
        out = {}
        for forced in (False, True):
            torch.manual_seed(4)
            m = med3d.resnet18segreg().to("cuda:0").train()
            ddist.attach(m, bucket_bytes=8 << 20, force=forced)
            assert (m._dist is not None) == forced
            opt = FusedAdam(m.parameters(), lr=1e-3, max_grad_norm=0.5)
            norms = []
            for _ in range(3):
                opt.zero_grad(set_to_none=True)
                dense, outs = m(x, lungs)
                (outs[0].sum() - 0.5 * outs[1].sum() + 0.1 * (dense[0] * dense[1]).mean()).backward()
                opt.step()
                norms.append((opt.last_grad_norm.cpu().clone(), opt.last_clip_coef.cpu().clone()))
            torch.cuda.synchronize()
            out[forced] = ({n: p.detach().cpu() for n, p in m.named_parameters()}, norms)
        torch.save(out, os.path.join(outdir, "w1clip.pt"))
    finally:
        dist.destroy_process_group()


def test_rccl_world1_clipped_data_parallel_step_equals_plain():
    import tempfile
    import torch.multiprocessing as mp
    from test_distributed_gpu import _run_ranks
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as outdir:
        _run_ranks([ctx.Process(target=_world1_clipped, args=(36700 + (os.getpid() % 2000), outdir))])
        out = torch.load(os.path.join(outdir, "w1clip.pt"))
    (p0, n0), (p1, n1) = out[False], out[True]
    for (a, ca), (b, cb) in zip(n0, n1):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(ca), _bits(cb))
        assert float(ca) < 1.0
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


def test_harness_accumulates_and_clips(tmp_path, caplog):
    """train.py --accumulate_grad_batches 2 --gradient_clip_val 0.5 over 5 batches: 3 optimizer steps (the last one on
    a single batch), counted by global_step and by every Adam step; the logged loss and norm are finite."""
    from bodyct_dram_emph_subtype_amd import train
    caplog.set_level(logging.INFO)
    mod = train.run_training_job(["--model_arch", "med3ddram18", "--target_size", "16", "32", "32", "--batch_size", "1",
                                  "--num_samples", "5", "--max_epochs", "1", "--accumulate_grad_batches", "2",
                                  "--gradient_clip_val", "0.5", "--model_path", str(tmp_path),
                                  "--log_every_n_steps", "1"])
    ck = torch.load(tmp_path / "subtyping_med3ddram18" / "checkpoints" / "epoch=00.ckpt", map_location="cpu",
                    weights_only=False)
    assert ck["global_step"] == 3
    states = ck["optimizer_states"][0]["state"]
    assert len(states) > 0 and all(float(s["step"]) == 3.0 for s in states.values())
    assert "max_grad_norm" not in ck["optimizer_states"][0]["param_groups"][0]
    assert int(mod.model.state_dict()["bn1.num_batches_tracked"]) == 5           # five forward passes, three steps
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())
    steps = re.findall(r"step (\d+) train_loss (\S+) lr \S+ grad_norm (\S+)", caplog.text)
    assert [int(s[0]) for s in steps] == [1, 2, 3], caplog.text
    assert all(math.isfinite(float(l)) and math.isfinite(float(n)) and float(n) > 0 for _, l, n in steps)
    epoch = re.findall(r"epoch 0: train_loss (\S+)", caplog.text)
    assert len(epoch) == 1 and math.isfinite(float(epoch[0]))
