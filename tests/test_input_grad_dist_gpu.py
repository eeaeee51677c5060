"""GPU: the input gradient and the eval-mode backward under distributed.attach -- one rank, backend nccl, collectives
forced on (the arena, the bucket all-reduces and the statistic all-reduces run for real; a 1-rank mean is the identity,
so everything must equal the unattached module bit for bit).  Eval mode: no SyncBN exchange in either direction;
attribution only: no gradient all-reduce at all."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_distributed_gpu import ROOT, _build, _inputs, _loss, _run_ranks

pytestmark = pytest.mark.gpu


def _world1(port, outdir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from bodyct_dram_emph_subtype_amd import distributed as ddist
        out = {}
        x, lungs = _inputs(1)
        for forced in (False, True):
            for train in (True, False):
                torch.manual_seed(4)
                m = _build("resnet18segreg").to("cuda:0")
                g = torch.Generator().manual_seed(9)
                for name, b in m.named_buffers():
                    if name.endswith("running_var"):
                        b.copy_((0.5 + torch.rand(b.shape, generator=g)).to(b.device))
                m.train(train)
                ctx = ddist.attach(m, bucket_bytes=8 << 20, force=forced)
                assert (m._dist is not None) == forced
                xd = x.cuda().requires_grad_()
                dense, outs = m(xd, lungs.cuda())
                _loss(0, dense, outs).backward()
                torch.cuda.synchronize()
                s1 = dict(ctx.stats) if forced else {}
                sal = m.input_gradient(x.cuda(), lungs.cuda(), out_grads=(torch.ones_like(outs[0]), None))
                torch.cuda.synchronize()
                s2 = dict(ctx.stats) if forced else {}
                out[(forced, train)] = ({n: p.grad.cpu() for n, p in m.named_parameters()}, xd.grad.cpu(), sal.cpu(), s1, s2)
        torch.save(out, os.path.join(outdir, "w1.pt"))
    finally:
        dist.destroy_process_group()


def test_world1_attached_input_gradient_and_eval_backward_equal_plain():
    import tempfile
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as outdir:
        _run_ranks([ctx.Process(target=_world1, args=(36100 + (os.getpid() % 2000), outdir))])
        out = torch.load(os.path.join(outdir, "w1.pt"))
    for train in (True, False):
        g0, x0, sal0, _, _ = out[(False, train)]
        g1, x1, sal1, s1, s2 = out[(True, train)]
        for n in g0:
            assert torch.equal(g0[n], g1[n]), (train, n)
        assert torch.equal(x0, x1) and torch.equal(sal0, sal1), train
        assert s1["grad_allreduce"] >= 1
        assert s2["grad_allreduce"] == s1["grad_allreduce"], "an attribution call reduced gradients"
        if train:
            assert s1["bn_allreduce"] == 2 * 22 and s2["bn_allreduce"] == 2 * 2 * 22      # forward + backward, 22 BN layers
        else:
            assert s1["bn_allreduce"] == 0 and s2["bn_allreduce"] == 0, "SyncBN exchange in eval mode"
