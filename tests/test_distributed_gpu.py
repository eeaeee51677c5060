"""GPU: the real engine under 2 data-parallel ranks (two processes sharing the one GPU of the
test box, gloo backend on device tensors -- RCCL needs one GPU per rank) against the oracle's
N-rank DDP+SyncBatchNorm emulation: BN statistics over the global batch,
loss_r from rank r's slice only, gradients averaged over ranks."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, rel_l2

pytestmark = pytest.mark.gpu
SHAPE = (1, 1, 16, 32, 32)


def _inputs(rank):
    """rank 1 holds TWO volumes, rank 0 one: SyncBN must weight by the all-reduced counts."""
    g = torch.Generator().manual_seed(500 + rank)
    shape = (1 + rank,) + SHAPE[1:]
    x = torch.randn(*shape, generator=g)
    lungs = (torch.rand(*shape, generator=g) > 0.3).float()
    return x, lungs


def _loss(rank, dense, outs):
    if outs[0].dim() == 2:      # cls head: logits [B,6], [B,3]
        return (1.0 + rank) * outs[0][:, 1].sum() - 0.5 * outs[1][:, 2].sum() + 0.1 * (dense[0][:, 0] * dense[1][:, 1]).mean()
    return (1.0 + rank) * outs[0].sum() - 0.5 * outs[1].sum() + 0.1 * (dense[0] * dense[1]).mean()


def _build(factory):
    from bodyct_dram_emph_subtype_amd import med3d
    kw = dict(n_classes=[6, 3]) if factory.endswith("cls") else {}
    return getattr(med3d, factory)(**kw)


def _worker(rank, world, port, outdir, factory, storage="f32"):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bodyct_dram_emph_subtype_amd import distributed as ddist
        torch.manual_seed(21 + rank)            # different init per rank: attach() must broadcast rank 0's
        m = _build(factory).to("cuda:0").train()
        if storage == "bf16":
            m.storage_dtype = torch.bfloat16
        ctx = ddist.attach(m, bucket_bytes=8 << 20)
        x, lungs = _inputs(rank)
        dense, outs = m(x.cuda(), lungs.cuda())
        from bodyct_dram_emph_subtype_amd.engine import forward_decisions
        pins = {k: v.cpu() for k, v in forward_decisions(dense[0].grad_fn.saved_state).items()}
        _loss(rank, dense, outs).backward()
        torch.cuda.synchronize()
        # the large weight gradients autograd hands to p.grad ARE the arena views the kernels wrote and RCCL
        # reduced in place (no concatenation, no copy-out)
        lo, nb = ctx.last_arena
        in_arena = [lo <= p.grad.data_ptr() < lo + nb for n, p in m.named_parameters() if p.numel() >= ddist.SMALL_NUMEL]
        grads = {n: p.grad.cpu() for n, p in m.named_parameters()}
        stats = {k: v.cpu() for k, v in m.state_dict().items() if "running" in k}
        # results go through a file: passing torch tensors through mp.Queue hands over fds that
        # die with the worker process
        torch.save((rank, grads, stats, [o.detach().cpu() for o in outs], all(in_arena), dict(ctx.stats), pins),
                   os.path.join(outdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _run_ranks(procs, timeout=300):
    """Start the rank processes, wait, and ALWAYS reap them: a rank still alive after the timeout (or after a
    sibling failed) is terminated, then killed, so a hung rank cannot keep holding the GPU after the test
    has reported its failure."""
    try:
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout)
        codes = [p.exitcode for p in procs]
        assert all(c == 0 for c in codes), f"rank exit codes {codes} (None = still running after {timeout} s)"
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(10)
            if p.is_alive():
                p.kill()
                p.join(10)


@pytest.mark.parametrize("factory", ["resnet18segreg", "resnet50segcls"])
def test_two_rank_engine_matches_ddp_syncbn_emulation(factory):
    from oracle import med3d_oracle as orc
    import tempfile
    ctx = mp.get_context("spawn")
    port = 33500 + (os.getpid() % 2000) + (7 if factory.endswith("cls") else 0)
    with tempfile.TemporaryDirectory() as outdir:
        _run_ranks([ctx.Process(target=_worker, args=(r, 2, port, outdir, factory)) for r in range(2)])
        res = [torch.load(os.path.join(outdir, f"rank{r}.pt")) for r in range(2)]
    torch.manual_seed(21)                        # rank 0's initial weights
    sd = {k: v.clone() for k, v in _build(factory).state_dict().items()}
    xs, ls = zip(*[_inputs(r) for r in range(2)])
    # the oracle runs on the linear piece the two ranks' forwards took (their ReLU / max-pool decisions,
    # concatenated along the batch like the inputs), in fp64 (yardstick) and fp32 (the reference arithmetic)
    pins = {k: torch.cat([res[0][6][k], res[1][6][k]], 0) for k in res[0][6]}
    ref, _ = orc.ddp_emulated_grads(sd, list(xs), list(ls), factory, _loss, pins=pins, dtype=torch.float64)
    ref32, _ = orc.ddp_emulated_grads(sd, list(xs), list(ls), factory, _loss, pins=pins)
    ns = {}
    d, o = orc.forward(sd, torch.cat(xs), torch.cat(ls), factory, train=True, new_stats=ns)
    assert res[0][4] and res[1][4], "weight gradients were copied out of the arena"
    nbn = sum(1 for k in sd if k.endswith("running_mean"))
    assert res[0][5]["bn_allreduce"] == 2 * nbn, res[0][5]      # one statistic all-reduce per BN layer per direction
    g0, g1 = res[0][1], res[1][1]
    for n in ref:
        assert torch.equal(g0[n], g1[n]), f"ranks disagree on {n}"          # averaged gradients are identical
        if n.endswith(".0.bias") and n.startswith("us"):
            continue
        e, e32 = rel_l2(g0[n], ref[n]), rel_l2(ref32[n], ref[n])
        assert e <= min(max(1e-4, 3.0 * e32), 2e-3), f"{n}: 2-rank hip {e:.2e} vs decision-pinned fp64 emulation (cpu fp32 {e32:.2e})"
    worst = max((rel_l2(g0[n], ref[n]), n) for n in ref if not (n.endswith(".0.bias") and n.startswith("us")))
    print("worst 2-rank gradient rel-L2 vs decision-pinned DDP+SyncBN emulation:", worst)
    # SyncBN: both ranks track the statistics of the GLOBAL batch
    for k in ("bn1.running_mean", "layer4.1.bn2.running_var", "us3.1.running_var"):
        assert torch.equal(res[0][2][k], res[1][2][k])
        assert np.allclose(res[0][2][k].numpy(), ns[k].numpy(), rtol=1e-3, atol=1e-5), k
    # per-rank scores = the global-batch forward, sliced (rank 0: sample 0, rank 1: samples 1-2)
    off = 0
    for r in range(2):
        b = 1 + r
        for i in range(2):
            ref_o = o[i][off:off + b].detach()
            assert float((res[r][3][i] - ref_o).abs().max()) < 1e-3 * max(1.0, float(ref_o.abs().max()))
        off += b


def _nccl_world1(port, outdir):
    """One rank, backend nccl (= RCCL), collectives forced on: ReduceOp.AVG + async_op on arena ranges, float64
    statistic all-reduces (in-place, sync and async) and their stream ordering run for real on the one GPU
    of the test box; the result must equal the plain single-GPU step bit for bit (a 1-rank mean is the
    identity)."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from bodyct_dram_emph_subtype_amd import distributed as ddist
        out = {}
        for forced in (False, True, "torch"):
            # True: the context's OWN RCCL communicators (rccl.py: ncclAllReduce on the data stream / a forked bucket
            # stream); "torch": the same collectives through torch.distributed's ProcessGroupNCCL (A/B switch)
            os.environ["DRAM_DIST_TRANSPORT"] = "torch" if forced == "torch" else "rccl"
            torch.manual_seed(4)
            m = _build("resnet18segreg").to("cuda:0").train()
            ctx = ddist.attach(m, bucket_bytes=8 << 20, force=bool(forced))
            assert (m._dist is not None) == bool(forced)
            if forced:
                assert (ctx._stat is not None) == (forced is True) and ctx.capturable == (forced is True)
            x, lungs = _inputs(1)
            for _ in range(2):                       # two steps: the arena / state is rebuilt every backward
                m.zero_grad(set_to_none=True)
                dense, outs = m(x.cuda(), lungs.cuda())
                _loss(0, dense, outs).backward()
            torch.cuda.synchronize()
            out[forced] = ({n: p.grad.cpu() for n, p in m.named_parameters()},
                           {k: v.cpu() for k, v in m.state_dict().items() if "running" in k}, dict(ctx.stats))
        torch.save(out, os.path.join(outdir, "w1.pt"))
    finally:
        dist.destroy_process_group()


def test_rccl_world1_forced_collectives_equal_plain_step():
    import tempfile
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as outdir:
        _run_ranks([ctx.Process(target=_nccl_world1, args=(35500 + (os.getpid() % 2000), outdir))])
        out = torch.load(os.path.join(outdir, "w1.pt"))
    (g0, s0, st0) = out[False]
    assert st0["bn_allreduce"] == 0
    for mode in (True, "torch"):
        g1, s1, st1 = out[mode]
        assert st1["bn_allreduce"] == 2 * 2 * 22 and st1["grad_allreduce"] >= 2 * 2
        for n in g0:
            assert torch.equal(g0[n], g1[n]), (mode, n)
        for k in s0:
            assert torch.equal(s0[k], s1[k]), (mode, k)


def _nccl_world1_graph(port, outdir):
    """The data-parallel step captured into ONE hipGraph with its collectives (own RCCL communicators: plain stream
    work): three replays against three eager data-parallel steps and three plain steps, from the same state."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from bodyct_dram_emph_subtype_amd import distributed as ddist
        from bodyct_dram_emph_subtype_amd.graph import GraphedTrainStep
        from bodyct_dram_emph_subtype_amd.optim import FusedAdam
        x, lungs = _inputs(1)
        batch = (x.cuda(), lungs.cuda())
        out = {}
        for mode in ("plain", "dp-eager", "dp-graph"):
            for storage in (torch.float32, torch.bfloat16):
                torch.manual_seed(4)
                m = _build("resnet18segreg").to("cuda:0").train()
                m.storage_dtype = storage
                ctx = ddist.attach(m, bucket_bytes=8 << 20, force=(mode != "plain"))
                opt = FusedAdam(m.parameters(), lr=1e-3, capturable=True)

                def loss_fn(xx, ll, m=m):
                    dense, outs = m(xx, ll)
                    return _loss(0, dense, outs)

                def eager(*b, opt=opt, loss_fn=loss_fn):
                    opt.zero_grad(set_to_none=True)
                    loss = loss_fn(*b)
                    loss.backward()
                    opt.step()
                    return loss.detach()
                if mode == "dp-graph":
                    step = GraphedTrainStep(m, opt, loss_fn, batch, warmup=2)
                    assert step.graph is not None, "the data-parallel step was not captured"
                else:
                    eager(*batch); eager(*batch)
                    step = eager
                before = dict(ctx.stats)
                for _ in range(3):
                    loss = step(*batch).clone()
                torch.cuda.synchronize()
                out[(mode, str(storage))] = (float(loss), {k: v.cpu() for k, v in m.state_dict().items()}, before, dict(ctx.stats))
        torch.save(out, os.path.join(outdir, "w1g.pt"))
    finally:
        dist.destroy_process_group()


def test_rccl_world1_data_parallel_step_captured_in_a_hipgraph():
    import tempfile
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as outdir:
        _run_ranks([ctx.Process(target=_nccl_world1_graph, args=(35700 + (os.getpid() % 2000), outdir))])
        out = torch.load(os.path.join(outdir, "w1g.pt"))
    for storage in ("torch.float32", "torch.bfloat16"):
        lp, sp, _, _ = out[("plain", storage)]
        for mode in ("dp-eager", "dp-graph"):
            l, sd, st_before, st_after = out[(mode, storage)]
            assert l == lp, (mode, storage, l, lp)
            for k in sp:
                assert torch.equal(sd[k], sp[k]), (mode, storage, k)
            # eager steps issue their collectives every step; a replayed graph issues none from the host
            issued = st_after["bn_allreduce"] - st_before["bn_allreduce"]
            assert issued == (3 * 2 * 22 if mode == "dp-eager" else 0), (mode, issued)


def _nccl_worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    try:
        from bodyct_dram_emph_subtype_amd import distributed as ddist
        from bodyct_dram_emph_subtype_amd.engine import forward_decisions
        torch.manual_seed(21 + rank)
        m = _build("resnet18segreg").to(f"cuda:{rank}").train()
        ddist.attach(m, bucket_bytes=8 << 20)
        x, lungs = _inputs(rank)
        dense, outs = m(x.cuda(rank), lungs.cuda(rank))
        pins = {k: v.cpu() for k, v in forward_decisions(dense[0].grad_fn.saved_state).items()}
        _loss(rank, dense, outs).backward()
        torch.cuda.synchronize()
        torch.save((rank, {n: p.grad.cpu() for n, p in m.named_parameters()}, pins), os.path.join(outdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL wants one device per rank)")
def test_two_rank_rccl_matches_ddp_syncbn_emulation():
    """The same 2-rank parity check on the real transport: one GPU per rank, backend nccl (RCCL over xGMI).
    Skipped on one-GPU boxes; runs wherever the suite sees two devices."""
    from oracle import med3d_oracle as orc
    import tempfile
    ctx = mp.get_context("spawn")
    port = 36500 + (os.getpid() % 2000)
    with tempfile.TemporaryDirectory() as outdir:
        _run_ranks([ctx.Process(target=_nccl_worker, args=(r, 2, port, outdir)) for r in range(2)])
        res = [torch.load(os.path.join(outdir, f"rank{r}.pt")) for r in range(2)]
    torch.manual_seed(21)
    sd = {k: v.clone() for k, v in _build("resnet18segreg").state_dict().items()}
    xs, ls = zip(*[_inputs(r) for r in range(2)])
    pins = {k: torch.cat([res[0][2][k], res[1][2][k]], 0) for k in res[0][2]}
    ref, _ = orc.ddp_emulated_grads(sd, list(xs), list(ls), "resnet18segreg", _loss, pins=pins, dtype=torch.float64)
    for n in ref:
        assert torch.equal(res[0][1][n], res[1][1][n]), f"ranks disagree on {n}"
        if n.endswith(".0.bias") and n.startswith("us"):
            continue
        assert rel_l2(res[0][1][n], ref[n]) <= 2e-4, n


def test_bench_gpus2_self_launches_its_ranks():
    """`python bench.py --gpus 2` as a BARE command (no outer torch.distributed.run; the reference's `--ngpus N`
    alone starts N ranks, train.py:24,100-104): bench.py starts the two ranks itself as child processes and relays
    rank 0's JSON line.  Rehearsed here on one GPU with gloo + --share-gpu (control flow only, not a measurement)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--config", "0",
           "--backend", "gloo", "--share-gpu", "--timeline", "off", "--full"]
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd="/tmp")
    try:
        out, err = proc.communicate(timeout=420)
    finally:
        if proc.poll() is None:
            proc.kill()
            proc.communicate()
    assert proc.returncode == 0, err[-3000:]
    lines = out.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), out      # ONE JSON line and nothing else on stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 2 and rec["value"] > 0
    assert rec["collectives_per_step"]["bn_allreduce"] == 2 * 38          # ResNet-34: 38 BN layers, both directions


def test_bench_line_is_alone_on_stdout_with_rccl_up():
    """`python bench.py --force-dist` (RCCL communicators at world size 1): RCCL prints a version banner on rank 0's
    stdout when its first communicator comes up; the bench line must still be the ONE line of stdout (the driver parses
    it), and it carries the data-parallel fields and the host issue time."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    import socket
    with socket.socket() as sk:                       # a free port (a leftover run on the box must not fail the rendezvous)
        sk.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(sk.getsockname()[1])
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "0", "--steps", "2", "--warmup", "1", "--force-dist",
           "--no-cpu-baseline", "--timeline", "off", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 1 and rec["value"] > 0 and rec["host_issue_ms_per_step"] > 0
    # config 0 replays a hipGraph by default, data parallel too: the host issues the collectives of the two warm-up
    # steps and of the capture only (per-step counts are those of the eager second pass)
    assert rec["collective_transport"] == "rccl-c-api" and rec["config"]["hip_graph"] is True
    assert rec["collectives_per_step"]["bn_allreduce"] > 0
    assert abs(rec["exposed_collective_ms"] - (rec["ms_per_step"] - rec["plain_ms_per_step"])) < 1e-6
    assert rec["stat_exchange_ms_bracketed"] >= 0


def test_default_bench_line_says_how_the_step_was_timed():
    """The line the driver records (`python bench.py`, config 1, fp32): a probe of untimed eager steps decides between the
    eager two-stream step and the replay of its hipGraph capture (a host that cannot keep ahead of the GPU) -- the line
    must say which and on what measurement, and --graph / --no-graph must override the probe."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "0", "--no-cpu-baseline", "--timeline", "off"]
    r = subprocess.run(base, env=env, capture_output=True, text=True, timeout=420, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    cfg = rec["config"]
    assert rec["dtype"] == "f32" and rec["n_gpus"] == 1 and rec["value"] > 0
    assert cfg["graph_choice"].startswith("auto: the host issued 4 untimed eager steps")
    assert cfg["graph_choice"].endswith("hipGraph replay" if cfg["hip_graph"] else "eager two-stream step")
    r = subprocess.run(base + ["--graph"], env=env, capture_output=True, text=True, timeout=420, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    cfg = json.loads(r.stdout.splitlines()[0])["config"]
    assert cfg["hip_graph"] is True and cfg["graph_choice"] is None and cfg["streams"] == 1
    # the fp32 data-parallel step over RCCL takes the same probe (agreed over the ranks) and says so
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        env = dict(env, MASTER_PORT=str(sk.getsockname()[1]))
    r = subprocess.run(base + ["--force-dist", "--full"], env=env, capture_output=True, text=True, timeout=420, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.splitlines()[0])
    cfg = rec["config"]
    assert rec["collective_transport"] == "rccl-c-api" and rec["plain_ms_per_step"] > 0
    assert cfg["graph_choice"].startswith("auto: the host issued 4 untimed eager steps")
    assert cfg["graph_choice"].endswith("hipGraph replay" if cfg["hip_graph"] else "eager two-stream step")


def test_plain_bench_line_is_lean_and_dumps_the_last_step():
    """A plain `python bench.py` measures the headline only (the CPU baseline and the roofline pass come with --full), and
    --dump-outputs DIR writes what the last timed step computed: float32 .npy files, <= 64 MB, whose loss is the line's."""
    import json
    import subprocess
    import tempfile
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    with tempfile.TemporaryDirectory() as d:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "0", "--steps", "3", "--warmup", "1",
               "--dump-outputs", d]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420, cwd="/tmp")
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == 1, r.stdout
        rec = json.loads(lines[0])
        assert "cpu_baseline" not in rec and "roofline" not in rec
        assert rec["steps"] == 3 and rec["unit"] == "volumes/sec" and rec["higher_is_better"] is True
        assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) < 1e-6 * rec["value"]        # config 0: batch 1
        arrays = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert {"loss", "dense_cle", "dense_pse", "out_cle", "out_pse", "params", "grads", "buffers"} <= set(arrays)
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["out_cle"].shape == (1, 6) and arrays["out_pse"].shape == (1, 3)
    assert abs(float(arrays["loss"][0]) - rec["loss"]) <= 1e-6 * max(1.0, abs(rec["loss"]))
    assert np.isfinite(arrays["grads"]).all() and np.abs(arrays["grads"]).max() > 0


def test_two_rank_bf16_storage_matches_ddp_syncbn_emulation():
    """The data-parallel path on bf16 activations (BASELINE configs[3] / [4] ask for bf16 + DDP): two ranks (1 + 2 volumes,
    gloo on device tensors) against the fp64 DDP + SyncBN emulation on the ranks' own decisions.  SyncBN statistics and
    the gradient arena are fp32 / double on both storage paths, so the only new error is the bf16 rounding of the
    activations: per-tensor relative L2 <= 1e-1 (as in tests/test_bf16_gpu.py), ranks bit-identical to each other."""
    from oracle import med3d_oracle as orc
    import tempfile
    factory = "resnet18segreg"
    ctx = mp.get_context("spawn")
    port = 37500 + (os.getpid() % 2000)
    with tempfile.TemporaryDirectory() as outdir:
        _run_ranks([ctx.Process(target=_worker, args=(r, 2, port, outdir, factory, "bf16")) for r in range(2)])
        res = [torch.load(os.path.join(outdir, f"rank{r}.pt")) for r in range(2)]
    torch.manual_seed(21)
    sd = {k: v.clone() for k, v in _build(factory).state_dict().items()}
    xs, ls = zip(*[_inputs(r) for r in range(2)])
    pins = {k: torch.cat([res[0][6][k], res[1][6][k]], 0) for k in res[0][6]}
    ref, _ = orc.ddp_emulated_grads(sd, list(xs), list(ls), factory, _loss, pins=pins, dtype=torch.float64)
    worst = (0.0, "")
    for n in ref:
        assert torch.equal(res[0][1][n], res[1][1][n]), f"ranks disagree on {n}"
        if n.endswith(".0.bias") and n.startswith("us"):
            continue
        e = rel_l2(res[0][1][n], ref[n])
        worst = max(worst, (e, n))
        assert e <= 1e-1, f"{n}: {e:.2e}"
    print(f"[2 ranks, bf16 storage] worst gradient vs decision-pinned fp64 DDP+SyncBN emulation: {worst}")
