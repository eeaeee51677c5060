"""Cost of fused gradient clipping: the optimizer step alone, on synthetic gradients with a network's parameter shapes.

  1. FusedAdam                                                    (no clipping)
  2. FusedAdam(max_grad_norm=1)                                   (norm launch + clipped update; no gradient rewritten)
  3. torch.nn.utils.clip_grad_norm_ + FusedAdam                   (what a user had to write before)
and, from the library's kernel timeline, the norm launch on its own: time, the algorithmic bytes it books, and the
bandwidth against the exact 4 B x parameters.

  python tools/grad_clip_bench.py [--factories resnet18segreg resnet50segreg] [--reps 30] [--out FILE]
Warm (5 unrecorded rounds); the three forms run interleaved, round by round, each step between two HIP events on the
stream with the host kept ahead of the GPU by nothing (synchronised before every step: the step is host-issued work of
tens of microseconds plus kernels of 0.1-1 ms, and a queue left over from the previous form would be billed to the
next); medians over --reps.  The gradients keep their addresses, so the optimizers' work lists are uploaded once.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factories", nargs="+", default=["resnet18segreg", "resnet50segreg"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import med3d, ops
    from bodyct_dram_emph_subtype_amd.optim import FusedAdam
    dram.load_library()
    dev = "cuda:0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for factory in args.factories:
        shapes = [tuple(p.shape) for p in getattr(med3d, factory)().parameters()]
        nparam = sum(int(torch.Size(s).numel()) for s in shapes)
        g = torch.Generator(device=dev).manual_seed(0)

        def make(**kw):
            ps = [torch.randn(s, device=dev, generator=g).requires_grad_(True) for s in shapes]
            for p in ps:
                p.grad = torch.randn(p.shape, device=dev, generator=g)
            return ps, FusedAdam(ps, lr=1e-4, **kw)

        (p0, o0), (p1, o1), (p2, o2) = make(), make(max_grad_norm=1.0), make()

        def plain():
            o0.step()

        def fused():
            o1.step()

        def torch_clip():
            torch.nn.utils.clip_grad_norm_(p2, 1.0)
            o2.step()

        forms = (("FusedAdam", plain), ("FusedAdam(max_grad_norm=1)", fused), ("torch clip_grad_norm_ + FusedAdam", torch_clip))
        ms = {name: [] for name, _ in forms}
        for r in range(5 + args.reps):
            for name, fn in forms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if r >= 5:
                    ms[name].append(a.elapsed_time(b))
        say(f"{factory}: {len(shapes)} tensors, {nparam} parameters ({4e-6 * nparam:.1f} MB of gradients)")
        for name, _ in forms:
            v = ms[name]
            say(f"  {name:36s} median {statistics.median(v):.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)})")
        # the norm launch alone, from the library's timeline (sum-of-squares kernel + one-block fold in one record)
        t, c, n = o1._cache
        tl = ops.KernelTimeline()
        rows = []
        for r in range(5 + args.reps):
            tl.start()
            try:
                with ops.launch_scope(dev):
                    ops.grad_norm_multi(t, c, n, o1._partials, o1._clip, 1.0)
                fam = tl.families()["optim"]
            finally:
                tl.stop()
            if r >= 5:
                rows.append((fam["ms"], fam["hbm_bytes"]))
        t_ms = statistics.median(r[0] for r in rows)
        say(f"  dram_grad_norm_multi alone           median {t_ms:.4f} ms  (min {min(r[0] for r in rows):.4f}); timeline books "
            f"{rows[0][1] / 1e6:.1f} MB ({n} chunks), exact 4 B x parameters = {4e-6 * nparam:.1f} MB -> "
            f"{4e-9 * nparam / (1e-3 * t_ms) / 1e3:.2f} TB/s")
        del p0, p1, p2, o0, o1, o2
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
