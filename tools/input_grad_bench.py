"""Timing of the input-gradient path with the library's kernel timeline ("input gradient").

  1. the stem data gradient (scatter GEMM + fold) against stem_fwd_kernel, same shape, same process
  2. model.input_gradient in eval mode against a full training forward + backward (wall clock around
     synchronised steps, and the sum of the timeline's kernel times)

  python tools/input_grad_bench.py [--shape 2 128 256 256] [--factory resnet18segcls] [--reps 15]
Warm (3 unrecorded runs), medians over --reps; one line per figure on stdout.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[2, 128, 256, 256])
    ap.add_argument("--factory", default="resnet18segcls")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--skip-network", action="store_true")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import med3d, ops
    dram.load_library()
    dev = "cuda:0"
    B, D, H, W = args.shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, D, H, W, generator=g).to(dev)
    w = (0.1 * torch.randn(64, 1, 7, 7, 7, generator=g)).to(dev)
    tl = ops.KernelTimeline()

    def variants(fn):
        tl.start()
        try:
            fn()
            fam = tl.families()
        finally:
            tl.stop()
        return fam

    with ops.launch_scope(dev):
        y, _ = ops.stem_fwd(x, w, False)
        dy = torch.randn(y.shape, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        for dt in (torch.float32, torch.bfloat16):
            dyt = dy.to(dt)
            rows = []
            for r in range(3 + args.reps):
                def both():
                    ops.stem_fwd(x, w, False)
                    ops.stem_bwd_data(dyt, w, (B, D, H, W))
                v = variants(both)["stem"]["variants"]
                if r >= 3:
                    rows.append((v[0][1], v[4][1], v[5][1]))
            fwd, sc, fold = (statistics.median(c) for c in zip(*rows))
            print(f"stem {B}x{D}x{H}x{W} dy={str(dt)[6:]}: stem_fwd_kernel {fwd:.3f} ms | stem_dgrad_kernel {sc:.3f} ms + "
                  f"fold {fold:.3f} ms = {sc + fold:.3f} ms ({(sc + fold) / fwd:.2f} x forward)  "
                  f"[min fwd {min(r[0] for r in rows):.3f}, min dgrad {min(r[1] + r[2] for r in rows):.3f}]", flush=True)
    if args.skip_network:
        return
    del y, dy, dyt
    torch.manual_seed(0)
    kw = dict(n_classes=[6, 3]) if args.factory.endswith("cls") else {}
    m = getattr(med3d, args.factory)(**kw).to(dev)
    x5 = x.reshape(B, 1, D, H, W)
    lungs = (torch.rand(B, 1, D, H, W, device=dev) > 0.3).float()

    def cot(outs):
        return [torch.ones_like(o) for o in outs]

    def train_step():
        m.train()
        m.zero_grad(set_to_none=True)
        dense, outs = m(x5, lungs)
        (outs[0].sum() + outs[1].sum()).backward()

    def attribution():
        m.eval()
        with torch.no_grad():
            outs = m(x5, lungs)[1]
        return m.input_gradient(x5, lungs, out_grads=cot(outs))

    def attribution_only():
        return m.input_gradient(x5, lungs, out_grads=ones)

    m.eval()
    with torch.no_grad():
        ones = cot(m(x5, lungs)[1])
    for name, fn in (("training forward + backward", train_step), ("input_gradient (eval)", attribution_only)):
        if name.startswith("input"):
            m.eval()
        wall, kern = [], []
        for r in range(3 + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fam = variants(fn)
            if r >= 3:
                wall.append(1e3 * (t1 - t0))
                kern.append(sum(d["ms"] for d in fam.values()))
        print(f"{args.factory} {B}x1x{D}x{H}x{W} {name}: wall {statistics.median(wall):.2f} ms (min {min(wall):.2f}), "
              f"sum of kernel times {statistics.median(kern):.2f} ms", flush=True)


if __name__ == "__main__":
    main()
