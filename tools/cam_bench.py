"""Cost of the fused class-activation maps (ops.cam) against the composition they replace, on config 1's target-layer
grid: A [2,64,128,128,32] (the us3 output), the reg head (NO = 2, sigmoid, 2x lung mask) and the cls head (NO = 9).

  fused     ops.cam(A, w, bias, gdense=None, gpool, lungs, sigmoid, method)      G never stored
  unfused   ops.head_bwd (writes the 32-channel G, plus the weight-gradient partials nobody wants) followed by the
            torch passes: gradcam  relu((G.mean over voxels * A).sum(channels));  hirescam  relu((G * A).sum);
            layercam  relu((relu(G) * A).sum)
and, for the fused call, the bytes the method has to move (A once per pass over it, the 4-B map, 1/8 of the mask per
voxel) over its median time, against the 6.3 TB/s DESIGN.md section 6 calls achievable.  With --forward: the median
time of a no-grad forward at config 1 (resnet18segcls, fp32) and config 2 (resnet18segreg, bf16 storage), 2x1x128x256x256,
and the fused call's share of it.

  python tools/cam_bench.py [--reps 30] [--forward] [--out FILE]
Warm (5 unrecorded rounds); fused and unfused run interleaved, round by round, each between two HIP events with the
device synchronised before it; medians over --reps.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 6.3
METHODS = ("gradcam", "hirescam", "layercam")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", type=int, nargs=4, default=[2, 64, 128, 128], help="B D H W of the target-layer grid")
    ap.add_argument("--forward", action="store_true", help="also time the no-grad forwards of configs 1 and 2")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import med3d, ops
    dram.load_library()
    dev = "cuda:0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, D, H, W = args.shape
    V = D * H * W
    g = torch.Generator(device=dev).manual_seed(0)
    fused_ms = {}
    say(f"target-layer grid {B}x{D}x{H}x{W}x32, medians of {args.reps} (5 warm-up rounds)")
    for dt, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        A = torch.randn(B, D, H, W, 32, device=dev, generator=g).relu().to(dt)
        for head, NO, sig in (("reg", 2, True), ("cls", 9, False)):
            w = 0.3 * torch.randn(NO, 32, device=dev, generator=g)
            bias = 0.2 * torch.randn(NO, device=dev, generator=g)
            gpool = torch.randn(B, NO, device=dev, generator=g) / V
            lungs = (torch.rand(B, 2 * D, 2 * H, 2 * W, device=dev, generator=g) > 0.3).float() if sig else None
            with ops.launch_scope(dev):
                dense = ops.head_fwd(A, w, bias, lungs, sig)[0] if sig else None     # (the forward's output; not timed)
            for method in METHODS:
                def fused():
                    with ops.launch_scope(dev):
                        return ops.cam(A, w, bias, None, gpool, lungs, sig, method, True)

                def unfused():
                    with ops.launch_scope(dev):
                        G = ops.head_bwd(A, w, dense, None, gpool, lungs, sig)[0].float()
                    Af = A.float()
                    if method == "gradcam":
                        m = (G.mean((1, 2, 3), keepdim=True) * Af).sum(-1)
                    elif method == "hirescam":
                        m = (G * Af).sum(-1)
                    else:
                        m = (G.relu() * Af).sum(-1)
                    return m.relu()

                ms = {"fused": [], "unfused": []}
                for r in range(5 + args.reps):
                    tf, tu = timed(fused), timed(unfused)
                    if r >= 5:
                        ms["fused"].append(tf)
                        ms["unfused"].append(tu)
                mf, mu = statistics.median(ms["fused"]), statistics.median(ms["unfused"])
                passes = 1 if method != "gradcam" else (2 if sig else 1)      # (the sum pass reads A only under the sigmoid)
                nbytes = B * V * (passes * 32 * A.element_size() + 4 + (0.5 * passes if sig else 0))
                fused_ms[(dname, head, method)] = mf
                say(f"  {dname} {head} (NO={NO}) {method:9s} fused {mf:.3f} ms (min {min(ms['fused']):.3f}, max {max(ms['fused']):.3f})"
                    f"  unfused {mu:.3f} ms (min {min(ms['unfused']):.3f})  x{mu / mf:.1f};  fused moves {nbytes / 1e6:.0f} MB -> "
                    f"{nbytes / (1e-3 * mf) / 1e12:.2f} TB/s = {100 * nbytes / (1e-3 * mf) / 1e12 / HBM_TBS:.0f} % of {HBM_TBS} TB/s")
        del A
    if args.forward:
        x = torch.randn(2, 1, 2 * D, 2 * H, 2 * W, device=dev, generator=g)
        lungs = (torch.rand(2, 1, 2 * D, 2 * H, 2 * W, device=dev, generator=g) > 0.3).float()
        for cfg, factory, dt, dname, head in ((1, "resnet18segcls", torch.float32, "fp32", "cls"),
                                              (2, "resnet18segreg", torch.bfloat16, "bf16", "reg")):
            torch.manual_seed(0)
            m = getattr(med3d, factory)().to(dev).eval()
            m.storage_dtype = dt

            def fwd():
                with torch.no_grad():
                    m(x, lungs)

            v = [timed(fwd) for r in range(3 + 10)][3:]
            mfwd = statistics.median(v)
            say(f"  no-grad forward, config {cfg} ({factory}, {dname} storage, 2x1x{2 * D}x{2 * H}x{2 * W}): median {mfwd:.2f} ms "
                f"(min {min(v):.2f}, n {len(v)}); the fused {head} call's share: "
                + ", ".join(f"{k} {100 * fused_ms[(dname, head, k)] / mfwd:.2f} %" for k in METHODS))
            del m
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
