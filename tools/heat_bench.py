"""Cost of the activation-map volumes (csrc/heat.hip) for both classification heads of one dense tensor
[2,9,64,128,128] (scan grid 128 x 256 x 256), lung a centred ellipsoid:

  full      models.heat_volumes(..., head="cls"): per head the peak pass, the amax glue and the write pass (uint8)
  slices    the same with zsel = 5 slices per sample (what draw_predictions runs)
  torch     the same uint8 volumes composed from torch ops on the same GPU, as the reference does it:
            F.interpolate(trilinear) -> relu -> channel sum -> / (amax + 1e-7) -> * lung -> clamp * 255 -> uint8

  python tools/heat_bench.py [--reps 15] [--out FILE]       device events, warm (3 unrecorded rounds), interleaved
  python tools/heat_bench.py --kernels-only                 a few rounds of `full` and `slices` alone, for a kernel
                                                            trace (rocprofv3 --kernel-trace --stats -- python ...)
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def torch_heat(dense_outs, lung):
    out = {}
    for name, d in zip(("cle", "pse"), dense_outs):
        up = F.interpolate(d, size=lung.shape[-3:], mode="trilinear")
        dp = F.relu(up[:, 1:]).sum(1)
        v = dp / (dp.amax(dim=(1, 2, 3), keepdim=True) + 1e-7) * lung
        out[name] = (v.clamp(0, 1) * 255).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--grid", type=int, nargs=3, default=[64, 128, 128])
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import models
    dram.load_library()
    dev = "cuda:0"
    B, (d, h, w) = 2, args.grid
    D, H, W = 2 * d, 2 * h, 2 * w
    g = torch.Generator(device=dev).manual_seed(0)
    dense = torch.randn(B, 9, d, h, w, device=dev, generator=g)
    heads = [dense[:, :6], dense[:, 6:]]
    z, y, x = ((torch.arange(n, device=dev).float() - (n - 1) / 2) / (0.4 * n) for n in (D, H, W))
    lung = ((z[:, None, None] ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2) <= 1.0)[None].expand(B, D, H, W).contiguous()
    lung_f = lung.float()
    zsel = [models.panel_slices(int(0.1 * D), int(0.9 * D), D)] * B
    runs = {"full": lambda: models.heat_volumes(heads, lung, "cls"),
            "slices": lambda: models.heat_volumes(heads, lung, "cls", zsel=zsel)}
    if args.kernels_only:
        for _ in range(5):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        return
    runs["torch"] = lambda: torch_heat(heads, lung_f)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ms = {k: [] for k in runs}
    for r in range(3 + args.reps):
        outs = {}
        for k, fn in runs.items():
            t, outs[k] = events(fn)
            if r >= 3:
                ms[k].append(t)
    diff = {n: (outs["full"][n].int() - outs["torch"][n].int()).abs() for n in ("cle", "pse")}
    same = all(torch.equal(outs["slices"][n][b], outs["full"][n][b, zsel[b]]) for n in diff for b in range(B))
    say(f"dense [{B},9,{d},{h},{w}] -> two uint8 volumes [{B},{D},{H},{W}]; medians of {args.reps} (3 warm-up rounds), device events")
    say(f"  bytes differing from the torch composition: " + ", ".join(
        f"{n} {int((v > 0).sum())} of {v.numel()} (largest step {int(v.max())})" for n, v in diff.items())
        + f"; slices equal the full volume's: {same}")
    out_bytes = 2 * B * D * H * W
    for k in runs:
        m = statistics.median(ms[k])
        say(f"  {k:7s} {m:8.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})"
            + (f"  x{statistics.median(ms['torch']) / m:.1f} under torch" if k != "torch" else "")
            + (f"; writes {out_bytes / 1e6:.0f} MB, reads the {B * 7 * d * h * w * 4 / 1e6:.0f} MB of the 5 + 2 class "
               f"channels in each of the two passes and {B * D * H * W / 1e6:.0f} MB lung per head" if k == "full" else ""))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
