"""Cost of transforms.prepare_case (csrc/case_prep.hip) on a synthetic two-lung lobes volume, D x 512 x 512 with
D = 300 and 600, uint8 lobes, int16 scan, spacing (0.7, 0.7, 0.7), border 5, two dilations:

  kernels   dram_lung_bbox (partial rows + fold) and dram_case_prepare, each between two HIP events, and the bytes each
            has to move (bbox: the lobes once; prepare: per crop voxel 2 B scan + 1 B lobes in, 2 + 1 + 1 B out) over
            its median time, against the 6.3 TB/s DESIGN.md section 6 calls achievable;
  call      the whole prepare_case call, host clock, device synchronised before and after (it holds the one read-back);
  readback  the box.tolist() of an already computed box (the host round trip alone);
  torch     the same work composed from torch ops on the same GPU, as a user would otherwise write it: nonzero-based
            bounding box (one read-back as well), max_pool3d(lung, 5, 1, 2) > 0, where, crops, the two masks.

  python tools/case_prep_bench.py [--reps 20] [--out FILE]
Warm (3 unrecorded rounds); ours and torch run interleaved, round by round; medians over --reps.
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 6.3
SPACING, BORDER, R, FILL, THR = (0.7, 0.7, 0.7), 5, 2, -2048, -910


def two_lungs(D, H, W, dev):
    z = torch.arange(D, device=dev).view(D, 1, 1).float()
    y = torch.arange(H, device=dev).view(1, H, 1).float()
    x = torch.arange(W, device=dev).view(1, 1, W).float()
    lobes = torch.zeros((D, H, W), dtype=torch.uint8, device=dev)
    for label, cx in ((1, 0.30 * W), (4, 0.70 * W)):
        inside = ((z - 0.5 * D) / (0.40 * D)) ** 2 + ((y - 0.5 * H) / (0.30 * H)) ** 2 + ((x - cx) / (0.16 * W)) ** 2 < 1
        lobes[inside] = label
    return lobes


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def torch_case(scan, lobes):
    lung = lobes > 0
    nz = lung.nonzero()
    lo, hi = nz.min(0).values.tolist(), (nz.max(0).values + 1).tolist()          # the read-back
    pads = [int(math.ceil(BORDER / s)) for s in SPACING]
    idx = tuple(slice(max(0, a - p), min(n, b + p)) for a, b, p, n in zip(lo, hi, pads, lung.shape))
    dl = F.max_pool3d(lung[None, None].half(), 2 * R + 1, 1, R)[0, 0] > 0
    image = torch.where(dl, scan, torch.tensor(FILL, dtype=torch.int16, device=scan.device))[idx].contiguous()
    lung_c = lung[idx].contiguous()
    return {"image": image, "lung_mask": lung_c, "ess_mask": (image < THR) & lung_c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--depths", type=int, nargs="+", default=[300, 600])
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import ops, transforms
    dram.load_library()
    dev = "cuda:0"
    L, p = ops._L(), ops._p
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for D in args.depths:
        H = W = 512
        n = D * H * W
        lobes = two_lungs(D, H, W, dev)
        scan = torch.randint(-1100, 200, (D, H, W), device=dev, dtype=torch.int16)
        case = transforms.prepare_case(scan, lobes, SPACING, BORDER, R, FILL, THR)
        ref = torch_case(scan, lobes)
        same = all(torch.equal(case[k], ref[k]) for k in ref)
        (z0, z1), (y0, y1), (x0, x1) = case["crop_slice"].tolist()
        crop = (z1 - z0, y1 - y0, x1 - x0)
        vox = crop[0] * crop[1] * crop[2]
        say(f"{D}x{H}x{W}: lung {int(case['lung_mask'].sum()) / n:.1%} of the volume, crop {crop}, equal to the torch composition: {same}; "
            f"medians of {args.reps} (3 warm-up rounds)")
        partial = torch.empty((L.dram_lung_bbox_nblk(n), 8), device=dev, dtype=torch.int32)
        box = torch.empty((8,), device=dev, dtype=torch.int32)
        image, lung, ess = (torch.empty(crop, device=dev, dtype=dt) for dt in (torch.int16, torch.uint8, torch.uint8))
        st = ops._stream

        def k_bbox():
            ops._chk(L.dram_lung_bbox(p(lobes), 1, p(partial), p(box), D, H, W, st()), "dram_lung_bbox")

        def k_prep():
            ops._chk(L.dram_case_prepare(p(scan), p(lobes), 1, p(image), p(lung), p(ess), None, D, H, W, z0, y0, x0, *crop, R,
                                         FILL, THR, st()), "dram_case_prepare")

        ms = {k: [] for k in ("bbox", "prepare", "call", "readback", "torch")}
        for r in range(3 + args.reps):
            t = {"bbox": events(k_bbox), "prepare": events(k_prep),
                 "call": wall(lambda: transforms.prepare_case(scan, lobes, SPACING, BORDER, R, FILL, THR)),
                 "readback": wall(box.tolist), "torch": wall(lambda: torch_case(scan, lobes))}
            if r >= 3:
                for k, v in t.items():
                    ms[k].append(v)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, nbytes in (("bbox", n), ("prepare", 7 * vox)):
            tbs = nbytes / (1e-3 * med[k]) / 1e12
            say(f"  {k:8s} kernel {med[k]:.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f}); moves {nbytes / 1e6:.0f} MB -> "
                f"{tbs:.2f} TB/s = {100 * tbs / HBM_TBS:.0f} % of {HBM_TBS} TB/s")
        say(f"  prepare_case call {med['call']:.3f} ms (min {min(ms['call']):.3f}); host read-back of the box alone "
            f"{med['readback']:.3f} ms; torch composition {med['torch']:.3f} ms (min {min(ms['torch']):.3f})  x{med['torch'] / med['call']:.1f}")
        del lobes, scan, case, ref, image, lung, ess
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
