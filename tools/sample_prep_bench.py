"""Device time of one training sample's preparation from an archive case: ``transforms.prepare_archive_sample`` on the
int16 data (csrc/sample_prep.hip: one integer statistics pass + one fused output pass) against the composition it
replaces -- ``prepare_image(scan)``, ``prepare_mask`` of the lung mask and of the torch-made em_mask, each through a
float32 copy of the full-size volume.  Default case: 400 x 512 x 512 int16 scan + uint8 lung mask -> (128, 224, 288).

  python tools/sample_prep_bench.py [--source 400 512 512] [--target 128 224 288] [--seconds 1.0] [--out FILE]

Both forms run in ONE process on the same tensors, alternating call by call after 3 warm-up rounds; every call sits
between two device events (the span holds the call's host glue wherever the device waits for it, as a training loop
would see it), repeated until each form has filled --seconds (at least 10 calls).  Reported per form: median, min, max
and the interquartile range; then the two kernels alone between events, with the bytes each has to move.  The counted
bytes per source voxel of both forms are printed next to the times.  Needs a GPU: there is no fallback.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(v):
    q = statistics.quantiles(v, n=4)
    return f"median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}, IQR {q[2] - q[0]:.3f}, n = {len(v)}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", type=int, nargs=3, default=[400, 512, 512])
    ap.add_argument("--target", type=int, nargs=3, default=[128, 224, 288])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_prep_bench measures on the GPU; none is visible")
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import ops, transforms as T
    dram.load_library()
    dev = "cuda:0"
    src, tgt = tuple(args.source), tuple(args.target)
    n, m = src[0] * src[1] * src[2], tgt[0] * tgt[1] * tgt[2]
    g = torch.Generator(device=dev).manual_seed(0)
    scan = torch.randint(-1300, 100, src, device=dev, dtype=torch.int16, generator=g)
    z = torch.arange(src[0], device=dev).view(-1, 1, 1).float() / src[0] - 0.5
    y = torch.arange(src[1], device=dev).view(1, -1, 1).float() / src[1] - 0.5
    x = torch.arange(src[2], device=dev).view(1, 1, -1).float() / src[2] - 0.5
    lung = ((z / 0.42) ** 2 + (y / 0.33) ** 2 + (x / 0.40) ** 2 < 1).to(torch.uint8)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fused():
        return T.prepare_archive_sample(scan, lung, tgt)

    def composition():                  # what a caller composed before: three float32 copies of the full-size volume
        lm = lung > 0
        return {"image": T.prepare_image(scan, tgt), "lung_mask": T.prepare_mask(lm, tgt),
                "em_mask": T.prepare_mask((scan < -950) & lm, tgt)}

    a, b = fused(), composition()
    same = torch.equal(a["lung_mask"], b["lung_mask"]) and torch.equal(a["em_mask"], b["em_mask"])
    diff = float((a["image"] - b["image"]).abs().max())
    say(f"{src} int16 + uint8 lung mask -> {tgt}: masks equal to the composition's: {same}; image max |fused - composition| "
        f"= {diff:.3e} (exact statistics against fp32-accumulated ones)")
    del a, b
    ms = {"fused": [], "composition": []}
    for _ in range(3):
        events(fused), events(composition)
    while min(sum(v) for v in ms.values()) < 1e3 * args.seconds or min(len(v) for v in ms.values()) < 10:
        ms["fused"].append(events(fused))
        ms["composition"].append(events(composition))
    for k, v in ms.items():
        say(f"  {k:12s} {spread(v)}")
    mf, mc = statistics.median(ms["fused"]), statistics.median(ms["composition"])
    say(f"  composition / fused = {mc / mf:.2f} (medians)")

    # the two kernels alone
    L, p, st = ops._L(), ops._p, ops._stream
    partial = torch.empty((L.dram_sample_stats_nblk(n), 2), device=dev, dtype=torch.int64)
    zidx = T.depth_indices(src[0], tgt[0], dev)
    mi = torch.tensor([0.4, 3.0], device=dev)
    oi = torch.empty(tgt, device=dev)
    ol, oe = torch.empty(tgt, device=dev, dtype=torch.uint8), torch.empty(tgt, device=dev, dtype=torch.uint8)

    def k_stats():
        ops._chk(L.dram_sample_stats_i16(p(scan), p(partial), n, -1150, -300, st()), "dram_sample_stats_i16")

    def k_prep():
        ops._chk(L.dram_prep_sample_i16(p(scan), p(lung), 1, p(zidx), p(mi), p(oi), p(ol), p(oe), *src, *tgt, -1150, -300,
                                        -950, st()), "dram_prep_sample_i16")

    planes = tgt[0] * src[1] * src[2]
    for name, fn, nbytes, what in (("stats", k_stats, 2 * n, "the scan once"),
                                   ("prep", k_prep, 3 * planes + 6 * m, "the selected planes of scan and mask at most, "
                                                                        "6 B per output voxel")):
        for _ in range(3):
            events(fn)
        v = [events(fn) for _ in range(20)]
        say(f"  {name:5s} kernel {spread(v)}; moves {nbytes / 1e6:.0f} MB ({what}) -> "
            f"{nbytes / (1e-3 * statistics.median(v)) / 1e12:.2f} TB/s")
    say(f"  counted HBM bytes per SOURCE voxel: fused 2 (statistics) + <= 3 D_out/D (output pass reads) + 6 per OUTPUT voxel; "
        f"composition 3 x (read + 4 B float32 copy written) + 4 (statistics) + torch em_mask passes, >= 12 B of float32 "
        f"temporaries in flight; here {n} source and {m} output voxels")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
