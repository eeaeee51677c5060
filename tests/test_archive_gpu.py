"""GPU: the fused int16 sample preparation (csrc/sample_prep.hip, transforms.prepare_archive_sample) and training from
a scan archive end to end.

The statistics are compared with Python-integer sums (equality); the masks with the reference composition of
tests/data_path_ref.py and with ``prepare_mask`` on the device (equality); the image with ``prep_image64``'s own
element-wise bound, which budgets statistics accumulated in fp32 -- exact statistics sit further inside it.  Every
output voxel of every case is compared."""
import ctypes
import functools
import logging
import math
import os
import re

import pytest
import torch

import data_path_ref as R
from archive_ref import write_archive, write_split

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LO, HI = -1150, -300
EDGE_VALUES = [-32768, 32767, -2048, LO, HI, LO - 1, LO + 1, HI - 1, HI + 1, 0, -725]


def T():
    from bodyct_dram_emph_subtype_amd import transforms
    return transforms


def lib():
    from bodyct_dram_emph_subtype_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ statistics
def stats_values(n, seed):
    """int16 values over the whole range with the edge values spread through them"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-1500, 200, (n,), generator=g).to(torch.int16)
    far = torch.randint(-32768, 32768, (n,), generator=g).to(torch.int16)
    v = torch.where(torch.rand(n, generator=g) < 0.1, far, v)
    for k, e in enumerate(EDGE_VALUES):
        v[(k * 7919) % n] = e                 # (n >= 2: small n keep the last ones written)
    if n >= 2:
        v[0], v[n - 1] = -32768, 32767
    return v


def int_sums(values, lo, hi):
    c = [min(max(int(x), lo), hi) - lo for x in values.tolist()]
    return sum(c), sum(x * x for x in c)


MULTI = 5 * 8192 + 3            # six blocks of the statistics kernel, not a multiple of 8


@pytest.mark.parametrize("n", [2, 7, 8, 9, 255, 4097, MULTI])
def test_window_sums_are_exact(n):
    host = stats_values(n, 100 + n)
    want = int_sums(host, LO, HI)
    for offset in (0, 1) if n != 4097 else (0, 1, 2, 3, 5, 7):
        buf = torch.zeros(n + 16, dtype=torch.int16, device=DEV)
        buf.fill_(12345)                      # anything read outside the view would show in the sums
        view = buf[offset:offset + n]
        view.copy_(host)
        assert view.data_ptr() % 16 == (2 * offset) % 16
        p1 = T().sample_window_sums(view, (LO, HI))
        p2 = T().sample_window_sums(view, (LO, HI))
        assert p1.dtype == torch.int64 and tuple(p1.shape) == (lib().dram_sample_stats_nblk(n), 2)
        assert torch.equal(p1, p2)                                   # bit-identical from call to call
        got = tuple(int(v) for v in p1.sum(0).tolist())
        assert got == want, (n, offset, got, want)
    assert (lib().dram_sample_stats_nblk(MULTI), lib().dram_sample_stats_nblk(2)) == (6, 1)


def test_window_sums_at_the_widest_span():
    """hi - lo = 4095, every voxel at the top: the largest c and c^2 the kernel adds up"""
    n = 4097
    v = torch.full((n,), 32767, dtype=torch.int16, device=DEV)
    got = T().sample_window_sums(v, (-2048, 2047)).sum(0).tolist()
    assert got == [4095 * n, 4095 * 4095 * n]
    v[::3] = -32768
    host = v.cpu()
    assert tuple(T().sample_window_sums(v, (-2048, 2047)).sum(0).tolist()) == int_sums(host, -2048, 2047)


# ------------------------------------------------------------------------------------------------ fused output pass
PASS_CASES = {
    "down": ((5, 7, 9), (3, 4, 5)),
    "up": ((3, 6, 6), (7, 11, 13)),               # depth repetition, in-plane upsampling
    "one": ((1, 5, 5), (1, 1, 1)),                # the extent-1 rule
    "identity": ((4, 9, 11), (4, 9, 11)),
    "slot": ((5, 9, 7), (3, 5, 3)),               # odd W; 45 voxels: slot 1 of the byte masks starts at an odd address
}
MASK_DTYPES = {"bool": torch.bool, "uint8": torch.uint8, "int16": torch.int16}


@functools.lru_cache(maxsize=None)
def pass_inputs(name):
    """(scan int16, {dtype name: lung}) on the host, built once per case"""
    src, _ = PASS_CASES[name]
    seed = 40 + sorted(PASS_CASES).index(name)
    scan = R.scan_volume(src, seed).round().to(torch.int16)
    flat = scan.view(-1)
    for k, e in enumerate((-951, -950, -949, -32768, 32767)):         # both sides of the emphysema threshold
        flat[(3 + 5 * k) % flat.numel()] = e
    return scan, {k: R.mask_volume(src, seed + 100, dt) for k, dt in MASK_DTYPES.items()}


@functools.lru_cache(maxsize=None)
def pass_reference(name, mask):
    """the reference composition on the host, computed once and shared: (image Ref, lung mask, em mask)"""
    _, target = PASS_CASES[name]
    scan, lungs = pass_inputs(name)
    lung = lungs[mask] > 0
    return (R.prep_image64(scan.double(), target), R.prep_mask_ref(lung, target),
            R.prep_mask_ref((scan < -950) & lung, target))


def check_sample(name, mask, got):
    ref, lung_ref, em_ref = pass_reference(name, mask)
    scan, lungs = pass_inputs(name)
    _, target = PASS_CASES[name]
    assert set(got) == {"image", "lung_mask", "em_mask"}
    assert got["image"].dtype == torch.float32 and tuple(got["image"].shape) == target
    for k, want in (("lung_mask", lung_ref), ("em_mask", em_ref)):
        assert got[k].dtype == torch.bool and tuple(got[k].shape) == target
        assert torch.equal(got[k].cpu(), want), (name, mask, k)
    lung_dev = lungs[mask].to(DEV) > 0
    assert torch.equal(got["lung_mask"], T().prepare_mask(lung_dev, target))
    assert torch.equal(got["em_mask"], T().prepare_mask((scan.to(DEV) < -950) & lung_dev, target))
    r = R.ratio(got["image"].cpu(), ref)
    print(f"{name}/{mask}: image error / bound = {r:.3f}")
    assert r <= 1.0, (name, mask, r)


@pytest.mark.parametrize("mask", list(MASK_DTYPES))
@pytest.mark.parametrize("name", ["down", "up", "one", "identity"])
def test_fused_pass_against_the_reference_composition(name, mask):
    scan, lungs = pass_inputs(name)
    got = T().prepare_archive_sample(scan.to(DEV), lungs[mask].to(DEV), PASS_CASES[name][1])
    check_sample(name, mask, got)


@pytest.mark.parametrize("mask", list(MASK_DTYPES))
def test_fused_pass_writes_one_slot_of_a_batch(mask):
    scan, lungs = pass_inputs("slot")
    _, target = PASS_CASES["slot"]
    batch = {"image": torch.full((2,) + target, 7.5, device=DEV),
             "lung_mask": torch.ones((2,) + target, dtype=torch.bool, device=DEV),
             "em_mask": torch.ones((2,) + target, dtype=torch.uint8 if mask == "uint8" else torch.bool, device=DEV)}
    before = {k: v[0].clone() for k, v in batch.items()}
    slot = {k: v[1] for k, v in batch.items()}
    assert slot["lung_mask"].data_ptr() % 2 == 1
    got = T().prepare_archive_sample(scan.to(DEV), lungs[mask].to(DEV), target, out=slot)
    assert all(got[k] is slot[k] for k in slot)
    for k in batch:
        assert torch.equal(batch[k][0], before[k]), k                     # slot 0 untouched
    check_sample("slot", mask, {k: (v.view(torch.bool) if v.dtype == torch.uint8 else v) for k, v in slot.items()})
    assert int(batch["em_mask"][1].view(torch.uint8).max()) <= 1          # bytes 0 / 1


def test_a_threshold_other_than_the_default():
    scan, lungs = pass_inputs("down")
    _, target = PASS_CASES["down"]
    lung = lungs["uint8"]
    for thr in (-949, -700.5, 40000, -40000):
        want = R.prep_mask_ref((scan.double() < thr) & (lung > 0), target)       # (an int16 comparison would wrap 40000)
        got = T().prepare_archive_sample(scan.to(DEV), lung.to(DEV), target, em_threshold=thr)
        assert torch.equal(got["em_mask"].cpu(), want), thr
        got = T().prepare_archive_sample(scan.to(DEV), lung.float().to(DEV), target, em_threshold=thr)    # composition
        assert torch.equal(got["em_mask"].cpu(), want), thr


def _codes(t):
    return torch.nan_to_num(t, nan=7.0, posinf=8.0, neginf=9.0)


@pytest.mark.parametrize("name", ["identity", "down"])
def test_constant_scan_gives_what_prepare_image_gives(name):
    """A constant in-window scan has variance 0: 1 / std is inf and the image inf * 0.  -725 is the middle of the
    window: windowed value 0.5, whose sums are exact in fp32 too, so ``prepare_image``'s variance is exactly 0 as
    well and both paths hold the same non-finite values."""
    src, target = PASS_CASES[name]
    scan = torch.full(src, -725, dtype=torch.int16, device=DEV)
    lung = torch.ones(src, dtype=torch.uint8, device=DEV)
    got = T().prepare_archive_sample(scan, lung, target)
    want = T().prepare_image(scan, target)
    torch.cuda.synchronize()
    assert not torch.isfinite(want).any()
    assert torch.equal(_codes(got["image"]), _codes(want))
    assert bool(got["lung_mask"].all()) and not bool(got["em_mask"].any())


# ------------------------------------------------------------------------------------------------ dispatch
def test_float_input_takes_the_composition():
    scan, lungs = pass_inputs("down")
    _, target = PASS_CASES["down"]
    for image, lung in ((scan.float(), lungs["bool"]), (scan, lungs["int16"].float()), (scan.double(), lungs["uint8"])):
        got = T().prepare_archive_sample(image.to(DEV), lung.to(DEV), target)
        assert set(got) == {"image", "lung_mask", "em_mask"}
        assert got["lung_mask"].dtype == got["em_mask"].dtype == torch.bool
        assert torch.equal(got["image"], T().prepare_image(image.to(DEV), target))
        lung_dev = lung.to(DEV) > 0
        assert torch.equal(got["lung_mask"], T().prepare_mask(lung_dev, target))
        assert torch.equal(got["em_mask"], T().prepare_mask((scan.to(DEV) < -950) & lung_dev, target))
    # a non-integral span is the float path's
    got = T().prepare_archive_sample(scan.float().to(DEV), lungs["bool"].to(DEV), target, from_span=(-1150.5, -300.25))
    assert torch.equal(got["image"], T().prepare_image(scan.float().to(DEV), target, (-1150.5, -300.25)))
    # ... and both paths agree with each other within the two bounds
    ref = pass_reference("down", "bool")[0]
    assert R.ratio(T().prepare_archive_sample(scan.float().to(DEV), lungs["bool"].to(DEV), target)["image"].cpu(), ref) <= 1.0


def _peak_over(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def test_int16_path_allocates_no_full_size_temporary():
    src, target = (64, 128, 128), (8, 16, 16)
    g = torch.Generator().manual_seed(9)
    scan = torch.randint(-1400, 200, src, generator=g).to(torch.int16).to(DEV)
    lung = (torch.rand(src, generator=g) > 0.4).to(DEV)
    n = scan.numel()
    out_bytes = target[0] * target[1] * target[2] * (4 + 1 + 1)
    T().prepare_archive_sample(scan, lung, target)                        # library load, first-call allocations
    fused, got = _peak_over(lambda: T().prepare_archive_sample(scan, lung, target))
    print(f"fused path: peak {fused} B over the inputs, outputs {out_bytes} B, {n} source voxels")
    assert fused - out_bytes < 1 * n
    for image, mask in ((scan, lung.float()), (scan.float(), lung)):      # the composition on the same case
        comp, want = _peak_over(lambda: T().prepare_archive_sample(image, mask, target))
        print(f"composition ({image.dtype}, {mask.dtype}): peak {comp} B")
        assert comp - out_bytes > 4 * n                                   # the test measures what it claims
        assert torch.equal(got["lung_mask"], want["lung_mask"]) and torch.equal(got["em_mask"], want["em_mask"])


# ------------------------------------------------------------------------------------------------ refusals
def test_abi_refuses_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib
    L = lib()
    BAD, UNSUP = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    scan = torch.zeros((2, 3, 4), dtype=torch.int16, device=DEV)
    lung = torch.ones((2, 3, 4), dtype=torch.uint8, device=DEV)
    partial = torch.full((4, 2), -77, dtype=torch.int64, device=DEV)
    zidx = torch.zeros(2, dtype=torch.int32, device=DEV)
    mi = torch.tensor([0.5, 2.0], device=DEV)
    oi = torch.full((2, 2, 2), -77.0, device=DEV)
    ol = torch.full((2, 2, 2), 77, dtype=torch.uint8, device=DEV)
    oe = torch.full((2, 2, 2), 77, dtype=torch.uint8, device=DEV)
    n = scan.numel()
    stats = [((None, p(partial), n, LO, HI), BAD), ((p(scan), None, n, LO, HI), BAD), ((p(scan), p(partial), 1, LO, HI), BAD),
             ((p(scan), p(partial), 0, LO, HI), BAD), ((p(scan), p(partial), n, HI, LO), BAD),
             ((p(scan), p(partial), n, LO, LO), BAD), ((p(scan), p(partial), n, -2048, 2048), BAD),
             ((p(scan), p(partial), 2 ** 31, LO, HI), UNSUP)]
    for args, want in stats:
        assert L.dram_sample_stats_i16(*args, s) == want, args
    good = dict(scan=p(scan), lung=p(lung), dt=1, zidx=p(zidx), mi=p(mi), oi=p(oi), ol=p(ol), oe=p(oe), D=2, H=3, W=4,
                Do=2, Ho=2, Wo=2, lo=LO, hi=HI, thr=-950)
    cases = [({k: None}, BAD) for k in ("scan", "lung", "zidx", "mi", "oi", "ol", "oe")]
    cases += [({k: 0}, BAD) for k in ("D", "H", "W", "Do", "Ho", "Wo")] + [({"D": -1}, BAD)]
    cases += [({"dt": 0}, BAD), ({"dt": 3}, BAD), ({"lo": HI, "hi": LO}, BAD), ({"hi": LO}, BAD),
              ({"lo": -2048, "hi": 2048}, BAD),
              ({"D": 2048, "H": 1024, "W": 1024}, UNSUP), ({"Do": 2048, "Ho": 1024, "Wo": 1024}, UNSUP)]
    for change, want in cases:
        a = dict(good, **change)
        assert L.dram_prep_sample_i16(*a.values(), s) == want, change
    torch.cuda.synchronize()
    assert int((partial != -77).sum()) == 0 and int((oi != -77).sum()) == 0        # nothing was launched
    assert int((ol != 77).sum()) == 0 and int((oe != 77).sum()) == 0
    assert L.dram_prep_sample_i16(*good.values(), s) == 0 and L.dram_sample_stats_i16(p(scan), p(partial), n, LO, HI, s) == 0
    torch.cuda.synchronize()
    assert int((ol == 1).sum()) == 8 and partial[0].tolist() == [n * (HI - LO), n * (HI - LO) ** 2]


def test_python_refuses_before_any_launch():
    """the twins of the ABI refusals one level up, raised before a kernel is launched: the destinations keep their fill"""
    scan = torch.zeros((2, 3, 4), dtype=torch.int16, device=DEV)
    lung = torch.ones((2, 3, 4), dtype=torch.uint8, device=DEV)
    tgt = (2, 2, 2)
    out = {"image": torch.full(tgt, -77.0, device=DEV), "lung_mask": torch.ones(tgt, dtype=torch.bool, device=DEV),
           "em_mask": torch.ones(tgt, dtype=torch.bool, device=DEV)}
    P = T().prepare_archive_sample
    for args, kw, exc in [
            ((scan, lung[:1], tgt), {}, ValueError), ((scan, lung, (2, 2, 0)), {}, ValueError),
            ((scan, lung, (2, 2)), {}, ValueError), ((scan, lung, tgt), {"from_span": (-1150.5, -300)}, ValueError),
            ((scan, lung, tgt), {"from_span": (-300, -1150)}, ValueError),
            ((scan, lung, tgt), {"from_span": (-2048, 2048)}, ValueError),
            ((scan.cpu(), lung, tgt), {}, TypeError), ((scan, lung.cpu(), tgt), {}, TypeError),
            ((scan.cpu().float(), lung.cpu(), tgt), {}, TypeError),
            ((scan, lung, tgt), {"out": {"image": out["image"]}}, ValueError),
            ((scan, lung, tgt), {"out": dict(out, image=out["image"].double())}, TypeError),
            ((scan, lung, tgt), {"out": dict(out, lung_mask=out["lung_mask"].float())}, TypeError),
            ((scan, lung, tgt), {"out": dict(out, em_mask=torch.ones((2, 2, 4), dtype=torch.bool, device=DEV)[:, :, ::2])}, ValueError),
            ((scan, lung, tgt), {"out": dict(out, image=torch.zeros((2, 2, 3), device=DEV))}, ValueError),
            ((scan, lung, tgt), {"out": dict(out, image=out["image"].cpu())}, ValueError)]:
        with pytest.raises(exc):
            P(*args, **{"out": out, **kw})
    with pytest.raises(ValueError):
        T().sample_window_sums(scan.view(-1)[:1])
    with pytest.raises(ValueError):
        T().sample_window_sums(scan, (-1150.5, -300))
    with pytest.raises(ValueError):
        T().sample_window_sums(scan[:, :, ::2])                     # not contiguous
    torch.cuda.synchronize()
    assert bool((out["image"] == -77).all()) and bool(out["lung_mask"].all()) and bool(out["em_mask"].all())


# ------------------------------------------------------------------------------------------------ end to end
SIZE = ("16", "32", "32")


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    root = tmp_path_factory.mktemp("archive")
    uids, labels = write_archive(str(root / "data"), n=8, shape=(12, 20, 24))
    return {"root": str(root / "data"), "uids": uids, "labels": labels,
            "train": write_split(root / "train.csv", uids[:5]), "valid": write_split(root / "valid.csv", uids[5:])}


def job_args(archive, model_path, *more):
    return ["--synthetic", "0", "--data_path", archive["root"], "--train_csv", archive["train"], "--valid_csv",
            archive["valid"], "--model_arch", "med3ddram18", "--target_size", *SIZE, "--batch_size", "1", "--num_samples",
            "1", "--max_epochs", "1", "--model_path", str(model_path), "--log_every_n_steps", "1", *more]


def test_training_job_from_an_archive(archive, tmp_path, caplog, monkeypatch):
    from bodyct_dram_emph_subtype_amd import dataset, train
    from bodyct_dram_emph_subtype_amd.data_sampler import SubtypingStratifiedSampler
    caplog.set_level(logging.INFO)
    loads = []
    real = dataset.COPDGeneSubtyping.get_data
    monkeypatch.setattr(dataset.COPDGeneSubtyping, "get_data", lambda self, uid: (loads.append(uid), real(self, uid))[1])
    mod = train.run_training_job(job_args(archive, tmp_path))
    ck = torch.load(tmp_path / "subtyping_med3ddram18" / "checkpoints" / "epoch=00.ckpt", map_location="cpu",
                    weights_only=False)
    train_uids, valid_uids = sorted(archive["uids"][:5]), sorted(archive["uids"][5:])
    classes = len({archive["labels"][u][0] for u in train_uids})
    assert ck["epoch"] == 0 and ck["global_step"] == classes             # --num_samples 1: one draw per present class
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())
    steps = re.findall(r"step (\d+) train_loss (\S+) lr", caplog.text)
    assert [int(s) for s, _ in steps] == list(range(1, classes + 1)), caplog.text
    assert all(math.isfinite(float(l)) for _, l in steps)
    epoch = re.search(r"epoch 0: train_loss (\S+) ", caplog.text)
    assert epoch and math.isfinite(float(epoch[1]))
    # the draws come from the train split; validation and the final test (no --test_csv) each read the valid split
    assert len(loads) == classes + 2 * len(valid_uids)
    assert set(loads[:classes]) <= set(train_uids)
    assert loads[classes:] == valid_uids + valid_uids
    assert re.search(r"test \(best = .*epoch=00.ckpt\)", caplog.text)
    assert mod.cle_class_weights.shape == (6,) and bool(torch.isfinite(mod.cle_class_weights).all())

    # the weights the first epoch starts from are the sampler's: a module and loaders built the same way
    args = train.build_parser().parse_args(job_args(archive, tmp_path))
    fresh = type(mod)(args)
    data, val, test = train.build_archive_data(args, fresh, 0, 1, torch.device(DEV))
    sampler = SubtypingStratifiedSampler(dataset.COPDGeneSubtyping(archive["root"], train_uids), 1, seed=0)
    assert fresh.cle_class_weights.dtype == torch.float32
    assert torch.equal(fresh.cle_class_weights, torch.tensor(sampler.cle_class_weights, dtype=torch.float32))
    assert torch.equal(fresh.pse_class_weights, torch.tensor(sampler.pse_class_weights, dtype=torch.float32))
    assert sampler.cle_class_weights != [1 / 6] * 6
    assert (len(data), len(val), len(test)) == (classes, len(valid_uids), len(valid_uids))
    assert data.sampler.indices(0) == sampler.indices(0) and data.drop_last and data.shuffle and not val.shuffle
    it = val.epoch(0)
    b = next(it)
    it.close()
    assert b["uid"] == valid_uids[:1] and b["image"].shape == (1, 16, 32, 32) and b["image"].is_cuda
    case = real(val.dataset, valid_uids[0])
    ref = R.prep_image64(case["image"].double(), (16, 32, 32))
    assert R.ratio(b["image"][0].cpu(), ref) <= 1.0
    assert torch.equal(b["em_mask"][0].cpu(), R.prep_mask_ref((case["image"] < -950) & case["lung_mask"], (16, 32, 32)))


def test_loader_augments_per_sample(archive):
    import random
    from bodyct_dram_emph_subtype_amd import dataset, transforms
    ds = dataset.COPDGeneSubtyping(archive["root"], sorted(archive["uids"]))
    size = (16, 32, 32)
    plain = dataset.ArchiveLoader(ds, 2, size, DEV)
    aug = dataset.ArchiveLoader(ds, 2, size, DEV, augment=transforms.TrainAugment(p=1.0, rng=random.Random(4)))
    it = plain.epoch(0)
    a = next(it)
    it.close()
    torch.manual_seed(21)                       # GaussianAddictive draws its noise on the device
    it = aug.epoch(0)
    b = next(it)
    it.close()
    assert set(a) == set(b) and b["uid"] == a["uid"] and torch.equal(a["index"], b["index"])
    for k in ("image", "lung_mask", "em_mask"):
        assert b[k].shape == a[k].shape == (2,) + size and b[k].dtype == a[k].dtype and b[k].is_cuda
    assert b["lung_mask"].dtype == b["em_mask"].dtype == torch.bool
    assert bool(torch.isfinite(b["image"]).all()) and not torch.equal(a["image"], b["image"])
    assert int(b["lung_mask"].view(torch.uint8).max()) <= 1 and int(b["em_mask"].view(torch.uint8).max()) <= 1
    # exactly what train.augment_batch makes of the plain batch with the same draws
    from bodyct_dram_emph_subtype_amd import train
    torch.manual_seed(21)
    want = train.augment_batch(a, transforms.TrainAugment(p=1.0, rng=random.Random(4)))
    for k in ("image", "lung_mask", "em_mask"):
        assert torch.equal(b[k], want[k]), k
