"""CPU: the host side of training from a scan archive -- the stratified sampler against values recorded from the
reference (tests/golden/sampler.json), the archive data set on a tiny archive in tmp_path, the loader's order, sharding,
threading and error paths with a torch stand-in for the device-side ``prepare``, and the parser."""
import json
import math
import os
import threading

import numpy as np
import pytest
import torch
from torch.utils.data import DistributedSampler

from archive_ref import write_archive, write_split
from conftest import GOLDEN

SIZE = (3, 4, 5)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "sampler.json")) as f:
        return json.load(f)


class Source:
    """what the sampler reads of a data set"""

    def __init__(self, cle, pse):
        self.series_uids = [f"case{i:03d}" for i in range(len(cle))]
        self.subtyping_labels = {u: {"cle": c, "pse": p} for u, c, p in zip(self.series_uids, cle, pse)}

    def __len__(self):
        return len(self.series_uids)


def sampler_for(rec, seed=0, balance=None):
    from bodyct_dram_emph_subtype_amd.data_sampler import SubtypingStratifiedSampler
    src = Source(rec["cle"], rec["pse"])
    return SubtypingStratifiedSampler(src, rec["balance_label_count"] if balance is None else balance, seed=seed), src


# ------------------------------------------------------------------------------------------------ sampler
CASES = ["all_present", "cle_4_missing", "pse_2_missing", "cle_1_and_5_missing", "pse_1_missing", "single_class"]


@pytest.mark.parametrize("name", CASES)
def test_sampler_values_are_the_references(golden, name):
    rec = golden[name]
    s, _ = sampler_for(rec)
    for key in ("cle_class_weights", "pse_class_weights"):
        got = getattr(s, key)
        assert isinstance(got, list) and len(got) == len(rec[key])
        assert np.abs(np.asarray(got) - np.asarray(rec[key])).max() <= 1e-12, (key, got, rec[key])
    for key in ("cle_statistics", "pse_statistics"):
        got = getattr(s, key)
        assert {str(k) for k in got} == set(rec[key])
        assert max(abs(got[int(k)] - v) for k, v in rec[key].items()) <= 1e-12
    assert s.num_samples == rec["num_samples"] == len(s)
    assert {str(k): v.tolist() for k, v in s.cle_label_groups.items()} == rec["cle_label_groups"]


def test_sampler_example_of_a_missing_middle_class(golden):
    s, _ = sampler_for(golden["cle_4_missing"])
    assert s.cle_class_weights == [0.2, 0.2, 0.2, 0.234375, 0.46875, 0.46875]
    assert s.cle_statistics[4] == 1e-5 and 4 not in s.cle_label_groups


def test_sampler_draws(golden):
    rec = golden["cle_4_missing"]
    k = 5                                                   # present CLE classes
    n_draws = 6000
    s, src = sampler_for(rec, seed=3, balance=n_draws // k)
    a, b, c = s.indices(0), s.indices(0), s.indices(1)
    assert a == b and a != c and len(a) == s.num_samples == n_draws
    assert sampler_for(rec, seed=3, balance=n_draws // k)[0].indices(0) == a      # every rank draws this list
    assert sampler_for(rec, seed=4, balance=n_draws // k)[0].indices(0) != a
    assert all(isinstance(i, int) and 0 <= i < len(src) for i in a)
    # class uniform among the present classes: a binomial count per class, 5 sigma
    sigma = math.sqrt(n_draws * (1 / k) * (1 - 1 / k))
    counts = np.bincount([rec["cle"][i] for i in a], minlength=6)
    assert counts[4] == 0
    for cls in (0, 1, 2, 3, 5):
        assert abs(counts[cls] - n_draws / k) <= 5 * sigma, (cls, counts)
    # ... then a member uniformly: class 0 holds cases 0..9
    members = np.bincount([i for i in a if rec["cle"][i] == 0], minlength=10)[:10]
    m = int(counts[0])
    assert np.abs(members - m / 10).max() <= 5 * math.sqrt(m * 0.1 * 0.9), members


def test_sampler_refuses_an_empty_source():
    from bodyct_dram_emph_subtype_amd.data_sampler import SubtypingStratifiedSampler
    with pytest.raises(ValueError):
        SubtypingStratifiedSampler(Source([], []), 4)


# ------------------------------------------------------------------------------------------------ data set
def test_dataset_reads_the_archive(tmp_path):
    from bodyct_dram_emph_subtype_amd import models
    from bodyct_dram_emph_subtype_amd.dataset import COPDGeneSubtyping
    from bodyct_dram_emph_subtype_amd.utils import read_csv_in_dict
    root = str(tmp_path / "archive")
    uids, labels = write_archive(root, file_labels=("1.2.38.case02",))
    split = write_split(tmp_path / "train.csv", uids[:6])
    got = COPDGeneSubtyping.get_series_uids(split)
    assert got == sorted(uids[:6]) and got != uids[:6]
    ds = COPDGeneSubtyping(root, got)
    assert len(ds) == 6
    assert ds.subtyping_labels == {u: {"cle": labels[u][0], "pse": labels[u][1]} for u in got}     # int(float("3.0"))
    assert all(type(v["cle"]) is int for v in ds.subtyping_labels.values())
    assert ds.cle_ratio_map is models.CLE_RATIO_MAP and ds.pse_ratio_map is models.PSE_RATIO_MAP
    assert COPDGeneSubtyping.cle_ratio_map is models.CLE_RATIO_MAP

    d = ds.get_data("1.2.39.case01")
    assert set(d) == {"image", "lung_mask", "cls_label", "pse_label", "uid"}
    assert d["image"].dtype == torch.int16 and d["lung_mask"].dtype == torch.bool and d["image"].shape == (4, 6, 7)
    assert (d["cls_label"], d["pse_label"], d["uid"]) == (1, 1, "1.2.39.case01")              # from the csv
    d = ds.get_data("1.2.38.case02")
    assert (d["cls_label"], d["pse_label"]) == (3, 0) != labels["1.2.38.case02"]              # the file's labels win
    item = ds[0]
    assert item["uid"] == got[0] and item["index"].tolist() == [0] and item["index"].dtype == torch.int64
    seen = COPDGeneSubtyping(root, got, transforms=lambda c: dict(c, seen=True)).get_data(got[0])
    assert seen["seen"] is True

    rows, names = read_csv_in_dict(os.path.join(root, "merged.csv"), "SeriesInstanceUID")
    assert names[0] == "SeriesInstanceUID" and set(rows) == set(uids) and rows[uids[3]]["site"] == "x"
    assert read_csv_in_dict(str(tmp_path / "nothing.csv"), "SeriesInstanceUID") == ({}, None)
    assert COPDGeneSubtyping.get_series_uids(str(tmp_path / "nothing.csv")) == []


def test_dataset_names_the_uid_it_cannot_find(tmp_path):
    from bodyct_dram_emph_subtype_amd.dataset import COPDGeneSubtyping
    root = str(tmp_path / "archive")
    uids, _ = write_archive(root, skip_files=("1.2.37.case03",), skip_rows=("1.2.36.case04",))
    with pytest.raises(FileNotFoundError, match="1.2.37.case03"):
        COPDGeneSubtyping(root, uids[:4])
    with pytest.raises(KeyError, match="1.2.36.case04"):
        COPDGeneSubtyping(root, [uids[0], uids[4]])
    with pytest.raises(KeyError, match="not-in-the-archive"):
        COPDGeneSubtyping(root, ["not-in-the-archive"])
    assert len(COPDGeneSubtyping(root, uids[:3])) == 3


# ------------------------------------------------------------------------------------------------ loader
def cpu_prepare(image, lung_mask, target_size, out=None):
    """torch stand-in for transforms.prepare_archive_sample: same signature, writes the slot views in place"""
    idx = [torch.linspace(0, n - 1, t).long() for n, t in zip(image.shape, target_size)]
    pick = lambda t: t[idx[0]][:, idx[1]][:, :, idx[2]]
    out["image"].copy_(pick(image.float()))
    out["lung_mask"].copy_(pick(lung_mask > 0))
    out["em_mask"].copy_(pick((image < -950) & (lung_mask > 0)))
    return out


def loader_for(ds, **kw):
    from bodyct_dram_emph_subtype_amd.dataset import ArchiveLoader
    kw.setdefault("prepare", cpu_prepare)
    return ArchiveLoader(ds, kw.pop("batch_size", 2), SIZE, "cpu", **kw)


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    from bodyct_dram_emph_subtype_amd.dataset import COPDGeneSubtyping
    root = str(tmp_path_factory.mktemp("archive"))
    uids, labels = write_archive(root, n=7)
    return COPDGeneSubtyping(root, sorted(uids)), labels


def reader_threads():
    return [t for t in threading.enumerate() if t.name.startswith("ArchiveLoader")]


def test_loader_batches_keep_the_contract(archive):
    ds, labels = archive
    loader = loader_for(ds, batch_size=3)
    batches = list(loader.epoch(0))
    assert len(batches) == len(loader) == 3 and [b["image"].shape[0] for b in batches] == [3, 3, 1]
    seen = []
    for b in batches:
        n = b["image"].shape[0]
        assert set(b) == {"image", "lung_mask", "em_mask", "cls_label", "pse_label", "index", "uid"}
        assert b["image"].dtype == torch.float32 and b["image"].shape == (n,) + SIZE
        for k in ("lung_mask", "em_mask"):
            assert b[k].dtype == torch.bool and b[k].shape == (n,) + SIZE
        for k in ("cls_label", "pse_label"):
            assert b[k].dtype == torch.int64 and b[k].shape == (n,)
        assert b["index"].dtype == torch.int64 and b["index"].shape == (n, 1)
        assert isinstance(b["uid"], list) and b["uid"] == [ds.series_uids[i] for i in b["index"][:, 0].tolist()]
        assert b["cls_label"].tolist() == [labels[u][0] for u in b["uid"]]
        assert b["pse_label"].tolist() == [labels[u][1] for u in b["uid"]]
        for j, u in enumerate(b["uid"]):                                  # slot j holds case u
            case = ds.get_data(u)
            want = cpu_prepare(case["image"], case["lung_mask"], SIZE,
                               {"image": torch.empty(SIZE), "lung_mask": torch.empty(SIZE, dtype=torch.bool),
                                "em_mask": torch.empty(SIZE, dtype=torch.bool)})
            assert all(torch.equal(b[k][j], want[k]) for k in want)
        seen += b["index"][:, 0].tolist()
    assert seen == list(range(7))                                         # sequential, unshuffled, nothing dropped
    assert not reader_threads()
    assert [len(loader_for(ds, batch_size=3, drop_last=True)), len(list(loader_for(ds, batch_size=3, drop_last=True).epoch(0)))] == [2, 2]


@pytest.mark.parametrize("form", ["sequential", "sampler"])
def test_loader_shards_as_distributed_sampler(archive, form):
    from bodyct_dram_emph_subtype_amd.data_sampler import SubtypingStratifiedSampler
    ds, _ = archive
    sampler = SubtypingStratifiedSampler(ds, 3, seed=11) if form == "sampler" else None      # 6 classes x 3 = 18 draws
    shuffle = form == "sampler"
    for epoch in (0, 2):
        base = sampler.indices(epoch) if sampler else list(range(len(ds)))
        got = []
        for rank in range(2):
            loader = loader_for(ds, sampler=sampler, shuffle=shuffle, rank=rank, world=2, seed=5, drop_last=shuffle)
            ref = DistributedSampler(range(len(base)), num_replicas=2, rank=rank, shuffle=shuffle, seed=5)
            ref.set_epoch(epoch)
            want = [base[p] for p in ref]
            assert loader.indices(epoch) == want
            full = len(want) // 2 * 2 if shuffle else len(want)           # drop_last drops the odd case
            out = [i for b in loader.epoch(epoch) for i in b["index"][:, 0].tolist()]
            assert out == want[:full]
            assert len(loader) == len(list(loader.epoch(epoch))) == (full + 1) // 2
            got.append(want)
        # the list DistributedSampler defines: the positions (permuted with seed + epoch when shuffling), padded with
        # their own head to a multiple of the world size, dealt out round-robin
        pos = list(range(len(base)))
        if shuffle:
            pos = torch.randperm(len(base), generator=torch.Generator().manual_seed(5 + epoch)).tolist()
        pos += pos[:-len(pos) % 2]
        assert len(pos) % 2 == 0 and len(pos) - len(base) in (0, 1)
        assert got[0] == [base[p] for p in pos[0::2]] and got[1] == [base[p] for p in pos[1::2]]
        assert sorted(got[0] + got[1]) == sorted(base[p] for p in pos)
    if sampler:
        assert loader_for(ds, sampler=sampler, shuffle=True, seed=5).indices(0) != \
            loader_for(ds, sampler=sampler, shuffle=True, seed=5).indices(1)


def test_loader_drop_last_and_len(archive):
    ds, _ = archive                                                        # 7 cases
    for world, B, drop, want in [(1, 2, False, 4), (1, 2, True, 3), (1, 7, True, 1), (1, 8, True, 0), (1, 8, False, 1),
                                 (2, 3, False, 2), (2, 3, True, 1), (3, 2, True, 1), (3, 2, False, 2)]:
        loader = loader_for(ds, batch_size=B, drop_last=drop, world=world, rank=world - 1)
        got = list(loader.epoch(0))
        assert len(loader) == len(got) == want, (world, B, drop)
        if drop:
            assert all(b["image"].shape[0] == B for b in got)
    assert not reader_threads()


def test_loader_reader_exception_arrives_in_the_consumer(archive):
    ds, _ = archive
    bad = ds.series_uids[4]

    class Broken:
        series_uids = ds.series_uids

        def __len__(self):
            return len(ds)

        def get_data(self, uid):
            if uid == bad:
                raise OSError(f"cannot read {uid}")
            return ds.get_data(uid)

    it = loader_for(Broken(), batch_size=2, prefetch=1).epoch(0)
    assert next(it)["index"][:, 0].tolist() == [0, 1]
    assert next(it)["index"][:, 0].tolist() == [2, 3]                      # the batches in front of it are whole
    with pytest.raises(OSError, match=bad):
        next(it)                                                           # cases 4, 5: raised at that batch
    assert not reader_threads()
    with pytest.raises(StopIteration):
        next(it)


@pytest.mark.parametrize("prefetch", [1, 2, 5])
def test_loader_stops_its_thread_when_the_loop_breaks(archive, prefetch):
    ds, _ = archive
    loader = loader_for(ds, batch_size=1, prefetch=prefetch)
    for i, b in enumerate(loader.epoch(0)):
        if i == 1:
            break
    assert not reader_threads()
    it = loader.epoch(0)
    next(it)
    assert len(reader_threads()) <= 1
    it.close()
    assert not reader_threads()
    it = loader.epoch(0)                                                   # never started: no thread either
    it.close()
    assert not reader_threads()


def test_loader_refuses_bad_arguments(archive):
    ds, _ = archive
    for kw in (dict(batch_size=0), dict(prefetch=0), dict(world=0), dict(rank=2, world=2), dict(rank=-1)):
        with pytest.raises(ValueError):
            loader_for(ds, **kw)


# ------------------------------------------------------------------------------------------------ parser / train.py
def test_parser_defaults_and_archive_requirements(tmp_path):
    from bodyct_dram_emph_subtype_amd import train
    a = train.build_parser().parse_args([])
    want = dict(model_arch="med3ddram50", lr=0.0001, ngpus=1, momentum=0.9, reload_only_weights=1, weight_decay=1e-5,
                ckp=None, target_size=(128, 224, 288), data_path="", train_csv="", valid_csv="", test_csv="",
                model_path="./models/", workers=2, batch_size=1, num_samples=128, local_rank=0, max_epochs=120,
                log_every_n_steps=5, synthetic=1, seed=0, augment=0, precision="32", gradient_clip_val=None,
                gradient_clip_algorithm="norm", accumulate_grad_batches=1, draw_predictions=0, prefetch=2)
    assert vars(a) == want
    train.check_archive_args(a)                                            # the synthetic default needs no archive
    out = tmp_path / "models"
    for argv, word in [(["--synthetic", "0"], "--data_path"),
                       (["--synthetic", "0", "--train_csv", "t.csv"], "--data_path"),
                       (["--synthetic", "0", "--data_path", str(tmp_path)], "--train_csv"),
                       (["--synthetic", "0", "--data_path", str(tmp_path / "none"), "--train_csv", "t.csv"], "not a folder"),
                       (["--synthetic", "0", "--data_path", str(tmp_path), "--train_csv", "t.csv", "--prefetch", "0"],
                        "--prefetch")]:
        with pytest.raises(SystemExit) as e:
            train.run_training_job(argv + ["--model_path", str(out)])
        assert word in str(e.value), (argv, e.value)
    assert not out.exists()                                                # refused before anything was set up


# ------------------------------------------------------------------------------------------------ prepare_archive_sample
def test_prepare_archive_sample_refuses_on_the_host():
    """shapes, target_size, span and host tensors are refused before the device is touched: all of this runs without
    one"""
    from bodyct_dram_emph_subtype_amd import transforms as T
    img = torch.zeros((3, 4, 5), dtype=torch.int16)
    lung = torch.ones((3, 4, 5), dtype=torch.bool)
    for bad in (lung[:2], lung[0], torch.ones((3, 4, 6), dtype=torch.bool)):
        with pytest.raises(ValueError, match="shape"):
            T.prepare_archive_sample(img, bad, (2, 2, 2))
    with pytest.raises(ValueError, match="shape"):
        T.prepare_archive_sample(img[:0], lung[:0], (2, 2, 2))
    for bad in ((2, 2), (2, 2, 0), (2, -1, 2), (2, 2.5, 2), None, (2, "a", 2), (2, 2, 2, 2)):
        with pytest.raises(ValueError, match="target_size"):
            T.prepare_archive_sample(img, lung, bad)
    with pytest.raises(ValueError, match="float"):                       # tells the caller to pass float
        T.prepare_archive_sample(img, lung, (2, 2, 2), from_span=(-1150.5, -300.0))
    for span in ((-300, -1150), (-300, -300), (-5000, 0)):
        with pytest.raises(ValueError, match="from_span"):
            T.prepare_archive_sample(img, lung, (2, 2, 2), from_span=span)
    with pytest.raises(TypeError, match="device"):
        T.prepare_archive_sample(img, lung, (2, 2, 2))
    with pytest.raises(TypeError, match="device"):
        T.prepare_archive_sample(img.float(), lung, (2, 2, 2), from_span=(-1150.5, -300.0))
    with pytest.raises(TypeError):
        T.prepare_archive_sample(img.numpy(), lung, (2, 2, 2))
    with pytest.raises(TypeError, match="int16"):
        T.sample_window_sums(img.float())
    with pytest.raises(ValueError, match="2 <= n"):
        T.sample_window_sums(img.view(-1)[:1])
    with pytest.raises(TypeError, match="device"):
        T.sample_window_sums(img)
