"""The training archive of the reference (dataset.py:96-155) and the loader that feeds the train step from it.

Archive layout: one folder with ``merged.csv`` (columns ``SeriesInstanceUID``, ``CT_Visual_Emph_Severity_P1``,
``CT_Visual_Emph_Paraseptal_P1``, anything else is ignored) and one ``<SeriesInstanceUID>.pth`` per case, a
``torch.save``d dict with ``image`` [D,H,W] (raw HU, int16) and ``lung_mask`` [D,H,W], optionally ``cls_label`` /
``pse_label``.  The train / valid / test splits are csv files with a ``SeriesInstanceUID`` column.

``COPDGeneSubtyping`` is the host side: csv reading, labels, ``get_data``.  ``ArchiveLoader`` replaces the reference's
``DataLoader`` + ``DistributedSampler`` (+ ``DistributedSamplerWrapper`` over the stratified sampler), models.py:99-157:
one background thread reads and pins cases ahead, the consuming thread uploads each case and runs
``transforms.prepare_archive_sample`` straight into its slot of the batch tensors -- B uploads and 2 B kernel
launches per batch, no full-size device temporary that outlives its sample.  SimpleITK reading and the predict-side
``SubtypingInference`` are not here: ``transforms.prepare_case`` / ``processor.predict_case`` take a scan at a time.
"""
from __future__ import annotations

if not __package__:          # imported top-level (this directory on sys.path): bind to the package, see _dropin.py
    import _dropin
    __package__ = _dropin.adopt(__name__)

import os
import queue
import threading
from typing import Callable, Dict, List, Optional, Sequence

import torch
from torch.utils.data import DistributedSampler

from . import models, transforms
from .utils import read_csv_in_dict

CLE_COLUMN, PSE_COLUMN = "CT_Visual_Emph_Severity_P1", "CT_Visual_Emph_Paraseptal_P1"


class COPDGeneSubtyping:
    cle_ratio_map = models.CLE_RATIO_MAP          # the objects the losses' band tables are built from
    pse_ratio_map = models.PSE_RATIO_MAP

    @classmethod
    def get_series_uids(cls, csv_file: str) -> List[str]:
        rows, _ = read_csv_in_dict(csv_file, "SeriesInstanceUID")
        return sorted(rows.keys())

    def __init__(self, archive_path: str, series_uids: Sequence[str], transforms: Optional[Callable] = None):
        self.archive_path = str(archive_path)
        self.transforms = transforms
        self.series_uids = list(series_uids)
        self.meta, _ = read_csv_in_dict(os.path.join(self.archive_path, "merged.csv"), "SeriesInstanceUID")
        self.subtyping_labels: Dict[str, Dict[str, int]] = {}
        for uid in self.series_uids:
            if uid not in self.meta:
                raise KeyError(f"COPDGeneSubtyping: series {uid!r} has no row in {self.archive_path}/merged.csv")
            if not os.path.exists(self._path(uid)):
                raise FileNotFoundError(f"COPDGeneSubtyping: series {uid!r} has no file {self._path(uid)}")
            row = self.meta[uid]
            self.subtyping_labels[uid] = {"cle": int(float(row[CLE_COLUMN])), "pse": int(float(row[PSE_COLUMN]))}

    def _path(self, uid: str) -> str:
        return os.path.join(self.archive_path, f"{uid}.pth")

    def __len__(self) -> int:
        return len(self.series_uids)

    def __getitem__(self, index: int) -> dict:
        d = self.get_data(self.series_uids[index])
        d["index"] = torch.LongTensor([index])
        return d

    def get_data(self, series_uid: str) -> dict:
        """The RAW case: 'image', 'lung_mask' as stored (host tensors), 'cls_label' / 'pse_label' (the file's where it
        holds them -- what the reference's batch carries -- else merged.csv's), 'uid'.  The windowing, the resize and
        em_mask are the device's work (``transforms.prepare_archive_sample``); a ``transforms`` callable given at
        construction is applied to the dict last, as the reference applies its own."""
        stored = torch.load(self._path(series_uid), map_location="cpu", weights_only=True)
        labels = self.subtyping_labels[series_uid]
        data = {"image": torch.as_tensor(stored["image"]), "lung_mask": torch.as_tensor(stored["lung_mask"]),
                "cls_label": int(stored["cls_label"]) if "cls_label" in stored else labels["cle"],
                "pse_label": int(stored["pse_label"]) if "pse_label" in stored else labels["pse"],
                "uid": series_uid}
        if self.transforms:
            data = self.transforms(data)
        return data


class _ReaderError:
    def __init__(self, exc: BaseException):
        self.exc = exc


class ArchiveLoader:
    """Batches of an archive data set in ``train.SyntheticSubtypeData``'s contract plus 'uid': image f32 [B,D,H,W],
    lung_mask / em_mask bool, cls_label / pse_label int64 [B], index int64 [B,1] (position in ``series_uids``), uid list.

    Order and sharding are ``DistributedSampler(num_replicas=world, rank=rank, shuffle=shuffle, seed=seed)`` with
    ``set_epoch(e)``: over ``range(len(dataset))`` (validation / test: shuffle=False, drop_last=False), or, with a
    ``sampler`` (``SubtypingStratifiedSampler``), over the positions of the list ``sampler.indices(e)`` as the
    reference's ``DistributedSamplerWrapper`` does (train: shuffle=True, drop_last=True).  ``drop_last`` is the
    DataLoader's: an incomplete last batch is dropped.

    ``prepare(image, lung_mask, target_size, out=slot)`` writes one sample into the given views of the batch tensors;
    ``augment`` (a ``transforms.TrainAugment``) is applied per sample afterwards, one parameter draw per sample, as
    ``train.augment_batch`` does.  One background thread does the CPU work (``torch.load``, pinning) up to ``prefetch``
    cases ahead; an exception it meets is raised in the consumer at the batch of that case, and closing the generator
    early stops and joins it."""

    def __init__(self, dataset, batch_size: int, target_size: Sequence[int], device, sampler=None, shuffle: bool = False,
                 drop_last: bool = False, rank: int = 0, world: int = 1, seed: int = 0, prefetch: int = 2,
                 prepare: Callable = transforms.prepare_archive_sample, augment: Optional[Callable] = None):
        if batch_size < 1 or prefetch < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("ArchiveLoader: batch_size, prefetch, world must be >= 1 and 0 <= rank < world")
        self.dataset, self.sampler = dataset, sampler
        self.B, self.size, self.device = int(batch_size), tuple(int(v) for v in target_size), torch.device(device)
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        self.rank, self.world, self.seed, self.prefetch = int(rank), int(world), int(seed), int(prefetch)
        self.prepare, self.augment = prepare, augment

    def _total(self) -> int:
        return len(self.sampler) if self.sampler is not None else len(self.dataset)

    def __len__(self) -> int:
        per_rank = -(-self._total() // self.world)             # DistributedSampler pads to a multiple of world
        return per_rank // self.B if self.drop_last else -(-per_rank // self.B)

    def indices(self, epoch: int) -> List[int]:
        """this rank's positions in ``series_uids`` for one epoch, in order"""
        base = self.sampler.indices(epoch) if self.sampler is not None else range(len(self.dataset))
        ds = DistributedSampler(range(len(base)), num_replicas=self.world, rank=self.rank, shuffle=self.shuffle,
                                seed=self.seed, drop_last=False)
        ds.set_epoch(epoch)
        return [int(base[p]) for p in ds]

    def _read(self, index: int) -> dict:
        case = self.dataset.get_data(self.dataset.series_uids[index])
        if self.device.type == "cuda":
            for k in ("image", "lung_mask"):
                case[k] = case[k].contiguous().pin_memory()
        case["index"] = index
        return case

    def epoch(self, epoch: int):
        order = self.indices(epoch)
        batches = [order[i:i + self.B] for i in range(0, len(order), self.B)]
        if self.drop_last:
            batches = [b for b in batches if len(b) == self.B]
        todo = [i for b in batches for i in b]
        q: "queue.Queue" = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        def reader():
            for index in todo:
                if stop.is_set():
                    return
                try:
                    item = self._read(index)
                except BaseException as exc:          # handed to the consumer, which raises it at this case
                    q.put(_ReaderError(exc))
                    return
                q.put(item)

        thread = threading.Thread(target=reader, name="ArchiveLoader-reader", daemon=True)
        thread.start()
        try:
            for b in batches:
                yield self._batch(len(b), q)
        finally:
            # The reader checks `stop` after every put, so from here on it puts one more item at the most.  It can block
            # only in a put() on a FULL queue: emptying the queue lets that put through and leaves room for it.
            stop.set()
            try:
                while True:
                    q.get_nowait()
            except queue.Empty:
                pass
            thread.join()

    def _batch(self, n: int, q) -> dict:
        dev = self.device
        batch = {"image": torch.empty((n,) + self.size, device=dev, dtype=torch.float32),
                 "lung_mask": torch.empty((n,) + self.size, device=dev, dtype=torch.bool),
                 "em_mask": torch.empty((n,) + self.size, device=dev, dtype=torch.bool)}
        keys = tuple(batch)
        cls, pse, idx, uids = [], [], [], []
        for b in range(n):
            case = q.get()
            if isinstance(case, _ReaderError):
                raise case.exc
            image = case["image"].to(dev, non_blocking=True)
            lung = case["lung_mask"].to(dev, non_blocking=True)
            slot = {k: batch[k][b] for k in keys}
            self.prepare(image, lung, self.size, out=slot)
            del image, lung                      # stream-ordered: the blocks go back to the allocator for the next case
            if self.augment is not None:
                new = self.augment(slot)
                for k in keys:
                    if new[k] is not slot[k]:
                        slot[k].copy_(new[k])
            cls.append(int(case["cls_label"]))
            pse.append(int(case["pse_label"]))
            idx.append(int(case["index"]))
            uids.append(case["uid"])
        batch["cls_label"] = torch.tensor(cls, dtype=torch.int64).to(dev)
        batch["pse_label"] = torch.tensor(pse, dtype=torch.int64).to(dev)
        batch["index"] = torch.tensor(idx, dtype=torch.int64).unsqueeze(-1).to(dev)
        batch["uid"] = uids
        return batch
