"""Class-balanced sampler of the training archive: the reference's ``data_sampler.py`` (:7-68).

``SubtypingStratifiedSampler`` carries the reference's attributes with the reference's values -- the per-class loss
weights ``cle_class_weights`` / ``pse_class_weights`` the modules start from (models.py:249-252, :556-561), the label
frequencies ``cle_statistics`` / ``pse_statistics``, the index groups and ``num_samples`` -- and draws the same way:
a CLE class uniformly among the classes present, then one of its cases uniformly, ``num_samples`` times.

One deliberate difference: the reference seeds numpy's global generator with ``int(time.time())`` per epoch, so two
ranks that start a second apart draw different lists (and the distributed wrapper then hands out positions of
DIFFERENT lists).  Here the draw of epoch ``e`` comes from ``numpy.random.RandomState(seed + e)``: every rank holds the
same list, and a run can be repeated.
"""
from __future__ import annotations

if not __package__:          # imported top-level (this directory on sys.path): bind to the package, see _dropin.py
    import _dropin
    __package__ = _dropin.adopt(__name__)

import logging
from typing import Dict, List, Sequence, Tuple

import numpy as np

N_CLE, N_PSE = 6, 3          # centrilobular severity 0..5, paraseptal 0..2 (dataset.py:15-28)


def balanced_class_weights(scores: Sequence[int], n_classes: int) -> Tuple[List[float], Dict[int, float]]:
    """(weights [n_classes], statistics {class: frequency}) of one label column, data_sampler.py:17-28.

    Over the classes PRESENT (k of them, sorted): the 'balanced' weight n / (k * count), divided by the sum of those
    weights and clipped to [0.2, 0.8].  An absent class c is then put in with ``list.insert(c, max(weights))`` in
    ascending order of c -- the current maximum, at its own index where the list is long enough and at the end where
    it is not, exactly as the reference builds its list -- and gets the statistic 1e-5."""
    labels, counts = np.unique(np.asarray(scores, dtype=np.int64), return_counts=True)
    w = len(scores) / (len(labels) * counts.astype(np.float64))
    weights = list(np.clip(w / np.sum(w), a_min=0.2, a_max=0.8))
    stats = {int(l): c / np.sum(counts) for l, c in zip(labels, counts)}
    for c in range(n_classes):
        if c not in stats:
            weights.insert(c, max(weights))
            stats[c] = 1e-5
    return [float(v) for v in weights], {k: float(v) for k, v in stats.items()}


class SubtypingStratifiedSampler:
    """data_source: anything with ``series_uids`` and ``subtyping_labels[uid] = {'cle': .., 'pse': ..}``
    (``dataset.COPDGeneSubtyping``); balance_label_count: draws per present CLE class and epoch (the reference passes
    ``--num_samples``, models.py:109)."""

    def __init__(self, data_source, balance_label_count: int, seed: int = 0):
        self.data_source = data_source
        self.balance_label_count = int(balance_label_count)
        self.seed = int(seed)
        uids = list(data_source.series_uids)
        if not uids:
            raise ValueError("SubtypingStratifiedSampler: the data source holds no case")
        cle = [int(float(data_source.subtyping_labels[u]["cle"])) for u in uids]
        pse = [int(float(data_source.subtyping_labels[u]["pse"])) for u in uids]
        self.cle_class_weights, self.cle_statistics = balanced_class_weights(cle, N_CLE)
        self.pse_class_weights, self.pse_statistics = balanced_class_weights(pse, N_PSE)
        logging.info(f"cle label weights: {self.cle_class_weights}")
        logging.info(f"pse label weights: {self.pse_class_weights}")
        logging.info(f"cle label statistics: {self.cle_statistics}")
        logging.info(f"pse label statistics: {self.pse_statistics}")
        cle_a, pse_a = np.asarray(cle), np.asarray(pse)
        self.cle_label_groups = {int(l): np.where(cle_a == l)[0] for l in np.unique(cle_a)}
        self.pse_label_groups = {int(l): np.where(pse_a == l)[0] for l in np.unique(pse_a)}
        self.num_samples = len(self.cle_label_groups) * self.balance_label_count

    def indices(self, epoch: int) -> List[int]:
        """The draw of one epoch: ``num_samples`` positions in ``series_uids``; the same list on every rank."""
        rs = np.random.RandomState(self.seed + int(epoch))
        keys = list(self.cle_label_groups.keys())
        out = []
        for _ in range(self.num_samples):
            label = rs.choice(keys)
            out.append(int(rs.choice(self.cle_label_groups[label])))
        return out

    def __len__(self) -> int:
        return self.num_samples
