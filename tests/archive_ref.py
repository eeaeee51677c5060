"""A tiny training archive in the reference's layout (dataset.py:96-155) for the archive tests: merged.csv, one
``<SeriesInstanceUID>.pth`` per case, split csv files.  A plain helper module."""
import csv
import os

import torch


def write_archive(root, n=8, shape=(4, 6, 7), file_labels=(), skip_files=(), skip_rows=()):
    """n cases case00.. in root: merged.csv (+ an unrelated column, labels written as floats), one .pth per case;
    -> (uids, {uid: (cle, pse)})"""
    os.makedirs(root, exist_ok=True)
    g = torch.Generator().manual_seed(5)
    uids = [f"1.2.{40 - i}.case{i:02d}" for i in range(n)]          # sorted order differs from the writing order
    labels = {u: (i % 6, i % 3) for i, u in enumerate(uids)}
    with open(os.path.join(root, "merged.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["SeriesInstanceUID", "site", "CT_Visual_Emph_Severity_P1", "CT_Visual_Emph_Paraseptal_P1"])
        for u in uids:
            if u not in skip_rows:
                w.writerow([u, "x", f"{labels[u][0]}.0", f"{labels[u][1]}.0"])
    for i, u in enumerate(uids):
        if u in skip_files:
            continue
        case = {"image": (torch.rand(shape, generator=g) * 1600 - 1400).to(torch.int16),
                "lung_mask": torch.rand(shape, generator=g) > 0.4}
        if u in file_labels:
            case["cls_label"], case["pse_label"] = torch.tensor(5 - labels[u][0]), torch.tensor(2 - labels[u][1])
        torch.save(case, os.path.join(root, f"{u}.pth"))
    return uids, labels


def write_split(path, uids):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["idx", "SeriesInstanceUID"])
        for i, u in enumerate(uids):
            w.writerow([i, u])
    return str(path)
