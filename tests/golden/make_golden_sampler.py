"""Record tests/golden/sampler.json by running the REFERENCE's own SubtypingStratifiedSampler (data_sampler.py:7-52,
with scikit-learn's compute_class_weight) on the CPU.

Run in the build container only (the reference checkout and scikit-learn are needed):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sampler.py

data_sampler.py is imported unmodified.  Its constructor calls ``Sampler.__init__(data_source)``, which the installed
torch no longer accepts: that one constructor is replaced by a no-op before the import.  The data source is a stand-in
with the two attributes the sampler reads.  Only numbers are committed -- never reference source.

Every label list holds class 0 of both columns: the reference's constructor logs ``label_groups[0]`` and cannot be built
without it.
"""
import json
import os
import sys
import types

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)


def expand(counts):
    return [c for c, n in enumerate(counts) for _ in range(n)]


def pair(cle_counts, pse_counts):
    """the two label columns of one case list: every class as often as asked, the PSE column cycled to the CLE length"""
    cle = expand(cle_counts)
    pse = expand(pse_counts)
    assert len(pse) == len(cle), (len(cle), len(pse))
    return cle, pse


CASES = {
    "all_present": pair((7, 4, 3, 3, 2, 1), (11, 6, 3)),
    "cle_4_missing": pair((10, 5, 3, 2, 0, 1), (12, 5, 4)),            # the issue's example
    "pse_2_missing": pair((3, 3, 2, 2, 1, 1), (8, 4, 0)),
    "cle_1_and_5_missing": pair((6, 0, 2, 2, 2, 0), (6, 3, 3)),         # list.insert past the end of a short list
    "pse_1_missing": pair((5, 1, 1, 1, 1, 1), (7, 0, 3)),
    "single_class": pair((9, 0, 0, 0, 0, 0), (9, 0, 0)),
}
BALANCE = 5


def main():
    from torch.utils.data.sampler import Sampler
    Sampler.__init__ = lambda self, *a, **k: None
    import data_sampler as ref

    rec = {}
    for name, (cle, pse) in CASES.items():
        uids = [f"case{i:03d}" for i in range(len(cle))]
        src = types.SimpleNamespace(series_uids=uids,
                                    subtyping_labels={u: {"cle": float(c), "pse": str(p)} for u, c, p in zip(uids, cle, pse)})
        s = ref.SubtypingStratifiedSampler(src, BALANCE)
        rec[name] = {
            "cle": cle, "pse": pse, "balance_label_count": BALANCE,
            "cle_class_weights": [float(v) for v in s.cle_class_weights],
            "pse_class_weights": [float(v) for v in s.pse_class_weights],
            "cle_statistics": {str(int(k)): float(v) for k, v in s.cle_statistics.items()},
            "pse_statistics": {str(int(k)): float(v) for k, v in s.pse_statistics.items()},
            "cle_label_groups": {str(int(k)): [int(i) for i in v] for k, v in s.cle_label_groups.items()},
            "num_samples": int(s.num_samples),
        }
        print(name, rec[name]["cle_class_weights"], rec[name]["pse_class_weights"], rec[name]["num_samples"])
    assert rec["cle_4_missing"]["cle_class_weights"] == [0.2, 0.2, 0.2, 0.234375, 0.46875, 0.46875]
    path = os.path.join(OUT, "sampler.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
