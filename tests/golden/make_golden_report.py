"""CPU characterisation of the whole predict report: ``processor.predict_case`` + ``processor.write_reports`` on CPU
tensors, every kernel wrapper replaced by its numpy yardstick (tests/densito_ref.py, edt_ref.py, ccl_ref.py,
regions_ref.py), for the 16 combinations of regions / densitometry / core_peel / clusters, each with and without
region names.  ``record()`` returns what tests/golden/predict_report.json holds; tests/test_predict_report_host.py
calls it on the code under test and compares string for string.

    python tests/golden/make_golden_report.py [out.json]

writes the json from the package of the checkout the script lies in.  The committed file is recorded at the commit
BEFORE a change to the report path (copy this script into a checkout of that commit and run it there), never from the
code a test then holds to it.
"""
import itertools
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ccl_ref as CC          # noqa: E402
import densito_ref as DR      # noqa: E402
import edt_ref as ER          # noqa: E402
import regions_ref as RR      # noqa: E402

SHAPE, SPACING, PEEL_MM, N = (12, 14, 16), (1.5, 0.8, 0.8), 2.0, 5
CROP, ORIGINAL = [[1, 13], [2, 16], [3, 19]], [15, 18, 22]
SWITCHES = ("regions", "densitometry", "core_peel", "clusters")
NAMES = {"plain": None, "named": {1: "RUL", 3: "RLL"}}
BASE_ARGS = ("centrilobular_json", "paraseptal_json", "output_json")
OUTPUT_IS_ENTRY = '[{"entity": "case", <the entry without its opening brace>]'
SWITCH_ARG = {"regions": "regions_json", "densitometry": "densitometry_json", "core_peel": "core_peel_json",
              "clusters": "clusters_json"}


def fixture():
    """(image int16, labels uint8) [12,14,16].  Lobes are slabs along y; lobe 4 has no voxel (so lobes 3 and 5 border
    background and lobe 5, two voxels thick, has no core); a few holes give lobe 1 a peel; six lung voxels carry label 9,
    some of them below -950 HU.  Low attenuation: lobe 1 holds clusters of 1, 2 and 5 voxels (a finite D), lobe 2 only
    single voxels and lobe 5 one pair (D is NaN), lobe 3 none.  Lobe 3 carries the HU that bring the sum over the whole
    lung to -1: its mean density is -1 / N, which "{:.3f}" prints as -0.000."""
    lab = CC.slab_lobes(SHAPE, N)
    lab[lab == 4] = 0
    lab[3:5, 1, 4:6] = 0
    lab[8, 0:2, 10] = 0
    lab[5, 4, 2:8] = 9
    img = np.full(SHAPE, -880, dtype=np.int64)
    img[:, :, 1::5] = -930                                     # below the ess threshold, above the LAA ones
    laa = [(2, 0, 3), (6, 2, 7), (6, 2, 8), (9, 1, 3), (9, 1, 4), (9, 1, 5), (9, 0, 4), (10, 1, 4),   # lobe 1: 1, 2, 5
           (1, 3, 3), (4, 5, 9), (7, 4, 12),                                                        # lobe 2: 1, 1, 1
           (5, 4, 3), (5, 4, 4), (5, 4, 6),                                                         # label 9
           (3, 12, 5), (3, 13, 5)]                                                                  # lobe 5: 2
    for v in laa:
        img[v] = -960
    img[0, 3, 0] = -1100                                       # below hu_lo: the first bin's tail
    fill = lab == 3
    need = -1 - int(img[(lab > 0) & ~fill].sum())
    q, r = divmod(need, int(fill.sum()))
    vals = np.full(int(fill.sum()), q, dtype=np.int64)
    vals[:r] += 1
    img[fill] = vals
    assert int(img[lab > 0].sum()) == -1 and int((lab > 0).sum()) > 2000 and abs(int(img.max())) < 32768
    return img.astype(np.int16), lab.astype(np.uint8)


def dense_maps():
    """cle, pse [1,12,14,16] float64, multiples of 1/256 and 1/1024: every sum over them is exact in any order"""
    i = torch.arange(int(np.prod(SHAPE)), dtype=torch.int64).reshape(1, *SHAPE)
    return ((i * 37) % 256).double() / 256.0, ((i * 91 + 5) % 256).double() / 1024.0


class Module:
    """``predict_step`` of the network side: the dense maps are fixed, already on the scan grid; the table is
    regions_ref's"""
    args = SimpleNamespace(n_regions=N)

    def predict_step(self, batch, batch_idx):
        ess = batch["ess_mask"]
        cle, pse = (d * (ess != 0).double() for d in dense_maps())
        lung_sum = batch["lung_mask"].double().sum()
        out = {"cle_dense_outs": cle.unsqueeze(1).float(), "pse_dense_outs": pse.unsqueeze(1).float(),
               "cle_precentages": (cle.sum().reshape(1) / lung_sum).float(),
               "pse_precentages": (pse.sum().reshape(1) / lung_sum).float(),
               "crop_slices": batch.get("crop_slice"), "original_size": batch.get("original_size"), "uids": batch.get("uid")}
        if batch.get("lobe_labels") is not None:
            n = int(batch["n_regions"]) if batch.get("n_regions") is not None else N
            out["region_table"] = RR.table64(cle, pse, ess, batch["lobe_labels"], n)
        return out


def stubs(processor, ops, transforms):
    """[(owner, attribute, replacement)]: the device side of predict_case, on CPU tensors"""
    img, lab = fixture()

    def prepare_case(scan, lobes, spacing, uid=None, want_lobes=False, **kw):
        image, labels = torch.from_numpy(img.copy()), torch.from_numpy(lab.copy())
        case = {"image": image, "lung_mask": labels > 0, "ess_mask": (image < -910) & (labels > 0),
                "crop_slice": torch.tensor(CROP, dtype=torch.int64), "original_size": torch.tensor(ORIGINAL, dtype=torch.int64),
                "uid": uid}
        if want_lobes:
            case["lobe_labels"] = labels
        return case

    def lobe_histogram(image, labels, n_regions=5, hu_lo=-1024, nbins=1024):
        h, s = DR.histogram(image.numpy(), labels.numpy(), n_regions, hu_lo, nbins)
        return torch.from_numpy(h), torch.from_numpy(s)

    def lung_zones(labels, spacing, peel_mm, n_regions=None, **kw):
        _, z, zl = ER.lung_zones(labels.numpy(), spacing, peel_mm, n_regions)
        return torch.from_numpy(z), torch.from_numpy(zl), None

    def laa_components(image, labels, threshold, n_regions, connectivity, by_lobe=True, want_sizes=False):
        key = CC.laa_key(image.numpy(), labels.numpy(), threshold, n_regions, by_lobe)
        comp, t, _ = CC.label(key, connectivity, n_regions)
        return torch.from_numpy(comp.astype(np.int32)), torch.from_numpy(t), None

    paste = lambda d, *a, **k: (None, torch.zeros(2, 2, 2, dtype=torch.uint8))
    return [(transforms, "prepare_case", prepare_case), (transforms, "prepare_sample", lambda case, target: dict(case)),
            (ops, "lobe_histogram", lobe_histogram), (ops, "lung_zones", lung_zones),
            (ops, "laa_components", laa_components), (processor, "resample_paste", paste)]


def record_one(processor, switches, names, tmp):
    """one combination -> {'entry': json text of metrics + error_messages, 'files': {argument: file text; output_json:
    ``OUTPUT_IS_ENTRY`` once the file is found to be the entry in its list wrapper}, 'refused': {argument: ValueError
    message}}"""
    scan = torch.zeros(ORIGINAL, dtype=torch.int16)
    entry = processor.predict_case(Module(), scan, scan.to(torch.uint8), SPACING, SHAPE, uid="case", region_names=names,
                                   peel_mm=PEEL_MM, **switches)
    assert sorted(entry) == ["entity", "error_messages", "full_cle", "full_pse", "metrics"] and entry["entity"] == "case"
    out = {"entry": json.dumps({"metrics": entry["metrics"], "error_messages": entry["error_messages"]}), "files": {},
           "refused": {}}
    allowed = BASE_ARGS + tuple(SWITCH_ARG[s] for s in SWITCHES if switches[s])
    paths = {a: os.path.join(tmp, a) for a in allowed}
    processor.write_reports([entry], **paths)
    for a, path in paths.items():
        with open(path, "rb") as f:
            out["files"][a] = f.read().decode("ascii")
        os.remove(path)
    # the results list repeats the entry: held to it here, byte for byte, and stored as this marker
    assert out["files"]["output_json"] == '[{"entity": "case", ' + out["entry"][1:] + "]"
    out["files"]["output_json"] = OUTPUT_IS_ENTRY
    for s in SWITCHES:
        if not switches[s]:
            path = os.path.join(tmp, SWITCH_ARG[s])
            try:
                processor.write_reports([entry], **{SWITCH_ARG[s]: path})
            except ValueError as e:
                out["refused"][SWITCH_ARG[s]] = str(e)
            assert not os.path.exists(path), SWITCH_ARG[s]
    return out


def record(processor=None, ops=None, transforms=None):
    """{'<r><d><c><k>/<plain|named>': record_one(...)} for all 32 runs; the three modules default to the package's"""
    if processor is None:
        from bodyct_dram_emph_subtype_amd import ops, processor, transforms
    patched = stubs(processor, ops, transforms)
    saved = [(owner, name, getattr(owner, name)) for owner, name, _ in patched]
    out = {}
    try:
        for owner, name, new in patched:
            setattr(owner, name, new)
        with tempfile.TemporaryDirectory() as tmp:
            for bits in itertools.product((False, True), repeat=4):
                switches = dict(zip(SWITCHES, bits))
                for tag, names in NAMES.items():
                    out["".join(str(int(b)) for b in bits) + "/" + tag] = record_one(processor, switches, names, tmp)
    finally:
        for owner, name, old in saved:
            setattr(owner, name, old)
    return out


if __name__ == "__main__":
    target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "predict_report.json")
    with open(target, "w") as f:
        json.dump(record(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{target}: {os.path.getsize(target)} bytes")
