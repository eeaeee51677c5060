"""Record tests/golden/case_prep.npz by running the REFERENCE's own SubtypingInference.get_data (dataset.py:57-92,
with utils.find_crops and scipy's binary_dilation) on the CPU.

Run in the build container only (the reference checkout and scipy are needed):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_case.py

dataset.py and utils.py are imported unmodified, their absent third-party imports (SimpleITK, cv2, ...) stubbed in
sys.modules the way make_golden.py does for models.py; `read_image` is replaced by the synthetic volumes of
tests/case_prep_ref.py::fixture_cases.  Only arrays are committed -- never reference source.
"""
import importlib
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, REF)

from case_prep_ref import KEYS, fixture_cases      # noqa: E402


def import_ref_dataset():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    for n in ("SimpleITK", "cv2", "hydra", "hydra.utils", "omegaconf", "pytorch_lightning", "pytorch_lightning.loggers",
              "matplotlib", "matplotlib.pyplot", "matplotlib.backends", "matplotlib.backends.backend_agg"):
        try:
            importlib.import_module(n)
        except Exception:
            mod(n)
    for name, attr in (("omegaconf", "OmegaConf"), ("matplotlib.backends.backend_agg", "FigureCanvasAgg"),
                       ("pytorch_lightning.loggers", "TensorBoardLogger")):
        if not hasattr(sys.modules[name], attr):
            setattr(sys.modules[name], attr, object)
    if not hasattr(sys.modules["matplotlib"], "pyplot"):
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    import dataset as ref_dataset
    return ref_dataset


def main():
    ref_dataset = import_ref_dataset()
    rec = {}
    for name, (scan, lobes, spacing, border) in fixture_cases().items():
        ds = ref_dataset.SubtypingInference("/nonexistent/scans", "/nonexistent/lobes", crop_border=border)
        ds.scan_files, ds.lobe_files = ["scan/" + name + ".mha"], ["lobe/" + name + ".mha"]
        vols = {ds.scan_files[0]: scan.numpy(), ds.lobe_files[0]: lobes.numpy()}
        ds.read_image = lambda path: (vols[path].copy(), (0.0, 0.0, 0.0), tuple(spacing), list(np.eye(3).flatten()))
        out = ds.get_data(0)
        assert out["uid"] == name
        rec[f"{name}:scan"], rec[f"{name}:lobes"] = scan.numpy(), lobes.numpy()
        rec[f"{name}:spacing"], rec[f"{name}:border"] = np.asarray(spacing, dtype=np.float64), np.asarray(border)
        for k in KEYS:
            rec[f"{name}:{k}"] = np.asarray(out[k])
        print(name, out["image"].shape, out["crop_slice"].tolist(), int(out["lung_mask"].sum()), int(out["ess_mask"].sum()))
    path = os.path.join(OUT, "case_prep.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
