"""Record tests/golden/heat.npz by driving the REFERENCE's own ScanCLSLightningModule._draw_predictions and
ScanRegLightningModule._draw_predictions (models.py:192-234, :455-493) on the CPU.

Run in the build container only (the reference checkout make_golden.py points at is needed):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_heat.py

models.py is imported unmodified through make_golden.py::import_ref_models (absent third-party imports stubbed).
`self` is a stub carrying what the method reads (trainer root / epoch / stage, the datamodule's series_uids), and
models.draw_mask_tile_singleview_heatmap is replaced by a function that captures its arguments: the windowed scan
and the four uint8 mask volumes are what is recorded.  Only arrays are committed -- never reference source.
"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, OUT)

import make_golden      # noqa: E402  (puts the reference checkout on sys.path)

GRID = (4, 6, 8)        # dense grid; the scan grid is twice that
B = 2


def inputs(kind, seed):
    g = torch.Generator().manual_seed(seed)
    size = tuple(2 * n for n in GRID)
    if kind == "cls":
        dense = [torch.randn(B, 6, *GRID, generator=g), torch.randn(B, 3, *GRID, generator=g)]
    else:
        dense = [torch.rand(B, 1, *GRID, generator=g), torch.rand(B, 1, *GRID, generator=g)]
    scans = torch.randn(B, 1, *size, generator=g)
    lungs = (torch.rand(B, 1, *size, generator=g) > 0.3).float()
    ems = (torch.rand(B, 1, *size, generator=g) > 0.8).float() * lungs
    return dense, scans, lungs, ems


def main():
    ref_models = make_golden.import_ref_models()
    captured = []

    def capture(image, masks_list, coord_mask, num_slices, output_path, **kw):
        captured.append((image, [m for ml in masks_list for m in ml], coord_mask, num_slices, str(output_path), kw))

    ref_models.draw_mask_tile_singleview_heatmap = capture
    rec = {}
    with tempfile.TemporaryDirectory() as root:
        for kind, cls, seed in (("cls", ref_models.ScanCLSLightningModule, 11), ("reg", ref_models.ScanRegLightningModule, 12)):
            dense, scans, lungs, ems = inputs(kind, seed)
            stage = ref_models.VALID_PHASE
            name = getattr(stage, "value", stage)          # Lightning's trainer.state.stage formats as "validate"
            uids = [f"case{i}" for i in range(B)]
            stub = SimpleNamespace(trainer=SimpleNamespace(
                default_root_dir=root, current_epoch=3, state=SimpleNamespace(stage=name),
                datamodule=SimpleNamespace(datasets={stage: SimpleNamespace(series_uids=uids)})))
            labels = [torch.tensor([1, 4]), torch.tensor([0, 2]), torch.tensor([1, 5]), torch.tensor([2, 2])]
            del captured[:]
            cls._draw_predictions(stub, scans, lungs, ems, dense, *labels, torch.arange(B), stage)
            assert len(captured) == B
            vols = []
            for b, (image, masks, coord, num, path, kw) in enumerate(captured):
                assert num == 5 and kw.get("coord_axis") == 0 and len(masks) == 4
                want = "_".join(str(int(labels[i][b])) for i in (0, 2, 1, 3))
                assert path.endswith(f"debug_input_data/3/{name}/case{b}_label_{want}"), path
                assert (coord == (lungs[b, 0].numpy() > 0)).all()
                vols.append(np.stack([image] + masks))
                assert vols[-1].dtype == np.uint8
            rec[f"{kind}:dense0"], rec[f"{kind}:dense1"] = dense[0].numpy(), dense[1].numpy()
            rec[f"{kind}:scans"] = scans[:, 0].numpy()
            rec[f"{kind}:lungs"] = lungs[:, 0].numpy().astype(np.uint8)
            rec[f"{kind}:ems"] = ems[:, 0].numpy().astype(np.uint8)
            rec[f"{kind}:volumes"] = np.stack(vols)            # [B, 5, D, H, W]: scan, lung, cle heat, pse heat, em
            print(kind, rec[f"{kind}:volumes"].shape, [int(v.max()) for v in rec[f"{kind}:volumes"][0]])
    path = os.path.join(OUT, "heat.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
