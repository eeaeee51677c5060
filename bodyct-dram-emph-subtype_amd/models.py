"""Host-side mirror of the reference's task modules (reference models.py:160-698).

``ScanCLSLightningModule`` / ``ScanRegLightningModule`` keep the reference's method
surface for the train / predict path -- ``forward``, ``training_step``, ``shared_step``,
``predict_step``, ``configure_optimizers`` -- on top of the HIP engine.  When
``pytorch_lightning`` is importable they subclass ``pl.LightningModule`` (so
``Trainer.fit`` / ``processor.py`` work unchanged); otherwise a plain ``nn.Module`` with the
same methods (this image has no Lightning).  The validation / test activation-map panels of
``_draw_predictions`` (models.py:192-234, :455-493) are ``draw_predictions`` / ``heat_volumes`` below, switched on by
``args.draw_predictions``; the confusion-matrix plots and csv dumps of the epoch-end hooks (models.py:278-379,
:594-682) are out of scope.

The dRAM losses (models.py:512-531 + metrics.py) run as fused HIP kernels
(csrc/head_loss.hip) behind ``torch.autograd.Function``; O(B) scalar algebra stays in torch.
"""
from __future__ import annotations

if not __package__:          # imported top-level (this directory on sys.path): bind to the package, see _dropin.py
    import _dropin
    __package__ = _dropin.adopt(__name__)

import os
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .optim import FusedAdam
from .utils import get_model_by_name

try:  # pragma: no cover - not installed in the build image
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    pl = None

    class _Base(nn.Module):
        """Minimal stand-in for pl.LightningModule (same hook names)."""

        def save_hyperparameters(self, *a, **k):
            pass

        def log(self, *a, **k):
            pass

TRAIN_PHASE, VALID_PHASE, TEST_PHASE, PREDICT_PHASE = "train", "validate", "test", "predict"

# dataset.py:99-112 (COPDGeneSubtyping.cle_ratio_map / pse_ratio_map)
CLE_RATIO_MAP = {0: (0.0, 0.01), 1: (0.01, 0.05), 2: (0.05, 0.1), 3: (0.1, 0.2), 4: (0.2, 0.3), 5: (0.3, 1.0001)}
PSE_RATIO_MAP = {0: (0.0, 0.01), 1: (0.01, 0.05), 2: (0.05, 1.0001)}
BETA, GAMMA = 0.7338, 0.2578   # models.py:414-415


def _band_table(ratio_map, tightness=1.0):
    """_generate_regression_labels (models.py:495-510) as a [n_classes, 2] lookup table."""
    rows = []
    for c in sorted(ratio_map):
        lb, ub = ratio_map[c]
        if lb < 1e-7:
            rows.append((0.0, 0.0))
        else:
            m, span = (lb + ub) / 2.0, (ub - lb) * tightness / 2.0
            assert m - span < m + span
            rows.append((m - span, m + span))
    return torch.tensor(rows, dtype=torch.float32)


_CLE_BANDS, _PSE_BANDS = _band_table(CLE_RATIO_MAP), _band_table(PSE_RATIO_MAP)


_BANDS_DEV: Dict[tuple, torch.Tensor] = {}


def _bands(which: str, device) -> torch.Tensor:
    key = (which, device)
    tab = _BANDS_DEV.get(key)
    if tab is None:      # one host->device copy per device (none per step: the step stays graph-capturable)
        tab = _BANDS_DEV[key] = (_CLE_BANDS if which == "cle" else _PSE_BANDS).to(device).contiguous()
    return tab


def generate_regression_labels(cls_targets: torch.Tensor, which: str) -> torch.Tensor:
    return _bands(which, cls_targets.device)[cls_targets.long()]


def interval_regression_loss(outs, reg_targets, weight_factors):
    """models.py:512-521 (O(B) scalars: torch glue)."""
    n = torch.cat([outs.unsqueeze(1), reg_targets], dim=1)
    n = BETA * n ** GAMMA
    K = (0.5 * (n[:, 2] - n[:, 1])) ** 2
    unh = (n[:, 0] - (n[:, 2] + n[:, 1]) / 2.0) ** 2 - K
    return (10.0 * F.leaky_relu(unh, negative_slope=0.0) * weight_factors).sum()


def ratio_to_label(ratios: torch.Tensor, which: str) -> torch.Tensor:
    """_ratio_to_label (models.py:533-537) without the per-sample .item() syncs."""
    rm = CLE_RATIO_MAP if which == "cle" else PSE_RATIO_MAP
    lo = torch.tensor([rm[k][0] for k in sorted(rm)], device=ratios.device)
    hi = torch.tensor([rm[k][1] for k in sorted(rm)], device=ratios.device)
    hit = (lo[None] <= ratios[:, None]) & (ratios[:, None] < hi[None])
    return hit.float().argmax(1).long()


class _SegLossFn(torch.autograd.Function):
    """(mul_loss, seg_loss) of _segmentation_loss (models.py:523-531): dice of the
    lung-masked maps + masked, class-balanced BCE (metrics.py:10-37), labels/masks
    nearest-resized on the fly (models.py:567-570).  One HBM pass forward, one backward."""

    @staticmethod
    def forward(ctx, cle, pse, lungs, ems, binary, smooth=1e-7, smoothness=0.85):
        """smooth: BinaryDice's constant (1e-7 at models.py:412); smoothness: the in-mask BCE weight
        (0.85 at models.py:529)."""
        B, D, H, W = cle.shape
        part = ops.segloss_fwd(cle, pse, lungs, ems, binary, smoothness)
        st, A1, A0, I, S1, S2 = part.double().sum(0).unbind(0)
        N = float(B * D * H * W)
        alpha = (1.0 - st / B).clamp(0.3, 0.7)          # metrics.py:18
        sw = alpha * st + (1.0 - alpha) * (N - st)       # sum of w
        seg = (alpha * A1 + (1.0 - alpha) * A0) / sw
        den = S1 + S2 + smooth                           # BinaryDice(1e-7), models.py:412
        mul = (2.0 * I + smooth) / den
        ctx.smooth, ctx.smoothness = float(smooth), float(smoothness)
        ctx.save_for_backward(cle, pse, lungs, ems, binary, torch.stack([alpha, sw, den, I]))
        return mul.float(), seg.float()

    @staticmethod
    def backward(ctx, g_mul, g_seg):
        cle, pse, lungs, ems, binary, sc = ctx.saved_tensors
        alpha, sw, den, I = sc.unbind(0)
        gm = g_mul.double() if g_mul is not None else torch.zeros((), dtype=torch.float64, device=cle.device)
        gs = g_seg.double() if g_seg is not None else torch.zeros((), dtype=torch.float64, device=cle.device)
        z = torch.zeros((), dtype=torch.float64, device=cle.device)
        coef = torch.stack([gm * 2.0 / den, gm * (2.0 * I + ctx.smooth) / (den * den), gs * alpha / sw,
                            gs * (1.0 - alpha) / sw, z, z, z, z]).float()
        gcle, gpse = ops.segloss_bwd(cle, pse, lungs, ems, binary, coef, ctx.smoothness)
        return gcle, gpse, None, None, None, None, None


def segmentation_loss(dense_cle, dense_pse, ems, lungs, binary):
    """dense_*: [B,1,d,h,w]; ems/lungs: full-res [B,1,D,H,W] float; binary [B] float."""
    B = dense_cle.shape[0]
    c4 = dense_cle.reshape(B, *dense_cle.shape[-3:]).contiguous()
    p4 = dense_pse.reshape(B, *dense_pse.shape[-3:]).contiguous()
    l4 = lungs.reshape(B, *lungs.shape[-3:]).contiguous()
    e4 = ems.reshape(B, *ems.shape[-3:]).contiguous()
    return _SegLossFn.apply(c4, p4, l4, e4, binary.float().contiguous())


class _RegLossFn(torch.autograd.Function):
    """The whole train loss of ScanRegLightningModule.shared_step (models.py:549-574) as three launches: the seg-loss
    pass over the dense maps, one O(B) tail kernel (fold, dice/BCE, both interval losses, the total, the backward's
    coefficients), and -- in backward -- the seg-loss gradient pass.  The four components come back detached."""

    @staticmethod
    def forward(ctx, cle, pse, lungs, ems, reg_cle, reg_pse, cle_labels, pse_labels, cle_w, pse_w):
        B, D, H, W = cle.shape
        binary = torch.logical_or(cle_labels > 0, pse_labels > 0).float()            # models.py:566
        part = ops.segloss_fwd(cle, pse, lungs, ems, binary, 0.85)                    # 0.85: models.py:529
        out, coef, greg = ops.regloss_tail(part, reg_cle, reg_pse, cle_labels, pse_labels, cle_w, pse_w,
                                           _bands("cle", cle.device), _bands("pse", cle.device), B * D * H * W,
                                           1e-7, BETA, GAMMA)                         # 1e-7: BinaryDice, models.py:412
        ctx.save_for_backward(cle, pse, lungs, ems, binary, coef, greg)
        loss, lc, lp, mul, seg = out.unbind(0)
        ctx.mark_non_differentiable(lc, lp, mul, seg)
        return loss, lc, lp, mul, seg

    @staticmethod
    def backward(ctx, g, *_):
        cle, pse, lungs, ems, binary, coef, greg = ctx.saved_tensors
        gcle, gpse = ops.segloss_bwd(cle, pse, lungs, ems, binary, coef * g, 0.85)
        gr = greg * g
        return gcle, gpse, None, None, gr[0], gr[1], None, None, None, None


def reg_train_loss(dense_outs, reg_outs, lungs, ems, cle_labels, pse_labels, cle_w, pse_w):
    """Train branch of ScanRegLightningModule.shared_step (models.py:549-574): loss = interval(cle) + interval(pse)
    + 2 dice + BCE.  Same terms as interval_regression_loss / segmentation_loss above, closed in one tail kernel."""
    B = dense_outs[0].shape[0]

    def vol(t):
        return t.reshape(B, *t.shape[-3:]).float().contiguous()

    def row(t, dtype=torch.float32):
        return t.reshape(B).to(dtype).contiguous()

    loss, lc, lp, mul, seg = _RegLossFn.apply(vol(dense_outs[0]), vol(dense_outs[1]), vol(lungs), vol(ems),
                                              row(reg_outs[0]), row(reg_outs[1]), row(cle_labels, torch.int64),
                                              row(pse_labels, torch.int64), row(cle_w), row(pse_w))
    return loss, dict(loss_cle=lc, loss_pse=lp, mul_loss=mul, seg_loss=seg)


def cls_train_loss(cls_outs, cle_labels, pse_labels, cle_cw, pse_cw):
    """models.py:248-258: two class-weighted cross-entropies on [B,6] / [B,3] (K16, glue)."""
    loss_cle = F.cross_entropy(cls_outs[0], cle_labels, weight=cle_cw)
    loss_pse = F.cross_entropy(cls_outs[1], pse_labels, weight=pse_cw)
    return loss_cle + loss_pse, dict(loss_cle=loss_cle, loss_pse=loss_pse)


def update_class_weights(weights: torch.Tensor, y_true: torch.Tensor, y_pred: torch.Tensor) -> torch.Tensor:
    """models.py:367-377: w <- w * (1 - per-class accuracy), renormalised; the accuracy is diag / row sums of the
    confusion matrix over the labels that occur (sklearn.metrics.confusion_matrix semantics)."""
    labels = torch.unique(torch.cat([y_true, y_pred]))
    if labels.numel() != weights.numel():
        raise ValueError(f"class-weight update: {labels.numel()} classes occur, {weights.numel()} weights "
                         "(the reference's element-wise product fails the same way)")
    hit = (y_true[None, :] == labels[:, None])
    acc = (hit & (y_pred[None, :] == labels[:, None])).sum(1).double() / hit.sum(1).double()
    w = weights.double().to(acc.device) * (1.0 - acc)
    return (w / w.sum()).to(weights.dtype).cpu()


# --------------------------------------------------------------------------- activation-map panels (_draw_predictions)
def _jet_table() -> np.ndarray:
    """The 256 x 3 uint8 RGB 'jet' map from the usual piecewise-linear formula: channel = clip(1.5 - |4 v - k|, 0, 1)
    with k = 3, 2, 1 for red, green, blue and v = i / 255."""
    v = np.arange(256, dtype=np.float64) / 255.0
    rgb = [np.clip(1.5 - np.abs(4.0 * v - k), 0.0, 1.0) for k in (3.0, 2.0, 1.0)]
    return np.floor(np.stack(rgb, axis=1) * 255.0 + 0.5).astype(np.uint8)


JET = _jet_table()


def _lung_bytes(lungs: torch.Tensor) -> torch.Tensor:
    """[B,D,H,W] or [B,1,D,H,W] mask -> contiguous uint8 [B,D,H,W]; bool / uint8 are read as they are (non-zero =
    lung), anything else is reduced with != 0."""
    if lungs.dim() == 5 and lungs.shape[1] == 1:
        lungs = lungs[:, 0]
    if lungs.dim() != 4:
        raise ValueError(f"lungs must be [B,D,H,W] or [B,1,D,H,W], got {tuple(lungs.shape)}")
    if lungs.dtype == torch.bool:
        return lungs.contiguous().view(torch.uint8)
    if lungs.dtype != torch.uint8:
        return (lungs != 0).view(torch.uint8)
    return lungs.contiguous()


def heat_volumes(dense_outs, lungs, head: str, *, zsel=None, want_f32: bool = False, want_u8: bool = True) -> dict:
    """The CLE and PSE heat volumes of the reference's ``_draw_predictions`` on the scan grid, from the dense head
    outputs ``dense_outs = (cle [B,C0,d,h,w], pse [B,C1,d,h,w])`` of ``module.forward`` and the lung mask
    ([B,D,H,W] or [B,1,D,H,W] with (D,H,W) = (2d,2h,2w); bool / uint8, a float mask is reduced with ``!= 0``):

      head "cls" (models.py:201-229)  sum_{c>=1} relu(up_c) / (its maximum over the volume + 1e-7) * lung
      head "reg" (models.py:464-488)  up_0 * lung

    with up = F.interpolate(dense, size=(D,H,W), mode='trilinear').  Fused HIP passes (csrc/heat.hip): the up-sampled
    channels are never written.  ``zsel`` [B,nz]: only those output z slices, [B,nz,H,W], bit-identical to the slices
    of the full volume.  -> {"cle": t, "pse": t}; t is the uint8 volume trunc(255 clamp(v, 0, 1)) (``want_u8``), the
    unclamped float32 volume (``want_f32``), or the pair (f32, u8) when both are asked for."""
    if head not in ("cls", "reg"):
        raise ValueError(f"heat_volumes: head must be 'cls' or 'reg', got {head!r}")
    if len(dense_outs) != 2:
        raise ValueError("heat_volumes: dense_outs is the pair (cle, pse) of module.forward")
    lung = _lung_bytes(lungs)
    out = {}
    for name, d in zip(("cle", "pse"), dense_outs):
        d = d.detach()
        if head == "cls":
            f32, u8 = ops.heat_volume(d, lung, "classsum", ops.heat_peak(d), zsel, want_f32, want_u8)
        else:
            f32, u8 = ops.heat_volume(d, lung, "plain", None, zsel, want_f32, want_u8)
        out[name] = (f32, u8) if (want_f32 and want_u8) else (u8 if want_u8 else f32)
    return out


def panel_slices(z0: int, z1: int, D: int, num_slices: int = 5) -> Optional[List[int]]:
    """The slices ``draw_mask_tile_singleview_heatmap`` (utils.py:125-127, :157-167) shows for ``coord_axis=0`` and its
    default ``flip_axis=0``, from the lung's half-open z extent [z0, z1) in a volume of D slices.  In the flipped
    frame the lung spans s = D - z1 .. e = D - z0 and every (e - s) // num_slices-th slice from s is taken; a lung
    thinner than num_slices falls back to the whole volume (s, e = 0, D - 1), and a stride that is still 0 raises
    ValueError (the reference's ``range(s, e, 0)`` does).  Returns ORIGINAL z indices in display order (the flipped
    frame's, i.e. descending), or None for an empty lung (z1 <= z0: the reference prints "no object found!")."""
    if z1 <= z0:
        return None
    s, e = D - z1, D - z0
    stride = (e - s) // num_slices
    if stride == 0:
        s, e = 0, D - 1
        stride = (e - s) // num_slices
    if stride == 0:
        raise ValueError(f"panel_slices: {D} slices cannot show {num_slices} (range() arg 3 must not be zero)")
    return [D - 1 - k for k in list(range(s, e, stride))[:num_slices]]


def sheet_from_panels(panels: np.ndarray) -> np.ndarray:
    """panels uint8 [5, num, H, W] (scan, lung, CLE heat, PSE heat, LAA-950) -> the tile sheet uint8 [5 H, num W, 3]
    (RGB): one column per slice; row 1 the scan slice in grey, rows 2-5 the jet-coloured mask blended half and half
    over it, (JET[mask] + grey + 1) >> 1.  No zoom, titles or padding (differences from the reference's JPG:
    INTEGRATION.md)."""
    panels = np.asarray(panels)
    if panels.dtype != np.uint8 or panels.ndim != 4:
        raise ValueError("sheet_from_panels: panels must be uint8 [rows, num, H, W]")
    grey = panels[0].astype(np.uint16)[..., None]                         # [num, H, W, 1]
    rows = [np.repeat(panels[0][..., None], 3, axis=-1)]
    rows += [((JET[m].astype(np.uint16) + grey + 1) >> 1).astype(np.uint8) for m in panels[1:]]
    return np.concatenate([np.concatenate(list(r), axis=1) for r in rows], axis=0)


def _window_minmax_u8(sel: torch.Tensor, mn: torch.Tensor, mx: torch.Tensor) -> torch.Tensor:
    """utils.windowing(scan, from_span=None).astype(np.uint8) on the selected slices, in the reference's float32
    operation order: clip, (x - min) / (max - min) * 255, truncate.  A constant volume (max == min) gives zeros where
    the reference divides 0 by 0."""
    rng = mx - mn
    q = (torch.minimum(torch.maximum(sel, mn), mx) - mn) / rng * 255.0
    return torch.where(rng > 0, q, torch.zeros_like(q)).to(torch.uint8)


def _save_sheet(path_stem: str, sheet: np.ndarray) -> str:
    try:
        from matplotlib.image import imsave
    except Exception:  # noqa: BLE001  (no matplotlib: keep the pixels)
        np.save(path_stem + ".npy", sheet)
        return path_stem + ".npy"
    imsave(path_stem + ".png", sheet)
    return path_stem + ".png"


class _ScanModule(_Base):
    _head = None          # "cls" | "reg": which maps _draw_predictions draws (set by the two modules)

    def __init__(self, args):
        self.args = args
        super().__init__()
        self.model = get_model_by_name(args.model_arch)
        self.save_hyperparameters()
        self.trace = True
        # per-class loss weights; the reference reads them from the datamodule's sampler
        # (models.py:248-252, 556-561) and rescales them each epoch (:369-379)
        self.cle_class_weights = torch.full((6,), 1.0 / 6)
        self.pse_class_weights = torch.full((3,), 1.0 / 3)

    def forward(self, x, lungs):
        return self.model(x, lungs)

    def training_step(self, batch, batch_idx):
        return self.shared_step(batch, batch_idx, TRAIN_PHASE)

    def validation_step(self, batch, batch_idx):
        return self.shared_step(batch, batch_idx, VALID_PHASE)

    def test_step(self, batch, batch_idx):
        return self.shared_step(batch, batch_idx, TEST_PHASE)

    # ---- activation-map panels (models.py:192-234 / :455-493) ----------------------------------------------
    def heat_volumes(self, dense_outs, lungs, **kw) -> dict:
        """``heat_volumes`` for this module's networks: the volumes themselves, e.g. to save next to
        ``predict_case``'s output."""
        return heat_volumes(dense_outs, lungs, self._head, **kw)

    def draw_predictions(self, batch, dense_outs, pred_cle, pred_pse, stage, batch_idx=0, epoch=0, root=None,
                         num_slices=5):
        """The reference's ``_draw_predictions``: per sample the five uint8 volumes it hands to
        ``draw_mask_tile_singleview_heatmap`` -- windowed scan, lung * 255, CLE heat, PSE heat, em * 255 -- at the
        ``num_slices`` slices that function shows (``panel_slices``), and the tile sheet.  Returns a list of
        dict(uid, z, panels, sheet, path): ``panels`` uint8 [5, num, H, W] and ``sheet`` uint8 [5 H, num W, 3] on the
        host, ``z`` the original slice indices in display order; all None but ``uid`` for an empty lung.  With ``root``
        the sheet is written to ``root/debug_input_data/<epoch>/<stage>/<uid>_label_<cle>_<predcle>_<pse>_<predpse>.png``
        (``.npy`` without matplotlib).  ``uid`` is the batch's 'uid' entry, else its 'index'.

        Only the shown slices of the heat volumes are computed and written (``heat_volumes(..., zsel=...)``); the scan's
        min / max come from one reduction pass, the windowing of the shown slices is float32 torch glue in the
        reference's operation order.  A constant scan gives a zero row where the reference gives NaN.  The lung's z
        extent (dram_lung_bbox) is read back once per drawn batch, so this path synchronises with the device and
        cannot be captured into a hipGraph."""
        from .transforms import _L, _chk, _p, _stream
        with torch.no_grad():
            scans = batch["image"].float().contiguous()
            lung = _lung_bytes(batch["lung_mask"])
            ems = batch["em_mask"]
            B, D, H, W = lung.shape
            if tuple(scans.shape) != (B, D, H, W) or tuple(ems.shape) != (B, D, H, W):
                raise ValueError("draw_predictions: image, lung_mask and em_mask must share one [B,D,H,W] shape")
            dev = lung.device
            lib = _L()
            boxes = torch.empty((B, 8), device=dev, dtype=torch.int32)
            part = torch.empty((lib.dram_lung_bbox_nblk(D * H * W), 8), device=dev, dtype=torch.int32)
            mm = []
            for b in range(B):
                lb = lung[b] if lung[b].data_ptr() % 16 == 0 else lung[b].clone()    # the bbox pass reads 16-byte vectors
                ops._req(lb, "lung_mask", torch.uint8)
                _chk(lib.dram_lung_bbox(_p(lb), 1, _p(part), _p(boxes[b]), D, H, W, _stream()), "dram_lung_bbox")
                ops._req(scans[b], "image")
                mp = torch.empty((lib.dram_minmax_nblk(D * H * W), 2), device=dev, dtype=torch.float32)
                _chk(lib.dram_minmax(_p(scans[b]), _p(mp), D * H * W, _stream()), "dram_minmax")
                mm.append((mp[:, 0].amin(), mp[:, 1].amax()))                         # O(nblk) glue
            zs = [panel_slices(z0, z1, D, num_slices) for z0, z1, *_ in boxes.tolist()]   # the one host read-back
            nz = max((len(z) for z in zs if z is not None), default=0)
            uids = batch["uid"] if batch.get("uid") is not None else batch["index"].reshape(-1).tolist()
            results = [dict(uid=uids[b], z=zs[b], panels=None, sheet=None, path=None) for b in range(B)]
            if nz == 0:
                return results
            zsel = [z if z is not None else [0] * nz for z in zs]
            heat = heat_volumes(dense_outs, lung, self._head, zsel=zsel)
            labels = [t.reshape(-1).tolist() for t in (batch["cls_label"], pred_cle, batch["pse_label"], pred_pse)]
            for b, z in enumerate(zs):
                if z is None:
                    continue
                zi = torch.tensor(z, device=dev)
                rows = [_window_minmax_u8(scans[b][zi], *mm[b]), (lung[b][zi] != 0).to(torch.uint8) * 255,
                        heat["cle"][b], heat["pse"][b], (ems[b][zi].float() * 255.0).to(torch.uint8)]
                panels = torch.stack(rows).cpu().numpy()
                res = results[b]
                res["panels"], res["sheet"] = panels, sheet_from_panels(panels)
                if root is not None:
                    folder = os.path.join(str(root), "debug_input_data", str(epoch), str(stage))
                    os.makedirs(folder, exist_ok=True)
                    cle, pcle, pse, ppse = (col[b] for col in labels)
                    res["path"] = _save_sheet(os.path.join(folder, f"{res['uid']}_label_{cle}_{pcle}_{pse}_{ppse}"),
                                              res["sheet"])
            return results

    def _maybe_draw(self, batch, batch_idx, stage, dense_outs, out):
        """models.py:266-272: the first ``args.draw_predictions`` validation / test batches, on rank 0 (the reference
        hard-codes 50; the default 0 draws nothing)."""
        if stage == TRAIN_PHASE or not int(getattr(self.args, "draw_predictions", 0) or 0) > batch_idx:
            return
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_rank():
            return
        self.draw_predictions(batch, dense_outs, out["pred_cle_labels"], out["pred_pse_labels"], stage, batch_idx,
                              epoch=self._draw_epoch(), root=getattr(self.args, "model_path", None))

    def _draw_epoch(self):
        """models.py:194-197: ``epoch_number`` when the caller set one (train.py does), else the trainer's epoch"""
        if hasattr(self, "epoch_number"):
            return self.epoch_number
        try:
            return int(self.current_epoch)
        except Exception:  # noqa: BLE001  (no Lightning, or no trainer attached)
            return 0

    # ---- epoch end (models.py:287-317 / :603-633, :367-379) ------------------------------------------------
    def training_epoch_end(self, step_outputs):
        return self.shared_epoch_end(step_outputs, TRAIN_PHASE)

    def validation_epoch_end(self, step_outputs):
        return self.shared_epoch_end(step_outputs, VALID_PHASE)

    def test_epoch_end(self, step_outputs):
        return self.shared_epoch_end(step_outputs, TEST_PHASE)

    def shared_epoch_end(self, step_outputs, phase):
        """Concatenate the step outputs, all-gather them over the ranks (utils.cat_all_gather), take the
        accuracies over everything gathered (models.py:300-301: BEFORE de-duplication), drop the samples the
        distributed sampler repeated (first occurrence per index, :303-309) and, in the train phase, rescale the
        per-class loss weights by (1 - per-class accuracy) (:367-379).  Plots / csv dumps are out of scope;
        returns what they would have been fed."""
        from .utils import cat_all_gather
        with torch.no_grad():
            cols = {k: cat_all_gather(torch.cat([o[k] for o in step_outputs]))
                    for k in ("pred_cle_labels", "cle_labels", "pred_pse_labels", "pse_labels")}
            indices = cat_all_gather(torch.cat([o["index"] for o in step_outputs]))
            acc_cle = (cols["pred_cle_labels"] == cols["cle_labels"]).float().mean()
            acc_pse = (cols["pred_pse_labels"] == cols["pse_labels"]).float().mean()
            order = torch.argsort(indices, stable=True)          # np.unique(indices, return_index=True)
            s = indices[order]
            first = torch.ones_like(s, dtype=torch.bool)
            first[1:] = s[1:] != s[:-1]
            keep = order[first]
            cols = {k: v[keep] for k, v in cols.items()}
            if phase == TRAIN_PHASE:
                for name in ("cle", "pse"):
                    w = getattr(self, f"{name}_class_weights")
                    seen = torch.unique(torch.cat([cols[f"{name}_labels"], cols[f"pred_{name}_labels"]])).numel()
                    if seen == w.numel():
                        setattr(self, f"{name}_class_weights",
                                update_class_weights(w, cols[f"{name}_labels"], cols[f"pred_{name}_labels"]))
                    else:       # the reference's element-wise product raises here (tiny epochs); keep the weights
                        import logging
                        logging.warning(f"{name}: only {seen} of {w.numel()} classes occurred this epoch; class weights kept")
            self.log(f"epoch_{phase}_acc_cle", acc_cle, on_step=False, on_epoch=True)
            self.log(f"epoch_{phase}_acc_pse", acc_pse, on_step=False, on_epoch=True)
            return dict(indices=indices[keep], acc_cle=acc_cle, acc_pse=acc_pse, **cols)

    def configure_optimizers(self):
        """models.py:381-394 / :685-698: Adam(lr=args.lr) + ExponentialLR(gamma=0.95)."""
        optimizer = FusedAdam(self.parameters(), lr=self.args.lr)
        scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.95, last_epoch=-1)
        return [optimizer], [scheduler]

    def configure_gradient_clipping(self, optimizer, *positional, gradient_clip_val=None, gradient_clip_algorithm=None,
                                    **_):
        """Lightning's hook behind --gradient_clip_val / --gradient_clip_algorithm (the reference's
        Trainer.add_argparse_args, train.py:46): instead of Lightning's in-place clip_gradients, which rewrites every
        gradient in torch arithmetic in front of each step, the flags become the fused optimizer's attributes and the
        clipping rides the update (optim.py); no gradient is rewritten.  Lightning 1.x passes optimizer_idx
        positionally in front of the two keywords, 2.x the keywords alone; (value, algorithm) may also be given
        positionally.  None or 0 switches clipping off, as in Lightning."""
        if len(positional) == 2:
            gradient_clip_val, gradient_clip_algorithm = positional
        elif len(positional) > 2 or (positional and not isinstance(positional[0], int)):
            raise TypeError("configure_gradient_clipping(optimizer[, optimizer_idx], gradient_clip_val=..., "
                            "gradient_clip_algorithm=...)")
        algorithm = getattr(gradient_clip_algorithm, "value", gradient_clip_algorithm) or "norm"
        if algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm must be 'norm' or 'value', got {gradient_clip_algorithm!r}")
        if not hasattr(optimizer, "max_grad_norm"):
            raise TypeError("gradient clipping needs a fused optimizer (optim.FusedAdam / FusedSGD)")
        val = None if gradient_clip_val is None or float(gradient_clip_val) == 0.0 else float(gradient_clip_val)
        if val is not None and val < 0:
            raise ValueError(f"gradient_clip_val must be >= 0, got {gradient_clip_val!r}")
        optimizer.max_grad_norm = val if algorithm == "norm" else None
        optimizer.clip_grad_value = val if algorithm == "value" else None


class ScanCLSLightningModule(_ScanModule):
    """reference models.py:160-394 (train/val step part)."""
    _head = "cls"

    def shared_step(self, batch, batch_idx, stage):
        with torch.set_grad_enabled(stage == TRAIN_PHASE):
            scans = batch["image"].unsqueeze(1)
            lungs = batch["lung_mask"].unsqueeze(1).float()
            cle_labels, pse_labels = batch["cls_label"], batch["pse_label"]
            indices = batch["index"].squeeze(-1) if "index" in batch else None
            dense_outs, cls_outs = self.forward(scans, lungs)
            out = {"pred_cle_labels": cls_outs[0].detach().argmax(-1), "pred_pse_labels": cls_outs[1].detach().argmax(-1),
                   "cle_labels": cle_labels.detach(), "pse_labels": pse_labels.detach(), "index": indices}
            if stage == TRAIN_PHASE:
                dev = scans.device
                loss, parts = cls_train_loss(cls_outs, cle_labels, pse_labels, self.cle_class_weights.to(dev),
                                             self.pse_class_weights.to(dev))
                for k, v in parts.items():
                    self.log(f"{TRAIN_PHASE}_{k}", v, on_step=True, on_epoch=True, prog_bar=True)
                self.log(f"{TRAIN_PHASE}_loss", loss, on_step=True, on_epoch=True, prog_bar=True)
                out["loss"] = loss
            else:
                self._maybe_draw(batch, batch_idx, stage, dense_outs, out)
            return out


class ScanRegLightningModule(_ScanModule):
    """reference models.py:397-698 (train/val/predict step part)."""
    _head = "reg"

    def __init__(self, args):
        super().__init__(args)
        self.beta, self.gamma = BETA, GAMMA

    def shared_step(self, batch, batch_idx, stage):
        with torch.set_grad_enabled(stage == TRAIN_PHASE):
            scans = batch["image"].unsqueeze(1)
            lungs = batch["lung_mask"].unsqueeze(1).float()
            ems = batch["em_mask"].unsqueeze(1).float()
            cle_labels, pse_labels = batch["cls_label"], batch["pse_label"]
            indices = batch["index"].squeeze(-1) if "index" in batch else None
            dense_outs, reg_outs = self.forward(scans, lungs)
            out = {"pred_cle_labels": ratio_to_label(reg_outs[0].detach(), "cle"),
                   "pred_pse_labels": ratio_to_label(reg_outs[1].detach(), "pse"),
                   "cle_labels": cle_labels.detach(), "pse_labels": pse_labels.detach(), "index": indices}
            if stage == TRAIN_PHASE:
                dev = scans.device
                cw = self.cle_class_weights.to(dev)[cle_labels.long()]   # per-sample weights, models.py:556-561
                pw = self.pse_class_weights.to(dev)[pse_labels.long()]
                loss, parts = reg_train_loss(dense_outs, reg_outs, lungs, ems, cle_labels, pse_labels, cw, pw)
                for k, v in parts.items():
                    self.log(f"{TRAIN_PHASE}_{k}", v, on_step=True, on_epoch=True, prog_bar=True)
                self.log(f"{TRAIN_PHASE}_loss", loss, on_step=True, on_epoch=True, prog_bar=True)
                out["loss"] = loss
            else:
                self._maybe_draw(batch, batch_idx, stage, dense_outs, out)
            return out

    def predict_step(self, batch, batch_idx: int, dataloader_idx: int = 0):
        """models.py:430-450: eval forward, dRAM up-projection to the scan grid x ess mask,
        percentages normalised by lungs.sum() over the WHOLE batch (:440-441).

        A batch that holds 'lobe_labels' ([B,D,H,W] uint8 on the network grid, ``transforms.prepare_labels``) takes the
        fused tail (``ops.upproject_regions``: both heads and a per-region table in one pass) and returns in addition
        'region_table' [B, n+1, 4] float64 (rows 0..n: sum cle, sum pse, #ess, #voxels; row 0 = label 0 and labels above
        n = the batch's optional 'n_regions' (an int, e.g. 2 x lobes for ``processor.core_peel``'s composite zone labels)
        or else ``args.n_regions``, default 5), 'cle_region_percentages' / 'pse_region_percentages' [B, n] (sum / #voxels of
        that sample's region, NaN for an absent region), 'region_voxels' [B, n] and 'region_ess_fraction' [B, n]."""
        with torch.no_grad():
            scans = batch["image"].unsqueeze(1)
            lungs = batch["lung_mask"].unsqueeze(1).float()
            if batch.get("lobe_labels") is not None:
                return self._predict_regions(batch, scans, lungs)
            ess = batch["ess_mask"].unsqueeze(1).float()
            dense_outs, _ = self.forward(scans, lungs)
            B = scans.shape[0]
            size = tuple(scans.shape[-3:])
            e4 = ess.reshape(B, *size).contiguous()
            res = {}
            lung_sum = lungs.sum()
            for name, d in (("cle", dense_outs[0]), ("pse", dense_outs[1])):
                up, part = ops.upproject(d.reshape(B, *d.shape[-3:]).contiguous(), e4, size)
                res[f"{name}_dense_outs"] = up.unsqueeze(1)
                res[f"{name}_precentages"] = part.sum(1) / lung_sum
            res.update(crop_slices=batch.get("crop_slice"), original_size=batch.get("original_size"),
                       uids=batch.get("uid"))
            return res

    def _predict_regions(self, batch, scans, lungs):
        """predict_step's tail for a batch with 'lobe_labels': one fused pass instead of the two up-projections."""
        def as_bytes(m, name):
            if m.dtype not in (torch.bool, torch.uint8):
                if name == "lobe_labels":
                    raise TypeError(f"predict_step: 'lobe_labels' must be uint8 (transforms.prepare_labels), got {m.dtype}")
                m = m != 0
            return m.contiguous().view(torch.uint8) if m.dtype == torch.bool else m.contiguous()

        dense_outs, _ = self.forward(scans, lungs)
        B = scans.shape[0]
        size = tuple(scans.shape[-3:])
        n = int(batch["n_regions"]) if batch.get("n_regions") is not None else int(getattr(self.args, "n_regions", 5))
        heads = [d.reshape(B, *d.shape[-3:]) for d in dense_outs[:2]]          # channel views: no copy
        if B > 1 and heads[0].stride(0) != heads[1].stride(0):
            heads = [h.contiguous() for h in heads]
        up_c, up_p, table = ops.upproject_regions(heads[0], heads[1], as_bytes(batch["ess_mask"], "ess_mask").reshape(B, *size),
                                                  as_bytes(batch["lobe_labels"], "lobe_labels").reshape(B, *size), size, n)
        lung_sum = lungs.sum()
        vox = table[:, 1:, 3]
        res = {"cle_dense_outs": up_c.unsqueeze(1), "cle_precentages": (table[:, :, 0].sum(1) / lung_sum).float(),
               "pse_dense_outs": up_p.unsqueeze(1), "pse_precentages": (table[:, :, 1].sum(1) / lung_sum).float(),
               "region_table": table, "cle_region_percentages": table[:, 1:, 0] / vox,
               "pse_region_percentages": table[:, 1:, 1] / vox, "region_voxels": vox.round().long(),
               "region_ess_fraction": table[:, 1:, 2] / vox}
        res.update(crop_slices=batch.get("crop_slice"), original_size=batch.get("original_size"), uids=batch.get("uid"))
        return res


def make_args(model_arch: str, lr: float = 1e-4, **kw) -> SimpleNamespace:
    """argparse-Namespace stand-in with the reference's flag names (train.py:20-54)."""
    return SimpleNamespace(model_arch=model_arch, lr=lr, **kw)
