"""Host side of ops._label_view (no GPU): the one check of a label-volume operand, through each of the five wrappers that
read label volumes in place.  Every refusal names its wrapper and comes before the library is even loaded; a bool tensor
and views that need a copy pass the host checks and end at the device check."""
import pytest
import torch


def _wrappers():
    from bodyct_dram_emph_subtype_amd import ops, transforms
    sp = (1.0, 0.7, 0.7)
    return {"prepare_labels": (lambda lab: transforms.prepare_labels(lab, (2, 3, 4)), None),
            "lobe_histogram": (lambda lab: ops.lobe_histogram(torch.zeros(2, 3, 4, dtype=torch.int16), lab), "labels"),
            "lung_zones": (lambda lab: ops.lung_zones(lab, sp, 3.0, n_regions=5), None),
            "label_components": (lambda lab: ops.label_components(lab), None),
            "laa_components": (lambda lab: ops.laa_components(torch.zeros(2, 3, 4, dtype=torch.int16), lab), "labels")}


@pytest.fixture
def no_library(monkeypatch):
    from bodyct_dram_emph_subtype_amd import ops, transforms

    def spy():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(ops, "_L", spy)
    monkeypatch.setattr(transforms, "_L", spy)


@pytest.mark.parametrize("fn", ["prepare_labels", "lobe_histogram", "lung_zones", "label_components", "laa_components"])
def test_label_operand_checks_of_every_wrapper(fn, no_library):
    call, second = _wrappers()[fn]
    lab = torch.zeros(2, 3, 4, dtype=torch.uint8)
    for bad in (lab.float(), lab.to(torch.int32)):
        with pytest.raises(TypeError, match=f"^{fn}: expected uint8, int16 or bool"):
            call(bad)
    for bad in (lab[0], lab[:, :, :0], lab[None]):                     # 2-D, empty, 4-D
        with pytest.raises(ValueError, match=f"^{fn}: .* must be a non-empty \\[D,H,W\\] tensor"):
            call(bad)
    if second is not None:                                             # the wrappers with an image beside the labels
        with pytest.raises(ValueError, match=f"^{fn}: {second} \\(2, 3, 3\\) must have the image's shape \\(2, 3, 4\\)"):
            call(lab[:, :, :3])
    # what passes the host checks ends at the device check: bool (seen as bytes), int16, and the views that are copied
    # first -- a non-unit x stride, a flipped volume (torch has no negative strides: flip is itself a copy)
    for good in (lab.bool(), lab.to(torch.int16), torch.zeros(2, 3, 8, dtype=torch.uint8)[:, :, ::2], lab.flip(2),
                 lab.permute(0, 2, 1).contiguous().permute(0, 2, 1), torch.zeros(2, 6, 4, dtype=torch.uint8)[:, ::2]):
        assert tuple(good.shape) == (2, 3, 4)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(good)


def test_n_regions_range_and_the_voxel_limit():
    from bodyct_dram_emph_subtype_amd import ops
    with pytest.raises(ValueError, match="^f: n_regions must be 1..15, got 16$"):
        ops._n_regions("f", 16)
    with pytest.raises(ValueError, match="^f: n_regions must be 1..7 \\(2 n <= 15 rows downstream\\), got 8$"):
        ops._n_regions("f", 8, 7)
    assert ops._n_regions("f", "7", 7) == 7 and ops._n_regions("f", 15) == 15 and ops._n_regions("f", 1.0) == 1
    with pytest.raises(ValueError, match="^f: volumes of 2\\^31 voxels or more"):
        ops._label_view("f", torch.zeros(1, 1, 1, dtype=torch.uint8).expand(2048, 1024, 1024), "key")
