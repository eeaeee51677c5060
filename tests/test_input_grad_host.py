"""Host side of the input-gradient feature (no GPU): CPU operands are rejected before anything is launched, and the
new entry points are part of the C ABI table."""
import pytest
import torch


def test_input_gradient_and_stem_bwd_data_reject_cpu_tensors():
    from bodyct_dram_emph_subtype_amd import med3d, ops
    torch.manual_seed(0)
    m = med3d.resnet18segreg().eval()
    x = torch.zeros(1, 1, 16, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.input_gradient(x, out_grads=(torch.ones(1), None))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x.requires_grad_())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.stem_bwd_data(torch.zeros(1, 4, 4, 4, 64), torch.zeros(64, 1, 7, 7, 7), (1, 8, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bn_bwd_apply_eval(torch.zeros(1, 2, 2, 2, 8), None, None, torch.ones(8), None, False)
    with pytest.raises(ValueError):
        ops.stem_bwd_data(torch.zeros(1, 4, 4, 4, 64), torch.zeros(64, 1, 7, 7, 7), (1, 0, 8, 8))


def test_new_entry_points_are_declared():
    from bodyct_dram_emph_subtype_amd import _lib
    for name in ("dram_stem_bwd_data_workspace", "dram_stem_bwd_data", "dram_stem_bwd_data_bf16",
                 "dram_bn_bwd_apply_eval", "dram_bn_bwd_apply_eval_bf16"):
        assert name in _lib.SIGNATURES, name
