"""CPU: the host side of gradient clipping / accumulation -- harness flags, optimizer arguments, the Lightning hook and
the C prototypes the binding reads from include/dram_hip.h."""
import ctypes
from ctypes import c_float, c_int, c_void_p

import pytest
import torch


def test_parser_flags_have_lightnings_names_and_defaults():
    from bodyct_dram_emph_subtype_amd import train
    a = train.build_parser().parse_args([])
    assert a.gradient_clip_val is None and a.gradient_clip_algorithm == "norm" and a.accumulate_grad_batches == 1
    a = train.build_parser().parse_args(["--gradient_clip_val", "0.5", "--gradient_clip_algorithm", "value",
                                         "--accumulate_grad_batches", "4"])
    assert a.gradient_clip_val == 0.5 and a.gradient_clip_algorithm == "value" and a.accumulate_grad_batches == 4
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--gradient_clip_algorithm", "l1"])


@pytest.mark.parametrize("name", ["FusedAdam", "FusedSGD"])
def test_optimizer_clip_arguments(name):
    from bodyct_dram_emph_subtype_amd import optim
    cls = getattr(optim, name)
    p = [torch.zeros(3, requires_grad=True)]
    with pytest.raises(ValueError):
        cls(p, max_grad_norm=1.0, clip_grad_value=1.0)
    with pytest.raises(ValueError):
        cls(p, max_grad_norm=-1.0)
    with pytest.raises(ValueError):
        cls(p, clip_grad_value=-0.5)
    plain, opt = cls(p), cls(p, max_grad_norm=2.0)
    assert (opt.max_grad_norm, opt.clip_grad_value, opt.last_grad_norm) == (2.0, None, None)
    assert (plain.max_grad_norm, plain.clip_grad_value) == (None, None)
    # plain attributes, not param_groups entries: state_dict() keeps its keys and old checkpoints keep loading
    assert opt.state_dict()["param_groups"][0].keys() == plain.state_dict()["param_groups"][0].keys()
    assert "max_grad_norm" not in opt.defaults and "clip_grad_value" not in opt.defaults
    opt.load_state_dict(plain.state_dict())
    assert opt.max_grad_norm == 2.0
    opt.clip_grad_value = 1.0                      # both set after the fact: refused when the step looks at them
    with pytest.raises(ValueError):
        opt._clip_on()


def test_drop_in_functions_reject_other_norms_and_negative_bounds():
    from bodyct_dram_emph_subtype_amd import optim
    p = [torch.zeros(3, requires_grad=True)]
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(p, 1.0, norm_type=1.0)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_(p, -1.0)
    with pytest.raises(ValueError):
        optim.clip_grad_value_(p, -1.0)


def test_configure_gradient_clipping_routes_the_flags_to_the_optimizer():
    from bodyct_dram_emph_subtype_amd import models
    from bodyct_dram_emph_subtype_amd.optim import FusedAdam
    hook = models._ScanModule.configure_gradient_clipping       # (the hook does not look at the module)
    opt = FusedAdam([torch.zeros(3, requires_grad=True)])
    hook(None, opt, gradient_clip_val=0.5, gradient_clip_algorithm="norm")
    assert (opt.max_grad_norm, opt.clip_grad_value) == (0.5, None)
    hook(None, opt, gradient_clip_val=0.25, gradient_clip_algorithm="value")
    assert (opt.max_grad_norm, opt.clip_grad_value) == (None, 0.25)
    hook(None, opt, gradient_clip_val=2.0)                       # Lightning's default algorithm
    assert (opt.max_grad_norm, opt.clip_grad_value) == (2.0, None)
    hook(None, opt, 0, gradient_clip_val=1.5, gradient_clip_algorithm="norm")     # Lightning 1.x: optimizer_idx in front
    assert (opt.max_grad_norm, opt.clip_grad_value) == (1.5, None)
    hook(None, opt, 3.0, "value")
    assert (opt.max_grad_norm, opt.clip_grad_value) == (None, 3.0)
    hook(None, opt)                                              # no flag: clipping off
    assert (opt.max_grad_norm, opt.clip_grad_value) == (None, None)
    with pytest.raises(ValueError):
        hook(None, opt, gradient_clip_val=1.0, gradient_clip_algorithm="l1")
    with pytest.raises(ValueError):
        hook(None, opt, gradient_clip_val=-1.0)
    with pytest.raises(TypeError):
        hook(None, torch.optim.SGD([torch.zeros(3, requires_grad=True)], lr=0.1), gradient_clip_val=1.0)


def test_new_prototypes_are_bound_from_the_header():
    from bodyct_dram_emph_subtype_amd import _lib
    work = [c_void_p, c_void_p, c_int]             # table, chunks, nchunks
    want = {
        "dram_grad_norm_multi": work + [c_void_p, c_void_p, c_float, c_void_p, c_void_p],
        "dram_grad_scale_multi": work + [c_void_p, c_void_p],
        "dram_adam_multi_clip": work + [c_float] * 8 + [c_void_p, c_void_p],
        "dram_adam_multi_dev_clip": work + [c_void_p, c_void_p, c_void_p],
        "dram_sgd_multi_clip": work + [c_float, c_float, c_float, c_int, c_float, c_void_p, c_void_p],
    }
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (ctypes.c_int, args), name
    # the plain entry points keep their signatures
    assert _lib.SIGNATURES["dram_adam_multi"] == (ctypes.c_int, work + [c_float] * 8 + [c_void_p])
    assert _lib.SIGNATURES["dram_adam_multi_dev"] == (ctypes.c_int, work + [c_void_p, c_void_p])
    assert _lib.SIGNATURES["dram_sgd_multi"] == (ctypes.c_int, work + [c_float, c_float, c_float, c_int, c_float, c_void_p])
    assert _lib.ABI_VERSION == 7
