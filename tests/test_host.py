"""CPU: host logic of the package -- C-ABI library loads and exports every declared symbol,
drop-in surface (factories, conf, state_dict contract), optimizer work tables, geometry."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_library_builds_and_exports_every_declared_symbol():
    from bodyct_dram_emph_subtype_amd import _build, _lib
    path = _build.build_library()
    header = open(os.path.join(ROOT, "include", "dram_hip.h")).read()
    declared = set(re.findall(r"\b(dram_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert declared <= exported, declared - exported
    assert len(_lib.SIGNATURES) == len(declared & exported)
    lib = _lib.load()                       # dlopen works without a GPU; no compute call is made
    assert lib.dram_version() == _lib.ABI_VERSION
    assert lib.dram_abi_hash().decode() == _build.abi_hash()
    assert b"gfx950" in lib.dram_build_info()
    # pure host-side entry points (no kernel launch)
    d = _lib.DramConvDesc(2, 16, 32, 32, 64, 16, 32, 32, 128, 3, 1, 4, 4)
    assert lib.dram_conv_num_mtiles(ctypes.byref(d)) == 2 * 64 * 1     # 4^3 residues x 1 tile, per sample
    assert lib.dram_conv3d_bwd_weight_workspace(ctypes.byref(d)) > 0
    bad = _lib.DramConvDesc(2, 16, 32, 32, 64, 15, 32, 32, 128, 3, 1, 4, 4)
    assert lib.dram_conv_num_mtiles(ctypes.byref(bad)) == -1            # inconsistent output dims rejected
    assert lib.dram_stem_num_tiles(2, 64, 128, 128) == 2 * 16 * 16 * 16
    assert [lib.dram_stem_fwd_blocks(n) for n in (1, 24, 8192)] == [1, 24, lib.dram_stem_fwd_blocks(1 << 30)]   # persistent
    assert ctypes.sizeof(_lib.DramTensorRef) == 40 and ctypes.sizeof(_lib.DramChunkRef) == 16


def test_binding_is_parsed_from_the_header():
    """_lib reads prototypes, structs and constants from include/dram_hip.h: one declaration of each kind against
    expectations written here by hand, the struct layouts as the C compiler lays them out, and the constants."""
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_ulonglong, c_void_p, sizeof
    from bodyct_dram_emph_subtype_amd import _lib
    P, I, LL, F, D, SZ, DP = c_void_p, c_int, c_longlong, c_float, c_double, c_size_t, POINTER(_lib.DramConvDesc)
    expect = {
        "dram_version": (I, []),
        "dram_abi_hash": (c_char_p, []),
        "dram_build_info": (c_char_p, []),
        "dram_profile_family_name": (c_char_p, [I]),
        "dram_stream_capture_id": (c_ulonglong, [P]),
        "dram_conv3d_bwd_weight": (I, [P, P, P, DP, P, SZ, P]),
        "dram_wino_workspace": (SZ, [DP, I]),
        "dram_colsum_nparts": (I, [LL, I]),
        "dram_pack_conv_weight_bf16_tiles": (LL, [I, I, I]),
        "dram_bn_bwd_apply": (I, [P, P, P, P, P, P, P, P, P, D, P, P, P, LL, I, I, P]),
        "dram_bn_bwd_apply_eval_bf16": (I, [P, P, P, P, P, P, P, LL, I, I, P]),
        "dram_adam_multi": (I, [P, P, I, F, F, F, F, F, F, F, F, P]),
        "dram_maxpool_fwd": (I, [P, P, P, I, I, I, I, I, P]),
        "dram_profile_read": (I, [P, I]),
        "dram_regloss_tail": (I, [P, I, P, P, P, P, P, P, P, I, P, I, I, D, D, D, D, P, P, P, P]),
        "dram_augment_mask": (I, [P, P, I, I, I, P, P]),
    }
    for name, (res, args) in expect.items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res and list(got_args) == args, (name, got_res, got_args)

    sizes = {"DramConvDesc": 56, "DramTensorRef": 40, "DramChunkRef": 16, "DramPackRef": 40, "DramProfRecord": 40,
             "DramAugment": 280}
    assert {n: sizeof(getattr(_lib, n)) for n in sizes} == sizes
    assert [f for f, _ in _lib.DramConvDesc._fields_] == ["B", "D", "H", "W", "Cin", "Do", "Ho", "Wo", "Cout", "k", "stride",
                                                          "pad", "dil", "flags"]
    assert [f for f, _ in _lib.DramPackRef._fields_] == ["w", "off_f", "off_b", "Cout", "Cin", "taps", "pad"]
    assert (_lib.DramAugment.boxes.offset, _lib.DramAugment.flip_axes.offset, _lib.DramAugment.box_hi.offset) == (8, 248, 268)
    assert (_lib.DramProfRecord.mfma_flops.offset, _lib.DramProfRecord.ms.offset) == (8, 32)
    a = _lib.DramAugment()
    assert len(a.boxes) == 10 and len(a.boxes[0]) == 6 and len(a.box_lo) == 3
    dt = np.dtype(_lib.DramTensorRef)
    assert dt.names == ("p", "g", "m", "v", "n") and dt.itemsize == 40
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 24, 32] and dt["p"] == np.dtype("<u8") and dt["n"] == np.dtype("<i8")
    assert np.dtype(_lib.DramChunkRef) == np.dtype([("tensor", "<i4"), ("pad", "<i4"), ("offset", "<i8")])

    assert (_lib.ABI_VERSION, _lib.OPT_CHUNK, _lib.DRAM_FOLD_TICKET_DOUBLES) == (7, 16384, 256)
    assert (_lib.DRAM_CONV_BWD_OVERLAPPED, _lib.DRAM_CONV_ROUNDING_TOLERANT) == (2, 1)
    assert (_lib.DRAM_OK, _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED, _lib.DRAM_ERR_WORKSPACE) == (0, -1, -2, -3)


def test_header_parser_refuses_what_it_does_not_understand():
    """A header the parser cannot fully understand must not yield a binding: every case raises, naming the culprit."""
    from bodyct_dram_emph_subtype_amd import _lib
    pre = "typedef void* dram_stream_t;\n"
    sigs, structs, consts = _lib.parse_header(
        pre + "#define DRAM_N (-3)\n/* int dram_no(int a); */\ntypedef struct S { const float* p; int32_t a, b[2][3]; } S;\n"
        "int dram_ok(const S* s, long long n,\n            dram_stream_t stream);\nsize_t dram_sz(void);\n")
    assert sigs == {"dram_ok": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]),
                    "dram_sz": (ctypes.c_size_t, [])}
    assert consts == {"DRAM_N": -3} and ctypes.sizeof(structs["S"]) == 40 and structs["S"].b.offset == 12
    for text, culprit in [
            (pre + "int dram_x(short a, dram_stream_t s);", "short"),               # unknown parameter type
            ("int dram_x(int a, dram_stream_t s);", "dram_stream_t"),              # ... a typedef the text does not have
            (pre + "int dram_x(int, dram_stream_t s);", "dram_x"),                  # unnamed parameters
            (pre + "int dram_x(const float*, dram_stream_t s);", "dram_x"),
            (pre + "int dram_x(long long, int b);", "dram_x"),
            ("typedef struct T { short a; } T;", "short"),                          # unknown field type
            ("typedef struct T { int32_t a; } U;", "T"),
            ("short dram_x(int a);", "dram_x"),                                     # unknown return type
            ("float* dram_x(int a);", "dram_x"),
            ("int dram_x(int a)\nint dram_y(void);", "dram_x"),                     # half-matched declarations
            ("int dram_x(int a); int dram_y(int b) { return b; }", "dram_y"),
            ("int dram_x(int a[3]);", "dram_x"),
            ("int dram_x(int a); int dram_x(int a);", "dram_x"),
            ("#define dram_m(a) dram_x(a)\nint dram_x(int a);", "dram_m"),          # a dram_...( that is no entry point
            ("#define DRAM_K (1 << 4)\n", "DRAM_K")]:                               # not a plain integer
        with pytest.raises(ValueError, match=culprit):
            _lib.parse_header(text)


def test_conv_plan_is_host_side_and_consistent(monkeypatch):
    """The library's conv plan (direct / 3-D Winograd pipeline / fused in-plane Winograd) is pure host
    logic: same answers without a GPU; packed-weight sizes, workspaces and forced modes agree."""
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    for k in ("DRAM_CONV_ALGO", "DRAM_WINO_TILING", "DRAM_W2D_V"):
        monkeypatch.delenv(k, raising=False)

    def desc(B, D, H, W, Ci, Co, k=3, s=1, dil=1):
        pad = dil * (k - 1) // 2
        o = lambda n: (n + 2 * pad - (dil * (k - 1) + 1)) // s + 1
        return _lib.DramConvDesc(B, D, H, W, Ci, o(D), o(H), o(W), Co, k, s, pad, dil)

    # BASELINE configs[1] layers (batch 2): (desc, forward plan, weight-gradient plan, Winograd points)
    table = [(desc(2, 16, 32, 32, 512, 512, dil=4), 1, 1, 216),    # layer4: F(4,3) on all three axes
             (desc(2, 16, 32, 32, 256, 256, dil=2), 1, 1, 216),    # layer3: 8x16x16 sub-lattices, 4x4x4 tiles too
             (desc(2, 16, 32, 32, 128, 128), 1, 1, 216),           # layer2: exactly 512 4x4x4 tiles
             (desc(1, 16, 32, 32, 128, 128), 1, 1, 144),           # ... batch 1: 256 of them -> the 4x4x2 tiling
             (desc(2, 64, 128, 128, 128, 64), 1, None, 216),       # decoder, wide input
             (desc(2, 64, 128, 128, 64, 64), 1, 1, 216),           # last decoder stage, narrow: the pipeline since round 4
             (desc(2, 32, 64, 64, 64, 64), 2, 1, None),            # layer1: fused in-plane kernel forward (F(2x2): 10x less
                                                                   # rounding); its weight gradient hands no error on: pipeline
             (desc(2, 64, 128, 128, 64, 32), 2, 2, None),          # us3: 32 output channels -> fused in-plane kernels
             (desc(2, 32, 64, 64, 64, 128, s=2), 0, 0, None),      # strided: direct
             (desc(2, 16, 32, 32, 512, 2048, k=1), 3, 3, None),    # 1x1x1 on a 256-multiple of voxels: plain GEMM
             (desc(1, 5, 6, 7, 128, 64, k=1), 0, 0, None)]         # 1x1x1, ragged voxel count: direct kernel
    for d, fwd, wg, pts in table:
        assert lib.dram_conv_algo(ctypes.byref(d)) == fwd, (d.Cin, d.Cout, d.D)
        if wg is not None:
            assert lib.dram_conv_wgrad_algo(ctypes.byref(d)) == wg, (d.Cin, d.Cout, d.D)
        if pts is not None:
            assert lib.dram_wino_num_points(ctypes.byref(d)) == pts
            assert lib.dram_wino_num_points_bwd(ctypes.byref(d)) == pts      # same tiling for the data gradient today
            assert lib.dram_wino_workspace(ctypes.byref(d), 0) >= 4 * pts * 256 * (d.Cin + d.Cout)
            assert lib.dram_wino_v_elems(ctypes.byref(d)) % (pts * 256 * d.Cin) == 0
    # small volumes keep the finer tiling (at least 512 tiles) and still prefer the pipeline to 16 direct workgroups
    small = desc(1, 8, 16, 16, 512, 512, dil=4)
    assert lib.dram_conv_algo(ctypes.byref(small)) == 1 and lib.dram_wino_num_points(ctypes.byref(small)) == 64
    # forced modes
    d = table[3][0]
    monkeypatch.setenv("DRAM_CONV_ALGO", "1")
    assert lib.dram_conv_algo(ctypes.byref(d)) == 0 and lib.dram_conv_wgrad_algo(ctypes.byref(d)) == 0
    monkeypatch.setenv("DRAM_CONV_ALGO", "2")
    assert lib.dram_conv_algo(ctypes.byref(d)) == 1 and lib.dram_conv_wgrad_algo(ctypes.byref(d)) == 1
    monkeypatch.setenv("DRAM_WINO_TILING", "2,2,2")
    assert lib.dram_wino_num_points(ctypes.byref(d)) == 64
    monkeypatch.setenv("DRAM_CONV_ALGO", "3")
    assert lib.dram_conv_algo(ctypes.byref(d)) == 2 and lib.dram_conv_wgrad_algo(ctypes.byref(d)) == 2
    assert lib.dram_wgrad_w2d_workspace(ctypes.byref(d)) > 0
    odd = desc(1, 9, 11, 13, 96, 64)                                 # Cin not a multiple of 64: no 3-D pipeline
    assert lib.dram_wino_applicable(ctypes.byref(odd)) == 0 and lib.dram_wino2d_applicable(ctypes.byref(odd)) == 1


def test_stray_switches_are_ignored_without_dram_tuning():
    """A/B / test switches count under DRAM_TUNING=1 only: with a stray DRAM_CONV_ALGO (and friends) in the
    environment but no DRAM_TUNING the library answers with its own plan, and the host-side switches keep their
    defaults (clean interpreter: the library caches DRAM_TUNING at first use)."""
    import subprocess
    import sys
    code = (
        "import ctypes, os\n"
        "from bodyct_dram_emph_subtype_amd import _lib, ops\n"
        "lib = _lib.load()\n"
        "d = _lib.DramConvDesc(2, 16, 32, 32, 512, 16, 32, 32, 512, 3, 1, 4, 4)\n"
        "print(lib.dram_conv_algo(ctypes.byref(d)), lib.dram_wino_num_points(ctypes.byref(d)),\n"
        "      ops.tuning_env('DRAM_WGRAD_STREAM', '1'))\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra):
        env = {k: v for k, v in os.environ.items() if not k.startswith("DRAM_")}
        env.update(extra, PYTHONPATH=root)
        return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()

    plain = run({})
    stray = run({"DRAM_CONV_ALGO": "1", "DRAM_WINO_TILING": "2,2,2", "DRAM_WGRAD_STREAM": "0"})
    tuned = run({"DRAM_CONV_ALGO": "1", "DRAM_WINO_TILING": "2,2,2", "DRAM_WGRAD_STREAM": "0", "DRAM_TUNING": "1"})
    assert plain == ["1", "216", "1"]
    assert stray == plain
    assert tuned == ["0", "64", "0"]


def test_factories_conf_and_state_dict_contract():
    from bodyct_dram_emph_subtype_amd import med3d, utils
    m = utils.get_model_by_name("med3ddram18")
    sd = m.state_dict()
    assert len(sd) == 141
    assert tuple(sd["conv1.weight"].shape) == (64, 1, 7, 7, 7)
    for k in ("layer4.1.bn2.running_var", "us1.conv_blocks.0.0.bias", "us3.1.num_batches_tracked", "fcs.1.weight"):
        assert k in sd
    assert tuple(sd["us1.conv_blocks.0.0.weight"].shape) == (64, 576, 3, 3, 3)
    assert m.get_target_layer() is m.us3
    n = {f: sum(p.numel() for p in getattr(med3d, f)(**kw).parameters())
         for f, kw in (("resnet18segcls", dict(n_classes=[6, 3])), ("resnet18segreg", {}), ("resnet50segreg", {}))}
    assert n == {"resnet18segcls": 34480329, "resnet18segreg": 34480098, "resnet50segreg": 47858402}
    r50 = utils.get_model_by_name("med3d50")
    assert tuple(r50.state_dict()["us1.conv_blocks.0.0.weight"].shape) == (64, 2304, 3, 3, 3)
    assert tuple(r50.fcs[0].weight.shape) == (6, 32, 1, 1, 1)
    # the engine's own (cheap) traversal hands out exactly nn.Module's named_parameters() / named_buffers(), also
    # after a conversion replaced the buffers and in a deep copy
    import copy
    for mod in (r50, r50.double(), copy.deepcopy(r50)):
        params, bufs = mod._named_tensors()
        ref_p, ref_b = list(mod.named_parameters()), list(mod.named_buffers())
        assert [k for k, _ in params] == [k for k, _ in ref_p] and all(a is b for (_, a), (_, b) in zip(params, ref_p))
        assert [k for k, _ in bufs] == [k for k, _ in ref_b] and all(a is b for (_, a), (_, b) in zip(bufs, ref_b))
    with pytest.raises(NotImplementedError):
        med3d.ResNetSegReg(med3d.BasicBlock, [2, 2, 2, 2], shortcut_type="B")
    with pytest.raises(FileNotFoundError):
        utils.get_model_by_name("nope")


def test_hydra_style_toplevel_import_of_the_dropin_modules():
    """SURVEY.md §8b B1 / INTEGRATION.md §A.1: with the package DIRECTORY on PYTHONPATH, what
    hydra.utils.instantiate does for `_target_: med3d.resnet18segreg` (reference utils.py:83-85,
    conf/med3ddram18.yaml:1) -- importlib.import_module("med3d") + getattr + call -- must give the drop-in
    factory, and the reference's sibling imports (`from metrics import ...`, `from models import ...`,
    `from utils import ...`) must resolve too.  Run in a clean interpreter from a foreign cwd."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg_dir = os.path.join(root, "bodyct-dram-emph-subtype_amd")
    code = (
        "import importlib, sys\n"
        "assert not any(p.rstrip('/').endswith('repo') for p in sys.path[:1]), sys.path\n"
        "mod = importlib.import_module('med3d')\n"              # hydra's _locate(): import the longest importable prefix
        "m = getattr(mod, 'resnet18segreg')()\n"
        "assert len(m.state_dict()) == 141\n"
        "import bodyct_dram_emph_subtype_amd.med3d as pm\n"
        "assert mod is pm and isinstance(m, pm.ResNetSegReg), (mod, pm)\n"
        "c = importlib.import_module('med3d').resnet50segcls(n_classes=[6, 3])\n"
        "assert tuple(c.fcs[0].weight.shape) == (6, 32, 1, 1, 1)\n"
        "from metrics import BinaryCrossEntropy, BinaryDice, dice_coef\n"
        "from utils import get_model_by_name, load_state_dict_greedy, cat_all_gather\n"
        "from models import ScanRegLightningModule, ScanCLSLightningModule\n"
        "import train, processor, transforms\n"
        "import inspect\n"
        "sig = inspect.signature(BinaryCrossEntropy.__call__)\n"
        "assert list(sig.parameters) == ['self', 'y', 'y_hat', 'mask', 'smoothness'], sig\n"
        "assert sig.parameters['smoothness'].default == 0.65 and sig.parameters['mask'].default is None\n"
        "assert type(get_model_by_name('med3ddram18')).__name__ == 'ResNetSegReg'\n"
        "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=pkg_dir)
    r = subprocess.run([sys.executable, "-c", code], cwd="/tmp", env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_greedy_loader():
    from bodyct_dram_emph_subtype_amd import med3d, utils
    a, b = med3d.resnet18segreg(), med3d.resnet18segreg()
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    sd["conv1.weight"] = torch.zeros(3)          # shape mismatch -> skipped
    sd["unexpected.key"] = torch.zeros(1)
    del sd["fcs.0.bias"]
    before = b.state_dict()["conv1.weight"].clone()
    utils.load_state_dict_greedy(b, sd)
    assert torch.equal(b.state_dict()["conv1.weight"], before)
    assert torch.equal(b.state_dict()["layer1.0.conv1.weight"], a.state_dict()["layer1.0.conv1.weight"])


def test_conv_geometry_and_optimizer_tables():
    from bodyct_dram_emph_subtype_amd import ops, optim
    g = ops.ConvGeom(2, 32, 64, 64, 64, 128, 3, 2, 1, 1)
    assert g.out_shape == (2, 16, 32, 32, 128) and g.taps == 27
    assert abs(g.flops - 2.0 * 2 * 16 * 32 * 32 * 128 * 64 * 27) < 1
    d = g.desc()
    assert (d.Do, d.Ho, d.Wo, d.k, d.stride) == (16, 32, 32, 3, 2)
    table, chunks = optim.build_tables([(1000, 2000, 3000, 4000, 40000), (5, 6, 7, 8, 10)])
    assert len(table) == 2 and len(chunks) == 3 + 1
    assert [int(c["offset"]) for c in chunks] == [0, 16384, 32768, 0]
    assert [int(c["tensor"]) for c in chunks] == [0, 0, 0, 1]
    with pytest.raises(RuntimeError):            # no CPU path for the optimizer either
        p = torch.zeros(4, requires_grad=True)
        p.grad = torch.ones(4)
        optim.FusedAdam([p]).step()


def test_loss_host_algebra_matches_oracle():
    """label tables / interval loss / ratio->label are host-side torch: check vs the oracle."""
    from bodyct_dram_emph_subtype_amd import models
    from oracle import med3d_oracle as orc
    cle = torch.tensor([0, 1, 2, 3, 4, 5])
    assert torch.allclose(models.generate_regression_labels(cle, "cle"),
                          orc.regression_labels(cle.tolist(), orc.CLE_RATIO_MAP))
    pse = torch.tensor([2, 0, 1])
    assert torch.allclose(models.generate_regression_labels(pse, "pse"),
                          orc.regression_labels(pse.tolist(), orc.PSE_RATIO_MAP))
    outs = torch.tensor([0.001, 0.03, 0.5, 0.12, 0.9, 0.31])
    w = torch.rand(6)
    a = models.interval_regression_loss(outs, models.generate_regression_labels(cle, "cle"), w)
    b = orc.interval_regression_loss(outs, orc.regression_labels(cle.tolist(), orc.CLE_RATIO_MAP), w)
    assert torch.allclose(a, b)
    assert torch.equal(models.ratio_to_label(outs, "cle"), orc.ratio_to_label(outs, orc.CLE_RATIO_MAP))
    assert torch.equal(models.ratio_to_label(outs, "pse"), orc.ratio_to_label(outs, orc.PSE_RATIO_MAP))


def test_trainer_harness_flags_and_checkpoint_roundtrip(tmp_path):
    """train.py surface: reference flag names/defaults, Lightning-shaped checkpoints, newest-file
    discovery, --reload_only_weights (greedy weights, fresh optimizer) vs full resume."""
    import time
    from bodyct_dram_emph_subtype_amd import models, train
    a = train.build_parser().parse_args([])
    assert (a.model_arch, a.lr, a.ngpus, a.batch_size, a.num_samples, a.reload_only_weights, a.max_epochs) == \
        ("med3ddram50", 1e-4, 1, 1, 128, 1, 120)
    assert tuple(a.target_size) == (128, 224, 288) and a.momentum == 0.9 and a.weight_decay == 1e-5
    args = train.build_parser().parse_args(["--model_arch", "med3ddram18", "--lr", "3e-4"])
    mod = models.ScanRegLightningModule(args)
    assert all(k.startswith("model.") for k in mod.state_dict())          # Lightning ckpt key contract
    opt = torch.optim.Adam(mod.parameters(), lr=args.lr)                  # CPU stand-in for the optimizer state
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.95)
    ck = train.checkpoint_dict(mod, opt, sched, 3, 42, args)
    assert set(ck) >= {"epoch", "global_step", "state_dict", "optimizer_states", "lr_schedulers"}
    assert train.find_checkpoint(tmp_path) is None
    torch.save(ck, tmp_path / "epoch=03.ckpt")
    time.sleep(0.05)
    torch.save({k: v + 1 for k, v in ck["state_dict"].items() if v.is_floating_point()}, tmp_path / "weights.pth")
    assert train.find_checkpoint(tmp_path).endswith("weights.pth")        # newest by ctime
    assert train.find_checkpoint(tmp_path, "epoch=03.ckpt").endswith("epoch=03.ckpt")
    fresh = models.ScanRegLightningModule(args)
    o2 = torch.optim.Adam(fresh.parameters(), lr=1.0)
    s2 = torch.optim.lr_scheduler.ExponentialLR(o2, gamma=0.95)
    assert train.restore(fresh, o2, s2, str(tmp_path / "epoch=03.ckpt"), reload_only_weights=False) == 4
    assert torch.equal(fresh.state_dict()["model.conv1.weight"], mod.state_dict()["model.conv1.weight"])
    assert abs(o2.param_groups[0]["lr"] - args.lr) < 1e-12               # optimizer state restored
    assert train.restore(fresh, o2, s2, str(tmp_path / "weights.pth"), reload_only_weights=True) == 0
    assert torch.allclose(fresh.state_dict()["model.conv1.weight"], mod.state_dict()["model.conv1.weight"] + 1)


def test_epoch_end_and_class_weight_update_match_reference_fixture():
    """models.py:287-317 / :367-379 through the package's module methods (pure torch glue: runs on CPU tensors),
    against the fixture recorded from the reference's own shared_epoch_end."""
    from bodyct_dram_emph_subtype_amd import models
    g = np.load(os.path.join(ROOT, "tests", "golden", "epoch_end.npz"))
    m = models.ScanCLSLightningModule.__new__(models.ScanCLSLightningModule)
    torch.nn.Module.__init__(m)
    m.cle_class_weights = torch.from_numpy(g["w_cle_before"])
    m.pse_class_weights = torch.from_numpy(g["w_pse_before"])
    t = {k: torch.from_numpy(g[k]) for k in ("index", "cle", "pse", "pred_cle", "pred_pse")}
    outs = [dict(pred_cle_labels=t["pred_cle"][i:i + 8], cle_labels=t["cle"][i:i + 8], pred_pse_labels=t["pred_pse"][i:i + 8],
                 pse_labels=t["pse"][i:i + 8], index=t["index"][i:i + 8]) for i in range(0, 40, 8)]
    r = m.training_epoch_end(outs)
    assert abs(float(r["acc_cle"]) - float(g["acc_cle"])) < 1e-7 and abs(float(r["acc_pse"]) - float(g["acc_pse"])) < 1e-7
    for a, b in (("indices", "dedup_indices"), ("pred_cle_labels", "dedup_pred_cle"), ("pred_pse_labels", "dedup_pred_pse"),
                 ("cle_labels", "dedup_cle"), ("pse_labels", "dedup_pse")):
        assert np.array_equal(r[a].numpy(), g[b]), a
    assert np.allclose(m.cle_class_weights.numpy(), g["w_cle_after"], rtol=1e-12)
    assert np.allclose(m.pse_class_weights.numpy(), g["w_pse_after"], rtol=1e-12)
    # validation phase: same gather / de-dup, weights untouched
    w = m.cle_class_weights.clone()
    m.validation_epoch_end(outs)
    assert torch.equal(w, m.cle_class_weights)


def test_processor_labels_reports_and_augment_parameter_boxes(tmp_path):
    from bodyct_dram_emph_subtype_amd import models, processor, transforms
    g = np.load(os.path.join(ROOT, "tests", "golden", "processor.npz"))
    for p, a, b in zip(g["pcts"], g["cle_scores"], g["pse_scores"]):
        assert processor.ratio_to_label(float(p), models.CLE_RATIO_MAP) == int(a)
        assert processor.ratio_to_label(float(p), models.PSE_RATIO_MAP) == int(b)
    with pytest.raises(IndexError):
        processor.ratio_to_label(1.5, models.CLE_RATIO_MAP)
    res = [{"entity": "scan0", "error_messages": [], "metrics": {"cle_severity_score": "3", "cle_lesion_percentage_per_lung": "0.123",
                                                                   "pse_severity_score": "1", "pse_lesion_percentage_per_lung": "0.020"}}]
    processor.write_reports(res, str(tmp_path / "c.json"), str(tmp_path / "p.json"), str(tmp_path / "o.json"))
    import json
    assert json.load(open(tmp_path / "c.json")) == {"score": 3, "percentage": 0.123}
    assert json.load(open(tmp_path / "p.json")) == {"score": 1, "percentage": 0.02}
    assert json.load(open(tmp_path / "o.json"))[0]["entity"] == "scan0"
    # augmentation parameters -> the C struct (integer boxes of intensity_transforms.py:226-235)
    a = np.load(os.path.join(ROOT, "tests", "golden", "augment.npz"))
    ap = transforms.AugmentParams(noise_sigma=0.045, box_centers=[tuple(c) for c in a["box_centers"]],
                                  box_sizes=[tuple(c) for c in a["box_sizes"]], flip_dims=(2, 0),
                                  crop_center=tuple(a["crop_center"]), crop_size=tuple(a["crop_size"]))
    st = ap.to_struct((12, 20, 28))
    assert st.flags == 15 and st.n_boxes == 3 and st.flip_axes == 5
    zeroed = (a["after_box"] == 0) & (a["after_noise"] != 0)
    box = np.zeros_like(zeroed)
    for b in range(3):
        z0, z1, y0, y1, x0, x1 = list(st.boxes[b])
        box[z0:z1, y0:y1, x0:x1] = True
    assert np.array_equal(box & (a["after_noise"] != 0), zeroed)
    draws = [transforms.TrainAugment(rng=__import__("random").Random(s)).draw() for s in range(200)]
    assert 60 < sum(d.noise_sigma is not None for d in draws) < 140 and all(len(d.box_centers) <= 10 for d in draws)
    assert all(0.03 <= d.noise_sigma <= 0.06 for d in draws if d.noise_sigma is not None)


def test_every_python_source_compiles_and_has_no_merge_markers():
    """bench.py, __graft_entry__.py, tools/ and the package are not imported by the CPU suite as a whole; a stray
    merge marker or syntax error must not wait for the GPU box to be found."""
    import glob
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for sub in ("bodyct-dram-emph-subtype_amd", "tools", "tests", "oracle", os.path.join("tests", "golden")):
        files += glob.glob(os.path.join(ROOT, sub, "*.py"))
    for f in files:
        src = open(f).read()
        compile(src, f, "exec")
        assert not any(ln.startswith(("<" * 7 + " ", ">" * 7 + " ")) for ln in src.splitlines()), f


def test_streaming_kernels_carry_no_hidden_lds_or_spills():
    """tools/isa_waits.py --table on the pool / up-sampling kernels (one hipcc -S, ~15 s): the kernels that declare no
    __shared__ memory must use none -- a private array indexed by a loop variable is silently moved to LDS by the
    compiler (upcat_bwd_src_kernel once carried 56 KB per workgroup that way: two workgroups per CU) -- and nothing
    may spill (scratch reloads count on vmcnt and drain prefetches)."""
    import shutil
    import sys
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not present")
    src = os.path.join(ROOT, "bodyct-dram-emph-subtype_amd", "csrc", "pool_up.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_waits.py"), "--table", src],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.splitlines() if " vgpr " in l]
    assert len(rows) >= 12, r.stdout
    for l in r.stdout.splitlines():
        if " vgpr " not in l:
            continue
        name = l.split("vgpr")[0].split(None, 1)[1].strip()
        vgpr, lds, spills = (int(l.split(k)[1].split()[0]) for k in ("vgpr", "lds", "spills"))
        assert spills == 0, l
        if not name.startswith(("upcat_fwd_tiled_kernel", "upproject_kernel")):       # the two kernels that declare LDS
            assert lds == 0, l
        assert vgpr <= 128, l


# the tuning switches of DESIGN.md, "Tuning switches": what the library reads through tune_env (csrc/common.h) ...
TUNE_ENV_CPP = {
    "DRAM_CONV_ALGO", "DRAM_WINO_TILING", "DRAM_MATH", "DRAM_W2D_V", "DRAM_IGEMM_V", "DRAM_IGEMM_V3_FORCE", "DRAM_WGRAD_V",
    "DRAM_NN_STREAM", "DRAM_NN_STREAM_DB", "DRAM_NN_PERSIST", "DRAM_UPCAT_UNTILED", "DRAM_BF16_NW", "DRAM_BF16_WGRAD",
}
# ... and what the package reads through ops.tuning_env
TUNE_ENV_PY = {
    "DRAM_UPMIX", "DRAM_BF16_S2", "DRAM_STEM_BF16", "DRAM_BWD_BNSTATS", "DRAM_BN_PROLOGUE", "DRAM_CONV_CAT",
    "DRAM_WGRAD_STREAM", "DRAM_SIDE_PRIORITY", "DRAM_INFLIGHT", "DRAM_GRAPH_STREAMS", "DRAM_DIST_TRANSPORT",
}
# settled A/B switches, retired with the kernel forms only they reached (suffixes: this file must not name them either)
RETIRED_SUFFIXES = ("WINO_NT", "WINO_HALF", "NN_NJ", "WINO_EPI", "TN64", "W2D_MARGIN", "W2D_MARGIN_BIG", "WGRAD_MARGIN",
                    "BF16_WGRAD_WGS", "BF16_ZWALK_WGS", "BF16_GEMM1_NB", "BF16_WGRAD1", "BF16_WGRAD_TILE", "BF16_ABL",
                    "POOL_VW", "POOL_BWD", "EW_SHAPE", "EW_U")


def test_tuning_switches_are_the_documented_set():
    """Every switch the library reads through tune_env() and the package through tuning_env() has a row in DESIGN.md's
    table (mirrored above): a new switch needs a row there, and a key in ops._PLAN_ENV if a plan function reads it.  The
    retired A/B switches are named nowhere in the sources, the tools or the tests."""
    import glob
    from bodyct_dram_emph_subtype_amd import ops
    pkg = os.path.join(ROOT, "bodyct-dram-emph-subtype_amd")

    def literals(files, call):
        found = set()
        for f in files:
            found |= set(re.findall(call + r"""\(\s*["'](DRAM_[A-Z0-9_]+)["']""", open(f).read()))
        return found

    csrc = glob.glob(os.path.join(pkg, "csrc", "*"))
    assert literals(csrc, "tune_env") == TUNE_ENV_CPP
    # (every tune_env argument is a literal the scan above can see: no computed names)
    calls = sum(len(re.findall(r"\btune_env\(", open(f).read())) for f in csrc)
    assert calls == sum(len(re.findall(r"""\btune_env\(\s*["']DRAM_""", open(f).read())) for f in csrc) + 1    # + the definition
    assert literals(glob.glob(os.path.join(pkg, "*.py")), "tuning_env") == TUNE_ENV_PY
    assert set(ops._PLAN_ENV) <= TUNE_ENV_CPP
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in TUNE_ENV_CPP | TUNE_ENV_PY:
        assert "| `%s` |" % name in design, name
    retired = re.compile(r"\bDRAM_(%s)\b" % "|".join(RETIRED_SUFFIXES))
    files = csrc + glob.glob(os.path.join(pkg, "*.py"))
    for sub in ("tools", "tests"):
        files += [f for f in glob.glob(os.path.join(ROOT, sub, "*")) if os.path.isfile(f)]
    for f in files:
        m = retired.search(open(f, errors="replace").read())
        assert m is None, (f, m.group(0))


def test_rccl_c_api_binding_loads_every_symbol_it_calls():
    """rccl.py binds librccl's C API by ctypes (the data-parallel transport under the nccl backend): the library torch
    ships must load here and export every entry point the module calls, with the by-value ncclUniqueId of rccl.h:40-43."""
    import ctypes
    from bodyct_dram_emph_subtype_amd import rccl
    L = rccl.lib()
    for name in ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclCommAbort", "ncclAllReduce", "ncclBroadcast",
                 "ncclGetErrorString"):
        assert getattr(L, name) is not None, name
    assert ctypes.sizeof(rccl._UniqueId) == rccl.NCCL_UNIQUE_ID_BYTES == 128
    assert (rccl.SUM, rccl.AVG) == (0, 4) and rccl._DTYPES[__import__("torch").float64] == 8
    # an id's zero bytes survive the trip into bytes and back (a c_char array FIELD reads as a NUL-terminated string)
    raw = bytes([7, 0, 0, 9] * 32)
    uid = rccl._UniqueId()
    ctypes.memmove(ctypes.byref(uid), raw, 128)
    assert rccl._uid_bytes(uid) == raw and len(bytes(uid.internal)) < 128
    assert b"success" in L.ncclGetErrorString(0).lower() or L.ncclGetErrorString(0)
