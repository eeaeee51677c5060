"""The launch ledger of the convolution wrappers (no GPU): one fixed table of calls of ``pack_conv_weight``,
``conv3d_fwd_keep``, ``conv3d_fwd_cat``, ``conv3d_bwd_data``, ``conv3d_bwd_data_bnstats`` and ``conv3d_bwd_weight`` on
'meta' tensors, against tests/golden/conv_dispatch.json: per call every library entry point it launches, in order, with
its arguments and the profiler span it ran in, and what the call returned -- or the exception it raised.

What stands in for the device: ``ops._L`` is a proxy that passes the host-only plan queries (``QUERIES``) on to the real
library -- the plan of a geometry is host code and is asked for real -- and writes every other entry point down
instead of calling it (it answers 0; ``dram_stream_capture_id``, the scratch buffer's question, is answered 0 and
not written); ``ops._stream`` hands out a null handle; ``ops._req`` is a copy of itself without
its two device lines (the GPU suites cover those); ``ops._p`` names its operand instead of taking its address: the role
of an input of the call (``x``, ``wf``, ...) or ``fresh(shape, dtype)`` for a tensor the wrapper allocated; the
profiler is a recorder with a ``span`` method.  Integers, the fields of the ``DramConvDesc`` (``flags`` last) and the
workspace byte count are written as they are.

The json was recorded with this file at the commit BEFORE the wrappers were put on one dispatch table
(``python tests/test_conv_dispatch_host.py --write FILE`` in a checkout of it; the commit is the json's 'parent').  Every
entry must match exactly.  Plan queries are not part of an entry: they may become fewer -- and once one call has
warmed the plan cache, a second identical call makes none at all."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys
from typing import NamedTuple

import torch

from conftest import GOLDEN, ROOT

LEDGER = os.path.join(GOLDEN, "conv_dispatch.json")
F32, BF16 = torch.float32, torch.bfloat16
# the library's host-only plan queries: forwarded, never written down
QUERIES = frozenset("""dram_conv_algo dram_conv_wgrad_algo dram_wino_num_points dram_wino_num_points_bwd dram_conv_num_mtiles
    dram_wino_num_stat_rows dram_wino2d_num_stat_rows dram_conv1x1_num_stat_rows dram_wino_num_stat_rows_bwd
    dram_wino_workspace dram_wino_v_elems dram_conv1x1_bwd_weight_workspace dram_wgrad_w2d_workspace
    dram_conv3d_bwd_weight_workspace dram_wino_prologue_supported dram_conv_bf16_supported dram_conv_bf16_num_stat_rows
    dram_conv3d_bwd_weight_bf16_workspace dram_pack_conv_weight_bf16_tiles""".split())
# every switch that changes a plan or a route: unset while the table runs, except where an entry sets one
SWITCHES = ("DRAM_CONV_ALGO", "DRAM_WINO_TILING", "DRAM_MATH", "DRAM_W2D_V", "DRAM_IGEMM_V", "DRAM_IGEMM_V3_FORCE",
            "DRAM_WGRAD_V", "DRAM_BF16_NW", "DRAM_BF16_WGRAD", "DRAM_NN_STREAM", "DRAM_BF16_S2", "DRAM_BN_PROLOGUE",
            "DRAM_CONV_CAT", "DRAM_BWD_BNSTATS")


# Set by an entry: the proxy answers the pipeline's weight-gradient workspace query with 0, what the library says of a
# geometry whose TN GEMM it cannot plan (today it plans them all) -- the weight gradient then runs the direct kernel.
NO_TN_PLAN = "TEST_CONV_DISPATCH_NO_TN_PLAN"


class Op(NamedTuple):
    """an input tensor of a call: its role in the ledger, its shape and type"""
    role: str
    shape: tuple
    dtype: torch.dtype = F32


class Packed(NamedTuple):
    """the packed weight ``pack_conv_weight(w, g=g, dtype=dtype)`` hands the consumer: 'wf' or 'wb'"""
    role: str
    g: object
    dtype: torch.dtype = F32
    grow: int = 0               # rows added to its leading dimension (a wrong shape)


class Recorder:
    """ops._L(), ops._stream(), ops._p() and the profiler of one recording"""

    def __init__(self, ops):
        self.ops, self.real = ops, ops._lib.load()
        self.lines, self.queries, self.roles, self.open = [], 0, {}, None
        self.stream = ctypes.c_void_p(None)

    def __getattr__(self, name):
        if not name.startswith("dram_"):
            raise AttributeError(name)
        fn = getattr(self.real, name)                   # an entry point the library does not have is an error here too
        if name in QUERIES:
            def query(*args):
                self.queries += 1
                if name == "dram_wino_workspace" and args[1] == 2 and os.environ.get(NO_TN_PLAN):
                    return 0
                return fn(*args)
            return query

        def launch(*args):
            if name != "dram_stream_capture_id":
                self.lines.append((f"[{self.open}] " if self.open else "") + f"{name}({', '.join(self.show(a) for a in args)})")
            return 0
        return launch

    @contextlib.contextmanager
    def span(self, family, flops, detail=""):
        """one ledger line per launch: the span it ran in goes in front of it"""
        self.open, n = f"{family} | {flops:.6g} | {detail}", len(self.lines)
        try:
            yield
        finally:
            if len(self.lines) == n:
                self.lines.append(f"[{self.open}] nothing launched")
            self.open = None

    def name(self, t):
        if t is None:
            return "null"
        role = self.roles.get(id(t))
        return role if role is not None else f"fresh({tuple(t.shape)}, {str(t.dtype).replace('torch.', '')})"

    def show(self, a):
        if a is None or isinstance(a, str):
            return a or "null"
        if a is self.stream:
            return "stream"
        if isinstance(a, torch.Tensor):
            return self.name(a)
        if isinstance(a, (tuple, list)):
            return "(" + ", ".join(self.show(v) for v in a) + ")"
        if type(a).__name__ == "CArgObject":            # ctypes.byref(DramConvDesc)
            return "desc(" + ",".join(str(getattr(a._obj, f)) for f, _ in a._obj._fields_) + ")"
        assert isinstance(a, (int, float)), a
        return repr(a)


def _req_without_device(t, name, dtype=F32, shape=None):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name}: expected a device tensor (libdram_hip has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


@contextlib.contextmanager
def recording():
    from bodyct_dram_emph_subtype_amd import ops
    rec = Recorder(ops)
    saved = {n: getattr(ops, n) for n in ("_L", "_stream", "_req", "_p", "_PROFILER")}
    plans = dict(ops._PLANS)
    env = {k: os.environ.pop(k, None) for k in SWITCHES}
    ops._L, ops._stream, ops._req, ops._p = (lambda: rec), (lambda: rec.stream), _req_without_device, rec.name
    ops.set_profiler(rec)
    try:
        yield rec
    finally:
        for n, v in saved.items():
            setattr(ops, n, v)
        for k, v in env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        ops._WORKSPACE.clear()
        ops._PLANS.clear()                              # (a plan made under NO_TN_PLAN must not outlive the recording)
        ops._PLANS.update(plans)


def outcome(rec, entry) -> list:
    """the ledger lines of one table entry: launches and spans in order, then '-> what it returned' or '!! the exception'"""
    fn, args, kw, env = entry
    ops = rec.ops
    os.environ.update(env)
    try:
        rec.roles, held = {}, []

        def tensor(a):
            if isinstance(a, Packed):
                w = torch.empty((a.g.Cout, a.g.Cin, a.g.k, a.g.k, a.g.k), device="meta")
                t = ops.pack_conv_weight(w, a.role == "wf", a.role == "wb", a.g, a.dtype)[a.role == "wb"]
                if a.grow:
                    t = torch.empty((t.shape[0] + a.grow,) + tuple(t.shape[1:]), dtype=t.dtype, device="meta")
                a = Op(a.role, None)
            elif isinstance(a, Op):
                t = torch.empty(a.shape(ops) if callable(a.shape) else a.shape, dtype=a.dtype, device="meta")
            elif isinstance(a, tuple) and not hasattr(a, "_fields"):
                return tuple(tensor(v) for v in a)
            else:
                return a
            held.append(t)
            rec.roles[id(t)] = a.role
            return t

        args, kw = [tensor(a) for a in args], {k: tensor(v) for k, v in kw.items()}
        ops._WORKSPACE.clear()                          # the scratch is grow-only: each call sees its own size
        rec.lines = []
        try:
            tail = "-> " + rec.show(getattr(ops, fn)(*args, **kw))
        except Exception as e:                          # noqa: BLE001 -- whatever escapes IS the outcome
            return [f"!! {type(e).__name__}: {e}"]      # of a refusal the type and the message, not how far it got
        return rec.lines + [tail]
    finally:
        for k in env:
            del os.environ[k]


def _table():
    """[(id, (wrapper, args, kwargs, environment))]: the ids are the json's keys"""
    from bodyct_dram_emph_subtype_amd import ops
    cases = []

    def geom(B, D, H, W, Ci, Co, k=3, s=1, dil=1):
        return ops.ConvGeom(B, D, H, W, Ci, Co, k, s, dil * (k - 1) // 2, dil)

    def add(name, fn, *args, env=None, **kw):
        assert name not in dict(cases), name
        cases.append((name, (fn, args, kw, dict(env or {}))))

    def flags(**kw):
        return "".join(k[0] if v else "-" for k, v in kw.items())

    def operands(g, dt):
        C = dict(x=Op("x", g.in_shape, dt), dy=Op("dy", g.out_shape, dt), bias=Op("bias", (g.Cout,)),
                 add=Op("add", g.in_shape, dt), gate=Op("gate", g.in_shape, dt), wf=Packed("wf", g, dt), wb=Packed("wb", g, dt),
                 w=Op("w", (g.Cout, g.Cin, g.k, g.k, g.k)), out=Op("out", (g.Cout, g.Cin, g.k, g.k, g.k)),
                 v=Op("v_cache", lambda o: (o.conv_plan(g).v_elems,)))
        C.update({n: Op(n, (g.Cin,)) for n in ("scale", "shift", "mean", "invstd")})
        return C

    def pipeline_forms(tag, g, env=None):
        """the forms only the Winograd pipeline has -- each is a launch or the wrapper's refusal, whatever the plan says"""
        o = operands(g, F32)
        add(f"{tag}/fwd/prologue", "conv3d_fwd_keep", o["x"], o["wf"], o["bias"], g, True, True, prologue=(o["scale"], o["shift"]),
            env=env)
        if g.Cin >= 128:
            x0, x1 = (Op(n, g.in_shape[:4] + (c,)) for n, c in (("x0", 64), ("x1", g.Cin - 64)))
            add(f"{tag}/fwd_cat", "conv3d_fwd_cat", x0, x1, o["wf"], o["bias"], g, True, True, env=env)
        for ovl in (False, True):
            add(f"{tag}/dgrad_bnstats/{flags(overlapped=ovl)}", "conv3d_bwd_data_bnstats", o["dy"], o["wb"], g, Op("bn_y", g.in_shape),
                o["mean"], o["invstd"], o["scale"], o["shift"], overlapped=ovl, env=env)
        add(f"{tag}/wgrad/cache", "conv3d_bwd_weight", None, o["dy"], g, v_cache=o["v"], env=env)
        add(f"{tag}/wgrad/x_and_cache", "conv3d_bwd_weight", o["x"], o["dy"], g, out=o["out"], v_cache=o["v"], env=env)

    def every_form(tag, g, env=None):
        o = operands(g, F32)
        for f, b in ((True, True), (True, False), (False, True), (False, False)):
            add(f"{tag}/pack/{flags(fwd=f, bwd=b)}", "pack_conv_weight", o["w"], f, b, g, env=env)
        for bias, stats, keep in ((None, False, False), (o["bias"], False, False), (None, True, False), (o["bias"], True, True)):
            add(f"{tag}/fwd/{flags(bias=bias, stats=stats, keep=keep)}", "conv3d_fwd_keep", o["x"], o["wf"], bias, g, stats, keep, env=env)
        for a, gt, ovl in ((None, None, False), (o["add"], None, False), (None, o["gate"], False), (None, None, True),
                           (o["add"], o["gate"], True)):
            add(f"{tag}/dgrad/{flags(add=a, gate=gt, overlapped=ovl)}", "conv3d_bwd_data", o["dy"], o["wb"], g, a, gt, ovl, env=env)
        add(f"{tag}/wgrad", "conv3d_bwd_weight", o["x"], o["dy"], g, env=env)
        add(f"{tag}/wgrad/out", "conv3d_bwd_weight", o["x"], o["dy"], g, out=o["out"], env=env)
        pipeline_forms(tag, g, env)

    def one_of_each(tag, g, env=None, dt=F32):
        o = operands(g, dt)
        add(f"{tag}/pack", "pack_conv_weight", o["w"], True, True, g, dt, env=env)
        add(f"{tag}/fwd", "conv3d_fwd_keep", o["x"], o["wf"], o["bias"], g, True, True, env=env)
        add(f"{tag}/dgrad", "conv3d_bwd_data", o["dy"], o["wb"], g, o["add"], o["gate"], True, env=env)
        add(f"{tag}/wgrad", "conv3d_bwd_weight", o["x"], o["dy"], g, env=env)

    # ------------------------------------------------ the config-1 layers of test_host.py's plan table
    layers = [("layer4", geom(2, 16, 32, 32, 512, 512, dil=4)), ("layer3", geom(2, 16, 32, 32, 256, 256, dil=2)),
              ("layer2", geom(2, 16, 32, 32, 128, 128)), ("layer2_b1", geom(1, 16, 32, 32, 128, 128)),
              ("decoder_wide", geom(2, 64, 128, 128, 128, 64)),         # its weight-gradient plan is the table's None
              ("decoder_last", geom(2, 64, 128, 128, 64, 64)), ("layer1", geom(2, 32, 64, 64, 64, 64)),
              ("us3", geom(2, 64, 128, 128, 64, 32)), ("strided", geom(2, 32, 64, 64, 64, 128, s=2)),
              ("gemm1x1", geom(2, 16, 32, 32, 512, 2048, k=1)), ("ragged1x1", geom(1, 5, 6, 7, 128, 64, k=1))]
    for tag, g in layers:                               # every form where a forward / weight-gradient pair of plans first shows
        (every_form if tag in ("layer4", "layer2_b1", "layer1", "us3", "strided", "gemm1x1") else one_of_each)(tag, g)
    pipeline_forms("decoder_wide", layers[4][1])
    one_of_each("tolerant/layer2", ops.ConvGeom(2, 16, 32, 32, 128, 128, 3, 1, 1, 1, ops._lib.DRAM_CONV_ROUNDING_TOLERANT))
    # ------------------------------------------------ the plan-changing switches, on layer2 at batch 1
    g = layers[3][1]
    for tag, env in (("algo1", {"DRAM_CONV_ALGO": "1"}), ("algo2", {"DRAM_CONV_ALGO": "2"}),
                     ("algo2_f222", {"DRAM_CONV_ALGO": "2", "DRAM_WINO_TILING": "2,2,2"}), ("algo3", {"DRAM_CONV_ALGO": "3"})):
        one_of_each(f"{tag}/layer2_b1", g, env)
        pipeline_forms(f"{tag}/layer2_b1", g, env)
    for tag, env in (("no_prologue", {"DRAM_BN_PROLOGUE": "0"}), ("no_cat", {"DRAM_CONV_CAT": "0"}),
                     ("no_bnstats", {"DRAM_BWD_BNSTATS": "0"})):
        pipeline_forms(f"{tag}/layer2_b1", g, env)
    # ------------------------------------------------ small shapes of the GPU convolution tests, as those set the plan
    for name, env, shapes, pipeline in (
            ("direct", {"DRAM_CONV_ALGO": "1"}, [(1, 6, 8, 10, 32, 32, 3, 1, 1), (1, 5, 9, 7, 64, 128, 3, 1, 2), (2, 10, 18, 34, 128, 64, 3, 2, 1),
                                                 (1, 9, 11, 13, 64, 64, 3, 2, 1), (2, 4, 6, 5, 128, 64, 1, 1, 1)], False),
            ("gemm1x1", {}, [(1, 4, 8, 8, 64, 64, 1, 1, 1), (1, 8, 16, 32, 512, 192, 1, 1, 1)], False),
            ("wino2d", {"DRAM_CONV_ALGO": "3"}, [(2, 9, 11, 13, 32, 64, 3, 1, 1), (1, 18, 10, 9, 64, 32, 3, 1, 1), (1, 33, 8, 8, 96, 96, 3, 1, 1)],
             False),
            ("wino444", {"DRAM_CONV_ALGO": "2", "DRAM_WINO_TILING": "4,4,4"},
             [(2, 7, 10, 9, 64, 128, 3, 1, 1), (1, 9, 12, 10, 128, 64, 3, 1, 2), (1, 2, 5, 3, 64, 64, 3, 1, 4)], True),
            ("wino222", {"DRAM_CONV_ALGO": "2", "DRAM_WINO_TILING": "2,2,2"}, [(2, 4, 8, 8, 192, 320, 3, 1, 1)], True),
            ("wino244", {"DRAM_CONV_ALGO": "2", "DRAM_WINO_TILING": "2,4,4"}, [(1, 6, 12, 12, 64, 64, 3, 1, 1)], True)):
        for s in shapes:
            tag = f"small/{name}/" + "x".join(map(str, s))
            one_of_each(tag, geom(*s), env)
            if pipeline:
                pipeline_forms(tag, geom(*s), env)
    # ------------------------------------------------ a pipeline geometry without a TN plan (no other entry uses this geometry)
    g_tn, no_tn = geom(1, 8, 8, 8, 128, 192), {"DRAM_CONV_ALGO": "2", NO_TN_PLAN: "1"}
    every_form("no_tn_plan", g_tn, no_tn)
    # ------------------------------------------------ bf16 storage: native 3x3x3 and 1x1x1, space to depth, casts
    s2 = geom(2, 32, 64, 64, 64, 128, s=2)
    for tag, g, env in (("native3", geom(2, 16, 32, 32, 128, 128), None), ("native1", geom(2, 16, 32, 32, 512, 2048, k=1), None),
                        ("s2d", s2, None), ("s2d_off", s2, {"DRAM_BF16_S2": "0"}), ("casts_odd", geom(1, 7, 8, 9, 64, 64, s=2), None),
                        ("casts_narrow", geom(1, 6, 8, 10, 48, 24), None)):
        one_of_each(f"bf16/{tag}", g, env, BF16)
        o = operands(g, BF16)
        add(f"bf16/{tag}/pack/fwd_only", "pack_conv_weight", o["w"], True, False, g, BF16, env=env)
        add(f"bf16/{tag}/fwd/plain", "conv3d_fwd_keep", o["x"], o["wf"], None, g, False, False, env=env)
        add(f"bf16/{tag}/dgrad/plain", "conv3d_bwd_data", o["dy"], o["wb"], g, env=env)
        add(f"bf16/{tag}/wgrad/out", "conv3d_bwd_weight", o["x"], o["dy"], g, out=o["out"], env=env)
    add("bf16/native3/pack/no_geometry", "pack_conv_weight", Op("w", (128, 128, 3, 3, 3)), True, True, None, BF16)
    add("bf16/native3/fwd/fp32_operands", "conv3d_fwd_keep", Op("x", (2, 16, 32, 32, 128)), Packed("wf", geom(2, 16, 32, 32, 128, 128)), None,
        geom(2, 16, 32, 32, 128, 128), True, True)
    # ------------------------------------------------ refusals
    g, gd = layers[2][1], layers[8][1]                                   # a pipeline geometry, a direct one
    o, od = operands(g, F32), operands(gd, F32)
    add("refuse/fwd/wf_shape", "conv3d_fwd_keep", o["x"], Packed("wf", g, grow=1), o["bias"], g, True, True)
    add("refuse/fwd/wf_shape_ahead_of_bias", "conv3d_fwd_keep", o["x"], Packed("wf", g, grow=1), Op("bias", (g.Cout + 1,)), g, True, True)
    add("refuse/fwd/x_shape_ahead_of_wf", "conv3d_fwd_keep", Op("x", g.out_shape[:4] + (3,)), Packed("wf", g, grow=1), None, g, False, False)
    add("refuse/fwd/bias_shape", "conv3d_fwd_keep", o["x"], o["wf"], Op("bias", (g.Cout + 1,)), g, False, False)
    add("refuse/fwd/prologue_direct", "conv3d_fwd_keep", od["x"], od["wf"], None, gd, True, False, prologue=(od["scale"], od["shift"]))
    add("refuse/fwd/prologue_ahead_of_x", "conv3d_fwd_keep", Op("x", (1,)), od["wf"], None, gd, True, False,
        prologue=(od["scale"], od["shift"]))
    add("refuse/fwd/prologue_bf16", "conv3d_fwd_keep", Op("x", g.in_shape, BF16), Packed("wf", g, BF16), None, g, True, False,
        prologue=(o["scale"], o["shift"]))
    add("refuse/fwd/prologue_scale_shape", "conv3d_fwd_keep", o["x"], o["wf"], None, g, True, False,
        prologue=(Op("scale", (g.Cin + 1,)), o["shift"]))
    add("refuse/fwd/bf16_bias_ahead_of_wf", "conv3d_fwd_keep", Op("x", g.in_shape, BF16), Packed("wf", g, BF16, grow=1),
        Op("bias", (g.Cout + 1,)), g, False, False)
    add("refuse/fwd/bf16_wf_shape", "conv3d_fwd_keep", Op("x", g.in_shape, BF16), Packed("wf", g, BF16, grow=1), None, g, False, False)
    for c0 in (32, 96):
        x0, x1 = (Op(n, g.in_shape[:4] + (c,)) for n, c in (("x0", c0), ("x1", g.Cin - c0)))
        add(f"refuse/fwd_cat/blocks_{c0}", "conv3d_fwd_cat", x0, x1, o["wf"], None, g, True, True)
    x0, x1 = (Op(n, g.in_shape[:4] + (64,)) for n in ("x0", "x1"))
    add("refuse/fwd_cat/blocks_short", "conv3d_fwd_cat", x0, Op("x1", g.in_shape[:4] + (128,)), o["wf"], None, g, True, True)
    add("refuse/fwd_cat/bf16", "conv3d_fwd_cat", Op("x0", x0.shape, BF16), Op("x1", x1.shape, BF16), o["wf"], None, g, True, True)
    add("refuse/fwd_cat/x1_shape", "conv3d_fwd_cat", x0, Op("x1", (1,) + g.in_shape[1:4] + (64,)), o["wf"], None, g, True, True)
    add("refuse/fwd_cat/wf_shape", "conv3d_fwd_cat", x0, x1, Packed("wf", g, grow=1), None, g, True, True)
    add("refuse/dgrad/wb_shape", "conv3d_bwd_data", o["dy"], Packed("wb", g, grow=1), g)
    add("refuse/dgrad/add_shape", "conv3d_bwd_data", o["dy"], o["wb"], g, Op("add", g.out_shape[:4] + (3,)))
    add("refuse/dgrad/add_dtype", "conv3d_bwd_data", Op("dy", g.out_shape, BF16), Packed("wb", g, BF16), g, o["add"])
    add("refuse/dgrad/gate_dtype", "conv3d_bwd_data", Op("dy", g.out_shape, BF16), Packed("wb", g, BF16), g, None, o["gate"])
    add("refuse/dgrad/add_bf16_of_fp32", "conv3d_bwd_data", o["dy"], o["wb"], g, Op("add", g.in_shape, BF16))
    add("refuse/dgrad/dy_dtype", "conv3d_bwd_data", Op("dy", g.out_shape, torch.float16), o["wb"], g)
    add("refuse/dgrad_bnstats/direct", "conv3d_bwd_data_bnstats", od["dy"], od["wb"], gd, Op("bn_y", gd.in_shape), od["mean"],
        od["invstd"], od["scale"], od["shift"])
    add("refuse/dgrad_bnstats/bf16", "conv3d_bwd_data_bnstats", Op("dy", g.out_shape, BF16), o["wb"], g, Op("bn_y", g.in_shape),
        o["mean"], o["invstd"], o["scale"], o["shift"])
    add("refuse/dgrad_bnstats/mean_shape", "conv3d_bwd_data_bnstats", o["dy"], o["wb"], g, Op("bn_y", g.in_shape),
        Op("mean", (g.Cin + 1,)), o["invstd"], o["scale"], o["shift"])
    add("refuse/wgrad/x_missing", "conv3d_bwd_weight", None, o["dy"], g)
    add("refuse/wgrad/x_missing_direct_with_cache", "conv3d_bwd_weight", None, od["dy"], gd, v_cache=od["v"])
    add("refuse/wgrad/x_missing_ahead_of_dy", "conv3d_bwd_weight", None, Op("dy", (1,)), g)
    add("refuse/wgrad/out_shape_ahead_of_x", "conv3d_bwd_weight", Op("x", (1,)), o["dy"], g, out=Op("out", (g.Cout, g.Cin, 27)))
    add("refuse/wgrad/v_cache_shape", "conv3d_bwd_weight", o["x"], o["dy"], g, v_cache=Op("v_cache", (7,)))
    add("refuse/wgrad/dy_dtype", "conv3d_bwd_weight", Op("x", g.in_shape, BF16), o["dy"], g)
    add("refuse/wgrad/x_dtype", "conv3d_bwd_weight", o["x"], Op("dy", g.out_shape, BF16), g)
    for tag, gn in (("cout_48", geom(1, 4, 4, 4, 64, 48)), ("cin_48_k1", geom(1, 4, 4, 4, 48, 64, k=1))):
        on = operands(gn, F32)                                            # the direct weight gradient has no plan for these
        add(f"refuse/wgrad/no_workspace/{tag}", "conv3d_bwd_weight", on["x"], on["dy"], gn)
    gn = geom(1, 4, 4, 4, 64, 48)
    add("refuse/fwd/stats_without_rows", "conv3d_fwd_keep", Op("x", gn.in_shape), Packed("wf", gn), None, gn, True, False)
    add("refuse/wgrad/x_missing_no_tn_plan", "conv3d_bwd_weight", None, Op("dy", g_tn.out_shape), g_tn,
        v_cache=Op("v_cache", lambda o: (o.conv_plan(g_tn).v_elems,)), env=no_tn)
    add("refuse/pack/w_dtype", "pack_conv_weight", Op("w", (64, 64, 3, 3, 3), BF16), True, True, g)
    return cases


def record() -> dict:
    with recording() as rec:
        return {name: outcome(rec, entry) for name, entry in _table()}


def test_every_call_launches_what_was_recorded():
    with open(LEDGER) as fh:
        ledger = json.load(fh)["calls"]
    got = record()
    assert list(got) == list(ledger), "the table and the ledger list other calls"
    wrong = {name: (got[name], ledger[name]) for name in got if got[name] != ledger[name]}
    assert not wrong, (len(wrong), dict(list(wrong.items())[:5]))


def test_the_ledger_reaches_every_algorithm_and_every_refusal():
    """what the recorded table must hold for the comparison above to mean something"""
    with open(LEDGER) as fh:
        doc = json.load(fh)
    assert len(doc["parent"]) == 40 and set(doc["parent"]) <= set("0123456789abcdef")
    calls = doc["calls"]
    launched = lambda lines, entry: any(line.split("] ")[-1].startswith(entry) for line in lines)
    every = [line for lines in calls.values() for line in lines]
    for entry in ("dram_conv3d_fwd(", "dram_wino_conv3d_fwd(", "dram_wino2d_conv3d_fwd(", "dram_conv1x1_fwd(", "dram_conv3d_fwd_bf16(",
                  "dram_wino_conv3d_fwd_bn(", "dram_wino_conv3d_fwd_cat(", "dram_conv3d_bwd_data(", "dram_wino_conv3d_bwd_data(",
                  "dram_wino2d_conv3d_bwd_data(", "dram_conv1x1_bwd_data(", "dram_conv3d_bwd_data_bf16(", "dram_wino_conv3d_bwd_data_bn(",
                  "dram_conv3d_bwd_weight(", "dram_wino_conv3d_bwd_weight(", "dram_wgrad_w2d(", "dram_conv1x1_bwd_weight(",
                  "dram_conv3d_bwd_weight_bf16(", "dram_pack_conv_weight(", "dram_wino_pack_weight(", "dram_wino2d_pack_weight(",
                  "dram_pack_conv_weight_bf16(", "dram_s2d_bf16(", "dram_d2s_bf16(", "dram_s2_embed_weight(", "dram_s2_extract_wgrad(",
                  "dram_cast_f32_to_bf16(", "dram_cast_bf16_to_f32(", "dram_wino_conv3d_bwd_weight(null, v_cache,"):
        assert launched(every, entry), entry
    # the pipeline geometry whose weight gradient reports no workspace runs the direct kernel, and needs x for it
    assert launched(calls["no_tn_plan/wgrad"], "dram_conv3d_bwd_weight(")
    assert launched(calls["no_tn_plan/wgrad/x_and_cache"], "dram_conv3d_bwd_weight(")
    assert launched(calls["no_tn_plan/fwd/---"], "dram_wino_conv3d_fwd(")
    assert calls["no_tn_plan/wgrad/cache"][-1].startswith("!! RuntimeError: conv3d_bwd_weight: x missing")
    for name, start in (("refuse/fwd/wf_shape", "!! ValueError: wf: expected shape"),
                        ("refuse/fwd/prologue_direct", "!! RuntimeError: conv3d_fwd_keep: no BatchNorm prologue"),
                        ("refuse/fwd_cat/blocks_32", "!! RuntimeError: conv3d_fwd_cat: not available"),
                        ("refuse/wgrad/x_missing", "!! RuntimeError: conv3d_bwd_weight: x missing"),
                        ("refuse/wgrad/no_workspace/cout_48", "!! RuntimeError: dram_conv3d_bwd_weight: unsupported geometry"),
                        ("refuse/fwd/stats_without_rows", "!! RuntimeError: dram_conv_num_mtiles rejected"),
                        ("refuse/dgrad/add_dtype", "!! TypeError: add: torch.float32 but the call's other activations are"),
                        ("refuse/wgrad/dy_dtype", "!! TypeError: dy: torch.float32 but the call's other activations are")):
        assert calls[name] == [calls[name][-1]] and calls[name][-1].startswith(start), (name, calls[name])
    assert all(lines[-1].startswith("!! ") for name, lines in calls.items() if name.startswith("refuse/")), "a refusal returned"


def test_a_warm_plan_cache_answers_every_call_without_asking_the_library():
    with recording() as rec:
        asked = {}
        for name, entry in _table():
            first = outcome(rec, entry)
            before = rec.queries
            assert outcome(rec, entry) == first, name
            if rec.queries != before:
                asked[name] = rec.queries - before
    assert not asked, asked


if __name__ == "__main__":                                              # record the ledger: --write FILE
    os.environ["DRAM_TUNING"] = "1"                                     # as tests/conftest.py: the switches count
    sys.path.insert(0, ROOT)
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    recorded = record()
    with open(sys.argv[sys.argv.index("--write") + 1], "w") as fh:              # one line per launch
        entries = ",\n".join(f"{json.dumps(name)}: [" + ",\n ".join(map(json.dumps, lines)) + "]" for name, lines in recorded.items())
        fh.write(f'{{"parent": "{head}", "calls": {{\n{entries}}}}}\n')
    print(len(recorded), "calls,", sum(len(v) - 1 for v in recorded.values()), "launches, recorded at", head)
