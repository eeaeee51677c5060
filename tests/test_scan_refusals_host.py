"""The refusal ledger of the scan-side volume ops (no GPU): one fixed table of bad calls on CPU tensors -- every ``raise``
of the ops.py wrappers and the processor.py functions that share their argument checks (the image, ``out``, sigma, radius,
spacing and threshold rules; the scan filters of ``predict_case``), each reached at the smallest input that triggers it,
plus per wrapper the call that is all in order and ends at the missing device -- against tests/golden/scan_refusals.json:
the exception type and the message up to the first ``got `` (how the offending value is rendered behind it is free).

The json was recorded with this table at the commit BEFORE the checks were folded into shared helpers
(``python tests/test_scan_refusals_host.py --write FILE`` in a checkout of it).  An entry may carry a second outcome,
'parent': there the earlier code let an exception of Python's own escape (``float(v) for v in 5``) and the function now
raises the ValueError it documents.  Nothing else may differ, and at most 5 % of the entries may."""
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

from conftest import GOLDEN

LEDGER = os.path.join(GOLDEN, "scan_refusals.json")
NAN, INF = float("nan"), float("inf")
SHAPE = (2, 3, 4)


def _table():
    """[(id, thunk)]: the ids are the json's keys"""
    from bodyct_dram_emph_subtype_amd import ops, processor
    i16, u8, f32, i32 = torch.int16, torch.uint8, torch.float32, torch.int32
    img = torch.zeros(SHAPE, dtype=i16)
    lab = torch.ones(SHAPE, dtype=u8)
    comp = torch.zeros(SHAPE, dtype=i32)
    huge = lambda dtype: torch.zeros(1, dtype=dtype).expand(2048, 1024, 1024)          # 2^31 voxels in one element
    wide = lambda dtype: torch.zeros((2, 3, 8), dtype=dtype)[:, :, ::2]                # the shape, x stride 2
    flat = lambda dtype: torch.zeros(SHAPE, dtype=dtype)
    cases = []

    def add(name, f, *args, **kw):
        assert name not in dict(cases), name
        cases.append((name, lambda: f(*args, **kw)))

    def volume(fn, call, dtype, name="image", other=f32):
        """the three refusals of the [D,H,W] operand; ``call(t)`` passes it"""
        add(f"{fn}/{name}/numpy", call, np.zeros(SHAPE, dtype=np.int16))
        add(f"{fn}/{name}/2d", call, flat(dtype)[0])
        add(f"{fn}/{name}/4d", call, flat(dtype)[None])
        add(f"{fn}/{name}/empty", call, flat(dtype)[:, :, :0])
        add(f"{fn}/{name}/dtype", call, flat(other))

    def output(fn, call, dtype, shape=SHAPE, name="out"):
        """the refusals of a caller's output; ``call(t)`` passes it (a 'meta' tensor is the one on another device)"""
        add(f"{fn}/{name}/dtype", call, torch.zeros(shape, dtype=torch.float64))
        add(f"{fn}/{name}/numpy", call, np.zeros(shape, dtype=np.int16))
        add(f"{fn}/{name}/shape", call, torch.zeros(shape[:2] + (shape[2] + 1,), dtype=dtype))
        add(f"{fn}/{name}/device", call, torch.zeros(shape, dtype=dtype, device="meta"))

    # ---------------------------------------------------------------------------------------- ops.median_filter3d
    f = ops.median_filter3d
    for k, size in enumerate(((3, 3), (1, 1, 1), (5, 3, 3), 3, (True, 3, 3))):
        add(f"median_filter3d/size/{k}", f, img, size)
    volume("median_filter3d", f, i16)
    add("median_filter3d/image/2^31", f, huge(i16))
    output("median_filter3d", lambda t, f=f: f(img, out=t), i16)
    add("median_filter3d/out/strided", f, img, out=wide(i16))
    add("median_filter3d/out/shared", f, img, out=img)
    add("median_filter3d/device", f, img)
    add("median_filter3d/device/view_and_out", f, wide(i16), (1, 3, 3), out=flat(i16))

    # ---------------------------------------------------------------------------------------- ops.gaussian_filter3d
    f = ops.gaussian_filter3d
    add("gaussian_filter3d/mode", f, img, 1.0, mode="reflect")
    for k, sigma in enumerate(("x", (1.0, 2.0), None, (1.0, "x", 1.0))):
        add(f"gaussian_filter3d/sigma/{k}", f, img, sigma)
    for k, sigma in enumerate((-1.0, INF, NAN, (1.0, 1.0, -0.5))):
        add(f"gaussian_filter3d/sigma/value{k}", f, img, sigma)
    for k, truncate in enumerate((0.0, -1.0, INF, NAN)):
        add(f"gaussian_filter3d/truncate/{k}", f, img, 1.0, truncate)
    add("gaussian_filter3d/radius", f, img, (1.0, 4.2, 1.0))
    volume("gaussian_filter3d", lambda t, f=f: f(t, 1.0), i16, other=u8)
    add("gaussian_filter3d/image/2^31", f, huge(f32), 1.0)
    add("gaussian_filter3d/out_dtype/float64", f, img, 1.0, out_dtype=torch.float64)
    add("gaussian_filter3d/out_dtype/int16_of_float32", f, flat(f32), 1.0, out_dtype=i16)
    for k, box in enumerate(([[0, 2], [0, 3]], [[0, 2], [0, 3], [0, 5]], [[1, 1], [0, 3], [0, 4]], 7, [[0, 2], [0, 3], "ab"])):
        add(f"gaussian_filter3d/box/{k}", f, img, 1.0, box=box)
    output("gaussian_filter3d", lambda t, f=f: f(img, 1.0, out=t), i16)
    add("gaussian_filter3d/out/dtype_of_out_dtype", f, img, 1.0, out=flat(i16), out_dtype=f32)
    add("gaussian_filter3d/out/box_shape", f, img, 1.0, box=[[0, 1], [0, 3], [0, 4]], out=flat(i16))
    add("gaussian_filter3d/out/strided", f, img, 1.0, out=wide(i16))
    add("gaussian_filter3d/out/shared", f, img, 1.0, out=img)
    add("gaussian_filter3d/device/int16", f, img, 1.0)
    add("gaussian_filter3d/device/float32_box_out", f, flat(f32), (0.0, 1.0, 2.0), mode="zero", box=[[0, 1], [0, 3], [0, 4]],
        out=torch.zeros((1, 3, 4), dtype=f32))

    # ---------------------------------------------------------------------------------------- the two radii, the tables
    for name, radius, taps in (("gaussian", ops.gaussian_radius, ops.gaussian_taps),
                               ("bilateral", ops.bilateral_radius, lambda s, t=2.0: ops.bilateral_tables(s, 60.0, t))):
        for k, sigma in enumerate((-0.5, INF, NAN)):
            add(f"{name}_radius/sigma/{k}", radius, sigma)
            add(f"{name}_tables/sigma/{k}", taps, sigma)
        for k, truncate in enumerate((0.0, -2.0, INF, NAN)):
            add(f"{name}_radius/truncate/{k}", radius, 1.0, truncate)
            add(f"{name}_tables/truncate/{k}", taps, 1.0, truncate)
    add("gaussian_taps/radius", ops.gaussian_taps, 4.2)
    add("gaussian_taps/radius/truncate", ops.gaussian_taps, 1.0, 17.0)
    for k, sigma in enumerate(("x", (1.0, 2.0), None)):
        add(f"bilateral_tables/sigma3/{k}", ops.bilateral_tables, sigma, 60.0)
    for k, sigma in enumerate((2.8, (1.0, 1.0, 3.0), (2.75, 1.0, 1.0))):
        add(f"bilateral_tables/radius/{k}", ops.bilateral_tables, sigma, 60.0)
    for k, hu in enumerate((0.0, -1.0, INF, NAN)):
        add(f"bilateral_tables/sigma_hu/{k}", ops.bilateral_tables, 1.0, hu)
    add("bilateral_tables/range_table", ops.bilateral_tables, 1.0, 290.0)

    # ---------------------------------------------------------------------------------------- ops.bilateral_filter3d
    f = ops.bilateral_filter3d
    for k, sigma in enumerate(("x", (1.0, 2.0), None)):
        add(f"bilateral_filter3d/sigma/{k}", f, img, sigma, 60.0)
    add("bilateral_filter3d/sigma/value", f, img, -1.0, 60.0)
    add("bilateral_filter3d/truncate", f, img, 1.0, 60.0, 0.0)
    add("bilateral_filter3d/radius", f, img, (1.0, 1.0, 2.8), 60.0)
    add("bilateral_filter3d/sigma_hu", f, img, 1.0, 0.0)
    add("bilateral_filter3d/range_table", f, img, 1.0, 400.0)
    volume("bilateral_filter3d", lambda t, f=f: f(t, 1.0, 60.0), i16)
    add("bilateral_filter3d/image/2^31", f, huge(i16), 1.0, 60.0)
    output("bilateral_filter3d", lambda t, f=f: f(img, 1.0, 60.0, out=t), i16)
    add("bilateral_filter3d/out/strided", f, img, 1.0, 60.0, out=wide(i16))
    add("bilateral_filter3d/out/shared", f, img, 1.0, 60.0, out=img)
    for k, within in enumerate((np.ones(SHAPE, dtype=np.uint8), lab[0], lab[:, :, :0])):
        add(f"bilateral_filter3d/within/{k}", f, img, 1.0, 60.0, within=within)
    add("bilateral_filter3d/within/dtype", f, img, 1.0, 60.0, within=flat(f32))
    add("bilateral_filter3d/within/shape", f, img, 1.0, 60.0, within=torch.ones((2, 3, 5), dtype=u8))
    add("bilateral_filter3d/device", f, img, 1.0, 60.0)
    add("bilateral_filter3d/device/within", f, img, (0.0, 1.0, 2.0), 60.0, within=lab)
    add("bilateral_filter3d/device/within_int16_view_out", f, wide(i16), 1.0, 60.0, within=wide(i16), out=flat(i16))

    # ---------------------------------------------------------------------------------------- ops.local_window
    f = ops.local_window
    for k, spacing in enumerate((5, None, (1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, INF, 1.0),
                                 (NAN, 1.0, 1.0), ("a", 1.0, 1.0), "abc")):
        add(f"local_window/spacing/{k}", f, spacing, 10.0)
    for k, mm in enumerate((True, "3", None, NAN, INF, 0, -1.0)):
        add(f"local_window/local_mm/{k}", f, (1.0, 1.0, 1.0), mm)
    add("local_window/rounds_to_zero/spacing", f, (0.0004, 1.0, 1.0), 10.0)
    add("local_window/rounds_to_zero/local_mm", f, (1.0, 1.0, 1.0), 0.0004)
    add("local_window/radius", f, (1.0, 0.25, 1.0), 10.0)
    add("local_window/one_voxel", f, (1.0, 1.0, 1.0), 1.9)

    # ---------------------------------------------------------------------------------------- ops.local_fraction3d
    f = ops.local_fraction3d
    store = torch.ones(48, dtype=u8)                                    # labels in its first half
    for k, radius in enumerate(((1, 1), 1, (1.0, 1, 1), (-1, 0, 0), (True, 1, 1), None)):
        add(f"local_fraction3d/radius/{k}", f, img, lab, -950, radius)
    add("local_fraction3d/radius/cap", f, img, lab, -950, (0, 17, 0))
    for k, t in enumerate((True, -950.5, 32769, -32769, None, "x", NAN, INF)):
        add(f"local_fraction3d/threshold/{k}", f, img, lab, t)
    volume("local_fraction3d", lambda t, f=f: f(t, lab), i16)
    for name, dtype in (("out", i16), ("out_u8", u8)):
        output("local_fraction3d", lambda t, name=name, f=f: f(img, lab, **{name: t}), dtype, name=name)
        add(f"local_fraction3d/{name}/shared_image", f, img, lab, **{name: img.view(dtype).view(-1)[:24].view(SHAPE)})
        add(f"local_fraction3d/{name}/shared_labels", f, img, store[:24].view(SHAPE),
            **{name: store.view(i16).view(SHAPE) if dtype == i16 else store[24:].view(SHAPE)})
    both = torch.zeros((2,) + SHAPE, dtype=i16)
    add("local_fraction3d/out_u8/shared_out", f, img, lab, out=both[0], out_u8=both[1].view(u8).view(-1)[:24].view(SHAPE))
    add("local_fraction3d/out/strided", f, img, lab, out=wide(i16))
    for k, view in enumerate((wide(u8), torch.zeros((2, 4, 3), dtype=u8).transpose(1, 2), flat(u8).expand(2, 2, 3, 4)[:, 0],
                              torch.zeros((2, 3, 7), dtype=u8).as_strided(SHAPE, (12, 3, 1)))):
        add(f"local_fraction3d/out_u8/strides/{k}", f, img, lab, out_u8=view)
    add("local_fraction3d/image/strided", f, wide(i16), lab)
    for k, labels in enumerate((np.ones(SHAPE, dtype=np.uint8), lab[0], lab[:, :, :0])):
        add(f"local_fraction3d/labels/{k}", f, img, labels)
    add("local_fraction3d/labels/dtype", f, img, flat(f32))
    add("local_fraction3d/labels/shape", f, img, torch.ones((2, 3, 5), dtype=u8))
    add("local_fraction3d/device", f, img, lab)
    add("local_fraction3d/device/all_outputs", f, img, wide(i16), -32768, (0, 0, 16), out=flat(i16),
        out_u8=torch.zeros((4, 6, 8), dtype=u8)[1:3, 2:5, 3:7], want_counts=True)

    # ---------------------------------------------------------------------------------------- ops.lobe_histogram
    f = ops.lobe_histogram
    add("lobe_histogram/n_regions/0", f, img, lab, 0)
    add("lobe_histogram/n_regions/16", f, img, lab, 16)
    for k, image in enumerate((np.zeros(SHAPE, dtype=np.int16), img[0], img[None], img[:, :, :0])):
        add(f"lobe_histogram/image/{k}", f, image, lab)
    add("lobe_histogram/image/2^31", f, huge(i16), huge(u8))
    for k, labels in enumerate((np.ones(SHAPE, dtype=np.uint8), lab[0], lab[:, :, :0])):
        add(f"lobe_histogram/labels/{k}", f, img, labels)
    add("lobe_histogram/labels/dtype", f, img, flat(f32))
    add("lobe_histogram/labels/shape", f, img, torch.ones((2, 3, 5), dtype=u8))
    add("lobe_histogram/device", f, img, lab)
    add("lobe_histogram/device/float_image", f, flat(f32), lab)             # its type is the device side's to refuse
    add("lobe_histogram/device/int16_view", f, img, wide(i16), 15, 0, 64)

    # ---------------------------------------------------------------------------------------- ops.laa_components
    f = ops.laa_components
    for k, image in enumerate((np.zeros(SHAPE, dtype=np.int16), img[0], img[None])):
        add(f"laa_components/image/{k}", f, image, lab)
    add("laa_components/image/empty", f, img[:, :, :0], lab[:, :, :0])      # not the image's refusal: the labels'
    add("laa_components/image/empty_labels_not", f, img[:, :, :0], lab)
    add("laa_components/image/dtype", f, flat(f32), lab)
    add("laa_components/image/2^31", f, huge(i16), huge(u8))
    for k, t in enumerate((-950.5, 32769, -32769, None, "x", NAN, INF)):
        add(f"laa_components/threshold/{k}", f, img, lab, t)
    add("laa_components/threshold/bool", f, img, lab, True)                 # taken as 1: ends at the device
    add("laa_components/connectivity", f, img, lab, connectivity=18)
    add("laa_components/n_regions", f, img, lab, n_regions=16)
    for k, labels in enumerate((np.ones(SHAPE, dtype=np.uint8), lab[0])):
        add(f"laa_components/labels/{k}", f, img, labels)
    add("laa_components/labels/dtype", f, img, flat(f32))
    add("laa_components/labels/shape", f, img, torch.ones((2, 3, 5), dtype=u8))
    add("laa_components/device", f, img, lab)
    add("laa_components/device/whole_lung_int16", f, img, wide(i16), 32768, 16, 26, by_lobe=False, want_sizes=True)

    # ---------------------------------------------------------------------------------------- ops.component_shapes
    f = ops.component_shapes
    volume("component_shapes", f, i32, name="components")
    add("component_shapes/components/2^31", f, huge(i32))
    add("component_shapes/zones/dtype", f, comp, zones=flat(i16))
    add("component_shapes/zones/numpy", f, comp, zones=np.zeros(SHAPE, dtype=np.uint8))
    add("component_shapes/zones/shape", f, comp, zones=torch.zeros((2, 3, 5), dtype=u8))
    for k, cap in enumerate((-1, 1.5)):
        add(f"component_shapes/max_components/{k}", f, comp, max_components=cap)
    for k, labels in enumerate((np.ones(SHAPE, dtype=np.uint8), lab[0])):
        add(f"component_shapes/labels/{k}", f, comp, labels)
    add("component_shapes/labels/dtype", f, comp, flat(f32))
    add("component_shapes/labels/shape", f, comp, torch.ones((2, 3, 5), dtype=u8))
    add("component_shapes/device", f, comp)
    add("component_shapes/device/labels_zones_cap", f, comp, wide(i16), flat(u8), 0)

    # ---------------------------------------------------------------------------------------- processor: parameters
    f = processor.local_laa_params
    for k, t in enumerate((True, "x", None, -950.5, 32769, -32769, NAN, INF)):
        add(f"local_laa_params/threshold/{k}", f, "f", t)
    for k, c in enumerate((0.105, 0.0, 1.01, "a", True, NAN, None)):
        add(f"local_laa_params/cuts/{k}", f, "f", -950, (0.1, c))
    for k, p in enumerate((0, 100, 50.5, True, "a", None)):
        add(f"local_laa_params/percentiles/{k}", f, "f", -950, (0.1,), (50, p))
    for name, parse, tag, n in (("gaussian_sigma_mm", processor.gaussian_sigma_mm, "gaussian", 1),
                                ("bilateral_params", processor.bilateral_params, "bilateral", 2)):
        for tail in sorted({(), (1.0,) * (n - 1), (1.0,) * (n + 1)}):
            add(f"{name}/length/{len(tail)}", parse, "f", (tag,) + tail)
        for k, bad in enumerate((0.0, -1.0, True, "1", None, NAN, INF)):
            for at in range(n):
                add(f"{name}/value/{k}/{at}", parse, "f", [tag] + [bad if a == at else 1.0 for a in range(n)])
    for name, voxels, cap_mm in (("gaussian_sigma_voxels", processor.gaussian_sigma_voxels, 2.1),
                                 ("bilateral_sigma_voxels", processor.bilateral_sigma_voxels, 1.4)):
        for k, spacing in enumerate(((1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, INF, 1.0),
                                     (NAN, 1.0, 1.0))):
            add(f"{name}/spacing/{k}", voxels, "f", spacing, 1.0)
        add(f"{name}/spacing/not_iterable", voxels, "f", 5, 1.0)
        add(f"{name}/spacing/string_entry", voxels, "f", ("a", 1.0, 1.0), 1.0)
        for k, mm in enumerate((0.0, -1.0, NAN, INF)):
            add(f"{name}/sigma_mm/{k}", voxels, "f", (1.0, 1.0, 1.0), mm)
        add(f"{name}/radius", voxels, "f", (0.5, 0.7, 0.7), cap_mm)
    add("gaussian_image/spacing", processor.gaussian_image, img, None, (1.0, 1.0), 1.0)
    add("gaussian_image/radius", processor.gaussian_image, img, None, (1.0, 0.1, 1.0), 1.0)
    add("gaussian_image/device", processor.gaussian_image, flat(f32), [[0, 1], [0, 3], [0, 4]], (2.5, 0.7, 0.5), 1.0)
    add("bilateral_image/spacing", processor.bilateral_image, img, lab, (1.0, 0.0, 1.0), 1.0, 60.0)
    add("bilateral_image/radius", processor.bilateral_image, img, lab, (1.0, 0.1, 1.0), 1.0, 60.0)
    add("bilateral_image/range_table", processor.bilateral_image, img, lab, (1.0, 1.0, 1.0), 1.0, 400.0)
    add("bilateral_image/device", processor.bilateral_image, img, lab, (1.0, 1.0, 1.0), 1.0, 60.0)
    add("filtered_image/size", processor.filtered_image, img, (3, 3))
    add("filtered_image/device", processor.filtered_image, img, (1, 3, 3))
    for k, bad in enumerate((("gaussian", 0.0), ("gaussian",), ("bilateral", 1.0), ("bilateral", 1.0, -60.0), ("box", 1.0),
                             (1, 1, 1), (3, 3), 3, None, "median3x3x3", ("median", 3, 3, 3))):
        add(f"filter_name/{k}", processor.filter_name, bad)

    # ---------------------------------------------------------------------------------------- processor.predict_case
    module = SimpleNamespace(args=SimpleNamespace(n_regions=5))
    wide_module = SimpleNamespace(args=SimpleNamespace(n_regions=6))
    spacing = (2.5, 0.7, 0.7)

    def run(sp=spacing, module=module, **kw):
        return processor.predict_case(module, img, lab, sp, SHAPE, **kw)

    add("predict_case/local_mm/needs_densitometry", run, local_mm=10.0)
    add("predict_case/local_kw/needs_local_mm", run, densitometry=True, local_kw={"threshold": -910})
    add("predict_case/local_kw/unknown", run, densitometry=True, local_mm=10.0, local_kw={"radius": 1, "box": 2})
    for k, mm in enumerate((0.0, True, "3", NAN)):
        add(f"predict_case/local_mm/{k}", run, densitometry=True, local_mm=mm)
    add("predict_case/local_mm/spacing", run, (2.5, 0.7), densitometry=True, local_mm=10.0)
    add("predict_case/local_mm/spacing_not_iterable", run, 1.0, densitometry=True, local_mm=10.0)
    add("predict_case/local_mm/radius", run, (2.5, 0.2, 0.7), densitometry=True, local_mm=10.0)
    add("predict_case/local_mm/one_voxel", run, densitometry=True, local_mm=1.0)
    for k, kw in enumerate(({"threshold": -950.5}, {"threshold": True}, {"threshold": None}, {"cuts": (0.105,)},
                            {"percentiles": (0,)}, {"n_regions": 16}, {"n_regions": 0})):
        add(f"predict_case/local_kw/{k}", run, densitometry=True, local_mm=10.0, local_kw=kw)
    add("predict_case/local_kw/n_regions_of_densitometry_kw", run, densitometry=True, local_mm=10.0,
        densitometry_kw={"n_regions": 16})
    add("predict_case/local_mm/ahead_of_the_filter", run, local_mm=10.0, scan_filter=(1, 1, 1))
    add("predict_case/local_kw/ahead_of_the_sections", run, densitometry=True, local_kw={"cuts": (0.5,)},
        scan_filter_sections=("regions",))
    for k, names in enumerate((("regions",), ("densitometry", "cluster"), ("",))):
        add(f"predict_case/scan_filter_sections/{k}", run, scan_filter_sections=names)
        add(f"predict_case/scan_filter_sections/{k}/ahead_of_the_filter", run, scan_filter_sections=names,
            scan_filter=("gaussian", 0.0))
    for k, bad in enumerate((("gaussian", 0.0), ("gaussian",), ("gaussian", 1.0, 2.0), ("gaussian", True),
                             ("bilateral", 1.0), ("bilateral", 1.0, 0.0), ("bilateral", NAN, 60.0), ("box", 1.0), (1, 1, 1),
                             (3, 3), (5, 3, 3), 3, "median3x3x3")):
        add(f"predict_case/scan_filter/{k}", run, scan_filter=bad)
        add(f"predict_case/scan_filter/{k}/sections_on", run, scan_filter=bad, densitometry=True, clusters=True)
    for kind, flt in (("gaussian", ("gaussian", 1.0)), ("bilateral", ("bilateral", 1.0, 60.0))):
        add(f"predict_case/scan_filter/{kind}/spacing", run, (2.5, 0.7), scan_filter=flt)
        add(f"predict_case/scan_filter/{kind}/spacing_zero", run, (2.5, 0.0, 0.7), scan_filter=flt)
        add(f"predict_case/scan_filter/{kind}/spacing_not_iterable", run, 1.0, scan_filter=flt)
        add(f"predict_case/scan_filter/{kind}/radius", run, (2.5, 0.7, 0.05), scan_filter=flt)
    add("predict_case/scan_filter/bilateral/range_table", run, scan_filter=("bilateral", 1.0, 400.0))
    for k, kw in enumerate(({"dilate_iterations": 0}, {"crop_border": 0}, {"crop_border": -1.0},
                            {"dilate_iterations": 0, "crop_border": 5})):
        add(f"predict_case/scan_filter/median/needs/{k}", run, scan_filter=(1, 3, 3), densitometry=True, **kw)
        add(f"predict_case/scan_filter/gaussian/needs_nothing/{k}", run, scan_filter=("gaussian", 1.0), densitometry=True, **kw)
        add(f"predict_case/scan_filter/bilateral/needs_nothing/{k}", run, scan_filter=["bilateral", 1, 60], clusters=True, **kw)
    add("predict_case/fissure_mm/needs_core_peel", run, fissure_mm=2.0)
    add("predict_case/fissure_mm/n_regions", run, module=wide_module, core_peel=True, fissure_mm=2.0)
    add("predict_case/core_peel/n_regions", run, core_peel=True, densitometry_kw={"n_regions": 4})
    add("predict_case/filter_ahead_of_fissure_mm", run, fissure_mm=2.0, scan_filter=(3, 3))
    add("predict_case/device", run)
    for k, flt in enumerate(((3, 3, 3), [1, 3, 3], ("gaussian", 1.0), ["gaussian", 2], ("bilateral", 1.0, 60.0))):
        add(f"predict_case/device/scan_filter/{k}", run, scan_filter=flt, densitometry=True, core_peel=True, clusters=True,
            regions=True, local_mm=10.0, local_kw={"threshold": -910.0, "cuts": (0.1, 1), "percentiles": (1, 99.0)})
    return cases


def outcome(thunk) -> dict:
    """{'type': the exception's class name (None: the call returned), 'text': its message up to the first 'got '}"""
    try:
        thunk()
    except Exception as e:                                              # noqa: BLE001 -- whatever escapes IS the outcome
        text = str(e)
        cut = text.find("got ")
        return {"type": type(e).__name__, "text": text if cut < 0 else text[:cut]}
    return {"type": None, "text": ""}


def test_every_refusal_is_the_recorded_one():
    with open(LEDGER) as fh:
        ledger = json.load(fh)
    table = _table()
    assert [name for name, _ in table] == list(ledger), "the table and the ledger list other calls"
    deviating = [name for name, entry in ledger.items() if "parent" in entry]
    assert len(deviating) <= math.floor(0.05 * len(table)), (len(table), len(deviating))
    wrong = {}
    for name, thunk in table:
        got, want = outcome(thunk), {k: ledger[name][k] for k in ("type", "text")}
        if got != want:
            wrong[name] = (got, want)
    assert not wrong, wrong


def test_a_deviation_only_replaces_an_exception_of_pythons_own():
    """what an entry's 'parent' may hold: an exception the earlier code did not raise itself -- its text names no function
    of ours -- and the new outcome is the documented ValueError"""
    with open(LEDGER) as fh:
        ledger = json.load(fh)
    for name, entry in ledger.items():
        assert entry["type"] is not None, name                                  # every call of the table is refused
        if "parent" in entry:
            assert entry["parent"]["type"] in ("TypeError", "ValueError", "OverflowError") and entry["type"] == "ValueError", name
            assert not entry["parent"]["text"].split(" ")[0].endswith(":") and entry["text"].split(" ")[0].endswith(":"), name
    ends = [name for name, entry in ledger.items() if "no CPU path" in entry["text"]]
    for fn in ("median_filter3d", "gaussian_filter3d", "bilateral_filter3d", "local_fraction3d", "lobe_histogram",
               "laa_components", "component_shapes", "predict_case"):
        assert any(name.startswith(f"{fn}/device") for name in ends), fn


if __name__ == "__main__":                                             # record the ledger: --write FILE [--parent OLD_FILE]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    recorded = {name: outcome(thunk) for name, thunk in _table()}
    if "--parent" in sys.argv:                                          # keep the parent's outcome beside a new one
        with open(sys.argv[sys.argv.index("--parent") + 1]) as fh:
            old = json.load(fh)
        for name, entry in recorded.items():
            if {k: old[name][k] for k in ("type", "text")} != entry:
                entry["parent"] = {k: old[name][k] for k in ("type", "text")}
    with open(sys.argv[sys.argv.index("--write") + 1], "w") as fh:
        json.dump(recorded, fh, indent=0, sort_keys=False)
        fh.write("\n")
    print(len(recorded), "entries,", sum("parent" in e for e in recorded.values()), "deviating")
