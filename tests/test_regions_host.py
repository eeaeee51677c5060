"""Host side of the regional predict tail (no GPU): the header declares dram_region_nblk / dram_upproject_regions /
dram_prep_labels and the built library exports them, every argument check of the two launchers is reached through
ctypes with dummy pointers (no launch is reached), the report code of processor (region_metrics, build_outputs'
merge, write_reports) on hand-made tables, the label resize of tests/regions_ref.py against the oracle's mask resize,
and the register / LDS / spill audit of csrc/regions.hip."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch

import regions_ref as RR
from conftest import ROOT

ENTRY_POINTS = ("dram_region_nblk", "dram_upproject_regions", "dram_prep_labels")


def test_entry_points_are_declared_and_exported():
    from ctypes import c_int as I, c_longlong as LL, c_void_p as P
    from bodyct_dram_emph_subtype_amd import _build, _lib
    expect = {"dram_region_nblk": [LL],
              "dram_upproject_regions": [P, P, LL, P, P, P, P, P, P] + [I] * 8 + [P],
              "dram_prep_labels": [P, I, LL, LL, P, P] + [I] * 6 + [P]}
    for name in ENTRY_POINTS:
        res, args = _lib.SIGNATURES[name]
        assert res is I and list(args) == expect[name], name
    path = _build.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRY_POINTS) <= exported, set(ENTRY_POINTS) - exported


def test_region_nblk_rule():
    """ceil(v / 1024) clamped to 1..1024, the shape of dram_upproject_nblk's rule"""
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    sizes = (1, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1, 151 * 512 * 512, (1 << 31) - 1)
    assert [lib.dram_region_nblk(v) for v in sizes] == [1, 1, 2, 1024, 1024, 1024, 1024]
    assert [lib.dram_region_nblk(v) for v in sizes] == [lib.dram_upproject_nblk(v) for v in sizes]
    assert lib.dram_region_nblk(0) == 1


def test_upproject_regions_refuses_bad_arguments_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DRAM_ERR_BAD_ARG, _lib.DRAM_ERR_UNSUPPORTED
    one = ctypes.c_void_p(16)                   # never dereferenced: the argument checks come first

    def call(cle=one, pse=one, stride=24, ess=one, labels=one, oc=one, op=one, partial=one, table=one, B=1,
             dense=(2, 3, 4), size=(5, 7, 11), n=5):
        return lib.dram_upproject_regions(cle, pse, stride, ess, labels, oc, op, partial, table, B, *dense, *size, n, None)

    for k in ("cle", "pse", "ess", "labels", "partial", "table"):       # null operands
        assert call(**{k: None}) == BAD, k
    assert call(oc=None) == BAD and call(op=None) == BAD                 # exactly one of the volumes
    assert call(B=0) == BAD
    for axis in range(3):                                                # sizes < 1
        for key, base in (("dense", (2, 3, 4)), ("size", (5, 7, 11))):
            for v in (0, -1):
                assert call(**{key: tuple(v if a == axis else s for a, s in enumerate(base))}) == BAD, (key, axis, v)
    for n in (0, -1, 16, 255):                                           # n_regions outside 1..15
        assert call(n=n) == BAD, n
    assert call(stride=23) == BAD and call(stride=0) == BAD and call(stride=-24) == BAD   # batch stride < D*H*W
    # 2^31 output voxels or more: unsupported, with and without the volumes
    assert call(size=(2048, 1024, 1024)) == UNS
    assert call(size=(2048, 1024, 1024), oc=None, op=None) == UNS
    assert call(size=(1 << 30, 2, 1)) == UNS
    assert call(size=(2048, 1024, 1024), n=16) == BAD                    # a bad argument is named first


def test_prep_labels_refuses_bad_arguments_before_any_launch():
    from bodyct_dram_emph_subtype_amd import _lib
    lib = _lib.load()
    BAD = _lib.DRAM_ERR_BAD_ARG
    one = ctypes.c_void_p(16)

    def call(labels=one, code=1, sz=12, sy=4, zidx=one, out=one, src=(2, 3, 4), size=(5, 7, 11)):
        return lib.dram_prep_labels(labels, code, sz, sy, zidx, out, *src, *size, None)

    for k in ("labels", "zidx", "out"):
        assert call(**{k: None}) == BAD, k
    for code in (0, 3, -1):
        assert call(code=code) == BAD, code
    assert call(sz=-12) == BAD and call(sy=-4) == BAD
    for axis in range(3):
        for key, base in (("src", (2, 3, 4)), ("size", (5, 7, 11))):
            assert call(**{key: tuple(0 if a == axis else s for a, s in enumerate(base))}) == BAD, (key, axis)


def test_python_wrappers_refuse_before_any_launch():
    from bodyct_dram_emph_subtype_amd import ops, transforms
    d, e = torch.zeros(1, 2, 3, 4), torch.zeros(1, 5, 7, 11, dtype=torch.uint8)
    for n in (0, 16):
        with pytest.raises(ValueError, match="n_regions"):
            ops.upproject_regions(d, d, e, e, (5, 7, 11), n_regions=n)
    with pytest.raises(ValueError):
        ops.upproject_regions(d[0], d, e, e, (5, 7, 11))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.upproject_regions(d, d, e, e, (5, 7, 11))
    with pytest.raises(TypeError):
        transforms.prepare_labels(torch.zeros(2, 3, 4), (5, 7, 11))
    with pytest.raises(ValueError):
        transforms.prepare_labels(torch.zeros(3, 4, dtype=torch.uint8), (5, 7, 11))
    with pytest.raises(RuntimeError, match="no CPU path"):
        transforms.prepare_labels(torch.zeros(2, 3, 4, dtype=torch.int16), (5, 7, 11))


# ------------------------------------------------------------------------------------------------ the report
TABLE = [[0.0, 0.0, 0.0, 700.0],            # row 0: background, no ess voxel
         [9.999, 0.6, 250.0, 1000.0],       # cle 0.009999 -> band 0 ("0.010" rounds up in print only)
         [10.0, 50.0, 1000.0, 1000.0],      # cle exactly 0.01 -> band 1; pse exactly 0.05 -> band 2
         [0.0, 0.0, 0.0, 0.0],              # absent (a lobectomy)
         [200.0, 40.0, 1.0, 4000.0],        # cle exactly 0.05 -> band 2; pse exactly 0.01 -> band 1
         [350.0, 0.0, 333.0, 1000.0]]       # cle 0.35 -> band 5


def test_region_metrics_formats_bands_names_and_absent_regions():
    from bodyct_dram_emph_subtype_amd import processor
    m = processor.region_metrics(torch.tensor(TABLE, dtype=torch.float64))
    assert tuple(m) == processor.REGION_KEYS
    assert m["cle_lesion_percentage_per_region"] == {"1": "0.010", "2": "0.010", "3": None, "4": "0.050", "5": "0.350"}
    assert m["cle_severity_score_per_region"] == {"1": "0", "2": "1", "3": None, "4": "2", "5": "5"}
    assert m["pse_lesion_percentage_per_region"] == {"1": "0.001", "2": "0.050", "3": None, "4": "0.010", "5": "0.000"}
    assert m["pse_severity_score_per_region"] == {"1": "0", "2": "2", "3": None, "4": "1", "5": "0"}
    assert m["region_voxels"] == {"1": "1000", "2": "1000", "3": "0", "4": "4000", "5": "1000"}
    assert m["region_ess_fraction"] == {"1": "0.250", "2": "1.000", "3": None, "4": "0.000", "5": "0.333"}
    assert processor.region_metrics(TABLE) == m                         # nested lists as well
    names = {1: "RUL", 2: "RML", 3: "RLL", 4: "LUL", 5: "LLL"}
    named = processor.region_metrics(TABLE, names)
    assert named["cle_severity_score_per_region"] == {"RUL": "0", "RML": "1", "RLL": None, "LUL": "2", "LLL": "5"}
    assert processor.region_metrics(TABLE, ["-", "RUL", "RML", "RLL", "LUL", "LLL"]) == named
    assert list(processor.region_metrics(TABLE, {1: "RUL"})["region_voxels"]) == ["RUL", "2", "3", "4", "5"]
    assert json.loads(json.dumps(m))["cle_lesion_percentage_per_region"]["3"] is None      # null in json
    for bad in ([[0.0] * 4], [[0.0] * 3] * 3):
        with pytest.raises(ValueError):
            processor.region_metrics(bad)


def _prediction(table=None):
    out = {"cle_dense_outs": torch.zeros(1, 1, 2, 2, 2), "pse_dense_outs": torch.zeros(1, 1, 2, 2, 2),
           "cle_precentages": torch.tensor([0.02]), "pse_precentages": torch.tensor([0.3]),
           "crop_slices": torch.tensor([[[0, 2], [0, 2], [0, 2]]]), "original_size": torch.tensor([[2, 2, 2]]), "uids": ["u"]}
    if table is not None:
        out["region_table"] = torch.tensor([table], dtype=torch.float64)
    return out


def test_build_outputs_merges_the_table_only_when_there_is_one(monkeypatch, tmp_path):
    from bodyct_dram_emph_subtype_amd import processor
    monkeypatch.setattr(processor, "resample_paste", lambda d, *a, **k: (None, torch.zeros(2, 2, 2, dtype=torch.uint8)))
    plain = processor.build_outputs([_prediction()])[0]
    assert plain["metrics"] == {"cle_severity_score": "1", "cle_lesion_percentage_per_lung": "0.020",
                                "pse_severity_score": "2", "pse_lesion_percentage_per_lung": "0.300"}
    assert plain["error_messages"] == []
    reg = processor.build_outputs([_prediction(TABLE)])[0]
    assert {k: reg["metrics"][k] for k in plain["metrics"]} == plain["metrics"]
    assert set(reg["metrics"]) == set(plain["metrics"]) | set(processor.REGION_KEYS)
    assert {k: reg["metrics"][k] for k in processor.REGION_KEYS} == processor.region_metrics(TABLE)
    assert reg["error_messages"] == []
    foreign = [list(r) for r in TABLE]
    foreign[0][2] = 17.0                                                # ess voxels in row 0: lung outside 1..n
    msg = processor.build_outputs([_prediction(foreign)], region_names={1: "RUL"})[0]
    assert len(msg["error_messages"]) == 1 and "17" in msg["error_messages"][0] and "1..5" in msg["error_messages"][0]
    assert "RUL" in msg["metrics"]["region_voxels"]

    paths = {k: str(tmp_path / f"{k}.json") for k in ("centrilobular_json", "paraseptal_json", "output_json", "regions_json")}
    processor.write_reports([reg], **paths)
    assert json.load(open(paths["centrilobular_json"])) == {"score": 1, "percentage": 0.02}
    assert json.load(open(paths["regions_json"])) == processor.region_metrics(TABLE)
    assert json.load(open(paths["regions_json"]))["region_ess_fraction"]["3"] is None
    assert json.load(open(paths["output_json"]))[0]["metrics"] == reg["metrics"]
    with pytest.raises(ValueError, match="regions_json"):
        processor.write_reports([plain], regions_json=paths["regions_json"])
    processor.write_reports([plain], output_json=paths["output_json"])               # as before
    assert json.load(open(paths["output_json"]))[0]["metrics"] == plain["metrics"]


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("shape,target", [((6, 10, 12), (9, 7, 12)), ((5, 9, 7), (3, 20, 15)), ((1, 4, 4), (4, 4, 9))])
def test_label_resize_is_the_oracles_mask_resize(shape, target):
    from oracle import med3d_oracle as orc
    g = torch.Generator().manual_seed(sum(shape))
    labels = torch.randint(0, 7, shape, generator=g, dtype=torch.int16)
    labels[0, 0, :2] = torch.tensor([300, -3], dtype=torch.int16)
    got = RR.resize_labels(labels, target)
    want = orc.prepare_mask(labels.float(), target).clamp(0, 255).to(torch.uint8)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert torch.equal(got > 0, orc.prepare_mask(labels > 0, target))    # labels > 0 is the resized lung mask
    assert int(got.max()) == 255 and int(RR.resize_labels(labels.clamp(0, 255).to(torch.uint8), target).max()) == 255


def test_table_yardstick_on_a_hand_made_case():
    o = torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]]])
    ess = torch.tensor([[[[1, 0], [1, 1]]]], dtype=torch.uint8)
    labels = torch.tensor([[[[1, 1], [2, 9]]]], dtype=torch.uint8)
    t = RR.table64(o, -o, ess, labels, 2)
    assert t.tolist() == [[[4.0, -4.0, 1.0, 1.0], [3.0, -3.0, 1.0, 2.0], [3.0, -3.0, 1.0, 1.0]]]
    c, p = RR.percentages(t)
    assert c.tolist() == [[1.5, 3.0]] and p.tolist() == [[-1.5, -3.0]]
    assert torch.isnan(RR.percentages(RR.table64(o, o, ess, labels, 3))[0][0, 2])


# ------------------------------------------------------------------------------------------------ the kernels' resources
def test_region_kernels_carry_no_hidden_lds_or_spills():
    """tools/isa_waits.py --table on csrc/regions.hip, the audit pool_up.hip gets: no spills (the per-region accumulators
    stay in registers), LDS only in the two kernels that declare it and only what they declare, at most 128 VGPRs."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not present")
    src = os.path.join(ROOT, "bodyct-dram-emph-subtype_amd", "csrc", "regions.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_waits.py"), "--table", src],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    declared = {"upproject_regions_kernel<8>": 4 * 8 * 4 * 4, "upproject_regions_kernel<16>": 4 * 16 * 4 * 4,
                "region_fold_kernel": 16 * 64 * 8}
    seen = set()
    for l in r.stdout.splitlines():
        if " vgpr " not in l:
            continue
        name = l.split("vgpr")[0].split(None, 1)[1].strip()
        vgpr, lds, spills = (int(l.split(k)[1].split()[0]) for k in ("vgpr", "lds", "spills"))
        assert spills == 0, l
        assert lds == declared.get(name, 0), l
        assert vgpr <= 128, l
        seen.add(name)
    assert set(declared) <= seen and any(n.startswith("prep_labels_kernel") for n in seen), r.stdout
