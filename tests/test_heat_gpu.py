"""GPU: the activation-map volumes of csrc/heat.hip (dram_heat_peak / dram_heat_volume) element by element against the
fp64 yardstick of tests/heat_ref.py, slice mode and determinism bit for bit, the reference's recorded panels
(tests/golden/heat.npz), the wrappers' rejections, and the validation step of both modules with the flag on and off.

Every case runs with torch.empty / torch.empty_like poisoned (floats NaN, uint8 0xFF): an unwritten voxel fails.
Every test prints its figures before it asserts (pytest -s).
"""
import os

import numpy as np
import pytest
import torch

import data_path_ref as R
import heat_ref as HR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heat.npz")


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    e0, el0 = torch.empty, torch.empty_like

    def fill(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(255)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(e0(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(el0(*a, **k)))
    yield
    torch.cuda.synchronize()


def lung_of(dense, seed=3, keep=0.7):
    B, _, d, h, w = dense.shape
    return torch.rand((B, 2 * d, 2 * h, 2 * w), generator=R.gen(seed)) < keep


def run(ops, dense, lung, mode, zsel=None):
    peak = ops.heat_peak(dense) if mode == "classsum" else None
    return ops.heat_volume(dense, lung, mode, peak, zsel, want_f32=True, want_u8=True) + (peak,)


def held(ops, dense, lung, mode, what, cap=0.005):
    """dense, lung: device tensors -> (f32, u8, peak) after the element-wise checks against fp64"""
    f32, u8, peak = run(ops, dense, lung, mode)
    ref = HR.heat64(dense.cpu(), lung.cpu(), mode)
    assert f32.dtype == torch.float32 and u8.dtype == torch.uint8 and f32.shape == u8.shape == ref.val.shape, what
    r = R.ratio(f32.cpu(), ref)
    outside, share, ok = HR.check_u8(u8.cpu(), ref, cap)
    print(f"[kernel/bound] {what}: {r:.3f}; u8 outside {outside}, open {100 * share:.3f} %")
    assert r <= 1.0, f"{what}: {r:.3f} of the element-wise bound"
    assert ok, f"{what}: {outside} bytes outside the range, {share:.4f} of the voxels open"
    return f32, u8, peak


# ------------------------------------------------------------------------------------------------ kernel vs fp64
def test_one_sample_six_channels(ops):
    dense = torch.randn(1, 6, 4, 4, 4, generator=R.gen(1)).to(DEV)
    held(ops, dense, lung_of(dense).to(DEV), "classsum", "classsum (1,6,(4,4,4))")


def test_both_heads_as_views_of_one_tensor(ops):
    base = torch.randn(2, 9, 4, 6, 8, generator=R.gen(2)).to(DEV)
    lung = lung_of(base).to(DEV)
    for name, view in (("cle", base[:, :6]), ("pse", base[:, 6:])):
        assert not view.is_contiguous() and view.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
        held(ops, view, lung, "classsum", f"classsum view {name} of [2,9,4,6,8]")


def test_plain_on_channel_views(ops):
    base = (3.0 * torch.rand(2, 2, 4, 4, 4, generator=R.gen(3)) - 1.0).to(DEV)
    lung = lung_of(base).to(DEV)
    for c in (0, 1):
        f32, u8, _ = held(ops, base[:, c:c + 1], lung, "plain", f"plain view {c} of [2,2,4,4,4]")
        # values below 0 and above 1: the bytes clamp, the floats do not
        assert float(f32.min()) < 0.0 and float(f32.max()) > 1.0
        assert int(u8.min()) == 0 and int(u8.max()) == 255
        assert bool((u8[f32 < 0] == 0).all()) and bool((u8[f32 >= 1] == 255).all())


def test_more_than_one_block(ops):
    dense = torch.randn(3, 6, 16, 32, 32, generator=R.gen(4)).to(DEV)
    assert ops._L().dram_heat_nblk(32 * 64 * 64) > 1
    held(ops, dense, lung_of(dense).to(DEV), "classsum", "classsum (3,6,(16,32,32))")


@pytest.mark.parametrize("where", ["first", "last", "outside"])
def test_planted_peak(ops, where):
    """the peak at output voxel (0,0,0) (weights {1, 0}: the planted value itself), at the last voxel (both taps
    clamped to n - 1), and at a voxel outside the lung (the peak is taken before the mask)"""
    dense = 0.1 * torch.randn(2, 3, 4, 4, 8, generator=R.gen(5))
    lung = lung_of(dense)
    src = {"first": (0, 0, 0), "last": (3, 3, 7), "outside": (2, 1, 5)}[where]
    dense[:, 1][(slice(None),) + src] = 7.0
    dp = HR.up2(dense.double()[:, 1:]).clamp(min=0).sum(1)
    at = [tuple(int(i) for i in np.unravel_index(int(v.argmax()), v.shape)) for v in dp]
    if where != "outside":
        assert at == [{"first": (0, 0, 0), "last": (7, 7, 15)}[where]] * 2
    for b, pos in enumerate(at):
        lung[(b,) + pos] = where != "outside"
    f32, u8, peak = held(ops, dense.to(DEV), lung.to(DEV), "classsum", f"peak planted {where}")
    assert torch.allclose(peak.cpu().double(), dp.amax(dim=(1, 2, 3)), rtol=1e-5, atol=0)
    got = [int(u8[(b,) + pos]) for b, pos in enumerate(at)]
    print(f"[peak {where}] at {at}: peak {peak.tolist()}, bytes there {got}, largest v {float(f32.max()):.7f}")
    if where == "outside":
        assert got == [0, 0] and float(f32.max()) < 1.0
    else:
        assert min(got) >= 254


def test_no_positive_class_channel(ops):
    """peak 0, every output exactly 0, no NaN.  With m = 0 + 1e-7 the general bound b_dp / m is of order 1 and says
    nothing here (it leaves most bytes open, so the 0.5 % cap on open voxels does not apply to this case); a weighted
    mean of non-positive values is non-positive in any arithmetic, so the statement held instead is exact equality."""
    dense = -torch.rand(2, 4, 4, 4, 8, generator=R.gen(6))
    dense[:, 0] = 5.0                                   # the background channel does not count
    f32, u8, peak = held(ops, dense.to(DEV), lung_of(dense).to(DEV), "classsum", "all class channels <= 0", cap=1.0)
    assert peak.tolist() == [0.0, 0.0]
    assert bool((f32 == 0).all()) and bool((u8 == 0).all())         # (NaN == 0 is False: no NaN either)


def test_channel_zero_is_ignored(ops):
    dense = torch.randn(2, 6, 4, 4, 8, generator=R.gen(7))
    lung = lung_of(dense).to(DEV)
    a = held(ops, dense.to(DEV), lung, "classsum", "channel 0 random")
    dense[:, 0] = 1e6
    b = held(ops, dense.to(DEV), lung, "classsum", "channel 0 = 1e6")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ slices, determinism
@pytest.mark.parametrize("mode", HR.MODES)
def test_slice_mode_is_the_full_volume_bit_for_bit(ops, mode):
    base = torch.randn(2, 7, 4, 6, 8, generator=R.gen(8)).to(DEV)
    dense = base[:, 1:] if mode == "classsum" else base[:, 3:4]
    lung = lung_of(dense).to(DEV)
    D = 8
    zsel = [[0, D - 1, 3, 3], [5, 0, D - 1, 1]]          # both ends, a repeat, per-sample different rows
    full_f, full_u, _ = run(ops, dense, lung, mode)
    for z in (zsel, torch.tensor(zsel), torch.tensor(zsel, dtype=torch.int32).to(DEV)):
        sl_f, sl_u, _ = run(ops, dense, lung, mode, zsel=z)
        assert tuple(sl_f.shape) == tuple(sl_u.shape) == (2, 4, 12, 16)
        for b in range(2):
            assert torch.equal(sl_f[b], full_f[b, zsel[b]]) and torch.equal(sl_u[b], full_u[b, zsel[b]])
    only_u8 = ops.heat_volume(dense, lung, mode, ops.heat_peak(dense) if mode == "classsum" else None, zsel)
    assert only_u8[0] is None and torch.equal(only_u8[1], sl_u)


def test_two_calls_are_bit_identical(ops):
    dense = torch.randn(3, 6, 16, 32, 32, generator=R.gen(9)).to(DEV)
    lung = lung_of(dense).to(DEV)
    a, b = run(ops, dense, lung, "classsum"), run(ops, dense, lung, "classsum")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not bool(torch.isnan(a[0]).any())


# ------------------------------------------------------------------------------------------------ wrappers
def test_wrappers_reject_bad_operands_before_any_launch(ops):
    dense = torch.randn(2, 6, 4, 4, 8, generator=R.gen(10)).to(DEV)
    lung = lung_of(dense).to(DEV)
    peak = ops.heat_peak(dense)
    with pytest.raises(RuntimeError):
        ops.heat_peak(dense.cpu())
    with pytest.raises(RuntimeError):
        ops.heat_volume(dense, lung.cpu(), "classsum", peak)
    with pytest.raises(RuntimeError):
        ops.heat_volume(dense, lung, "classsum", peak.cpu())
    with pytest.raises(ValueError, match="twice the dense grid"):
        ops.heat_volume(dense, lung[:, :, :, :8], "classsum", peak)
    with pytest.raises(ValueError, match="twice the dense grid"):
        ops.heat_volume(dense, lung[:1], "classsum", peak)
    with pytest.raises(ValueError, match="bool or uint8"):
        ops.heat_volume(dense, lung.float(), "classsum", peak)
    for bad in ([[0, 8], [0, 1]], [[0, 1], [-1, 1]]):
        with pytest.raises(ValueError, match=r"\[0, 8\)"):
            ops.heat_volume(dense, lung, "classsum", peak, zsel=bad)
    with pytest.raises(ValueError, match="zsel must be"):
        ops.heat_volume(dense, lung, "classsum", peak, zsel=[[0, 1]])
    with pytest.raises(ValueError, match="needs the peak"):
        ops.heat_volume(dense, lung, "classsum")
    with pytest.raises(ValueError, match="one channel"):
        ops.heat_volume(dense, lung, "plain")
    with pytest.raises(ValueError):
        ops.heat_peak(dense[:, :1])
    with pytest.raises(ValueError, match="contiguous"):
        ops.heat_peak(dense.permute(0, 1, 2, 4, 3))
    assert ops.heat_volume(dense, lung.view(torch.uint8), "classsum", peak)[1].dtype == torch.uint8


# ------------------------------------------------------------------------------------------------ modules, golden
@pytest.fixture(scope="module")
def modules():
    from bodyct_dram_emph_subtype_amd import models
    torch.manual_seed(21)
    return {"cls": models.ScanCLSLightningModule(models.make_args("med3d18")).to(DEV).eval(),
            "reg": models.ScanRegLightningModule(models.make_args("med3ddram18")).to(DEV).eval()}


@pytest.mark.parametrize("kind,mode", [("cls", "classsum"), ("reg", "plain")])
def test_golden_panels(modules, kind, mode):
    """the five uint8 volumes the reference fed its drawing function: heat bytes within the fp64 range, scan / lung /
    LAA-950 bytes exact, at the slices its slice rule shows"""
    from bodyct_dram_emph_subtype_amd import models
    g = np.load(GOLDEN)
    vol = torch.from_numpy(g[f"{kind}:volumes"])
    dense = [torch.from_numpy(g[f"{kind}:dense{i}"]).to(DEV) for i in (0, 1)]
    lung = torch.from_numpy(g[f"{kind}:lungs"]).bool()
    B, D = lung.shape[:2]
    full = models.heat_volumes(dense, lung.to(DEV), kind)
    for name, row, d in (("cle", 2, dense[0]), ("pse", 3, dense[1])):
        ref = HR.heat64(d.cpu(), lung, mode)
        outside, share, ok = HR.check_u8(full[name].cpu(), ref)
        differ = int((full[name].cpu() != vol[:, row]).sum())
        print(f"[golden {kind} {name}] outside {outside}, open {100 * share:.3f} %, bytes differing from the recording {differ}")
        assert ok
    batch = {"image": torch.from_numpy(g[f"{kind}:scans"]).to(DEV), "lung_mask": lung.to(DEV),
             "em_mask": torch.from_numpy(g[f"{kind}:ems"]).bool().to(DEV), "cls_label": torch.tensor([1, 4]).to(DEV),
             "pse_label": torch.tensor([0, 2]).to(DEV), "index": torch.arange(B).unsqueeze(-1).to(DEV)}
    res = modules[kind].draw_predictions(batch, dense, torch.tensor([1, 5]).to(DEV), torch.tensor([2, 2]).to(DEV), "validate")
    assert [r["uid"] for r in res] == [0, 1] and all(r["path"] is None for r in res)
    for b, r in enumerate(res):
        zs = torch.nonzero(lung[b].flatten(1).any(1)).flatten()
        assert r["z"] == models.panel_slices(int(zs[0]), int(zs[-1]) + 1, D) and len(r["z"]) == 5
        assert r["panels"].shape == (5, 5, 12, 16) and r["panels"].dtype == np.uint8
        for row in (0, 1, 4):
            assert (r["panels"][row] == vol[b, row][r["z"]].numpy()).all(), (b, row)
        for row, name in ((2, "cle"), (3, "pse")):
            assert (r["panels"][row] == full[name][b, r["z"]].cpu().numpy()).all(), (b, row)
        assert (r["sheet"] == models.sheet_from_panels(r["panels"])).all() and r["sheet"].shape == (60, 80, 3)


def _batch(B, dims, seed):
    g = torch.Generator().manual_seed(seed)
    image = torch.randn(B, *dims, generator=g)
    lung = torch.rand(B, *dims, generator=g) > 0.35
    lung[:, :3] = False                                  # the lung does not start at slice 0
    return {"image": image.to(DEV), "lung_mask": lung.to(DEV), "em_mask": ((image < -0.5) & lung).to(DEV),
            "cls_label": torch.randint(0, 6, (B,), generator=g).to(DEV), "pse_label": torch.randint(0, 3, (B,), generator=g).to(DEV),
            "index": torch.arange(B).unsqueeze(-1).to(DEV), "uid": [f"case{i}" for i in range(B)]}


@pytest.mark.parametrize("kind", ["cls", "reg"])
def test_validation_step_draws_only_when_asked(modules, kind, tmp_path, monkeypatch):
    from bodyct_dram_emph_subtype_amd import models
    mod = modules[kind]
    batch = _batch(2, (16, 32, 32), 5)
    calls = []
    real = mod.draw_predictions

    def spy(batch_, dense_outs, *a, **k):
        calls.append((dense_outs, real(batch_, dense_outs, *a, **k)))
        return calls[-1][1]

    monkeypatch.setattr(mod, "draw_predictions", spy)
    monkeypatch.setattr(mod.args, "model_path", str(tmp_path), raising=False)
    off = mod.validation_step(batch, 0)                  # no flag at all: today's behaviour
    monkeypatch.setattr(mod.args, "draw_predictions", 1, raising=False)
    late = mod.validation_step(batch, 1)                 # batch_idx >= N
    assert not calls and not list(tmp_path.rglob("*"))
    on = mod.validation_step(batch, 0)
    assert len(calls) == 1
    for other in (late, on):
        assert off.keys() == other.keys()
        assert all(torch.equal(off[k], other[k]) for k in off)
    dense_outs, res = calls[0]
    files = sorted(p.name for p in (tmp_path / "debug_input_data" / "0" / "validate").iterdir())
    assert len(files) == 2 and len(res) == 2
    dense_again, _ = mod.forward(batch["image"].unsqueeze(1), batch["lung_mask"].unsqueeze(1).float())
    print(f"[{kind}] files {files}; forward repeats bit for bit: "
          f"{[torch.equal(a, b) for a, b in zip(dense_outs, dense_again)]}")
    want = models.heat_volumes(dense_outs, batch["lung_mask"], kind, zsel=[r["z"] for r in res])
    labels = [batch["cls_label"].tolist(), on["pred_cle_labels"].tolist(), batch["pse_label"].tolist(),
              on["pred_pse_labels"].tolist()]
    for b, r in enumerate(res):
        assert r["z"] == models.panel_slices(3, 16, 16) == [15, 13, 11, 9, 7]
        assert os.path.basename(r["path"]) == files[b]
        assert files[b].rsplit(".", 1)[0] == f"case{b}_label_" + "_".join(str(col[b]) for col in labels)
        assert (r["panels"][2] == want["cle"][b].cpu().numpy()).all() and (r["panels"][3] == want["pse"][b].cpu().numpy()).all()
        assert (r["panels"][1] == (batch["lung_mask"][b, r["z"]].cpu().numpy() * 255)).all()
        assert (r["panels"][4] == (batch["em_mask"][b, r["z"]].cpu().numpy() * 255)).all()
        assert r["sheet"].shape == (5 * 32, 5 * 32, 3)
