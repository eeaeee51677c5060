"""GPU: the memory-bound kernels in every launch form their size selects, at the production sizes that select it,
element by element against an fp64 reference on the device.

The toy shapes of test_kernels_gpu.py reach only the smallest form of these kernels: the one-block statistic fold,
the cached (not non-temporal) BatchNorm pass, one head / loss / up-projection block.  Here every case

  * runs with every buffer an ops wrapper allocates POISONED (`poison`: floating tensors NaN, uint8 0xFF -- an invalid
    max-pool tap), so an element a kernel did not write cannot pass as a correct one left over by an earlier call;
  * asserts the form it claims, with the library's own sizing exports (dram_fold_partials_stages, dram_colsum_nparts,
    dram_bn_bwd_apply_nparts, dram_head_nblk, dram_segloss_nblk, dram_upproject_nblk, dram_window_stats_nblk) and a
    one-line mirror of the non-temporal rule (ew_stream: tensor bytes >= 256 MiB) and of the fixed-quad rule
    (256 % (C / 4) == 0), so a threshold that moves cannot silently move a case out of its form;
  * holds every element to a bound derived from the kernel's arithmetic (u = 2^-24 per fp32 rounding, 2^-8 relative
    for the one bf16 rounding of a store), never to a whole-tensor relative L2: a dropped block or a stale stage row
    touches a small fraction of a 10^8-element tensor and fails here all the same.

test_census_every_form_the_networks_reach_is_covered runs a full-size config-1 step and a config-2 bf16 step with the
ops wrappers of these families instrumented, and fails on any (function, dtype, form) no case table below covers.
"""
import inspect
import math
import struct

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
U = 2.0 ** -24              # fp32 unit roundoff
UB = 2.0 ** -8              # bf16 unit roundoff (8 significant bits): half an ulp, relative
NT_BYTES = 256 << 20        # csrc/common.h ew_stream: streaming cache policy for tensors of >= 256 MiB
CHUNK = 1 << 25             # elements per fp64 reference chunk (256 MB of doubles)


@pytest.fixture(scope="module")
def ops():
    from bodyct_dram_emph_subtype_amd import ops as o
    import bodyct_dram_emph_subtype_amd as pkg
    pkg.load_library()
    return o


class _Poison:
    keep = None             # predicate: allocations to hold on to (self.kept) for inspection


@pytest.fixture
def poison(monkeypatch):
    """torch.empty / torch.empty_like return poisoned memory for the duration of a test: floating tensors (outputs,
    partial-sum rows, float64 fold buffers) NaN, uint8 tensors 0xFF.  The fold kernels' own memset of their ticket
    words still zeroes those."""
    e0, el0 = torch.empty, torch.empty_like
    rec = _Poison()
    rec.kept = []

    def fill(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(255)
        if rec.keep is not None and rec.keep(t):
            rec.kept.append(t)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(e0(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(el0(*a, **k)))
    yield rec
    rec.kept.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class Excess:
    """max over elements of |got - ref| - bound, on the device (NaN counts as +inf: an unwritten element)."""

    def __init__(self, what):
        self.what, self.parts = what, []

    def add(self, got, ref, bound):
        d = (got.double() - ref).abs() - bound
        self.parts.append(torch.nan_to_num(d, nan=math.inf).amax())

    def check(self):
        v = float(torch.stack(self.parts).amax())
        assert v <= 0.0, f"{self.what}: exceeds its bound by {v:.3e}"


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(shape, seed, dtype=F32, scale=1.0, offset=0.0):
    return (torch.randn(shape, generator=gen(seed), device=DEV) * scale + offset).to(dtype)


def rand(shape, seed, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=gen(seed), device=DEV) * (hi - lo) + lo


def row_chunks(rows, C):
    step = max(1, CHUNK // C)
    for r0 in range(0, rows, step):
        yield slice(r0, min(rows, r0 + step))


def store_bound(ref, dtype, err32):
    """bound of a stored result whose fp32 arithmetic is within err32 of the fp64 value: fp32 storage err32; bf16
    storage one more rounding of the fp32 value to 8 significant bits (half an ulp <= 2^-8 |value|)."""
    return err32 if dtype == F32 else UB * ref.abs() + (1.0 + UB) * err32


# ------------------------------------------------------------------------------------------------ regime keys
# One function per instrumented ops wrapper, with the wrapper's own parameters: the form the call takes, from the
# library's sizing exports and the two mirrored rules.  The census binds each recorded call to these.
def _L(ops):
    return ops._L()


def nt(t):
    return t.numel() * t.element_size() >= NT_BYTES


def fixed_quad(C):
    return 256 % (C // 4) == 0


def fold_form(ops, Pn):
    return "S=1" if _L(ops).dram_fold_partials_stages(Pn) == 1 else "S>1"


def colreduce_form(ops, rows, C):
    nparts = _L(ops).dram_colsum_nparts(rows, C)
    assert 1 <= nparts <= 1024, nparts          # csrc/bn.hip rows_per_block: the one colreduce form
    return f"y{(C // 4 + 255) // 256}"


def _mask(relu, z):
    return "none" if not relu else ("z" if z is not None else "scale")


def k_reduce_partials(ops, partial, tail=None, want_f32=False):
    return (fold_form(ops, partial.shape[0]), "tail" if tail is not None else "", "f32" if want_f32 else "")


def k_bn_fold_finalize(ops, partial, count, gamma, beta, running_mean, running_var, momentum, eps):
    return (fold_form(ops, partial.shape[0]),)


def k_bn_apply(ops, y, scale, shift, residual, rs, relu):
    C = y.shape[-1]
    identity = residual is not None and rs == 1 and tuple(residual.shape) == tuple(y.shape)
    if residual is not None and not identity:
        return ("shortcut-a",)
    res = "identity" if identity else "none"
    if fixed_quad(C):
        return ("shot-nt" if nt(y) else "shot", res)
    return ("generic", res)


def k_bn_bwd_reduce(ops, dz, z, y, mean, invstd, relu, scale=None, shift=None):
    return (colreduce_form(ops, y.numel() // y.shape[-1], y.shape[-1]), _mask(relu, z))


def k_bn_bwd_apply(ops, dz, z, y, mean, invstd, gamma, sums, count, relu, scale=None, shift=None, want_colsum=False,
                   count_dev=None):
    C = y.shape[-1]
    rows = y.numel() // C
    if not fixed_quad(C):
        assert _L(ops).dram_bn_bwd_apply_nparts(rows, C) < 1           # no column sums: the caller takes colsum
        form = "generic"
    elif want_colsum:
        assert _L(ops).dram_bn_bwd_apply_nparts(rows, C) == -(-rows * (C // 4) // 4096)   # one row per 4 096 quads
        form = "shot1-colsum"
    else:
        form = "shot2-nt" if nt(y) else "shot1"
    return (form, _mask(relu, z), "colsum" if want_colsum else "")


def k_colsum(ops, a):
    return (colreduce_form(ops, a.numel() // a.shape[-1], a.shape[-1]),)


def _vw(t, *counts):
    return "vw8" if t.dtype == BF16 and all(c % 8 == 0 for c in counts) else "vw4"


def k_maxpool_fwd(ops, x):
    return (_vw(x, x.shape[-1]),)


def k_bn_maxpool_fwd(ops, y, scale, shift):
    return (_vw(y, y.shape[-1]),)


def k_maxpool_bwd(ops, dy, argmax, in_shape, add_=None):
    if add_ is None:
        return (_vw(dy, dy.shape[-1]), "none")
    st = add_.stride(3)
    aligned = add_.data_ptr() % 16 == 0
    return (_vw(dy, dy.shape[-1], st, 0 if aligned else 1), "dense" if st == add_.shape[-1] else "slice")


def _head_form(ops, x, NO, lungs, sigmoid):
    vps = x.shape[1] * x.shape[2] * x.shape[3]
    NOT = 2 if NO <= 2 else (9 if NO <= 9 else 16)
    mode = "plain" if not sigmoid else ("sig-lungs" if lungs is not None else "sig")
    return (f"NO{NOT}", mode, "capped" if _L(ops).dram_head_nblk(vps) == 512 else "uncapped")


def k_head_fwd(ops, x, w, bias, lungs, sigmoid):
    return _head_form(ops, x, w.shape[0], lungs, sigmoid)


def k_head_bwd(ops, x, w, dense, gdense, gpool, lungs, sigmoid):
    return _head_form(ops, x, w.shape[0], lungs, sigmoid)


def _seg_form(ops, cle):
    return ("capped" if _L(ops).dram_segloss_nblk(cle.numel()) == 1024 else "uncapped",)


def k_segloss_fwd(ops, cle, pse, lungs, ems, binary, smoothness=0.85):
    return _seg_form(ops, cle)


def k_segloss_bwd(ops, cle, pse, lungs, ems, binary, coef, smoothness=0.85):
    return _seg_form(ops, cle)


def k_regloss_tail(ops, partial, *rest):
    return ("loop" if partial.shape[0] > 256 else "one-pass",)


def k_upproject(ops, dense, ess, size):
    return ("capped" if _L(ops).dram_upproject_nblk(ess[0].numel()) == 1024 else "uncapped",)


KEYS = {n[2:]: f for n, f in dict(globals()).items() if n.startswith("k_")}


def act_dtype(args):
    for v in args.values():
        if isinstance(v, torch.Tensor) and v.dtype in (F32, BF16):
            return str(v.dtype).replace("torch.", "")
    return "float32"


def key_of(ops, name, *a, **k):
    ba = inspect.signature(KEYS[name]).bind(ops, *a, **k)
    ba.apply_defaults()
    args = dict(ba.arguments)
    args.pop("ops")
    return (name, act_dtype(args), KEYS[name](ops, *a, **k))


def meta(shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


# ------------------------------------------------------------------------------------------------ 2. statistic folds
FOLD_PN = [1, 1024, 1025, 8192, 40000]
FOLD_S = {1: 1, 1024: 1, 1025: 3, 8192: 16, 40000: 64}       # stage rows: one block / ticket / ticket at the 64 cap
FOLD_C = [64, 80, 2048]                                        # 80: a partial column group in both modes
FOLD_EPS = 1e-12

def to_f32(v):
    """v rounded to float32 (what a kernel's float argument widens back to double)"""
    return struct.unpack("f", struct.pack("f", v))[0]


MOM, EPS = to_f32(0.1), to_f32(1e-5)


def fold_partials(Pn, C, seed):
    """[Pn, 2, C]: per part one 'element' v (sum) and v^2 + e (sum of squares, e >= 0: a non-negative variance)."""
    v = randn((Pn, C), seed, offset=0.5)
    e = rand((Pn, C), seed + 1)
    return torch.stack([v, v * v + e], 1).contiguous()


def check_sums(got, part, what):
    """got [R, C] float64 against the fp64 device sum of the same fp32 partial rows.  The fold adds in double: a term
    passes through <= Pn / (16 S) lane additions, the 16-lane fold and the S stage rows (<= 2 600 + 16 + 64 roundings of
    2^-53 for every Pn here), the reference's tree sum through fewer -- 1e-12 of sum |term| bounds both with room."""
    ref = part.double().sum(0)
    mag = part.double().abs().sum(0)
    ex = Excess(what)
    ex.add(got.reshape(ref.shape), ref, FOLD_EPS * mag)
    ex.check()
    return ref, mag


@pytest.mark.parametrize("C", FOLD_C)
@pytest.mark.parametrize("Pn", FOLD_PN)
def test_statistic_fold_and_finalize(ops, poison, Pn, C):
    """ops.reduce_partials (plain, with tail, with want_f32, R = 1 and 2) and ops.bn_fold_finalize: sums within 1e-12 of
    sum |term| of the fp64 sums; finalize's mean, invstd, scale, shift and running-stat update within two fp32
    roundings (2^-23) of the fp64 formulas on those sums (count = Pn, so Pn = 1 is the count = 1 case)."""
    L = _L(ops)
    assert L.dram_fold_partials_stages(Pn) == FOLD_S[Pn]
    part = fold_partials(Pn, C, seed=Pn + C)
    ref, mag = check_sums(ops.reduce_partials(part), part, "reduce_partials")
    flat, view = ops.reduce_partials(part, tail=12345.0)
    check_sums(view, part, "reduce_partials(tail)")
    assert float(flat[-1]) == 12345.0 and flat.shape == (2 * C + 1,)
    sums, f32 = ops.reduce_partials(part, want_f32=True)
    check_sums(sums, part, "reduce_partials(want_f32)")
    for r in range(2):                               # the float copy is the double total rounded once
        assert torch.equal(f32[r], sums[r].float()), r
    check_sums(ops.reduce_partials(part.reshape(Pn, 1, 2 * C)), part.reshape(Pn, 1, 2 * C), "reduce_partials(R=1)")
    _, (s1,) = ops.reduce_partials(part.reshape(Pn, 1, 2 * C), want_f32=True)
    assert torch.equal(s1, ops.reduce_partials(part.reshape(Pn, 1, 2 * C)).reshape(-1).float())

    gamma = randn((C,), 7, scale=0.2, offset=1.0)
    beta = randn((C,), 8, scale=0.2)
    rm, rv = randn((C,), 9, scale=0.1), rand((C,), 10, 0.5, 1.5)
    rm0, rv0 = rm.double(), rv.double()
    count = float(Pn)
    mean, invstd, scale, shift = ops.bn_fold_finalize(part, count, gamma, beta, rm, rv, MOM, EPS)
    m = ref[0] / count
    var = (ref[1] / count - m * m).clamp_min(0.0)
    istd = 1.0 / torch.sqrt(var + EPS)
    g, b = gamma.double(), beta.double()
    unb = var * (count / (count - 1.0)) if count > 1 else var
    ex = Excess(f"bn_fold_finalize Pn={Pn} C={C}")
    ex.add(mean, m, 2 * U * m.abs() + 1e-9 * mag[0] / count)
    ex.add(invstd, istd, 2 * U * istd)
    ex.add(scale, g * istd, 2 * U * (g * istd).abs())
    ex.add(shift, b - m * g * istd, 2 * U * (b.abs() + (m * g * istd).abs()) + 1e-9 * mag[0] / count)
    ex.add(rm, (1 - MOM) * rm0 + MOM * m, 2 * U * ((1 - MOM) * rm0.abs() + MOM * m.abs()) + 1e-9 * mag[0] / count)
    ex.add(rv, (1 - MOM) * rv0 + MOM * unb, 2 * U * ((1 - MOM) * rv0 + MOM * unb))
    ex.check()


def test_ticket_fold_is_deterministic_and_its_tickets_are_per_call(ops, poison):
    """S = 16 (8 192 parts): 32 folds on one stream bit-identical to the first (which is within the bound); then folds
    of different data in flight together on the data stream and on ops.side_stream -- each call's ticket words are its
    own (csrc/bn.hip FOLD_XMAX comment), so both results stay exact whatever the interleaving."""
    Pn, C = 8192, 64
    assert _L(ops).dram_fold_partials_stages(Pn) == 16
    pa, pb = fold_partials(Pn, C, 101), fold_partials(Pn, C, 202)
    first = ops.reduce_partials(pa)
    check_sums(first, pa, "S=16 fold")
    again = [ops.reduce_partials(pa) for _ in range(31)]
    assert all(torch.equal(r, first) for r in again)
    g1, b1 = randn((C,), 3, offset=1.0), randn((C,), 4)
    fin0 = torch.stack(ops.bn_fold_finalize(pa, float(Pn), g1, b1, torch.zeros(C, device=DEV), torch.ones(C, device=DEV),
                                            MOM, EPS))
    for _ in range(7):
        fin = torch.stack(ops.bn_fold_finalize(pa, float(Pn), g1, b1, torch.zeros(C, device=DEV),
                                               torch.ones(C, device=DEV), MOM, EPS))
        assert torch.equal(fin, fin0)
    first_b = ops.reduce_partials(pb)
    check_sums(first_b, pb, "S=16 fold (second data)")
    cur, side = torch.cuda.current_stream(), ops.side_stream(0)
    side.wait_stream(cur)
    outs_a, outs_b = [], []
    for _ in range(16):
        outs_a.append(ops.reduce_partials(pa))
        with ops.on_stream(side):
            outs_b.append(ops.reduce_partials(pb))
    cur.wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(r, first) for r in outs_a)
    assert all(torch.equal(r, first_b) for r in outs_b)


@pytest.mark.parametrize("nparts,S", [(64, 1), (65, 3), (5000, 64)])
def test_abi_reduce_partials_single_and_two_stage(ops, poison, nparts, S):
    """dram_reduce_partials (C ABI only): the single pass up to 64 parts, the two-stage form above, tail behind."""
    L = _L(ops)
    assert L.dram_reduce_partials_stages(nparts) == S
    R, C = 2, 80
    part = fold_partials(nparts, C, nparts)
    sums = torch.empty((R * C + 1,), device=DEV, dtype=F64)
    scratch = torch.empty((S * R * C,), device=DEV, dtype=F64) if S > 1 else None
    rc = L.dram_reduce_partials(ops._p(part), ops._p(sums), ops._p(scratch), nparts, R, C, 3.5, 1, ops._stream())
    assert rc == 0
    check_sums(sums[:R * C].view(R, C), part, f"dram_reduce_partials nparts={nparts}")
    assert float(sums[-1]) == 3.5


# ------------------------------------------------------------------------------------------------ 3. BatchNorm
BN_CASES = [
    # id, y shape [B,D,H,W,C], dtype, residual (None | "id" | ("a", rs, residual shape)), claimed bn_apply form
    ("stem-f32", (2, 64, 128, 128, 64), F32, None, "shot-nt"),                 # 537 MB
    ("stem-bf16", (2, 64, 128, 128, 64), BF16, None, "shot-nt"),               # exactly 256 MiB
    ("stem-less-bf16", (2, 63, 128, 128, 64), BF16, None, "shot"),             # just below it
    ("layer1-f32", (2, 32, 64, 64, 64), F32, None, "shot"),
    ("layer1-id-f32", (2, 32, 64, 64, 64), F32, "id", "shot"),
    ("layer1-id-bf16", (2, 32, 64, 64, 64), BF16, "id", "shot"),
    ("decoder-c32-f32", (2, 64, 128, 128, 32), F32, None, "shot-nt"),
    ("decoder-c32-bf16", (2, 64, 128, 128, 32), BF16, None, "shot"),
    ("shortcut-a-s2-f32", (2, 16, 32, 32, 128), F32, ("a", 2, (2, 32, 64, 64, 64)), "shortcut-a"),
    ("shortcut-a-s2-bf16", (2, 16, 32, 32, 128), BF16, ("a", 2, (2, 31, 63, 64, 64)), "shortcut-a"),
    ("shortcut-a-pad-f32", (1, 32, 64, 64, 256), F32, ("a", 1, (1, 32, 64, 64, 64)), "shortcut-a"),
    ("r50-layer4-f32", (1, 16, 32, 32, 2048), F32, None, "generic"),
    ("r50-layer4-id-f32", (1, 16, 32, 32, 2048), F32, "id", "generic"),
    ("config4-bf16", (1, 128, 256, 256, 64), BF16, None, "shot-nt"),           # 537 M elements
]


def bn_case_calls(case):
    """(name, args, kwargs) of every instrumented call the BatchNorm case makes, with meta tensors (the census's
    static table, and what the case asserts about its own calls)."""
    _, shape, dt, res, _ = case
    y = meta(shape, dt)
    C = shape[-1]
    r = None if res is None else (y if res == "id" else meta(res[2], dt))
    rs = res[1] if isinstance(res, tuple) else 1
    vec = meta((C,))
    sums = meta((2, C), F64)
    calls = [("bn_apply", (y, vec, vec, r, rs, True), {})]
    for zsrc in (["z", "scale"] if res is None else ["z"]):
        z = y if zsrc == "z" else None
        calls.append(("bn_bwd_reduce", (y, z, y, vec, vec, True, vec, vec), {}))
        for wc in (False, True):
            calls.append(("bn_bwd_apply", (y, z, y, vec, vec, vec, sums, 1.0, True, vec, vec), dict(want_colsum=wc)))
    calls.append(("colsum", (y,), {}))
    return calls


def _bn_inputs(case):
    _, shape, dt, res, _ = case
    y = randn(shape, 1, dt, scale=2.0, offset=0.5)
    if res is None:
        return y, None, 1
    if res == "id":
        return y, randn(shape, 2, dt), 1
    return y, randn(res[2], 2, dt), res[1]


def _shortcut_full(r, rs, shape):
    B, D, H, W, C = shape
    sub = r.double()[:, ::rs, ::rs, ::rs, :][:, :D, :H, :W, :]
    return F.pad(sub, (0, C - r.shape[-1])).reshape(-1, C)


@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_batchnorm_apply_backward_colsum(ops, poison, case):
    """bn_apply, bn_bwd_reduce (mask from z, and from scale / shift), bn_bwd_apply (with and without want_colsum) and
    colsum, element by element against fp64 on the same operands:
      bn_apply: |z - ref| <= 4 u (|y scale| + |shift| + |res|) (fma + residual add; the shortcut-A kernel's unfused
        multiply-add one more), bf16 plus the store rounding;
      bn_bwd_apply: |dy - ref| <= 8 u |gamma invstd| (|g| + |mean g| + |xhat mean(g xhat)|) -- the batch means rounded to
        float, xhat two roundings, the product one, the two subtractions and the two scalings one each;
      column sums (fp32 per thread, then the double fold): |S - ref| <= kappa u sum |term| + per-term error, kappa = the
        fp32 additions a term passes through: rows per thread + row groups + 2 for colreduce (rows_per_block / (256 /
        min(C/4, 256)) + 256 / min(C/4, 256) + 2), 16 quads per thread + 256 / (C/4) + 2 for bn_bwd_apply's column sums."""
    cid, shape, dt, res, form = case
    C = shape[-1]
    rows = math.prod(shape[:-1])
    calls = bn_case_calls(case)
    assert key_of(ops, *calls[0][:1], *calls[0][1])[2][0] == form
    y, r, rs = _bn_inputs(case)
    scale = randn((C,), 3, scale=0.5, offset=1.0)
    shift = randn((C,), 4, scale=0.3)
    mean = randn((C,), 5, scale=0.1, offset=0.5)
    invstd = rand((C,), 6, 0.3, 0.8)
    gamma = randn((C,), 7, scale=0.2, offset=1.0)
    sc, sh = scale.double(), shift.double()
    mu, ist, ga = mean.double(), invstd.double(), gamma.double()

    assert k_bn_apply(ops, y, scale, shift, r, rs, True)[0] == form
    z = ops.bn_apply(y, scale, shift, r, rs, True)
    yf, zf = y.view(rows, C), z.view(rows, C)
    rsmall = _shortcut_full(r, rs, shape) if (r is not None and res != "id") else None
    ex = Excess(f"{cid} bn_apply")
    for sl in row_chunks(rows, C):
        yy = yf[sl].double()
        if r is None:
            rr = torch.zeros((), device=DEV, dtype=F64)
        elif res == "id":
            rr = r.view(rows, C)[sl].double()
        else:
            rr = rsmall[sl]
        pre = yy * sc + sh + rr
        ref = pre.clamp_min(0.0)
        ex.add(zf[sl], ref, store_bound(ref, dt, 4 * U * ((yy * sc).abs() + sh.abs() + rr.abs())))
    ex.check()
    del rsmall

    dz = randn(shape, 11, dt, offset=0.3)
    dzf = dz.view(rows, C)
    count = float(rows)
    rpb = max(64, -(-rows // 1024))
    lanes = min(C // 4, 256)
    kappa_red = rpb / (256 // lanes) + 256 // lanes + 2
    kappa_cs = 16 + 256 // (C // 4) + 2 if fixed_quad(C) else None
    for zsrc in (["z", "scale"] if r is None else ["z"]):
        zm = z if zsrc == "z" else None
        part = ops.bn_bwd_reduce(dz, zm, y, mean, invstd, True, scale, shift)
        assert part.shape == (_L(ops).dram_colsum_nparts(rows, C), 2, C)
        sums = ops.reduce_partials(part)
        ref_s = torch.zeros((2, C), device=DEV, dtype=F64)
        mag_s = torch.zeros((2, C), device=DEV, dtype=F64)
        for sl in row_chunks(rows, C):
            g = dzf[sl].double() * (zf[sl] > 0)
            gx = g * ((yf[sl].double() - mu) * ist)
            ref_s[0] += g.sum(0)
            ref_s[1] += gx.sum(0)
            mag_s[0] += g.abs().sum(0)
            mag_s[1] += gx.abs().sum(0)
        ex = Excess(f"{cid} bn_bwd_reduce mask={zsrc}")
        ex.add(sums, ref_s, (kappa_red + 3) * U * mag_s)
        ex.check()

        dy = ops.bn_bwd_apply(dz, zm, y, mean, invstd, gamma, sums, count, True, scale, shift)
        dy2, cp = ops.bn_bwd_apply(dz, zm, y, mean, invstd, gamma, sums, count, True, scale, shift, want_colsum=True)
        assert torch.equal(dy2, dy)
        del dy2
        mg, mgx = sums[0] / count, sums[1] / count
        dyf = dy.view(rows, C)
        ex = Excess(f"{cid} bn_bwd_apply mask={zsrc}")
        cs_ref = torch.zeros(C, device=DEV, dtype=F64)
        cs_mag = torch.zeros(C, device=DEV, dtype=F64)
        cs_err = torch.zeros(C, device=DEV, dtype=F64)
        for sl in row_chunks(rows, C):
            g = dzf[sl].double() * (zf[sl] > 0)
            xh = (yf[sl].double() - mu) * ist
            ref = ga * ist * (g - mg - xh * mgx)
            err = 8 * U * (ga * ist).abs() * (g.abs() + mg.abs() + (xh * mgx).abs())
            ex.add(dyf[sl], ref, store_bound(ref, dt, err))
            cs_ref += ref.sum(0)
            cs_mag += ref.abs().sum(0)
            cs_err += err.sum(0)
        ex.check()
        if cp is None:
            assert not fixed_quad(C)
        else:
            assert cp.shape == (_L(ops).dram_bn_bwd_apply_nparts(rows, C), 1, C)
            ex = Excess(f"{cid} bn_bwd_apply column sums mask={zsrc}")
            ex.add(ops.reduce_partials(cp)[0], cs_ref, cs_err + kappa_cs * U * cs_mag)
            ex.check()
        del dy, cp
    cs = ops.reduce_partials(ops.colsum(dz))[0]
    ref_c = torch.zeros(C, device=DEV, dtype=F64)
    mag_c = torch.zeros(C, device=DEV, dtype=F64)
    for sl in row_chunks(rows, C):
        ref_c += dzf[sl].double().sum(0)
        mag_c += dzf[sl].double().abs().sum(0)
    ex = Excess(f"{cid} colsum")
    ex.add(cs, ref_c, kappa_red * U * mag_c)
    ex.check()


# ------------------------------------------------------------------------------------------------ 4. pooling
POOL_CASES = [("stem-f32", (2, 64, 128, 128, 64), F32), ("stem-bf16", (2, 64, 128, 128, 64), BF16)]


def pool_case_calls(case):
    _, shape, dt = case
    B, D, H, W, C = shape
    y = meta(shape, dt)
    vec = meta((C,))
    out = meta((B, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2, C), dt)
    am = meta(out.shape, torch.uint8)
    wide = meta(shape[:-1] + (C + 64,), dt)[..., 64:]
    return [("bn_maxpool_fwd", (y, vec, vec), {}), ("maxpool_fwd", (y,), {}),
            ("maxpool_bwd", (out, am, shape, None), {}), ("maxpool_bwd", (out, am, shape, y), {}),
            ("maxpool_bwd", (out, am, shape, wide), {})]


@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_maxpool_at_the_stem_shape(ops, poison, case):
    """bn_maxpool_fwd, maxpool_fwd and maxpool_bwd (no add, a dense add, the add as a channel slice of a wider tensor)
    at the stem shape, on post-ReLU data (ties at 0 everywhere): pooled values EXACT, taps exactly F.max_pool3d's
    indices (first maximum in scan order), dx within (n + 1) u of sum |routed dy| + |add| (n <= 8 windows overlap)."""
    cid, shape, dt = case
    B, D, H, W, C = shape
    y = randn(shape, 1, dt)
    scale = randn((C,), 2, scale=0.3, offset=1.0)
    shift = randn((C,), 3, scale=0.3)
    z, pooled, am = ops.bn_maxpool_fwd(y, scale, shift)
    rows = B * D * H * W
    ex = Excess(f"{cid} bn_maxpool_fwd z")
    yf, zf = y.view(rows, C), z.view(rows, C)
    for sl in row_chunks(rows, C):
        yy = yf[sl].double()
        ref = (yy * scale.double() + shift.double()).clamp_min(0.0)
        ex.add(zf[sl], ref, store_bound(ref, dt, 4 * U * ((yy * scale.double()).abs() + shift.double().abs())))
    ex.check()
    assert float((z == 0).float().mean()) > 0.2                       # ties at 0
    x64 = z.permute(0, 4, 1, 2, 3).double().contiguous().requires_grad_(True)
    p_ref, idx = F.max_pool3d(x64, 3, 2, 1, return_indices=True)
    Do, Ho, Wo = p_ref.shape[2:]
    ar = lambda n: torch.arange(n, device=DEV)
    kz = idx // (H * W) - (2 * ar(Do) - 1).view(1, 1, Do, 1, 1)
    ky = (idx // W) % H - (2 * ar(Ho) - 1).view(1, 1, 1, Ho, 1)
    kx = idx % W - (2 * ar(Wo) - 1).view(1, 1, 1, 1, Wo)
    taps = (kz * 9 + ky * 3 + kx).to(torch.uint8).permute(0, 2, 3, 4, 1)
    assert torch.equal(pooled.double(), p_ref.detach().permute(0, 2, 3, 4, 1)), "bn_maxpool_fwd pooled values"
    assert torch.equal(am, taps), "bn_maxpool_fwd taps"
    p2, am2 = ops.maxpool_fwd(z)
    assert torch.equal(p2, pooled) and torch.equal(am2, taps), "maxpool_fwd"
    del p2, am2, kz, ky, kx
    gy = randn(pooled.shape, 4, dt)
    gy64 = gy.permute(0, 4, 1, 2, 3).double()
    (routed,) = torch.autograd.grad(p_ref, x64, gy64, retain_graph=True)
    (routed_abs,) = torch.autograd.grad(p_ref, x64, gy64.abs())
    routed = routed.permute(0, 2, 3, 4, 1)
    routed_abs = routed_abs.permute(0, 2, 3, 4, 1)
    del x64, p_ref, idx
    addt = randn(shape, 5, dt)
    wide = torch.cat([torch.zeros(shape[:-1] + (64,), device=DEV, dtype=dt), addt], -1)
    for what, add in (("no add", None), ("dense add", addt), ("slice add", wide[..., 64:])):
        dx = ops.maxpool_bwd(gy, am, shape, add)
        a64 = addt.double() if add is not None else 0.0
        ref = routed + a64
        err = 9 * U * (routed_abs + (a64.abs() if add is not None else 0.0))
        ex = Excess(f"{cid} maxpool_bwd {what}")
        ex.add(dx, ref, store_bound(ref, dt, err))
        ex.check()
        del dx, ref, err


# ------------------------------------------------------------------------------------------------ 4. heads
HEAD_CASES = [
    # id, mode, NO, (B, D, H, W), dtype, claimed grid
    ("cls-cap-f32", "cls", 9, (2, 64, 128, 128), F32, "capped"),          # 1 048 576 voxels: 512 blocks, at the cap
    ("cls-cap-bf16", "cls", 9, (2, 64, 128, 128), BF16, "capped"),
    ("cls-over-f32", "cls", 9, (2, 65, 128, 128), F32, "capped"),         # above the cap: more strides per block
    ("reg-cap-f32", "reg", 2, (2, 64, 128, 128), F32, "capped"),
    ("reg-cap-bf16", "reg", 2, (2, 64, 128, 128), BF16, "capped"),
    ("reg-over-f32", "reg", 2, (1, 72, 128, 128), F32, "capped"),
    ("reg_nolungs-cap-f32", "reg_nolungs", 2, (2, 64, 128, 128), F32, "capped"),
    ("no12-cap-f32", "cls", 12, (1, 64, 128, 128), F32, "capped"),        # the <16> template
    ("cls-small-f32", "cls", 9, (2, 32, 64, 64), F32, "uncapped"),
    ("reg-small-bf16", "reg", 2, (1, 32, 64, 64), BF16, "uncapped"),
]


def head_case_calls(case):
    _, mode, NO, (B, D, H, W), dt, _ = case
    x = meta((B, D, H, W, 32), dt)
    lungs = meta((B, 2 * D, 2 * H, 2 * W)) if mode == "reg" else None
    w, b = meta((NO, 32)), meta((NO,))
    sig = mode != "cls"
    dense = meta((B, NO, D, H, W))
    return [("head_fwd", (x, w, b, lungs, sig), {}),
            ("head_bwd", (x, w, dense if sig else None, dense, meta((B, NO)), lungs, sig), {})]


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_head_at_and_above_the_block_cap(ops, poison, case):
    """head_fwd / head_bwd against the fp64 1x1x1 convolution + sigmoid + nearest-lung pooling:
      dense: |d - ref| <= 48 u (|b| + sum |x w|) (x 1/4 through the sigmoid) + 6 u |ref| (expf and the division);
      pooled sums (per block fp32, folded here in fp64): kappa u sum |term| + sum of the dense bounds, kappa =
        strides per thread + 6 (wave) + 3 (four waves);
      dx: (NO + 6) u sum_c |dp_c w_c|; weight / bias gradient sums: (256 + strides + 6) u sum |dp x|."""
    cid, mode, NO, (B, D, H, W), dt, grid = case
    vps = D * H * W
    nblk = _L(ops).dram_head_nblk(vps)
    sig = mode != "cls"
    x = randn((B, D, H, W, 32), 1, dt)
    w = randn((NO, 32), 2, scale=0.3)
    b = randn((NO,), 3, scale=0.1)
    lungs = (rand((B, 2 * D, 2 * H, 2 * W), 4) > 0.4).float() if mode == "reg" else None
    assert k_head_fwd(ops, x, w, b, lungs, sig)[2] == grid
    dense, partial = ops.head_fwd(x, w, b, lungs, sig)
    X = x.view(B, vps, 32).double()
    W64, b64 = w.double(), b.double()
    pre = X @ W64.T + b64
    A = X.abs() @ W64.abs().T + b64.abs()
    ref = torch.sigmoid(pre) if sig else pre
    err = 48 * U * A * (0.25 if sig else 1.0) + 6 * U * ref.abs()
    del pre, A
    dn = dense.view(B, NO, vps).transpose(1, 2)
    ex = Excess(f"{cid} head_fwd dense")
    ex.add(dn, ref, err)
    ex.check()
    Lg = lungs[:, ::2, ::2, ::2].reshape(B, vps, 1).double() if lungs is not None else torch.ones(B, vps, 1, device=DEV,
                                                                                                 dtype=F64)
    term = ref * Lg if sig else ref
    iters = -(-vps // (nblk * 256))
    kappa = iters + 6 + 3
    ps = partial.double().sum(1)
    ex = Excess(f"{cid} head_fwd pooled sums")
    ex.add(ps[:, :NO], term.sum(1), kappa * U * term.abs().sum(1) + (err * (Lg if sig else 1.0)).sum(1))
    ex.add(ps[:, NO], Lg.sum((1, 2)), kappa * U * Lg.sum((1, 2)))
    ex.check()
    del term, err

    gpool = randn((B, NO), 5)
    gdense = randn((B, NO, D, H, W), 6, scale=0.01)
    dx, wpart = ops.head_bwd(x, w, dense if sig else None, gdense, gpool, lungs, sig)
    s = dn.double()
    gd = gdense.view(B, NO, vps).transpose(1, 2).double()
    gp = gpool.double().view(B, 1, NO)
    dp = (gp * (Lg if sig else 1.0) + gd)
    if sig:
        dp = dp * s * (1.0 - s)
    ex = Excess(f"{cid} head_bwd dx")
    dref = dp @ W64
    ex.add(dx.view(B, vps, 32), dref, store_bound(dref, dt, (NO + 6) * U * (dp.abs() @ W64.abs())))
    ex.check()
    del dref
    nparts = _L(ops).dram_head_bwd_nparts(vps)
    assert wpart.shape == (B * nparts, NO, 33)
    wg = ops.reduce_partials(wpart.reshape(B * nparts, 1, NO * 33)).reshape(NO, 33)
    Xb = torch.cat([X, torch.ones(B, vps, 1, device=DEV, dtype=F64)], -1)
    wref = torch.einsum("bvc,bvk->ck", dp, Xb)
    wmag = torch.einsum("bvc,bvk->ck", dp.abs(), Xb.abs())
    ex = Excess(f"{cid} head_bwd weight/bias gradient sums")
    ex.add(wg, wref, (256 + -(-((vps + 255) // 256) // nparts) + 6) * U * wmag)
    ex.check()


# ------------------------------------------------------------------------------------------------ 4. dRAM losses
SEG_CASES = [("2.1M", (2, 64, 128, 128), "uncapped"), ("8.4M", (1, 128, 256, 256), "capped")]
SEG_EXTRA_KEYS = [("segloss_fwd", "float32", ("uncapped",)), ("segloss_bwd", "float32", ("uncapped",))]


def seg_inputs(dims, seed):
    B, D, H, W = dims
    cle = rand((B, D, H, W), seed, 0.0, 0.6)
    pse = rand((B, D, H, W), seed + 1, 0.0, 0.6)
    lungs = (rand((B, 2 * D, 2 * H, 2 * W), seed + 2) > 0.4).float()
    ems = (rand((B, 2 * D, 2 * H, 2 * W), seed + 3) > 0.7).float() * lungs
    binary = torch.tensor([1.0, 0.0][:B] if B > 1 else [1.0], device=DEV)
    return cle, pse, lungs, ems, binary


@pytest.mark.parametrize("case", SEG_CASES, ids=[c[0] for c in SEG_CASES])
def test_segloss_block_sums_and_gradient_fields(ops, poison, case):
    """segloss_fwd's six sums and segloss_bwd's two fields against the fp64 formulas of csrc/head_loss.hip (the clamp
    decisions from the kernel's own fp32 p = cle + pse, rounded once as the kernel does): sums within
    (strides + 6 + 2 + 4) u sum |term| (4 u: the fp32 log and its scaling), fields within 8 u of the sum of their terms'
    magnitudes."""
    cid, dims, grid = case
    B, D, H, W = dims
    total = B * D * H * W
    nblk = _L(ops).dram_segloss_nblk(total)
    cle, pse, lungs, ems, binary = seg_inputs(dims, 21)
    assert k_segloss_fwd(ops, cle, pse, lungs, ems, binary)[0] == grid
    part = ops.segloss_fwd(cle, pse, lungs, ems, binary)
    assert part.shape == (nblk, 6)
    L = lungs[:, ::2, ::2, ::2].double()
    t = ems[:, ::2, ::2, ::2].double() * binary.double().view(B, 1, 1, 1)
    c, q = cle.double(), pse.double()
    p32 = cle + pse                                                 # the kernel's fp32 sum
    t32 = ems[:, ::2, ::2, ::2] * binary.view(B, 1, 1, 1)
    pc32 = p32.clamp(0.0, 1.0)
    pt = torch.where(t32 > 0, pc32, 1.0 - pc32).double()            # t in {0, 1}: the kernel's fp32 pt, exactly
    lo, hi = to_f32(1e-6), to_f32(1.0 - to_f32(1e-6))
    ptc = pt.clamp(lo, hi)
    cw = 0.85 * L + (1 - L)
    nl = -cw * torch.log(ptc)
    terms = [t, nl * t, nl * (1 - t), (c * L) * (q * L), c * L, q * L]
    kappa = -(-total // (nblk * 256)) + 6 + 2 + 4
    s = part.double().sum(0)
    ex = Excess(f"segloss_fwd {cid}")
    for k, tm in enumerate(terms):
        ex.add(s[k], tm.sum(), kappa * U * tm.abs().sum())
    ex.check()
    st, A1, A0, I, S1, S2 = [float(v) for v in s]
    alpha = min(max(1.0 - st / B, 0.3), 0.7)
    sw = alpha * st + (1 - alpha) * (total - st)
    den = S1 + S2 + 1e-7
    coef = torch.tensor([2.0 * 2 / den, 2.0 * (2 * I + 1e-7) / den ** 2, alpha / sw, (1 - alpha) / sw, 0, 0, 0, 0],
                        dtype=F32, device=DEV)
    k0, k1, k2, k3 = coef[:4].double()
    gc, gp = ops.segloss_bwd(cle, pse, lungs, ems, binary, coef)
    inr = (pt >= lo) & (pt <= hi) & (p32 >= 0) & (p32 <= 1)
    gb = torch.where(inr, -cw * (2 * t - 1) / ptc * (k2 * t + k3 * (1 - t)), torch.zeros((), device=DEV, dtype=F64))
    ex = Excess(f"segloss_bwd {cid}")
    for got, other in ((gc, q), (gp, c)):
        ref = k0 * other * L * L - k1 * L + gb
        ex.add(got, ref, 8 * U * ((k0 * other * L * L).abs() + (k1 * L).abs() + gb.abs()))
    ex.check()


def test_regression_train_loss_tail_folds_1024_rows(ops, poison):
    """models.reg_train_loss at 8.4 M voxels (1 x 128 x 256 x 256 dense maps): segloss_fwd writes 1 024 block rows and
    regloss_tail_kernel loops over all of them; loss and parts against oracle.reg_train_loss in fp64 within 1e-5
    relative (the fp32 block sums carry <= (32 + 12) u = 2.6e-6 each, the dice / BCE ratios double it, the O(B)
    interval terms are double)."""
    from bodyct_dram_emph_subtype_amd import models
    from oracle import med3d_oracle as orc
    dims = (1, 128, 256, 256)
    assert _L(ops).dram_segloss_nblk(math.prod(dims)) == 1024
    cle, pse, lungs, ems, _ = seg_inputs(dims, 31)
    B = 1
    reg = [rand((B,), 40 + i, 0.05, 0.85) for i in range(2)]
    cl, pl = torch.tensor([3], device=DEV), torch.tensor([1], device=DEV)
    cw, pw = rand((B,), 44, 0.1, 1.1), rand((B,), 45, 0.1, 1.1)
    vol = lambda v: v.view(B, 1, *v.shape[1:])
    seen = []
    real = ops.regloss_tail

    def spy(partial, *a, **k):
        seen.append(partial.shape[0])
        return real(partial, *a, **k)

    from unittest import mock
    with mock.patch.object(ops, "regloss_tail", spy):
        loss, parts = models.reg_train_loss([vol(cle), vol(pse)], reg, vol(lungs), vol(ems), cl, pl, cw, pw)
    assert seen == [1024]
    with torch.no_grad():
        # oracle.reg_train_loss term by term: its O(B) interval terms on the host (its band tables are host tensors),
        # the segmentation terms on the device
        bands = lambda lab, rmap: orc.regression_labels(lab.tolist(), rmap).double()
        lc = orc.interval_regression_loss(reg[0].double().cpu(), bands(cl, orc.CLE_RATIO_MAP), cw.double().cpu())
        lp = orc.interval_regression_loss(reg[1].double().cpu(), bands(pl, orc.PSE_RATIO_MAP), pw.double().cpu())
        binary = torch.logical_or(cl > 0, pl > 0).double()
        size = dims[1:]
        seg_labels = F.interpolate(vol(ems).double() * binary.view(B, 1, 1, 1, 1), size, mode="nearest")
        lung_labels = F.interpolate(vol(lungs).double(), size=size, mode="nearest")
        mul, seg = orc.segmentation_loss(vol(cle).double(), vol(pse).double(), seg_labels, lung_labels)
        parts_ref = dict(loss_cle=lc, loss_pse=lp, mul_loss=mul, seg_loss=seg)
        l_ref = float(lc) + float(lp) + 2.0 * float(mul) + float(seg)
    assert abs(float(loss) - float(l_ref)) <= 1e-5 * max(1.0, abs(float(l_ref))), (float(loss), float(l_ref))
    for k, v in parts_ref.items():
        assert abs(float(parts[k]) - float(v)) <= 1e-5 * max(1.0, abs(float(v))), (k, float(parts[k]), float(v))


# ------------------------------------------------------------------------------------------------ 4. up-projection
UP_CASES = [("2x128x256x256", (2, 64, 128, 128), (128, 256, 256)), ("scan-151x512x512", (1, 64, 128, 128), (151, 512, 512))]


@pytest.mark.parametrize("case", UP_CASES, ids=[c[0] for c in UP_CASES])
def test_upproject_grid_stride(ops, poison, case):
    """upproject against F.interpolate(trilinear, align_corners=True) in fp64, times ess: per element
    sum over axes of |fp32 source-position error| (<= 2 u (in - 1) + u) x the local spread of dense, plus 8 u max |dense|;
    per-sample block sums (folded in fp64) within kappa u sum |out| + the element bounds, kappa = strides + 9."""
    cid, (B, D, H, W), size = case
    vps = math.prod(size)
    nblk = _L(ops).dram_upproject_nblk(vps)
    assert nblk == 1024 and vps > 1024 * 256                   # capped grid: every thread strides
    dense = rand((B, D, H, W), 51)
    ess = (rand((B,) + size, 52) > 0.5).float()
    assert k_upproject(ops, dense, ess, size)[0] == "capped"
    out, partial = ops.upproject(dense, ess, size)
    assert partial.shape == (B, nblk)
    ref = F.interpolate(dense.double()[:, None], size=size, mode="trilinear", align_corners=True)[:, 0] * ess.double()
    spread = float(dense.max() - dense.min())
    pos = sum(2 * U * (n - 1) + U for n in (D, H, W))
    eb = (pos * spread + 8 * U * float(dense.abs().max())) * ess.double()
    ex = Excess(f"upproject {cid}")
    ex.add(out, ref, eb)
    kappa = -(-vps // (nblk * 256)) + 9
    ex.add(partial.double().sum(1), ref.sum((1, 2, 3)), kappa * U * ref.abs().sum((1, 2, 3)) + eb.sum((1, 2, 3)))
    ex.check()


# ------------------------------------------------------------------------------------------------ 4. scan reductions
SCAN = (301, 512, 512)       # ~79 M voxels: 1 024 blocks (the cap), every thread strides ~301 times, ragged last stride


def scan_volume(seed):
    return rand(SCAN, seed, -1400.0, 200.0)


def test_window_stats_of_prepare_image(ops, poison):
    """transforms.prepare_image at a scan-sized volume: the block sums of the window / z-score statistics (its
    dram_window_stats partial rows, kept from the poisoned allocation) against the fp64 sums of the same windowed scan
    -- (strides + 9 + 3) u sum |term|, the 3 for window01's subtraction, division and the square -- and the mean and
    standard deviation prepare_image derives from them against the fp64 statistics (the variance is a one-pass
    difference: its bound is the propagated sum bounds)."""
    from bodyct_dram_emph_subtype_amd import transforms
    n = math.prod(SCAN)
    nblk = _L(ops).dram_window_stats_nblk(n)
    assert nblk == 1024 and n > nblk * 256
    scan = scan_volume(61)
    poison.keep = lambda t: tuple(t.shape) == (nblk, 2) and t.dtype == F32
    out = transforms.prepare_image(scan, SCAN)
    assert len(poison.kept) == 1
    partial = poison.kept[0]
    lo, hi = transforms.FROM_SPAN
    w = ((scan.double().clamp(lo, hi) - lo) / (hi - lo)).reshape(-1)
    kappa = -(-n // (nblk * 256)) + 9 + 3
    s = partial.double().sum(0)
    S1, S2 = w.sum(), (w * w).sum()
    ex = Excess("window_stats block sums")
    ex.add(s[0], S1, kappa * U * S1)
    ex.add(s[1], S2, kappa * U * S2)
    ex.check()
    mean = s[0] / n
    var = (s[1] - n * mean * mean) / (n - 1)
    m_ref = S1 / n
    v_ref = w.var()                                              # unbiased, two-pass in fp64
    d1, d2 = kappa * U * S1, kappa * U * S2
    assert float((mean - m_ref).abs()) <= float(d1 / n) + 1e-12
    assert float((var - v_ref).abs()) <= float((d2 + 2 * m_ref * d1 + d1 * d1 / n) / (n - 1)) + 1e-12 * float(v_ref)
    assert bool(torch.isfinite(out).all())


def test_minmax_per_block(ops, poison):
    """dram_minmax (through ops._L()) at a scan-sized volume: every block's min / max EXACTLY the min / max over the
    elements of its grid-stride sequence (element i belongs to block (i // 256) % nblk), extremes planted in the ragged
    last stride."""
    L = _L(ops)
    n = math.prod(SCAN)
    nblk = L.dram_minmax_nblk(n)
    assert nblk == 1024
    x = scan_volume(71).reshape(-1)
    x[n - 1] = -5000.0
    x[n - 300] = 9000.0
    part = torch.empty((nblk, 2), device=DEV, dtype=F32)
    assert L.dram_minmax(ops._p(x), ops._p(part), n, ops._stream()) == 0
    per = nblk * 256
    padn = -(-n // per) * per
    lo = torch.cat([x, torch.full((padn - n,), math.inf, device=DEV)]).view(-1, nblk, 256).amin((0, 2))
    hi = torch.cat([x, torch.full((padn - n,), -math.inf, device=DEV)]).view(-1, nblk, 256).amax((0, 2))
    assert torch.equal(part[:, 0], lo) and torch.equal(part[:, 1], hi)
    assert float(part[:, 0].amin()) == -5000.0 and float(part[:, 1].amax()) == 9000.0


# ------------------------------------------------------------------------------------------------ 5. census
def covered_keys(ops):
    """(function, dtype, form) of every call the case tables above make."""
    calls = []
    for case in BN_CASES:
        calls += bn_case_calls(case)
    for case in POOL_CASES:
        calls += pool_case_calls(case)
    for case in HEAD_CASES:
        calls += head_case_calls(case)
    keys = {key_of(ops, n, *a, **k) for n, a, k in calls}
    for Pn in FOLD_PN:
        p = meta((Pn, 2, 64))
        for a, k in (((p,), {}), ((p, 1.0), {}), ((p,), dict(want_f32=True))):
            keys.add(key_of(ops, "reduce_partials", *a, **k))
        keys.add(key_of(ops, "bn_fold_finalize", p, 1.0, *[meta((64,))] * 4, MOM, EPS))
    for _, dims, _ in SEG_CASES:
        c = meta(dims)
        keys.add(key_of(ops, "segloss_fwd", c, c, c, c, c))
        keys.add(key_of(ops, "segloss_bwd", c, c, c, c, c, c))
    keys.add(key_of(ops, "regloss_tail", meta((1024, 6))))
    for _, _, size in UP_CASES:
        keys.add(key_of(ops, "upproject", meta((1, 4, 4, 4)), meta((1,) + size), size))
    return keys


def test_census_tables_declare_the_forms_their_cases_claim(ops):
    """the static table of the census agrees with the cases' own claims"""
    for case in BN_CASES:
        assert key_of(ops, *bn_case_calls(case)[0][:1], *bn_case_calls(case)[0][1])[2][0] == case[4], case[0]
    for case in HEAD_CASES:
        assert key_of(ops, "head_fwd", *head_case_calls(case)[0][1])[2][2] == case[5], case[0]
    assert {FOLD_S[p] > 1 for p in FOLD_PN} == {False, True}


CENSUS_OPS = sorted(KEYS)


def test_census_every_form_the_networks_reach_is_covered(ops, monkeypatch, capsys):
    """One eager full-size config-1 train step (resnet18segcls, batch 2, 1 x 128 x 256 x 256, fp32) and one config-2
    step in bf16 storage (resnet18segreg + the dRAM loss, same size) with every ops wrapper of the families above
    recording (function, dtype, form); every recorded form must be one a case of this module covers."""
    from bodyct_dram_emph_subtype_amd import med3d, models
    covered = covered_keys(ops)
    seen = set()
    for name in CENSUS_OPS:
        real = getattr(ops, name)

        def wrap(*a, _real=real, _name=name, **k):
            seen.add(key_of(ops, _name, *a, **k))
            return _real(*a, **k)

        monkeypatch.setattr(ops, name, wrap)
    dims = (128, 256, 256)
    for cfg, factory, B, dt in ((1, "resnet18segcls", 2, F32), (2, "resnet18segreg", 2, BF16)):
        torch.manual_seed(cfg)
        kw = dict(n_classes=[6, 3]) if factory.endswith("cls") else {}
        m = getattr(med3d, factory)(**kw).to(DEV).train()
        if dt == BF16:
            m.storage_dtype = BF16
        x = randn((B, 1) + dims, 80 + cfg)
        lungs = (rand((B, 1) + dims, 90 + cfg) > 0.3).float()
        dense, outs = m(x, lungs)
        if factory.endswith("cls"):
            loss = models.cls_train_loss(outs, torch.tensor([1, 4], device=DEV), torch.tensor([0, 2], device=DEV),
                                         torch.ones(6, device=DEV), torch.ones(3, device=DEV))[0]
            loss = loss + 1e-3 * dense[0].float().mean()
        else:
            ems = (x < -1.0).float() * lungs
            loss, _ = models.reg_train_loss(dense, outs, lungs, ems, torch.tensor([3, 0], device=DEV),
                                             torch.tensor([1, 0], device=DEV), torch.ones(B, device=DEV),
                                             torch.ones(B, device=DEV))
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        del m, x, lungs, dense, outs, loss
        torch.cuda.empty_cache()
    with capsys.disabled():
        print(f"\n[census] {len(seen)} forms reached by config 1 (fp32) and config 2 (bf16):")
        for k in sorted(seen, key=str):
            print(f"  {k}")
    missing = sorted(seen - covered, key=str)
    assert not missing, f"forms the networks reach that no case covers: {missing}"
