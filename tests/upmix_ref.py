"""The fp64 yardstick of csrc/upmix.hip (the tap / trilinear gather of the first decoder convolution): plain torch and
numpy, no GPU.  The 1-D operator's indices and weights follow the kernel's own fp32 recipe (lin_src in csrc/common.h,
which is also what torch's fp32 trilinear does) and enter every sum as exact float64 operands, so what is left between
a kernel and this file is the kernel's own fma chain.  `fused` selects the weight of the FORWARD kernels
(lin_src_fused in csrc/upmix.hip): the same indices, w1 = fl32(scale u - i0) with the product unrounded -- one fma --
where the recipe (the transposed kernel's) rounds s = fl32(scale u) first.  The per-pass functions work on the kernel's layouts

    forward   In[outer][Ni][m][3][C]  ->  Out[outer][2 Ni][m][C]
    backward  G[outer][2 Ni][m][C]    ->  H[outer][Ni][m][3][C]

accumulate in float64 and return, next to the result, the absolute sum  sum |w| |x|  of every output element: the
quantity the element-wise rounding bounds of tests/test_upmix_forms_gpu.py are multiples of.  A term inside the range
follows IEEE arithmetic (a zero weight times Inf is NaN, as in torch); a term outside it is absent.
tests/test_upmix_ref_host.py holds this file to exact rational weights and to F.interpolate in float64."""
import numpy as np
import torch

F64 = torch.float64


def lin_terms(Ni, fused=False):
    """per destination u in [0, 2 Ni): (i0, i1: int64 arrays; w0, w1: float32 arrays) of lin_src(u, scale, Ni) with
    scale = fl32(fl32(Ni - 1) / fl32(2 Ni - 1)), every operation rounded to fp32 as in the kernel.
    fused: w1 = fma(scale, u, -i0): scale u - i0 is exact in float64 (24 + 8 bits), then ONE rounding to fp32"""
    f = np.float32
    scale = f(Ni - 1) / f(2 * Ni - 1)            # 0 for Ni = 1
    u = np.arange(2 * Ni)
    s = (scale * u.astype(f)).astype(f)
    i0 = np.minimum(s.astype(np.int64), Ni - 1)
    i1 = i0 + (i0 < Ni - 1)
    w1 = (np.float64(scale) * u - i0).astype(f) if fused else (s - i0.astype(f)).astype(f)
    w0 = (f(1) - w1).astype(f)
    assert scale.dtype == f and s.dtype == f and w0.dtype == f and w1.dtype == f
    return i0, i1, w0, w1


def lin_weights(Ni, fused=False):
    """the dense 1-D operator A [2 Ni, Ni], float64: A[u][i0(u)] += w0(u), A[u][i1(u)] += w1(u)"""
    i0, i1, w0, w1 = lin_terms(Ni, fused)
    A = np.zeros((2 * Ni, Ni), dtype=np.float64)
    u = np.arange(2 * Ni)
    np.add.at(A, (u, i0), w0.astype(np.float64))
    np.add.at(A, (u, i1), w1.astype(np.float64))
    return A


def _terms(Ni, device, fused=False):
    i0, i1, w0, w1 = lin_terms(Ni, fused)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(device)
    return t(i0, torch.int64), t(i1, torch.int64), t(w0, F64), t(w1, F64)


def axis_fwd_ref(In, Ni, m, C, fused=False):
    """In: float64, numel outer * Ni * m * 3 * C -> (Out [outer, 2 Ni, m, C], its absolute sum), float64:
    Out[o][v][m][c] = sum_k [0 <= u = v + k - 1 < 2 Ni] (w0(u) In[o][i0(u)][m][k][c] + w1(u) In[o][i1(u)][m][k][c])
    fused: the forward kernels' weights (lin_terms)"""
    assert In.dtype == F64
    In = In.reshape(-1, Ni, m, 3, C)
    i0, i1, w0, w1 = _terms(Ni, In.device, fused)
    out = torch.zeros((In.shape[0], 2 * Ni, m, C), dtype=F64, device=In.device)
    mag = torch.zeros_like(out)
    for k in range(3):
        v = torch.arange(max(0, 1 - k), min(2 * Ni, 2 * Ni + 1 - k), device=In.device)     # 0 <= u < 2 Ni
        u = v + (k - 1)
        x0, x1 = In[:, i0[u], :, k, :], In[:, i1[u], :, k, :]
        a0, a1 = w0[u].view(1, -1, 1, 1), w1[u].view(1, -1, 1, 1)
        out[:, v] += a0 * x0 + a1 * x1
        mag[:, v] += a0.abs() * x0.abs() + a1.abs() * x1.abs()
    return out, mag


def axis_bwd_ref(G, Ni, m, C):
    """the transpose: G float64, numel outer * 2 Ni * m * C -> (H [outer, Ni, m, 3, C], its absolute sum):
    H[o][n][m][k][c] = sum_u [0 <= v = u - k + 1 < 2 Ni] ([i0(u) == n] w0(u) + [i1(u) == n] w1(u)) G[o][v][m][c]"""
    assert G.dtype == F64
    G = G.reshape(-1, 2 * Ni, m, C)
    i0, i1, w0, w1 = _terms(Ni, G.device)
    H = torch.zeros((G.shape[0], Ni, m, 3, C), dtype=F64, device=G.device)
    mag = torch.zeros_like(H)
    for k in range(3):
        v = torch.arange(max(0, 1 - k), min(2 * Ni, 2 * Ni + 1 - k), device=G.device)
        u = v + (k - 1)
        g = G[:, v]
        for idx, w in ((i0, w0), (i1, w1)):
            a = w[u].view(1, -1, 1, 1)
            hk, mk = torch.zeros_like(H[:, :, :, k]), torch.zeros_like(H[:, :, :, k])
            hk.index_add_(1, idx[u], a * g)
            mk.index_add_(1, idx[u], a.abs() * g.abs())
            H[:, :, :, k] += hk
            mag[:, :, :, k] += mk
    return H, mag


def fwd_passes(B, Ds, Hs, Ws):
    """the (outer, Ni, m) of the x, y and z pass of ops.upmix_gather_fwd"""
    return [(B * Ds * Hs, Ws, 9), (B * Ds, Hs, 2 * Ws * 3), (B, Ds, 4 * Hs * Ws)]


def bwd_passes(B, Ds, Hs, Ws):
    """the (outer, Ni, m) of the z, y and x pass of ops.upmix_gather_bwd"""
    return [(B, Ds, 4 * Hs * Ws), (B * Ds, Hs, 2 * Ws * 3), (B * Ds * Hs, Ws, 9)]


def gather_fwd_ref(b, Co, fused=False):
    """b [B,Ds,Hs,Ws,27 Co] float64 (column t Co + co, t = (kz 3 + ky) 3 + kx) -> (y [B,2Ds,2Hs,2Ws,Co], M): the three
    passes; M is the composed absolute sum |Az| |Ay| |Ax| |b|; fused: as in axis_fwd_ref"""
    B, Ds, Hs, Ws, N = b.shape
    assert N == 27 * Co
    y, mag = b, b.abs()
    for outer, Ni, m in fwd_passes(B, Ds, Hs, Ws):
        y, mag = axis_fwd_ref(y, Ni, m, Co, fused)[0], axis_fwd_ref(mag, Ni, m, Co, fused)[1]
    shape = (B, 2 * Ds, 2 * Hs, 2 * Ws, Co)
    return y.reshape(shape), mag.reshape(shape)


def gather_bwd_ref(dy, Co):
    """dy [B,2Ds,2Hs,2Ws,Co] float64 -> (h [B,Ds,Hs,Ws,27 Co], its composed absolute sum): the transposed passes in
    reverse order"""
    B, Do, Ho, Wo, C = dy.shape
    assert C == Co and not (Do | Ho | Wo) & 1
    Ds, Hs, Ws = Do // 2, Ho // 2, Wo // 2
    h, mag = dy, dy.abs()
    for outer, Ni, m in bwd_passes(B, Ds, Hs, Ws):
        h, mag = axis_bwd_ref(h, Ni, m, Co)[0], axis_bwd_ref(mag, Ni, m, Co)[1]
    shape = (B, Ds, Hs, Ws, 27 * Co)
    return h.reshape(shape), mag.reshape(shape)
