"""fp64 references of the convolution forward and data gradient, written as plain tap loops (one float64 matmul per
tap) on whatever device the operands live on.  Tensors are NDHWC, as the kernels take them; w is [Co, Ci, k, k, k].

  conv_reference      y[b,z,y,x,co] = bias[co] + sum_{tap,ci} xpad[b, z s + kz dil, y s + ky dil, x s + kx dil, ci] w[co][ci][tap]
                      and, with want_mag, A = sum |x| |w| (+ |bias|) per output element (the scale of a rounding bound);
  dgrad_reference     dx = the transpose of that map applied to dy, written as the TRANSPOSED loop: every tap scatter-adds
                      dy @ w[:, :, tap] into the shifted (strided) slice of the padded gradient it was gathered from.  It
                      is deliberately not conv_reference on flipped weights: that is what the kernels do, and a mistake
                      shared by both would cancel;
  to_bf16_rne         float64 -> float32 -> bfloat16 (round to nearest even) for values whose first step is exact.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64


def out_extent(n, k, stride, pad, dil):
    return (n + 2 * pad - (dil * (k - 1) + 1)) // stride + 1


def _taps(k, dil):
    for tap in range(k ** 3):
        kz, ky, kx = tap // (k * k), (tap // k) % k, tap % k
        yield tap, kz * dil, ky * dil, kx * dil


def conv_reference(x, w, bias, k, stride, pad, dil, want_mag=False):
    """x [B,D,H,W,Ci], w [Co,Ci,k,k,k], bias [Co] or None (any floating type, one device) -> y [B,Do,Ho,Wo,Co] float64
    and A (same shape; None without want_mag)."""
    assert k in (1, 3) and tuple(w.shape[2:]) == (k, k, k)
    B, D, H, W, Ci = x.shape
    Co = w.shape[0]
    assert w.shape[1] == Ci
    Do, Ho, Wo = (out_extent(n, k, stride, pad, dil) for n in (D, H, W))
    xp = F.pad(x.to(F64), (0, 0) + (pad, pad) * 3)
    wt = w.to(F64).reshape(Co, Ci, k ** 3)
    y = torch.zeros((B * Do * Ho * Wo, Co), dtype=F64, device=x.device)
    A = torch.zeros_like(y) if want_mag else None
    for tap, z0, y0, x0 in _taps(k, dil):
        xs = xp[:, z0:z0 + (Do - 1) * stride + 1:stride, y0:y0 + (Ho - 1) * stride + 1:stride,
                x0:x0 + (Wo - 1) * stride + 1:stride].reshape(-1, Ci)
        y += xs @ wt[:, :, tap].T
        if want_mag:
            A += xs.abs() @ wt[:, :, tap].abs().T
    if bias is not None:
        y += bias.to(F64)
        if want_mag:
            A += bias.to(F64).abs()
    shape = (B, Do, Ho, Wo, Co)
    return y.view(shape), (A.view(shape) if want_mag else None)


def dgrad_reference(dy, w, in_shape, k, stride, pad, dil, want_mag=False):
    """dy [B,Do,Ho,Wo,Co], w [Co,Ci,k,k,k], in_shape (B,D,H,W,Ci) -> dx [B,D,H,W,Ci] float64 and A = sum |dy| |w| (same
    shape; None without want_mag)."""
    assert k in (1, 3) and tuple(w.shape[2:]) == (k, k, k)
    B, D, H, W, Ci = in_shape
    Co = w.shape[0]
    Do, Ho, Wo = (out_extent(n, k, stride, pad, dil) for n in (D, H, W))
    assert tuple(dy.shape) == (B, Do, Ho, Wo, Co) and w.shape[1] == Ci
    d2 = dy.to(F64).reshape(-1, Co)
    wt = w.to(F64).reshape(Co, Ci, k ** 3)
    padded = (B, D + 2 * pad, H + 2 * pad, W + 2 * pad, Ci)
    dxp = torch.zeros(padded, dtype=F64, device=dy.device)
    Ap = torch.zeros_like(dxp) if want_mag else None
    for tap, z0, y0, x0 in _taps(k, dil):
        sl = (slice(None), slice(z0, z0 + (Do - 1) * stride + 1, stride), slice(y0, y0 + (Ho - 1) * stride + 1, stride),
              slice(x0, x0 + (Wo - 1) * stride + 1, stride))
        dxp[sl] += (d2 @ wt[:, :, tap]).view(B, Do, Ho, Wo, Ci)
        if want_mag:
            Ap[sl] += (d2.abs() @ wt[:, :, tap].abs()).view(B, Do, Ho, Wo, Ci)
    crop = (slice(None),) + tuple(slice(pad, pad + n) for n in (D, H, W))
    return dxp[crop].contiguous(), (Ap[crop].contiguous() if want_mag else None)


def to_bf16_rne(t64):
    """float64 -> float32 -> bfloat16, round to nearest even.  Two roundings in a row are not one: the function refuses
    values whose float32 image is not the value itself (it is for the exact regime: integers below 2^24)."""
    assert t64.dtype == F64
    t32 = t64.to(torch.float32)
    if not torch.equal(t32.to(F64), t64):
        raise ValueError("to_bf16_rne: the float64 -> float32 step is inexact for some element")
    return t32.to(torch.bfloat16)
