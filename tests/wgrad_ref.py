"""fp64 references of the convolution weight gradient, written as plain tap loops (one float64 matmul per tap) on
whatever device the operands live on.  Tensors are NDHWC, as the kernels take them.

  wgrad_reference     dw[co][ci][tap] = sum_{b,z,y,x} dy[b,z,y,x,co] * xpad[b, z s + kz dil, y s + ky dil, x s + kx dil, ci]
                      and, with want_mag, A_w = sum |dy| |x| per element (the scale of a rounding bound);
  wino_reference      the same gradient for k = 3, stride 1, pad 1 THROUGH the in-plane Winograd F(2x2, 3x3) domain,
                      dw = G^T (sum (A dy A^T) .* (B^T x B)) G per z tap, with the two magnitude sums a rounding bound of
                      that arithmetic is built from: M = sum |A dy A^T| |B^T x B| and M_abs = sum (|A| |dy| |A^T|) (|B^T| |x| |B|).
"""
import torch
import torch.nn.functional as F

F64 = torch.float64


def out_extent(n, k, stride, pad, dil):
    return (n + 2 * pad - (dil * (k - 1) + 1)) // stride + 1


def wgrad_reference(x, dy, k, stride, pad, dil, want_mag=False):
    """x [B,D,H,W,Ci], dy [B,Do,Ho,Wo,Co] (any floating type, one device) -> dw [Co,Ci,k,k,k] float64 and A_w (same
    shape; None without want_mag)."""
    assert k in (1, 3)
    B, D, H, W, Ci = x.shape
    Bo, Do, Ho, Wo, Co = dy.shape
    assert Bo == B and (Do, Ho, Wo) == tuple(out_extent(n, k, stride, pad, dil) for n in (D, H, W))
    xp = F.pad(x.to(F64), (0, 0) + (pad, pad) * 3)
    dyt = dy.to(F64).reshape(-1, Co).T.contiguous()
    dyt_abs = dyt.abs() if want_mag else None
    dw = torch.zeros((Co, Ci, k ** 3), dtype=F64, device=x.device)
    Aw = torch.zeros_like(dw) if want_mag else None
    for tap in range(k ** 3):
        kz, ky, kx = tap // (k * k), (tap // k) % k, tap % k
        z0, y0, x0 = kz * dil, ky * dil, kx * dil
        xs = xp[:, z0:z0 + (Do - 1) * stride + 1:stride, y0:y0 + (Ho - 1) * stride + 1:stride,
                x0:x0 + (Wo - 1) * stride + 1:stride].reshape(-1, Ci)
        dw[:, :, tap] = dyt @ xs
        if want_mag:
            Aw[:, :, tap] = dyt_abs @ xs.abs()
    shape = (Co, Ci, k, k, k)
    return dw.view(shape), (Aw.view(shape) if want_mag else None)


# F(2x2, 3x3) for a weight gradient: the 4 x 4 input tile is transformed by B^T . B, the 2 x 2 tile of dy by A . A^T
# (A is the transpose of the forward's output transform), the 4 x 4 product sum by G^T . G into the 3 x 3 taps.
BT = [[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, -1.0]]
A = [[1.0, 0.0], [1.0, 1.0], [1.0, -1.0], [0.0, -1.0]]
GT = [[1.0, 0.5, 0.5, 0.0], [0.0, 0.5, -0.5, 0.0], [0.0, 0.5, 0.5, 1.0]]


def wino_reference(x, dy):
    """x [B,D,H,W,Ci], dy [B,D,H,W,Co] (k = 3, stride 1, pad 1, dilation 1) -> dict of float64 tensors:
      U     [Co,Ci,3,4,4]  the Winograd-domain sums per z tap a and point (i, j)
      dw    [Co,Ci,3,3,3]  G^T U G
      M     [Co,Ci,3,4,4]  sum |A dy A^T| |B^T x B|
      M_abs [Co,Ci,3,4,4]  sum (|A| |dy| |A^T|) (|B^T| |x| |B|)   (>= M: no cancellation inside a transform)
    2 x 2 tiles that reach past an odd extent are filled with zeros, like the kernel's."""
    B, D, H, W, Ci = x.shape
    Co = dy.shape[-1]
    assert tuple(dy.shape[:4]) == (B, D, H, W)
    dev = x.device
    bt, am, gt = (torch.tensor(m, dtype=F64, device=dev) for m in (BT, A, GT))
    ny, nx = (H + 1) // 2, (W + 1) // 2
    # input tiles [B, D+2, ny, nx, Ci, 4, 4]: rows 2 ty - 1 .. 2 ty + 2; one zero plane on either side in z
    xp = F.pad(x.to(F64), (0, 0, 1, 2 * nx - W + 1, 1, 2 * ny - H + 1, 1, 1))
    xt = xp.unfold(2, 4, 2).unfold(3, 4, 2)
    dt = F.pad(dy.to(F64), (0, 0, 0, 2 * nx - W, 0, 2 * ny - H)).unfold(2, 2, 2).unfold(3, 2, 2)   # [B,D,ny,nx,Co,2,2]
    assert xt.shape[2:4] == (ny, nx) and dt.shape[2:4] == (ny, nx)

    def tr(m, t):                                                   # m t m^T on the last two axes
        return torch.einsum("ip,...pq,jq->...ij", m, t, m)

    def points(t, C):                                               # [B,Z,ny,nx,C,4,4] -> [Z, 16, B ny nx, C]
        return t.permute(1, 5, 6, 0, 2, 3, 4).reshape(t.shape[1], 16, -1, C)

    V, Vabs = points(tr(bt, xt), Ci), points(tr(bt.abs(), xt.abs()), Ci)
    E, Eabs = points(tr(am, dt), Co), points(tr(am.abs(), dt.abs()), Co)
    out = {k: torch.zeros((3, 16, Co, Ci), dtype=F64, device=dev) for k in ("U", "M", "M_abs")}
    for a in range(3):
        for z in range(D):                                          # input plane z + a - 1 is plane z + a of the padded tiles
            out["U"][a] += E[z].transpose(1, 2) @ V[z + a]
            out["M"][a] += E[z].abs().transpose(1, 2) @ V[z + a].abs()
            out["M_abs"][a] += Eabs[z].transpose(1, 2) @ Vabs[z + a]
    out = {k: v.permute(2, 3, 0, 1).reshape(Co, Ci, 3, 4, 4) for k, v in out.items()}
    out["dw"] = tr(gt, out["U"])
    return out


def gt_abs(t):
    """|G^T| t |G| on the last two axes: a bound in the Winograd domain [.., 4, 4] carried to the taps [.., 3, 3]"""
    g = torch.tensor(GT, dtype=F64, device=t.device).abs()
    return torch.einsum("ip,...pq,jq->...ij", g, t, g)
