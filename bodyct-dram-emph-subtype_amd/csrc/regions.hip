// regions.hip -- the tail of the predict path with a lobe map: both heads' dRAM volumes up-projected to the network
// grid (trilinear, align_corners=True) times the ess mask, as dram_upproject stores them, and a per-region table
//   T[b][r] = { sum o_cle, sum o_pse, #(ess != 0), #voxels }   over the voxels with labels == r,  r = 0 .. n_regions
// (row 0: label 0 and every label above n_regions), in ONE pass: the index math, the weights and the ess / label
// bytes are shared between the heads, the masks are read as bytes (10 B per voxel with both volumes stored, 2 B for
// the table alone).  The per-region accumulators stay in registers: a compare-select over the rows, unrolled over a
// template row count (a private array indexed by the label would go to scratch); the two counts share one integer
// (ess count in the upper half, voxel count in the lower: a thread strides at most 2^13 times).  Per block one
// partial row, folded per sample in index order in double by a second launch: no atomics, no ticket word, no memset,
// bit-identical from call to call.  dram_prep_labels: the lobe crop resized by prep_mask_kernel's nearest rule, read
// through its strides in its own integer type and clamped to a byte.
#include "common.h"

namespace {

// The value upproject_kernel (pool_up.hip) stores, rounding for rounding.  Its source expression
//   wz0 * (wy0 * (wx0 * a000 + wx1 * a001) + wy1 * (wx0 * a010 + wx1 * a011)) + wz1 * (...),  w1 = scale * dst - i0
// leaves the compiler free to fuse either product of every sum into an fma, and which one it fuses is decided per
// kernel (here two heads share the weights, so the pairing differs): the same text does NOT give the same bits.  The
// two functions below therefore spell out, with contraction off, the form that kernel is compiled to -- the taps'
// weight is fma(scale, dst, -i0); of each pair of products the one marked `rn` is rounded and the other fused; the two
// z terms are both rounded before their sum.  tests/test_regions_gpu.py holds the result to dram_upproject's bit for
// bit at every launch form, so a compiler that decides otherwise for that kernel is noticed there.
__device__ __forceinline__ void up_src(int dst, float scale, int in, int& i0, int& i1, float& w0, float& w1) {
#pragma clang fp contract(off)
  const float d = (float)dst;
  i0 = (int)(scale * d);
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  w1 = __builtin_fmaf(scale, d, -(float)i0);
  w0 = 1.f - w1;
}

__device__ __forceinline__ float up_value(const float* __restrict__ p, int r00, int r01, int r10, int r11, int x0,
                                          int x1, float wz0, float wz1, float wy0, float wy1, float wx0, float wx1) {
#pragma clang fp contract(off)
  const float x00 = __builtin_fmaf(wx1, p[r00 + x1], /* rn */ wx0 * p[r00 + x0]);
  const float x01 = __builtin_fmaf(wx0, p[r01 + x0], /* rn */ wx1 * p[r01 + x1]);
  const float x10 = __builtin_fmaf(wx0, p[r10 + x0], /* rn */ wx1 * p[r10 + x1]);
  const float x11 = __builtin_fmaf(wx1, p[r11 + x1], /* rn */ wx0 * p[r11 + x0]);
  const float y0 = __builtin_fmaf(wy0, x00, /* rn */ wy1 * x01);
  const float y1 = __builtin_fmaf(wy1, x11, /* rn */ wy0 * x10);
  const float a = wz0 * y0, b = wz1 * y1;
  return a + b;
}

// out = trilinear(dense -> (Do,Ho,Wo), align_corners) * ess for both heads; per-block region sums.
// NR: rows the accumulators are unrolled over (>= n_regions + 1).  Offsets inside a sample are 32-bit (the host
// checks D*H*W and Do*Ho*Wo < 2^31); sample bases are 64-bit.
template <int NR>
__global__ __launch_bounds__(256) void upproject_regions_kernel(
    const float* __restrict__ cle, const float* __restrict__ pse, long bstride, const uint8_t* __restrict__ ess,
    const uint8_t* __restrict__ labels, float* __restrict__ out_cle, float* __restrict__ out_pse,
    float* __restrict__ partial, int D, int H, int W, int Do, int Ho, int Wo, float sz, float sy, float sx, int vps,
    int nblk, int n_regions) {
  __shared__ float sm[4][NR][4];
  const int b = blockIdx.y;
  const float* pc = cle + (long)b * bstride;
  const float* pp = pse + (long)b * bstride;
  const uint8_t* eb = ess + (long)b * vps;
  const uint8_t* lb = labels + (long)b * vps;
  float sc[NR], sp[NR];
  unsigned cnt[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) { sc[r] = 0.f; sp[r] = 0.f; cnt[r] = 0u; }
  // (zo, yo, xo) of the linear index v: divided once, then advanced by the stride's own (dz, dy, dx) with carries
  const unsigned stride = gridDim.x * 256u;
  const int dx = (int)(stride % (unsigned)Wo), dy = (int)(stride / (unsigned)Wo % (unsigned)Ho);
  const int dz = (int)(stride / (unsigned)Wo / (unsigned)Ho);
  unsigned v = blockIdx.x * 256u + threadIdx.x;
  int xo = (int)(v % (unsigned)Wo), yo = (int)(v / (unsigned)Wo % (unsigned)Ho), zo = (int)(v / (unsigned)Wo / (unsigned)Ho);
  for (; v < (unsigned)vps; v += stride) {
    int z0, z1, y0, y1, x0, x1;
    float wz0, wz1, wy0, wy1, wx0, wx1;
    up_src(zo, sz, D, z0, z1, wz0, wz1);
    up_src(yo, sy, H, y0, y1, wy0, wy1);
    up_src(xo, sx, W, x0, x1, wx0, wx1);
    const int r00 = (z0 * H + y0) * W, r01 = (z0 * H + y1) * W, r10 = (z1 * H + y0) * W, r11 = (z1 * H + y1) * W;
    const float vc = up_value(pc, r00, r01, r10, r11, x0, x1, wz0, wz1, wy0, wy1, wx0, wx1);
    const float vp = up_value(pp, r00, r01, r10, r11, x0, x1, wz0, wz1, wy0, wy1, wx0, wx1);
    const bool e = eb[v] != 0;
    const int lab = lb[v];
    const float ef = e ? 1.f : 0.f;
    const float oc = vc * ef, op = vp * ef;
    if (out_cle) {
      out_cle[(long)b * vps + v] = oc;
      out_pse[(long)b * vps + v] = op;
    }
    const int row = lab > n_regions ? 0 : lab;
    const unsigned inc = e ? 0x10001u : 1u;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const bool m = row == k;
      sc[k] += m ? oc : 0.f;
      sp[k] += m ? op : 0.f;
      cnt[k] += m ? inc : 0u;
    }
    xo += dx;
    const int cx = xo >= Wo ? 1 : 0;
    xo -= cx ? Wo : 0;
    yo += dy + cx;
    const int cy = yo >= Ho ? 1 : 0;
    yo -= cy ? Ho : 0;
    zo += dz + cy;
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const float a0 = wave_sum(sc[k]), a1 = wave_sum(sp[k]);
    const float a2 = wave_sum((float)(cnt[k] >> 16)), a3 = wave_sum((float)(cnt[k] & 0xffffu));   // exact: < 2^24
    if ((threadIdx.x & 63) == 0) { sm[wave][k][0] = a0; sm[wave][k][1] = a1; sm[wave][k][2] = a2; sm[wave][k][3] = a3; }
  }
  __syncthreads();
  const int cols = (n_regions + 1) * 4;
  if ((int)threadIdx.x < cols) {
    const int k = threadIdx.x >> 2, c = threadIdx.x & 3;
    partial[((long)b * nblk + blockIdx.x) * cols + threadIdx.x] = sm[0][k][c] + sm[1][k][c] + sm[2][k][c] + sm[3][k][c];
  }
}

// table[b][col] = sum_k partial[b][k][col] in double: 16 slices of consecutive k, each summed in index order, then the
// slices in order.  block (64, 16), grid B.
__global__ __launch_bounds__(1024) void region_fold_kernel(const float* __restrict__ partial, double* __restrict__ table,
                                                           int nblk, int cols) {
  __shared__ double sm[16][64];
  const int b = blockIdx.x, c = threadIdx.x, g = threadIdx.y;
  const int per = (nblk + 15) / 16;
  const int k0 = g * per, k1 = min(nblk, k0 + per);
  double s = 0.0;
  if (c < cols) {
    const float* p = partial + (long)b * nblk * cols + c;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) s += (double)p[(long)k * cols];
  }
  sm[g][c] = s;
  __syncthreads();
  if (g == 0 && c < cols) {
    double t = sm[0][c];
#pragma unroll
    for (int j = 1; j < 16; ++j) t += sm[j][c];
    table[(long)b * cols + c] = t;
  }
}

// out[zo][yo][xo] = clamp(labels[zidx[zo]][ys][xs], 0, 255): prep_mask_kernel's rule on an integer source with strides
template <typename LT>
__global__ void prep_labels_kernel(const LT* __restrict__ labels, long stride_z, long stride_y,
                                   const int* __restrict__ zidx, uint8_t* __restrict__ out, int D, int H, int W, int Do,
                                   int Ho, int Wo, float sy, float sx) {
  const long total = (long)Do * Ho * Wo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long r = i;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho);
    const int zo = (int)(r / Ho);
    int ys = (int)floorf((float)yo * sy), xs = (int)floorf((float)xo * sx);
    if (ys > H - 1) ys = H - 1;
    if (xs > W - 1) xs = W - 1;
    const int zs = min(max(zidx[zo], 0), D - 1);
    const int v = (int)labels[zs * stride_z + ys * stride_y + xs];
    out[i] = (uint8_t)min(max(v, 0), 255);
  }
}

inline float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

inline int grid_for(long n) {
  long b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" int dram_region_nblk(long long vps) {
  long long b = (vps + 1023) / 1024;
  return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

extern "C" int dram_upproject_regions(const float* cle, const float* pse, long long dense_batch_stride,
                                      const uint8_t* ess, const uint8_t* labels, float* out_cle, float* out_pse,
                                      float* partial, double* table, int B, int D, int H, int W, int Do, int Ho, int Wo,
                                      int n_regions, dram_stream_t stream) {
  if (!cle || !pse || !ess || !labels || !partial || !table || (out_cle == nullptr) != (out_pse == nullptr) || B < 1 ||
      D < 1 || H < 1 || W < 1 || Do < 1 || Ho < 1 || Wo < 1 || n_regions < 1 || n_regions > 15 ||
      dense_batch_stride < (long long)D * H * W)
    return DRAM_ERR_BAD_ARG;
  const long long vps = (long long)Do * Ho * Wo;
  if (vps >= (1LL << 31) || (long long)D * H * W >= (1LL << 31) || B > 65535) return DRAM_ERR_UNSUPPORTED;
  const int nblk = dram_region_nblk(vps), cols = (n_regions + 1) * 4;
  hipStream_t s = (hipStream_t)stream;
  {
    DramProf prof(DRAM_FAM_POOL_UP, 7, 0.0,
                  (double)B * (8.0 * D * H * W + (out_cle ? 10.0 : 2.0) * (double)vps + 4.0 * nblk * cols), s);
    const dim3 grid(nblk, B), block(256);
    if (n_regions < 8)
      hipLaunchKernelGGL((upproject_regions_kernel<8>), grid, block, 0, s, cle, pse, (long)dense_batch_stride, ess, labels,
                         out_cle, out_pse, partial, D, H, W, Do, Ho, Wo, ac_scale(D, Do), ac_scale(H, Ho), ac_scale(W, Wo),
                         (int)vps, nblk, n_regions);
    else
      hipLaunchKernelGGL((upproject_regions_kernel<16>), grid, block, 0, s, cle, pse, (long)dense_batch_stride, ess, labels,
                         out_cle, out_pse, partial, D, H, W, Do, Ho, Wo, ac_scale(D, Do), ac_scale(H, Ho), ac_scale(W, Wo),
                         (int)vps, nblk, n_regions);
    DRAM_LAUNCH_CHECK();
  }
  DramProf prof(DRAM_FAM_POOL_UP, 8, 0.0, (double)B * cols * (4.0 * nblk + 8.0), s);
  hipLaunchKernelGGL(region_fold_kernel, dim3(B), dim3(64, 16), 0, s, partial, table, nblk, cols);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_prep_labels(const void* labels, int label_dtype, long long stride_z, long long stride_y,
                                const int* zidx, uint8_t* out, int D, int H, int W, int Do, int Ho, int Wo,
                                dram_stream_t stream) {
  if (!labels || !zidx || !out || (label_dtype != 1 && label_dtype != 2) || D < 1 || H < 1 || W < 1 || Do < 1 || Ho < 1 ||
      Wo < 1 || stride_z < 0 || stride_y < 0)
    return DRAM_ERR_BAD_ARG;
  const long total = (long)Do * Ho * Wo;
  hipStream_t s = (hipStream_t)stream;
  DramProf prof(DRAM_FAM_PREP, 10, 0.0, (double)total * (1.0 + label_dtype), s);
  const dim3 grid(grid_for(total)), block(256);
  const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
  with_label_type(label_dtype, [&](auto t) {
    using LT = decltype(t);
    hipLaunchKernelGGL((prep_labels_kernel<LT>), grid, block, 0, s, (const LT*)labels, (long)stride_z, (long)stride_y, zidx,
                       out, D, H, W, Do, Ho, Wo, sy, sx);
  });
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
