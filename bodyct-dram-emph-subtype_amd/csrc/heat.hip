// heat.hip -- the activation-map volumes of the reference's _draw_predictions (models.py:192-234 classification,
// :455-493 regression): the dense head outputs [C][d][h][w] of one head, up-sampled x2 to the scan grid
// (F.interpolate(mode='trilinear'), align_corners=False), and
//   CLASSSUM  dp = sum_{c>=1} max(up_c, 0);  v = dp / (max over the volume of dp + 1e-7) * lung
//   PLAIN     v = up_0 * lung
// written as float and / or as uint8 = trunc(255 * clamp(v, 0, 1)) (utils.windowing(., (0, 1)).astype(uint8)).
// The up-sampled channels [C][2d][2h][2w] are never stored: the peak pass (per-block maxima, folded by the caller) and
// the write pass both recompute them from dense, which is 1/8 of one output channel per channel and stays in cache.
//
// At exactly x2 output k samples the source at max(k/2 - 0.25, 0): taps i0 = max((k-1)>>1, 0), i1 = min((k+1)>>1,
// n-1) with weights {0.75, 0.25} (k odd), {0.25, 0.75} (k even) and {0, 1} at k = 0 -- exact in fp32, and the border
// clamps are clamps of the indices, not branches.  One thread owns 8 consecutive output x (W % 8 == 0): per source row
// one aligned 16-byte load of source x 4t..4t+3 and the two neighbours at clamped indices; four rows (z0/z1 x y0/y1)
// per channel, all independent, are in flight together.  x is interpolated first, then y, then z (ATen's nesting),
// every product-sum as one fmaf of fixed shape, so a slice-mode result equals the full result's slices bit for bit.
// Offsets inside a sample are 32-bit (hosts check D*H*W < 2^31); sample / channel bases are 64-bit.
#include "common.h"

namespace {

struct HeatGeom {
  int d, h, w, D, H, W;
  long stride_b, stride_c;
};

__device__ __forceinline__ float mix2(float a, float wa, float b, float wb) { return fmaf(wb, b, wa * a); }

// taps of output index k on a source axis of n points
__device__ __forceinline__ void heat_taps(int k, int n, int& i0, int& i1, float& w0, float& w1) {
  i0 = max((k - 1) >> 1, 0);
  i1 = min((k + 1) >> 1, n - 1);
  w1 = k == 0 ? 1.f : ((k & 1) ? 0.25f : 0.75f);
  w0 = 1.f - w1;
}

// the 8 outputs x = 8t .. 8t+7 of one source row
__device__ __forceinline__ void heat_row(float (&o)[8], const float* __restrict__ row, int t, int w) {
  const float4 q = *reinterpret_cast<const float4*>(row + 4 * t);
  const float l = row[max(4 * t - 1, 0)];
  const float r = row[min(4 * t + 4, w - 1)];
  const float wl1 = t == 0 ? 1.f : 0.75f;
  o[0] = mix2(l, 1.f - wl1, q.x, wl1);
  o[1] = mix2(q.x, 0.75f, q.y, 0.25f);
  o[2] = mix2(q.x, 0.25f, q.y, 0.75f);
  o[3] = mix2(q.y, 0.75f, q.z, 0.25f);
  o[4] = mix2(q.y, 0.25f, q.z, 0.75f);
  o[5] = mix2(q.z, 0.75f, q.w, 0.25f);
  o[6] = mix2(q.z, 0.25f, q.w, 0.75f);
  o[7] = mix2(q.w, 0.75f, r, 0.25f);
}

// dp[e] at output (z, y, 8t + e) of sample base `db` (= dense + b * stride_b)
template <int MODE>
__device__ __forceinline__ void heat_dp(float (&dp)[8], const float* __restrict__ db, const HeatGeom& g, int C, int z,
                                        int y, int t) {
  int z0, z1, y0, y1;
  float wz0, wz1, wy0, wy1;
  heat_taps(z, g.d, z0, z1, wz0, wz1);
  heat_taps(y, g.h, y0, y1, wy0, wy1);
  const int r00 = (z0 * g.h + y0) * g.w, r01 = (z0 * g.h + y1) * g.w;
  const int r10 = (z1 * g.h + y0) * g.w, r11 = (z1 * g.h + y1) * g.w;
#pragma unroll
  for (int e = 0; e < 8; ++e) dp[e] = 0.f;
  const int c0 = MODE == DRAM_HEAT_CLASSSUM ? 1 : 0;
  const int c1 = MODE == DRAM_HEAT_CLASSSUM ? C : 1;
  for (int c = c0; c < c1; ++c) {
    const float* __restrict__ p = db + c * g.stride_c;
    float a[8], b2[8], e2[8], f[8];
    heat_row(a, p + r00, t, g.w);
    heat_row(b2, p + r01, t, g.w);
    heat_row(e2, p + r10, t, g.w);
    heat_row(f, p + r11, t, g.w);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float up = mix2(mix2(a[e], wy0, b2[e], wy1), wz0, mix2(e2[e], wy0, f[e], wy1), wz1);
      dp[e] = MODE == DRAM_HEAT_CLASSSUM ? dp[e] + fmaxf(up, 0.f) : up;
    }
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ----------------------------------------------------------------------------- peak pass (CLASSSUM)
// grid (nblk, B), grid-stride inside a sample; partial [B][nblk] = the block's maximum of dp (>= 0)
__global__ __launch_bounds__(256) void heat_peak_kernel(const float* __restrict__ dense, HeatGeom g, int C,
                                                        float* __restrict__ partial) {
  __shared__ float red[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* __restrict__ db = dense + b * g.stride_b;
  const int W8 = g.W >> 3, items = g.D * g.H * W8;
  float m = 0.f;
  for (int i = blockIdx.x * 256 + tid; i < items; i += gridDim.x * 256) {
    const int t = i % W8, r = i / W8;
    float dp[8];
    heat_dp<DRAM_HEAT_CLASSSUM>(dp, db, g, C, r / g.H, r % g.H, t);
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, dp[e]);
  }
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) partial[b * gridDim.x + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ----------------------------------------------------------------------------- write pass
// grid (ceil(nzo * H * W/8 / 256), B): one-shot blocks, 8 output x per thread; nzo = zsel ? nz : D
template <int MODE>
__global__ __launch_bounds__(256) void heat_volume_kernel(const float* __restrict__ dense, HeatGeom g, int C,
                                                          const uint8_t* __restrict__ lung,
                                                          const float* __restrict__ peak, const int* __restrict__ zsel,
                                                          int nzo, float* __restrict__ outf,
                                                          uint8_t* __restrict__ outb) {
  const int b = blockIdx.y;
  const int W8 = g.W >> 3, items = nzo * g.H * W8;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const int t = i % W8, r = i / W8, y = r % g.H, zi = r / g.H;
  int z = zi;
  if (zsel) z = min(max(zsel[b * nzo + zi], 0), g.D - 1);
  float dp[8];
  heat_dp<MODE>(dp, dense + b * g.stride_b, g, C, z, y, t);
  const int plane = g.H * g.W;
  const uint2 lb = *reinterpret_cast<const uint2*>(lung + ((long)b * g.D + z) * plane + y * g.W + 8 * t);
  float v[8];
  if (MODE == DRAM_HEAT_CLASSSUM) {
    const float m = peak[b] + 1e-7f;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = dp[e] / m;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = dp[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] *= (((e < 4 ? lb.x : lb.y) >> (8 * (e & 3))) & 0xffu) ? 1.f : 0.f;
  const long o = ((long)b * nzo + zi) * plane + y * g.W + 8 * t;
  if (outf) {
    *reinterpret_cast<float4*>(outf + o) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(outf + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
  if (outb) {   // utils.windowing(v, from_span=(0, 1)) then .astype(np.uint8), as resample_paste_kernel
    unsigned q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      double c = (double)v[e];
      c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
      q[e] = (unsigned)(c * 255.0);
    }
    *reinterpret_cast<uint2*>(outb + o) = make_uint2(q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24),
                                                     q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24));
  }
}

inline int heat_blocks(long long voxels) {
  long long b = (voxels + 2047) / 2048;     // 256 threads x 8 voxels
  return (int)(b > 512 ? 512 : (b < 1 ? 1 : b));
}

// shared argument checks -> the geometry
inline int heat_args(const float* dense, long long stride_b, long long stride_c, int C, int B, int d, int h, int w, int D,
                     int H, int W, HeatGeom* g) {
  if (!dense || B < 1 || C < 1 || d < 1 || h < 1 || w < 1 || stride_b < 0 || stride_c < 0) return DRAM_ERR_BAD_ARG;
  if (D != 2 * (long long)d || H != 2 * (long long)h || W != 2 * (long long)w) return DRAM_ERR_BAD_ARG;
  if ((w & 3) || (stride_b & 3) || (stride_c & 3) || ((uintptr_t)dense & 15)) return DRAM_ERR_BAD_ARG;
  if (B > 65535 || (long long)D * H * W >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  g->d = d; g->h = h; g->w = w; g->D = D; g->H = H; g->W = W;
  g->stride_b = (long)stride_b; g->stride_c = (long)stride_c;
  return DRAM_OK;
}

}  // namespace

extern "C" int dram_heat_nblk(long long voxels_per_sample) { return heat_blocks(voxels_per_sample); }

extern "C" int dram_heat_peak(const float* dense, long long stride_b, long long stride_c, int C, float* partial, int B,
                              int d, int h, int w, int D, int H, int W, dram_stream_t stream) {
  HeatGeom g;
  const int rc = heat_args(dense, stride_b, stride_c, C, B, d, h, w, D, H, W, &g);
  if (rc != DRAM_OK) return rc;
  if (!partial || C < 2) return DRAM_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  DramProf prof(DRAM_FAM_HEAD_LOSS, 7, 0.0, 4.0 * B * (C - 1) * (double)d * h * w, s);
  hipLaunchKernelGGL(heat_peak_kernel, dim3(heat_blocks((long long)D * H * W), B), dim3(256), 0, s, dense, g, C, partial);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_heat_volume(const float* dense, long long stride_b, long long stride_c, int C, const uint8_t* lung,
                                const float* peak, const int* zsel, int nz, float* out_f32, uint8_t* out_u8, int mode,
                                int B, int d, int h, int w, int D, int H, int W, dram_stream_t stream) {
  HeatGeom g;
  const int rc = heat_args(dense, stride_b, stride_c, C, B, d, h, w, D, H, W, &g);
  if (rc != DRAM_OK) return rc;
  if (!lung || (!out_f32 && !out_u8) || ((uintptr_t)lung & 7) || ((uintptr_t)out_f32 & 15) || ((uintptr_t)out_u8 & 7))
    return DRAM_ERR_BAD_ARG;
  if (mode == DRAM_HEAT_CLASSSUM ? (C < 2 || !peak) : (mode != DRAM_HEAT_PLAIN || C != 1)) return DRAM_ERR_BAD_ARG;
  if (zsel && nz <= 0) return DRAM_ERR_BAD_ARG;
  const int nzo = zsel ? nz : D;
  if ((long long)nzo * H * W >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  const int items = nzo * H * (W >> 3);
  hipStream_t s = (hipStream_t)stream;
  DramProf prof(DRAM_FAM_HEAD_LOSS, 8, 0.0,
                (double)B * (4.0 * (mode == DRAM_HEAT_CLASSSUM ? C - 1 : 1) * d * h * w +
                             (double)nzo * H * W * (1.0 + (out_f32 ? 4.0 : 0.0) + (out_u8 ? 1.0 : 0.0))), s);
  const dim3 grid((items + 255) / 256, B), block(256);
  if (mode == DRAM_HEAT_CLASSSUM)
    hipLaunchKernelGGL((heat_volume_kernel<DRAM_HEAT_CLASSSUM>), grid, block, 0, s, dense, g, C, lung, peak, zsel, nzo,
                       out_f32, out_u8);
  else
    hipLaunchKernelGGL((heat_volume_kernel<DRAM_HEAT_PLAIN>), grid, block, 0, s, dense, g, C, lung, peak, zsel, nzo, out_f32,
                       out_u8);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
