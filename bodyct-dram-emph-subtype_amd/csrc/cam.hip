// cam.hip -- class-activation maps at the target layer (the us3 output A that the heads read): Grad-CAM, HiResCAM,
// LayerCAM of a score s with cotangents (gdense, gpool) on the head outputs.  The gradient at the layer,
//   G[b,v,k] = d s / d A[b,v,k] = sum_c w[c][k] * dpre[b,c,v]      (dpre exactly as dram_head_bwd defines it),
// has rank NO per voxel, so it is formed in registers from the voxel's own 32 channels and never written:
//   hirescam / layercam   one pass over A:  M = r(sum_k G * A)  /  r(sum_k max(G, 0) * A)
//   gradcam               alpha[b,k] = (1/V) sum_v G[b,v,k] = (1/V) sum_c w[c][k] * (sum_v dpre[b,c,v]):
//                         a sum pass (per-block partial sums of dpre, folded in double by dram_fold_partials) and a
//                         combine pass M = r(sum_k alpha[b,k] * A).
// Deterministic: fixed-order block sums, no atomics.  A is read as head_fwd_kernel reads it: one voxel per lane, its
// whole 128-B (fp32) / 64-B (bf16) channel vector in 16-byte loads.  Element offsets are 32-bit (hosts check < 2^31).
#include "common.h"

namespace {

// LDS image of the head: w[NO][32] at c * 32 + k, bias[NO] behind NOT rows
template <int NOT>
__device__ __forceinline__ void load_head(float* wl, const float* __restrict__ w, const float* __restrict__ bias, int NO) {
  for (int i = threadIdx.x; i < NO * 32; i += 256) wl[i] = w[i];
  for (int i = threadIdx.x; i < NO; i += 256) wl[NOT * 32 + i] = bias[i];
}

template <typename T>
__device__ __forceinline__ void load_voxel(float4 (&xv)[8], const T* __restrict__ x, int voxel) {
#pragma unroll
  for (int k = 0; k < 8; ++k) xv[k] = ld4<T>(x, voxel * 32 + 4 * k);
}

__device__ __forceinline__ float lung_at(const float* __restrict__ lungs, const NearGeom& ng, int b, int v, int H, int W) {
  if (!lungs) return 1.f;
  const int xo = v % W, r = v / W;
  return lungs[near_index(ng, b, r / H, r % H, xo)];
}

// dpre[c] = (gdense[b][c][v] + gpool[b][c] * L) * (sigmoid ? s (1 - s) : 1), s = sigmoid(bias[c] + w[c] . x) summed in
// head_fwd_kernel's order (the value `dense` holds); plane = b * NO * vps + v
template <int NOT>
__device__ __forceinline__ void dpre_of(float (&dp)[NOT], const float4 (&xv)[8], const float* wl,
                                        const float* __restrict__ gdense, const float (&gp)[NOT], float L, int plane,
                                        int vps, int NO, int sigmoid) {
#pragma unroll
  for (int c = 0; c < NOT; ++c) {
    dp[c] = 0.f;
    if (c < NO) {
      float g = gp[c] * (sigmoid ? L : 1.f);
      if (gdense) g += gdense[plane + c * vps];
      if (sigmoid) {
        float s = wl[NOT * 32 + c];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          s += xv[k].x * wl[c * 32 + 4 * k] + xv[k].y * wl[c * 32 + 4 * k + 1] + xv[k].z * wl[c * 32 + 4 * k + 2] +
               xv[k].w * wl[c * 32 + 4 * k + 3];
        }
        s = 1.f / (1.f + expf(-s));
        g *= s * (1.f - s);
      }
      dp[c] = g;
    }
  }
}

// ----------------------------------------------------------------------------- hirescam / layercam: one pass
// grid (ceil(vps / 256), B): one-shot blocks, one voxel per thread
template <int NOT, typename T>
__global__ __launch_bounds__(256) void cam_point_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ gdense,
                                                        const float* __restrict__ gpool, const float* __restrict__ lungs,
                                                        NearGeom ng, float* __restrict__ out, int H, int W, int vps,
                                                        int NO, int sigmoid, int positive_part, int relu) {
  __shared__ float wl[NOT * 32 + NOT];
  load_head<NOT>(wl, w, bias, NO);
  __syncthreads();
  const int b = blockIdx.y;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= vps) return;
  float gp[NOT];
#pragma unroll
  for (int c = 0; c < NOT; ++c) gp[c] = (c < NO) ? gpool[b * NO + c] : 0.f;
  float4 xv[8];
  load_voxel<T>(xv, x, b * vps + v);
  float dp[NOT];
  dpre_of<NOT>(dp, xv, wl, gdense, gp, lung_at(lungs, ng, b, v, H, W), b * NO * vps + v, vps, NO, sigmoid);
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < NOT; ++c) {
      if (c < NO) {
        g.x += dp[c] * wl[c * 32 + 4 * k];
        g.y += dp[c] * wl[c * 32 + 4 * k + 1];
        g.z += dp[c] * wl[c * 32 + 4 * k + 2];
        g.w += dp[c] * wl[c * 32 + 4 * k + 3];
      }
    }
    if (positive_part) {
      g.x = fmaxf(g.x, 0.f); g.y = fmaxf(g.y, 0.f); g.z = fmaxf(g.z, 0.f); g.w = fmaxf(g.w, 0.f);
    }
    m += g.x * xv[k].x + g.y * xv[k].y + g.z * xv[k].z + g.w * xv[k].w;
  }
  out[b * vps + v] = relu ? fmaxf(m, 0.f) : m;
}

// ----------------------------------------------------------------------------- gradcam: sum pass
// grid (nblk, B), grid-stride inside a sample; partial [nblk][B][NO]: block sums of dpre.  Without the sigmoid dpre
// does not depend on A, and A is not read.
template <int NOT, typename T>
__global__ __launch_bounds__(256) void cam_sum_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, const float* __restrict__ gdense,
                                                      const float* __restrict__ gpool, const float* __restrict__ lungs,
                                                      NearGeom ng, float* __restrict__ partial, int H, int W, int vps,
                                                      int NO, int sigmoid) {
  __shared__ float wl[NOT * 32 + NOT];
  __shared__ float red[4][NOT];
  const int tid = threadIdx.x;
  load_head<NOT>(wl, w, bias, NO);
  __syncthreads();
  const int b = blockIdx.y;
  float gp[NOT], acc[NOT];
#pragma unroll
  for (int c = 0; c < NOT; ++c) {
    gp[c] = (c < NO) ? gpool[b * NO + c] : 0.f;
    acc[c] = 0.f;
  }
  for (int v = blockIdx.x * 256 + tid; v < vps; v += gridDim.x * 256) {
    asm volatile("" ::: "memory");       // the weights stay in LDS (head_fwd_kernel: hoisted, they cost 366 VGPRs)
    float4 xv[8];
    if (sigmoid) {
      load_voxel<T>(xv, x, b * vps + v);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) xv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float dp[NOT];
    dpre_of<NOT>(dp, xv, wl, gdense, gp, lung_at(lungs, ng, b, v, H, W), b * NO * vps + v, vps, NO, sigmoid);
#pragma unroll
    for (int c = 0; c < NOT; ++c) acc[c] += dp[c];
  }
#pragma unroll
  for (int c = 0; c < NOT; ++c) {
    const float s = wave_sum(acc[c]);
    if ((tid & 63) == 0) red[tid >> 6][c] = s;
  }
  __syncthreads();
  if (tid < NO) partial[(blockIdx.x * gridDim.y + b) * NO + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// ----------------------------------------------------------------------------- gradcam: combine pass
// alpha[b][k] = (sum_c w[c][k] * sums[b][c]) / V in double, then one pass over A.  grid (ceil(vps / 256), B)
template <typename T>
__global__ __launch_bounds__(256) void cam_combine_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                          const double* __restrict__ sums, float* __restrict__ out,
                                                          int vps, int NO, int relu) {
  __shared__ float al[32];
  const int b = blockIdx.y;
  if (threadIdx.x < 32) {
    double a = 0.0;
    for (int c = 0; c < NO; ++c) a += (double)w[c * 32 + threadIdx.x] * sums[b * NO + c];
    al[threadIdx.x] = (float)(a / (double)vps);
  }
  __syncthreads();
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= vps) return;
  float4 xv[8];
  load_voxel<T>(xv, x, b * vps + v);
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    m += al[4 * k] * xv[k].x + al[4 * k + 1] * xv[k].y + al[4 * k + 2] * xv[k].z + al[4 * k + 3] * xv[k].w;
  out[b * vps + v] = relu ? fmaxf(m, 0.f) : m;
}

inline int cam_blocks(long long vps) {
  long long b = (vps + 2047) / 2048;
  return (int)(b > 512 ? 512 : (b < 1 ? 1 : b));
}

// shared argument checks; the kernels index with 32-bit element offsets
inline int cam_args(const void* x, const float* w, const void* out, int B, int D, int H, int W, int NO) {
  if (!x || !w || !out || B < 1 || D < 1 || H < 1 || W < 1 || NO < 1 || NO > 16) return DRAM_ERR_BAD_ARG;
  if (B > 65535 || (long long)B * D * H * W * 32 >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  return DRAM_OK;
}

}  // namespace

extern "C" int dram_cam_nblk(long long voxels_per_sample) { return cam_blocks(voxels_per_sample); }

template <typename T>
static int cam_point_impl(const T* x, const float* w, const float* bias, const float* gdense, const float* gpool,
                          const float* lungs, int Dl, int Hl, int Wl, float* out, int B, int D, int H, int W, int NO,
                          int sigmoid, int method, int relu, dram_stream_t stream) {
  const int rc = cam_args(x, w, out, B, D, H, W, NO);
  if (rc != DRAM_OK) return rc;
  if (!bias || !gpool || (method != DRAM_CAM_HIRESCAM && method != DRAM_CAM_LAYERCAM)) return DRAM_ERR_BAD_ARG;
  if (lungs && (Dl < 1 || Hl < 1 || Wl < 1)) return DRAM_ERR_BAD_ARG;
  const int vps = D * H * W;
  const NearGeom ng = make_near(lungs ? Dl : 1, lungs ? Hl : 1, lungs ? Wl : 1, D, H, W);
  dim3 grid((vps + 255) / 256, B), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int pos = method == DRAM_CAM_LAYERCAM;
  DramProf prof(DRAM_FAM_HEAD_LOSS, 4, 0.0,
                (double)B * vps * (32.0 * sizeof(T) + 4.0 + 4.0 * ((gdense ? NO : 0) + (lungs ? 0.125 : 0.0))), s);
  if (NO <= 2)
    hipLaunchKernelGGL((cam_point_kernel<2, T>), grid, block, 0, s, x, w, bias, gdense, gpool, lungs, ng, out, H, W, vps, NO, sigmoid, pos, relu);
  else if (NO <= 9)
    hipLaunchKernelGGL((cam_point_kernel<9, T>), grid, block, 0, s, x, w, bias, gdense, gpool, lungs, ng, out, H, W, vps, NO, sigmoid, pos, relu);
  else
    hipLaunchKernelGGL((cam_point_kernel<16, T>), grid, block, 0, s, x, w, bias, gdense, gpool, lungs, ng, out, H, W, vps, NO, sigmoid, pos, relu);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
extern "C" int dram_cam_point(const float* x, const float* w, const float* bias, const float* gdense, const float* gpool,
                              const float* lungs, int Dl, int Hl, int Wl, float* out, int B, int D, int H, int W, int NO,
                              int sigmoid, int method, int relu, dram_stream_t stream) {
  return cam_point_impl<float>(x, w, bias, gdense, gpool, lungs, Dl, Hl, Wl, out, B, D, H, W, NO, sigmoid, method, relu, stream);
}
extern "C" int dram_cam_point_bf16(const void* x, const float* w, const float* bias, const float* gdense,
                                   const float* gpool, const float* lungs, int Dl, int Hl, int Wl, float* out, int B, int D,
                                   int H, int W, int NO, int sigmoid, int method, int relu, dram_stream_t stream) {
  return cam_point_impl<bf16_t>((const bf16_t*)x, w, bias, gdense, gpool, lungs, Dl, Hl, Wl, out, B, D, H, W, NO, sigmoid,
                                method, relu, stream);
}

template <typename T>
static int cam_sum_impl(const T* x, const float* w, const float* bias, const float* gdense, const float* gpool,
                        const float* lungs, int Dl, int Hl, int Wl, float* partial, int B, int D, int H, int W, int NO,
                        int sigmoid, dram_stream_t stream) {
  const int rc = cam_args(x, w, partial, B, D, H, W, NO);
  if (rc != DRAM_OK) return rc;
  if (!bias || !gpool) return DRAM_ERR_BAD_ARG;
  if (lungs && (Dl < 1 || Hl < 1 || Wl < 1)) return DRAM_ERR_BAD_ARG;
  const int vps = D * H * W;
  const NearGeom ng = make_near(lungs ? Dl : 1, lungs ? Hl : 1, lungs ? Wl : 1, D, H, W);
  dim3 grid(cam_blocks(vps), B), block(256);
  hipStream_t s = (hipStream_t)stream;
  DramProf prof(DRAM_FAM_HEAD_LOSS, 5, 0.0,
                (double)B * vps * ((sigmoid ? 32.0 * sizeof(T) : 0.0) + 4.0 * ((gdense ? NO : 0) + (lungs ? 0.125 : 0.0))), s);
  if (NO <= 2)
    hipLaunchKernelGGL((cam_sum_kernel<2, T>), grid, block, 0, s, x, w, bias, gdense, gpool, lungs, ng, partial, H, W, vps, NO, sigmoid);
  else if (NO <= 9)
    hipLaunchKernelGGL((cam_sum_kernel<9, T>), grid, block, 0, s, x, w, bias, gdense, gpool, lungs, ng, partial, H, W, vps, NO, sigmoid);
  else
    hipLaunchKernelGGL((cam_sum_kernel<16, T>), grid, block, 0, s, x, w, bias, gdense, gpool, lungs, ng, partial, H, W, vps, NO, sigmoid);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
extern "C" int dram_cam_sum(const float* x, const float* w, const float* bias, const float* gdense, const float* gpool,
                            const float* lungs, int Dl, int Hl, int Wl, float* partial, int B, int D, int H, int W, int NO,
                            int sigmoid, dram_stream_t stream) {
  return cam_sum_impl<float>(x, w, bias, gdense, gpool, lungs, Dl, Hl, Wl, partial, B, D, H, W, NO, sigmoid, stream);
}
extern "C" int dram_cam_sum_bf16(const void* x, const float* w, const float* bias, const float* gdense, const float* gpool,
                                 const float* lungs, int Dl, int Hl, int Wl, float* partial, int B, int D, int H, int W,
                                 int NO, int sigmoid, dram_stream_t stream) {
  return cam_sum_impl<bf16_t>((const bf16_t*)x, w, bias, gdense, gpool, lungs, Dl, Hl, Wl, partial, B, D, H, W, NO, sigmoid,
                              stream);
}

template <typename T>
static int cam_combine_impl(const T* x, const float* w, const double* sums, float* out, int B, int D, int H, int W, int NO,
                            int relu, dram_stream_t stream) {
  const int rc = cam_args(x, w, out, B, D, H, W, NO);
  if (rc != DRAM_OK) return rc;
  if (!sums) return DRAM_ERR_BAD_ARG;
  const int vps = D * H * W;
  hipStream_t s = (hipStream_t)stream;
  DramProf prof(DRAM_FAM_HEAD_LOSS, 6, 0.0, (double)B * vps * (32.0 * sizeof(T) + 4.0), s);
  hipLaunchKernelGGL((cam_combine_kernel<T>), dim3((vps + 255) / 256, B), dim3(256), 0, s, x, w, sums, out, vps, NO, relu);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
extern "C" int dram_cam_combine(const float* x, const float* w, const double* sums, float* out, int B, int D, int H, int W,
                                int NO, int relu, dram_stream_t stream) {
  return cam_combine_impl<float>(x, w, sums, out, B, D, H, W, NO, relu, stream);
}
extern "C" int dram_cam_combine_bf16(const void* x, const float* w, const double* sums, float* out, int B, int D, int H,
                                     int W, int NO, int relu, dram_stream_t stream) {
  return cam_combine_impl<bf16_t>((const bf16_t*)x, w, sums, out, B, D, H, W, NO, relu, stream);
}
