// optim.hip -- multi-tensor Adam / SGD weight update (one launch for every parameter).
// Replaces torch.optim.Adam.step at reference models.py:385-387 / :689-691 (defaults
// betas=(0.9,0.999), eps=1e-8, weight_decay=0, no amsgrad) and the SGD(momentum,
// weight_decay) alternative the reference keeps as arguments (train.py:25,27;
// models.py:388-389).  HBM-bound: 28 B/param (read p,g,m,v; write p,m,v).
#include "common.h"

namespace {

// ONE element's update, the same instruction sequence on the vector and the scalar path (contraction pinned: left to
// the compiler the two paths fused differently, and a parameter whose gradient arrived 4-byte aligned -- a view of the
// data-parallel step's small-gradient bucket -- moved one ulp away from the same update of an aligned gradient).
// CLIP selects what happens to the scaled gradient on its way in (the *_clip entry points; 0 = the plain update):
//   CLIP_NORM   gg = (g * gscale) * cn          cn = clip[3], the coefficient dram_grad_norm_multi left there
//   CLIP_VALUE  gg = clamp(g * gscale, -cv, cv) cv = clip[1]; comparisons, so a NaN stays a NaN (torch.clamp)
// Everything behind gg is the one code for all three.
enum { CLIP_NONE = 0, CLIP_NORM = 1, CLIP_VALUE = 2 };
template <int CLIP>
__device__ __forceinline__ float clip_grad(const float g, const float gscale, const float cn, const float cv) {
#pragma clang fp contract(off)
  float gg = g * gscale;
  if constexpr (CLIP == CLIP_NORM) gg = gg * cn;
  if constexpr (CLIP == CLIP_VALUE) gg = gg < -cv ? -cv : (gg > cv ? cv : gg);
  return gg;
}
// the clip array selects its own mode: clip[1] (the value bound) is negative when the global norm is clipped
__device__ __forceinline__ bool clip_by_value(const float* __restrict__ clip) { return clip[1] >= 0.f; }

template <int CLIP>
__device__ __forceinline__ void adam1(float& p, const float g, float& m, float& v, const float b1, const float b2,
                                      const float eps, const float wd, const float step, const float rs2,
                                      const float gscale, const float cn, const float cv) {
#pragma clang fp contract(off)
  float gg = clip_grad<CLIP>(g, gscale, cn, cv);
  if (wd != 0.f) gg = __builtin_fmaf(wd, p, gg);
  m = __builtin_fmaf(b1, m, (1.f - b1) * gg);
  v = __builtin_fmaf(b2, v, ((1.f - b2) * gg) * gg);
  p -= (step * m) / __builtin_fmaf(sqrtf(v), rs2, eps);
}

template <int CLIP>
__device__ __forceinline__ void adam_chunk(const DramTensorRef* __restrict__ table,
                                           const DramChunkRef* __restrict__ chunks, float lr, float b1, float b2,
                                           float eps, float wd, float bc1, float bc2, float gscale, float cn = 1.f,
                                           float cv = 0.f) {
  const DramChunkRef ch = chunks[blockIdx.x];
  const DramTensorRef t = table[ch.tensor];
  const long n = t.n - ch.offset < DRAM_OPT_CHUNK ? t.n - ch.offset : DRAM_OPT_CHUNK;
  float* p = t.p + ch.offset;
  const float* g = t.g + ch.offset;
  float* m = t.m + ch.offset;
  float* v = t.v + ch.offset;
  const float step = lr / bc1;
  const float rs2 = 1.f / sqrtf(bc2);
  // torch: denom = sqrt(v)/sqrt(bc2) + eps ; p -= (lr/bc1) * m / denom
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  if (vec) {
    const long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256) {
      float4 pv = reinterpret_cast<float4*>(p)[i];
      const float4 gv = reinterpret_cast<const float4*>(g)[i];
      float4 mv = reinterpret_cast<float4*>(m)[i];
      float4 vv = reinterpret_cast<float4*>(v)[i];
      adam1<CLIP>(pv.x, gv.x, mv.x, vv.x, b1, b2, eps, wd, step, rs2, gscale, cn, cv);
      adam1<CLIP>(pv.y, gv.y, mv.y, vv.y, b1, b2, eps, wd, step, rs2, gscale, cn, cv);
      adam1<CLIP>(pv.z, gv.z, mv.z, vv.z, b1, b2, eps, wd, step, rs2, gscale, cn, cv);
      adam1<CLIP>(pv.w, gv.w, mv.w, vv.w, b1, b2, eps, wd, step, rs2, gscale, cn, cv);
      reinterpret_cast<float4*>(p)[i] = pv;
      reinterpret_cast<float4*>(m)[i] = mv;
      reinterpret_cast<float4*>(v)[i] = vv;
    }
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256)
      adam1<CLIP>(p[i], g[i], m[i], v[i], b1, b2, eps, wd, step, rs2, gscale, cn, cv);
  } else {
    // (16-byte alignment is not guaranteed: a data-parallel step hands over small gradients as views of one bucket)
    for (long i = threadIdx.x; i < n; i += 256)
      adam1<CLIP>(p[i], g[i], m[i], v[i], b1, b2, eps, wd, step, rs2, gscale, cn, cv);
  }
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const DramTensorRef* __restrict__ table,
                                                         const DramChunkRef* __restrict__ chunks, float lr, float b1,
                                                         float b2, float eps, float wd, float bc1, float bc2,
                                                         float gscale) {
  adam_chunk<CLIP_NONE>(table, chunks, lr, b1, b2, eps, wd, bc1, bc2, gscale);
}

// The same launch with the gradient clipped on its way in; the mode is uniform over the launch (one scalar load).
__global__ __launch_bounds__(256) void adam_multi_clip_kernel(const DramTensorRef* __restrict__ table,
                                                              const DramChunkRef* __restrict__ chunks, float lr, float b1,
                                                              float b2, float eps, float wd, float bc1, float bc2,
                                                              float gscale, const float* __restrict__ clip) {
  if (clip_by_value(clip)) adam_chunk<CLIP_VALUE>(table, chunks, lr, b1, b2, eps, wd, bc1, bc2, gscale, 1.f, clip[1]);
  else adam_chunk<CLIP_NORM>(table, chunks, lr, b1, b2, eps, wd, bc1, bc2, gscale, clip[3]);
}

// Graph-replayable form: every hyper-parameter AND the step count live in device memory, so a captured
// hipGraph of the train step stays valid while lr decays (ExponentialLR) and the bias corrections change.
// hyper = [lr, b1, b2, eps, wd, grad_scale, step]; step is advanced by adam_advance_kernel first.  The step slot
// holds the BITS of an int32 (exact for 2^31 steps; a float counter would stall at 2^24).
__global__ void adam_advance_kernel(float* __restrict__ hyper) {
  if (threadIdx.x == 0 && blockIdx.x == 0) reinterpret_cast<int*>(hyper)[6] += 1;
}
__global__ __launch_bounds__(256) void adam_multi_dev_kernel(const DramTensorRef* __restrict__ table,
                                                             const DramChunkRef* __restrict__ chunks,
                                                             const float* __restrict__ hyper) {
  const float b1 = hyper[1], b2 = hyper[2];
  const double t = (double)reinterpret_cast<const int*>(hyper)[6];
  // torch: bias_correction = 1 - beta ** step, evaluated in double on the host
  const float bc1 = (float)(1.0 - pow((double)b1, t)), bc2 = (float)(1.0 - pow((double)b2, t));
  adam_chunk<CLIP_NONE>(table, chunks, hyper[0], b1, b2, hyper[3], hyper[4], bc1, bc2, hyper[5]);
}

__global__ __launch_bounds__(256) void adam_multi_dev_clip_kernel(const DramTensorRef* __restrict__ table,
                                                                  const DramChunkRef* __restrict__ chunks,
                                                                  const float* __restrict__ hyper,
                                                                  const float* __restrict__ clip) {
  const float b1 = hyper[1], b2 = hyper[2];
  const double t = (double)reinterpret_cast<const int*>(hyper)[6];
  const float bc1 = (float)(1.0 - pow((double)b1, t)), bc2 = (float)(1.0 - pow((double)b2, t));
  if (clip_by_value(clip))
    adam_chunk<CLIP_VALUE>(table, chunks, hyper[0], b1, b2, hyper[3], hyper[4], bc1, bc2, hyper[5], 1.f, clip[1]);
  else adam_chunk<CLIP_NORM>(table, chunks, hyper[0], b1, b2, hyper[3], hyper[4], bc1, bc2, hyper[5], clip[3]);
}

template <int CLIP>
__device__ __forceinline__ void sgd_chunk(const DramTensorRef* __restrict__ table,
                                          const DramChunkRef* __restrict__ chunks, float lr, float mom, float wd,
                                          int first, float gscale, float cn = 1.f, float cv = 0.f) {
  const DramChunkRef ch = chunks[blockIdx.x];
  const DramTensorRef t = table[ch.tensor];
  const long n = t.n - ch.offset < DRAM_OPT_CHUNK ? t.n - ch.offset : DRAM_OPT_CHUNK;
  float* p = t.p + ch.offset;
  const float* g = t.g + ch.offset;
  float* m = t.m ? t.m + ch.offset : nullptr;
  for (long i = threadIdx.x; i < n; i += 256) {
    float gg;
    if constexpr (CLIP == CLIP_NONE) gg = g[i] * gscale;
    else gg = clip_grad<CLIP>(g[i], gscale, cn, cv);
    if (wd != 0.f) gg += wd * p[i];
    if (mom != 0.f && m) {
      const float bb = first ? gg : mom * m[i] + gg;
      m[i] = bb;
      gg = bb;
    }
    p[i] -= lr * gg;
  }
}

__global__ __launch_bounds__(256) void sgd_multi_kernel(const DramTensorRef* __restrict__ table,
                                                        const DramChunkRef* __restrict__ chunks, float lr, float mom,
                                                        float wd, int first, float gscale) {
  sgd_chunk<CLIP_NONE>(table, chunks, lr, mom, wd, first, gscale);
}
__global__ __launch_bounds__(256) void sgd_multi_clip_kernel(const DramTensorRef* __restrict__ table,
                                                             const DramChunkRef* __restrict__ chunks, float lr, float mom,
                                                             float wd, int first, float gscale,
                                                             const float* __restrict__ clip) {
  if (clip_by_value(clip)) sgd_chunk<CLIP_VALUE>(table, chunks, lr, mom, wd, first, gscale, 1.f, clip[1]);
  else sgd_chunk<CLIP_NORM>(table, chunks, lr, mom, wd, first, gscale, clip[3]);
}

// ---------------------------------------------------------------------------------------------------------
// Global gradient norm (torch.nn.utils.clip_grad_norm_, norm_type 2) over the same work list: block b writes the
// double sum of squares of chunk b, a one-block kernel folds the partials and leaves norm and coefficient in clip[].
// Nothing depends on which block ran when: no atomics, no ticket.
//
// Element i of a chunk belongs to lane (i / 4) % 256 and is the (i / 1024) * 4 + i % 4 -th term of that lane's
// chain, on the 16-byte path and on the scalar path alike (a gradient that is a view into the data-parallel
// step's small-gradient bucket is only 4-byte aligned): the sum is a function of the values alone.
__device__ __forceinline__ double block_sum_256(double s, double* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);     // a fixed pairing of lanes
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const DramTensorRef* __restrict__ table,
                                                         const DramChunkRef* __restrict__ chunks,
                                                         double* __restrict__ partials) {
  __shared__ double sm[4];
  const DramChunkRef ch = chunks[blockIdx.x];
  const DramTensorRef t = table[ch.tensor];
  const long n = t.n - ch.offset < DRAM_OPT_CHUNK ? t.n - ch.offset : DRAM_OPT_CHUNK;
  const float* g = t.g + ch.offset;
  const bool vec = (((uintptr_t)g & 15) == 0);
  double s = 0.0;
  if (vec && n == DRAM_OPT_CHUNK) {
    // a whole aligned chunk: the 16 loads of a lane are in flight together, summed in the order of the loop below
    float4 x[DRAM_OPT_CHUNK / 1024];
#pragma unroll
    for (int k = 0; k < DRAM_OPT_CHUNK / 1024; ++k) x[k] = reinterpret_cast<const float4*>(g)[threadIdx.x + 256 * k];
#pragma unroll
    for (int k = 0; k < DRAM_OPT_CHUNK / 1024; ++k) {
      s += (double)x[k].x * (double)x[k].x;
      s += (double)x[k].y * (double)x[k].y;
      s += (double)x[k].z * (double)x[k].z;
      s += (double)x[k].w * (double)x[k].w;
    }
  } else {
    for (long i = 4 * (long)threadIdx.x; i < n; i += 1024) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);      // (elements past the end add +0.0 to a non-negative sum)
      if (vec && i + 4 <= n) {
        x = *reinterpret_cast<const float4*>(g + i);
      } else {
        x.x = g[i];
        if (i + 1 < n) x.y = g[i + 1];
        if (i + 2 < n) x.z = g[i + 2];
        if (i + 3 < n) x.w = g[i + 3];
      }
      s += (double)x.x * (double)x.x;
      s += (double)x.y * (double)x.y;
      s += (double)x.z * (double)x.z;
      s += (double)x.w * (double)x.w;
    }
  }
  s = block_sum_256(s, sm);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One block: lane t sums partials t, t + 1024, ... in that order, the block folds its 1 024 lanes in a fixed tree.
// clip[2] = (float)(|grad_scale| sqrt(sum)), clip[3] = min(1, clip[0] / (clip[2] + 1e-6f)) in fp32 -- torch's
// clip_grad_norm_ arithmetic, a NaN norm giving a NaN coefficient as torch.clamp does.
__global__ __launch_bounds__(1024) void grad_norm_fold_kernel(const double* __restrict__ partials, int nparts,
                                                              float* __restrict__ clip, float gscale,
                                                              const float* __restrict__ hyper) {
  __shared__ double sm[1024];
  double s = 0.0;
  int p = threadIdx.x;
  for (; p + 3 * 1024 < nparts; p += 4 * 1024) {
    const double a = partials[p], b = partials[p + 1024], c = partials[p + 2048], d = partials[p + 3072];
    s += a;
    s += b;
    s += c;
    s += d;
  }
  for (; p < nparts; p += 1024) s += partials[p];
  sm[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int w = 512; w > 0; w >>= 1) {
    if (threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    const float gs = hyper ? hyper[5] : gscale;
    const float norm = (float)(fabs((double)gs) * sqrt(sm[0]));
    const float c = clip[0] / (norm + 1e-6f);
    clip[2] = norm;
    clip[3] = c > 1.f ? 1.f : c;
  }
}

// g = (g * clip[3]) or clamp(g, -clip[1], clip[1]) in place: torch.nn.utils.clip_grad_norm_ / clip_grad_value_ for
// callers who look at the gradients afterwards (the optimizers never rewrite a gradient).  Element-wise, so the two
// paths cannot differ.
template <int CLIP>
__device__ __forceinline__ void grad_scale_chunk(float* __restrict__ g, const long n, const float cn, const float cv) {
  if ((((uintptr_t)g) & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256) {
      float4 x = reinterpret_cast<float4*>(g)[i];
      x.x = clip_grad<CLIP>(x.x, 1.f, cn, cv);
      x.y = clip_grad<CLIP>(x.y, 1.f, cn, cv);
      x.z = clip_grad<CLIP>(x.z, 1.f, cn, cv);
      x.w = clip_grad<CLIP>(x.w, 1.f, cn, cv);
      reinterpret_cast<float4*>(g)[i] = x;
    }
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) g[i] = clip_grad<CLIP>(g[i], 1.f, cn, cv);
  } else {
    for (long i = threadIdx.x; i < n; i += 256) g[i] = clip_grad<CLIP>(g[i], 1.f, cn, cv);
  }
}
__global__ __launch_bounds__(256) void grad_scale_multi_kernel(const DramTensorRef* __restrict__ table,
                                                               const DramChunkRef* __restrict__ chunks,
                                                               const float* __restrict__ clip) {
  const DramChunkRef ch = chunks[blockIdx.x];
  const DramTensorRef t = table[ch.tensor];
  const long n = t.n - ch.offset < DRAM_OPT_CHUNK ? t.n - ch.offset : DRAM_OPT_CHUNK;
  float* g = const_cast<float*>(t.g) + ch.offset;     // the one launch that writes through DramTensorRef.g
  if (clip_by_value(clip)) grad_scale_chunk<CLIP_VALUE>(g, n, 1.f, clip[1]);
  else grad_scale_chunk<CLIP_NORM>(g, n, clip[3], 0.f);
}

}  // namespace

extern "C" int dram_adam_multi(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float lr,
                               float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                               float bias_corr2, float grad_scale, dram_stream_t stream) {
  if (!table || !chunks || nchunks < 1 || bias_corr1 <= 0.f || bias_corr2 <= 0.f) return DRAM_ERR_BAD_ARG;
  // 28 B per parameter (r p,g,m,v; w p,m,v); the chunk count bounds the parameter count from above
  DramProf prof(DRAM_FAM_OPTIM, 0, 0.0, 28.0 * (double)nchunks * 16384.0, (hipStream_t)stream);
  hipLaunchKernelGGL(adam_multi_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table, chunks, lr, beta1,
                     beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_adam_multi_dev(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float* hyper,
                                   dram_stream_t stream) {
  if (!table || !chunks || nchunks < 1 || !hyper) return DRAM_ERR_BAD_ARG;
  DramProf prof(DRAM_FAM_OPTIM, 2, 0.0, 28.0 * (double)nchunks * 16384.0, (hipStream_t)stream);
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper);
  DRAM_LAUNCH_CHECK();
  hipLaunchKernelGGL(adam_multi_dev_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table, chunks,
                     (const float*)hyper);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_sgd_multi(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float lr,
                              float momentum, float weight_decay, int first_step, float grad_scale,
                              dram_stream_t stream) {
  if (!table || !chunks || nchunks < 1) return DRAM_ERR_BAD_ARG;
  DramProf prof(DRAM_FAM_OPTIM, 1, 0.0, (momentum != 0.f ? 20.0 : 12.0) * (double)nchunks * 16384.0, (hipStream_t)stream);
  hipLaunchKernelGGL(sgd_multi_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table, chunks, lr, momentum,
                     weight_decay, first_step, grad_scale);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_grad_norm_multi(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, double* partials,
                                    float* clip, float grad_scale, const float* hyper, dram_stream_t stream) {
  if (!table || !chunks || nchunks < 1 || !partials || !clip) return DRAM_ERR_BAD_ARG;
  DramProf prof(DRAM_FAM_OPTIM, 3, 0.0, 4.0 * (double)nchunks * 16384.0, (hipStream_t)stream);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table, chunks, partials);
  DRAM_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_norm_fold_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)partials,
                     nchunks, clip, grad_scale, hyper);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_grad_scale_multi(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks,
                                     const float* clip, dram_stream_t stream) {
  if (!table || !chunks || nchunks < 1 || !clip) return DRAM_ERR_BAD_ARG;
  DramProf prof(DRAM_FAM_OPTIM, 7, 0.0, 8.0 * (double)nchunks * 16384.0, (hipStream_t)stream);
  hipLaunchKernelGGL(grad_scale_multi_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table, chunks, clip);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_adam_multi_clip(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                                    float bias_corr2, float grad_scale, const float* clip, dram_stream_t stream) {
  if (!table || !chunks || nchunks < 1 || bias_corr1 <= 0.f || bias_corr2 <= 0.f || !clip) return DRAM_ERR_BAD_ARG;
  DramProf prof(DRAM_FAM_OPTIM, 4, 0.0, 28.0 * (double)nchunks * 16384.0, (hipStream_t)stream);
  hipLaunchKernelGGL(adam_multi_clip_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table, chunks, lr, beta1,
                     beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale, clip);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_adam_multi_dev_clip(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float* hyper,
                                        const float* clip, dram_stream_t stream) {
  if (!table || !chunks || nchunks < 1 || !hyper || !clip) return DRAM_ERR_BAD_ARG;
  DramProf prof(DRAM_FAM_OPTIM, 6, 0.0, 28.0 * (double)nchunks * 16384.0, (hipStream_t)stream);
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper);
  DRAM_LAUNCH_CHECK();
  hipLaunchKernelGGL(adam_multi_dev_clip_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table, chunks,
                     (const float*)hyper, clip);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_sgd_multi_clip(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float lr,
                                   float momentum, float weight_decay, int first_step, float grad_scale,
                                   const float* clip, dram_stream_t stream) {
  if (!table || !chunks || nchunks < 1 || !clip) return DRAM_ERR_BAD_ARG;
  DramProf prof(DRAM_FAM_OPTIM, 5, 0.0, (momentum != 0.f ? 20.0 : 12.0) * (double)nchunks * 16384.0, (hipStream_t)stream);
  hipLaunchKernelGGL(sgd_multi_clip_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table, chunks, lr, momentum,
                     weight_decay, first_step, grad_scale, clip);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_version(void) { return DRAM_ABI_VERSION; }
extern "C" const char* dram_build_info(void) { return "libdram_hip gfx950 fp32-mfma"; }
#ifndef DRAM_ABI_HASH
#error "build through _build.py (it passes -DDRAM_ABI_HASH=<sha1 of include/dram_hip.h>)"
#endif
extern "C" const char* dram_abi_hash(void) { return DRAM_ABI_HASH; }

extern "C" unsigned long long dram_stream_capture_id(dram_stream_t stream) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo((hipStream_t)stream, &status, &id) != hipSuccess) return 0;
  if (status != hipStreamCaptureStatusActive) return 0;
  return id ? id : ~0ull;                            // (never 0 while capturing)
}
