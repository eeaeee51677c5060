// sample_prep.hip -- one archive case (int16 scan + lung mask, dataset.py:147-155) -> one training sample, straight from
// the int16 data: the deterministic transforms of prep.hip (IntensityWindow -> Standardize -> Interpolate, models.py:59-63)
// and em_mask = (image < -950) & (lung_mask > 0) (dataset.py:149) without a float32 copy of any full-size volume.
//
// Two kernels.  sample_stats: c = clamp(x, lo, hi) - lo is an integer in [0, hi - lo] and the windowed value of the
// reference is c / (hi - lo), so the volume statistics follow from the two INTEGER sums of c and c^2: exact, and the
// same bits whatever the block order (no atomics, every block writes its own row: no memset).  The scan is read as
// 16-byte vectors, eight int16 per lane, between a scalar head (up to the first 16-byte boundary) and a scalar tail.
// prep_sample: one gather pass over the OUTPUT grid that writes the image (the arithmetic of prep_image_kernel on
// the exactly converted taps), the lung mask and the emphysema mask (the nearest rule of prep_mask_kernel; a gather
// commutes with the voxel-wise mask logic, so this is thresholding at full size and resizing afterwards, bit for bit).
#include "common.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_VEC = 8;                       // int16 per 16-byte load
constexpr int SP_UNROLL = 4;                    // vector loads in flight per lane
constexpr long SP_MIN_PER_BLOCK = (long)SP_THREADS * SP_VEC * SP_UNROLL;
constexpr int SP_MAX_BLOCKS = 2048;             // 8 workgroups of 4 waves per CU on 256 CUs

typedef unsigned long long u64;

struct Acc {
  u64 s1, s2;
  // c <= 4095: eight of them sum below 2^15 and their squares below 2^27 -- one 32-bit pair per vector, widened once
  __device__ __forceinline__ void add_vec(const uint4 q, const int lo, const int hi) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    unsigned a = 0, b = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x0 = (int)(short)(w[k] & 0xffffu), x1 = (int)w[k] >> 16;
      const unsigned c0 = (unsigned)(min(max(x0, lo), hi) - lo), c1 = (unsigned)(min(max(x1, lo), hi) - lo);
      a += c0 + c1;
      b += c0 * c0 + c1 * c1;
    }
    s1 += a;
    s2 += b;
  }
  __device__ __forceinline__ void add_one(const int x, const int lo, const int hi) {
    const unsigned c = (unsigned)(min(max(x, lo), hi) - lo);
    s1 += c;
    s2 += c * c;
  }
};

// partial[blk] = {sum c, sum c^2} over the block's share of the vectors; block 0 adds the scalar head and tail.
// head: elements in front of the first 16-byte boundary (0..7), nvec: whole vectors behind it.
__global__ __launch_bounds__(SP_THREADS) void sample_stats_kernel(const int16_t* __restrict__ scan,
                                                                  long long* __restrict__ partial, const long n,
                                                                  const int head, const long nvec, const int lo,
                                                                  const int hi) {
  __shared__ u64 sm[2][SP_THREADS];
  Acc acc{0, 0};
  const uint4* __restrict__ v = reinterpret_cast<const uint4*>(scan + head);
  const long stride = (long)gridDim.x * SP_THREADS;
  long i = blockIdx.x * (long)SP_THREADS + threadIdx.x;
  for (; i + (SP_UNROLL - 1) * stride < nvec; i += SP_UNROLL * stride) {
    uint4 q[SP_UNROLL];
#pragma unroll
    for (int u = 0; u < SP_UNROLL; ++u) q[u] = v[i + u * stride];
#pragma unroll
    for (int u = 0; u < SP_UNROLL; ++u) acc.add_vec(q[u], lo, hi);
  }
  for (; i < nvec; i += stride) acc.add_vec(v[i], lo, hi);
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    const long tail0 = head + nvec * SP_VEC;                 // first element behind the vectors
    if (t < head) acc.add_one(scan[t], lo, hi);
    if (t >= SP_VEC && t < 2 * SP_VEC && tail0 + (t - SP_VEC) < n) acc.add_one(scan[tail0 + (t - SP_VEC)], lo, hi);
  }
  sm[0][threadIdx.x] = acc.s1;
  sm[1][threadIdx.x] = acc.s2;
  __syncthreads();
  for (int s = SP_THREADS / 2; s > 0; s >>= 1) {             // integer sums: exact in any order
    if (threadIdx.x < s) {
      sm[0][threadIdx.x] += sm[0][threadIdx.x + s];
      sm[1][threadIdx.x] += sm[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) partial[blockIdx.x * 2 + threadIdx.x] = (long long)sm[threadIdx.x][0];
}

struct PrepGeom {
  int H, W, Do, Ho, Wo;
  float sy, sx;        // bilinear, align_corners=True: (in - 1) / (out - 1), 0 for an output extent of 1
  float ny, nx;        // nearest: (float)in / out
  int lo, hi, thr;
  float span;          // (float)(hi - lo)
};

template <typename LT>
__global__ __launch_bounds__(SP_THREADS) void prep_sample_kernel(const int16_t* __restrict__ scan,
                                                                 const LT* __restrict__ lung, const int* __restrict__ zidx,
                                                                 const float* __restrict__ mean_invstd,
                                                                 float* __restrict__ out_image,
                                                                 uint8_t* __restrict__ out_lung,
                                                                 uint8_t* __restrict__ out_em, const PrepGeom g) {
  const unsigned total = (unsigned)g.Do * (unsigned)g.Ho * (unsigned)g.Wo;      // < 2^31 (checked by the caller)
  const float mean = mean_invstd[0], inv = mean_invstd[1];
  const unsigned step = gridDim.x * (unsigned)SP_THREADS;
  // (i < total < 2^31 and step <= 2^20: i + step does not wrap)
  for (unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x; i < total; i += step) {
    unsigned r = i;
    const int xo = (int)(r % (unsigned)g.Wo); r /= (unsigned)g.Wo;
    const int yo = (int)(r % (unsigned)g.Ho);
    const int zo = (int)(r / (unsigned)g.Ho);
    const long plane = (long)zidx[zo] * g.H * g.W;
    const int16_t* p = scan + plane;
    // image: the four windowed taps, mixed as prep_image_kernel mixes them
    const float fy = g.sy * (float)yo, fx = g.sx * (float)xo;
    int y0 = (int)fy, x0 = (int)fx;
    if (y0 > g.H - 1) y0 = g.H - 1;
    if (x0 > g.W - 1) x0 = g.W - 1;
    const int y1 = y0 + (y0 < g.H - 1 ? 1 : 0), x1 = x0 + (x0 < g.W - 1 ? 1 : 0);
    const float wy1 = fy - (float)y0, wx1 = fx - (float)x0;
    const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
    const int t00 = p[(long)y0 * g.W + x0], t01 = p[(long)y0 * g.W + x1];
    const int t10 = p[(long)y1 * g.W + x0], t11 = p[(long)y1 * g.W + x1];
    // (v - lo) of an in-window integer is exact in float either way: this IS window01 of the converted value
    const float w00 = (float)(min(max(t00, g.lo), g.hi) - g.lo) / g.span;
    const float w01 = (float)(min(max(t01, g.lo), g.hi) - g.lo) / g.span;
    const float w10 = (float)(min(max(t10, g.lo), g.hi) - g.lo) / g.span;
    const float w11 = (float)(min(max(t11, g.lo), g.hi) - g.lo) / g.span;
    const float v = wy0 * (wx0 * w00 + wx1 * w01) + wy1 * (wx0 * w10 + wx1 * w11);
    out_image[i] = (v - mean) * inv;
    // masks: the nearest source voxel
    const long nn = plane + (long)nearest_src(yo, g.ny, g.H) * g.W + nearest_src(xo, g.nx, g.W);
    const bool in_lung = lung[nn] > 0;
    out_lung[i] = in_lung ? 1 : 0;
    out_em[i] = (in_lung && (int)scan[nn] < g.thr) ? 1 : 0;
  }
}

inline bool span_ok(int lo, int hi) {
  return hi > lo && (long long)hi - lo <= 4095 && lo >= -65536 && hi <= 65536;
}

}  // namespace

extern "C" int dram_sample_stats_nblk(long long n) {
  long long b = (n + SP_MIN_PER_BLOCK - 1) / SP_MIN_PER_BLOCK;
  return (int)(b > SP_MAX_BLOCKS ? SP_MAX_BLOCKS : (b < 1 ? 1 : b));
}

extern "C" int dram_sample_stats_i16(const int16_t* scan, long long* partial, long long n, int lo, int hi,
                                     dram_stream_t stream) {
  if (!scan || !partial || n < 2 || !span_ok(lo, hi) || ((uintptr_t)scan & 1)) return DRAM_ERR_BAD_ARG;
  if (n >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  long long head = (long long)(((16 - ((uintptr_t)scan & 15)) & 15) / 2);
  if (head > n) head = n;
  const long long nvec = (n - head) / SP_VEC;
  DramProf prof(DRAM_FAM_PREP, 10, 0.0, 2.0 * (double)n, (hipStream_t)stream);
  hipLaunchKernelGGL(sample_stats_kernel, dim3(dram_sample_stats_nblk(n)), dim3(SP_THREADS), 0, (hipStream_t)stream,
                     scan, partial, (long)n, (int)head, (long)nvec, lo, hi);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_prep_sample_i16(const int16_t* scan, const void* lung, int lung_dtype, const int* zidx,
                                    const float* mean_invstd, float* out_image, uint8_t* out_lung, uint8_t* out_em,
                                    int D, int H, int W, int Do, int Ho, int Wo, int lo, int hi, int em_threshold,
                                    dram_stream_t stream) {
  if (!scan || !lung || !zidx || !mean_invstd || !out_image || !out_lung || !out_em || D < 1 || H < 1 || W < 1 ||
      Do < 1 || Ho < 1 || Wo < 1 || !span_ok(lo, hi) || (lung_dtype != 1 && lung_dtype != 2))
    return DRAM_ERR_BAD_ARG;
  const long long total = (long long)Do * Ho * Wo;
  if ((long long)D * H * W >= (1LL << 31) || total >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  PrepGeom g;
  g.H = H; g.W = W; g.Do = Do; g.Ho = Ho; g.Wo = Wo;
  g.sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
  g.sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
  g.ny = (float)H / (float)Ho;
  g.nx = (float)W / (float)Wo;
  g.lo = lo; g.hi = hi; g.thr = em_threshold;
  g.span = (float)(hi - lo);
  long long nb = (total + SP_THREADS - 1) / SP_THREADS;
  if (nb > 4096) nb = 4096;
  // read: the Do selected planes of the scan (2 B) and of the mask, written: 4 + 1 + 1 B per output voxel
  DramProf prof(DRAM_FAM_PREP, 11, 0.0, (double)Do * H * W * (2.0 + lung_dtype) + 6.0 * (double)total, (hipStream_t)stream);
  if (lung_dtype == 1)
    hipLaunchKernelGGL(prep_sample_kernel<uint8_t>, dim3((unsigned)nb), dim3(SP_THREADS), 0, (hipStream_t)stream, scan,
                       (const uint8_t*)lung, zidx, mean_invstd, out_image, out_lung, out_em, g);
  else
    hipLaunchKernelGGL(prep_sample_kernel<int16_t>, dim3((unsigned)nb), dim3(SP_THREADS), 0, (hipStream_t)stream, scan,
                       (const int16_t*)lung, zidx, mean_invstd, out_image, out_lung, out_em, g);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
