// densito.hip -- the per-lobe CT histogram behind the densitometry of the predict report (LAA-950 / -910, Perc15, mean
// lung density, lobe volume): ONE pass over the int16 crop of the scan and the lobe labels (3-4 B per voxel) gives
//   hist[r][bin]  voxels of row r per 1-HU bin, bin = clamp(hu, hu_lo, hu_lo + nbins - 1) - hu_lo
//   sums[r]       { voxel count, sum of the raw HU values }
// for the rows r = 0 .. n_regions (label r -> row r, label > n_regions -> row 0, label <= 0 -> nowhere).
//
// Design.  Lung HU values pile into ~200 bins of one or two rows at a time, so the counters are LDS integers
// (ds_add_u32, no return value) and the question is what a wave does when its lanes meet on one counter.  Figures:
// DESIGN.md section 4h (a 350 x 300 x 400 crop, 38 % lung, single launches between device events).
//   * ONE counter image per workgroup, 32-bit counters: rows * nbins * 4 B, instantiated at 8192 / 16384 / 32768
//     counters = 32 / 64 / 128 KiB of the CU's 160 KiB, + 4.1 KiB for the fold of the sums below: 36 992 / 69 760 /
//     135 296 B per workgroup.  The library default (6 rows x 1024 bins = 6144 counters) takes the 32 KiB form, 16 rows
//     x 2048 bins the 128 KiB one.  32-bit counters cannot overflow: a workgroup sees fewer than 2^31 voxels, also
//     when every one of them has one label and one value.
//   * Wave-private copies (wave w counts in copy w mod 2 or mod 4, which the 160 KiB would pay for) were measured and
//     NOT taken: the same time within 3 %.  An LDS atomic is executed by the CU's LDS unit one wave-instruction at a
//     time; lanes of one instruction that meet on a counter are serialised there whichever copy they address, and
//     instructions of different waves never overlap anyway.  With all adds removed the pass is only 8-9 us of 46
//     shorter: the counters are not what it waits for.
//   * Run-length inside the thread: a thread owns 8 x-consecutive voxels (one 16-byte image load); consecutive voxels
//     with the same (row, bin) are merged into one add of their count, and a group without a lung voxel issues none.
//     The label is constant over long x-runs, so this removes adds without cross-lane traffic; in the worst case
//     (every voxel equal) a thread issues ONE add per 8 voxels.
//   * Match-and-count across the wave (a ballot loop per distinct key) was not built: with ~200 live bins a wave of
//     64 keys holds tens of distinct ones, and the adds cost too little (above) to pay for the loop.
//   * The sums come from the counters, not from a second set of contended adds: at the end a workgroup has
//     count_r = sum_bin c[r][bin] and sum_r = sum_bin c[r][bin] * (hu_lo + bin) + excess_r, where excess_r collects
//     hu - clamp(hu) of the voxels in the two tails only (a 64-bit LDS add, rare in a lung).  All of it is exact
//     integer arithmetic.
//   * No division in the loop: (z, y, x) of a thread's group is divided once and advanced by the stride's own
//     (dz, dy, dx) with carries, as upproject_regions_kernel does (two 32-bit divisions per group, and counting the
//     groups that hold no lung voxel, cost 15 % of the pass).
//     Two groups in flight per thread, and the next group's loads issued before the present one is counted, were
//     measured and gave nothing (the first was slower): 16 waves per CU already cover the latency.
// Launch: 1024 threads per workgroup, ceil(voxels / 8192) workgroups capped at 256 = one per CU; every thread strides
// over groups of 8 voxels.  The cap bounds the scratch (256 x 24 KiB at the defaults, written once and read once):
// 512 workgroups were 5 % slower in the pass and 50 % in the fold, 1024 slower still.  Each workgroup writes ALL of its
// partial rows; a second launch folds them in index order (64 columns x 16 slices of consecutive workgroups per block,
// as region_fold_kernel).  No global atomics, no ticket word, no memset, never synchronises; integer sums, so
// bit-identical from call to call.
//
// Loads: the image group is one 16-byte load when the image base is 16-byte aligned (group g starts at voxel 8 g) and
// the group lies inside the volume; the labels of a group that lies inside one x-row are one 8- / 16-byte load of
// whatever alignment the view gives them (rows of a crop start anywhere); a group that crosses a row end -- W no
// multiple of 8 -- or the end of the volume takes the labels, and at the end of the volume the image, voxel by voxel.
#include "common.h"

namespace {

constexpr int TPB = 1024;        // threads per workgroup
constexpr int VPT = 8;           // voxels per thread and step: 16 B of the image
constexpr int MAX_WG = 256;     // one workgroup per CU
constexpr int MAX_ROWS = 16;

struct __attribute__((packed, aligned(1))) lab8_u8 { uint8_t v[VPT]; };
struct __attribute__((packed, aligned(2))) lab8_i16 { int16_t v[VPT]; };
template <typename LT> struct LabVec;
template <> struct LabVec<uint8_t> { typedef lab8_u8 type; };
template <> struct LabVec<int16_t> { typedef lab8_i16 type; };

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The 8 voxels v0 .. v0 + 7 of a group that starts at (z, y, x0): HU values and labels; a voxel past the end of the
// volume gets label 0.  Returns whether any of them is lung (label > 0).
template <typename LT>
__device__ __forceinline__ bool load_group(const int16_t* __restrict__ img, const LT* __restrict__ lab, long sz, long sy,
                                           int H, int W, unsigned total, int img_vec, unsigned v0, int z, int y, int x0,
                                           int (&hu)[VPT], int (&lb)[VPT]) {
  const bool full = v0 + VPT <= total;
  if (full && img_vec) {
    const int4 q = *reinterpret_cast<const int4*>(img + v0);
    const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      hu[2 * j] = (int)(short)(w[j] & 0xffff);
      hu[2 * j + 1] = w[j] >> 16;
    }
  } else {
#pragma unroll
    for (int j = 0; j < VPT; ++j) hu[j] = v0 + j < total ? (int)img[v0 + j] : 0;
  }
  if (full && x0 + VPT <= W) {
    const typename LabVec<LT>::type q = *reinterpret_cast<const typename LabVec<LT>::type*>(lab + z * sz + y * sy + x0);
#pragma unroll
    for (int j = 0; j < VPT; ++j) lb[j] = (int)q.v[j];
  } else {                                                    // walk over the row ends (W may be below 8)
    int zz = z, yy = y, xx = x0;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      lb[j] = v0 + j < total ? (int)lab[zz * sz + yy * sy + xx] : 0;
      if (++xx == W) {
        xx = 0;
        if (++yy == H) { yy = 0; ++zz; }
      }
    }
  }
  bool any = false;
#pragma unroll
  for (int j = 0; j < VPT; ++j) any |= lb[j] > 0;
  return any;
}

// key = row * nbins + bin, -1 for a voxel that is counted nowhere; equal x-neighbours become one add of their count
__device__ __forceinline__ void count_group(const int (&hu)[VPT], const int (&lb)[VPT], unsigned* cnt,
                                            unsigned long long* excess, int n_regions, int hu_lo, int hu_hi, int nbins) {
  int prev = -1;
  unsigned run = 0;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int row = lb[j] <= 0 ? -1 : (lb[j] > n_regions ? 0 : lb[j]);
    const int c = min(max(hu[j], hu_lo), hu_hi);
    const int key = row < 0 ? -1 : row * nbins + (c - hu_lo);
    if (row >= 0 && c != hu[j]) atomicAdd(&excess[row], (unsigned long long)(long long)(hu[j] - c));
    if (key == prev) {
      ++run;
    } else {
      if (prev >= 0) atomicAdd(&cnt[prev], run);
      prev = key;
      run = 1;
    }
  }
  if (prev >= 0) atomicAdd(&cnt[prev], run);
}

// NC: counters the LDS image is declared with (>= (n_regions + 1) * nbins).  total < 2^31, so 8 * group + 7 fits 32 bits.
template <typename LT, int NC>
__global__ __launch_bounds__(TPB) void lobe_hist_kernel(const int16_t* __restrict__ img, const LT* __restrict__ lab,
                                                        long sz, long sy, int H, int W, unsigned total, int n_regions,
                                                        int hu_lo, int nbins, int img_vec,
                                                        unsigned* __restrict__ part_hist,
                                                        long long* __restrict__ part_sums) {
  __shared__ unsigned cnt[NC];
  __shared__ unsigned long long excess[MAX_ROWS];
  __shared__ long long red[TPB / 64][MAX_ROWS][2];
  const int used = (n_regions + 1) * nbins;
  for (int i = threadIdx.x; i < used; i += TPB) cnt[i] = 0u;
  if (threadIdx.x < MAX_ROWS) excess[threadIdx.x] = 0ull;
  __syncthreads();

  const unsigned ngroups = (total + (VPT - 1)) / VPT;
  const unsigned stride = gridDim.x * (unsigned)TPB;
  const int hu_hi = hu_lo + nbins - 1;
  // (z, y, x0) of the group's first voxel: divided once, then advanced by the stride's own (dz, dy, dx) with carries
  const unsigned dv = stride * VPT;
  const int dx = (int)(dv % (unsigned)W), dy = (int)(dv / (unsigned)W % (unsigned)H), dz = (int)(dv / (unsigned)W / (unsigned)H);
  unsigned g = blockIdx.x * (unsigned)TPB + threadIdx.x;
  int x0 = (int)(g * VPT % (unsigned)W), y = (int)(g * VPT / (unsigned)W % (unsigned)H), z = (int)(g * VPT / (unsigned)W / (unsigned)H);
  for (; g < ngroups; g += stride) {
    int hu[VPT], lb[VPT];
    if (load_group<LT>(img, lab, sz, sy, H, W, total, img_vec, g * VPT, z, y, x0, hu, lb))
      count_group(hu, lb, cnt, excess, n_regions, hu_lo, hu_hi, nbins);
    x0 += dx;
    const int cx = x0 >= W ? 1 : 0;
    x0 -= cx ? W : 0;
    y += dy + cx;
    const int cy = y >= H ? 1 : 0;
    y -= cy ? H : 0;
    z += dz + cy;
  }
  __syncthreads();

  // all rows of this workgroup's partial image, and count / sum of each row from its counters
  unsigned* ph = part_hist + (long)blockIdx.x * used;
  const int wave = threadIdx.x >> 6;
  for (int row = 0; row <= n_regions; ++row) {
    long long c = 0, s = 0;
    for (int b = threadIdx.x; b < nbins; b += TPB) {
      const unsigned k = cnt[row * nbins + b];
      ph[row * nbins + b] = k;
      c += (long long)k;
      s += (long long)k * (long long)(hu_lo + b);
    }
    c = wave_sum_ll(c);
    s = wave_sum_ll(s);
    if ((threadIdx.x & 63) == 0) { red[wave][row][0] = c; red[wave][row][1] = s; }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * (n_regions + 1)) {
    const int row = threadIdx.x >> 1, col = threadIdx.x & 1;
    long long a = col ? (long long)excess[row] : 0ll;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) a += red[w][row][col];
    part_sums[(long)blockIdx.x * 2 * (n_regions + 1) + threadIdx.x] = a;
  }
}

// hist[col] = sum_k part_hist[k][col], sums[col] = sum_k part_sums[k][col]: 16 slices of consecutive k, each summed in
// index order, then the slices in order.  block (64, 16); blocks 0 .. used / 64 - 1 fold 64 histogram columns each
// (used is a multiple of 64), the last block the 2 * rows columns of the sums.
__global__ __launch_bounds__(1024) void lobe_hist_fold_kernel(const unsigned* __restrict__ part_hist,
                                                              const long long* __restrict__ part_sums,
                                                              long long* __restrict__ hist, long long* __restrict__ sums,
                                                              int nblk, int used, int scols) {
  __shared__ long long sm[16][64];
  const int c = threadIdx.x, g = threadIdx.y;
  const int per = (nblk + 15) / 16;
  const int k0 = g * per, k1 = min(nblk, k0 + per);
  const bool is_sums = (int)blockIdx.x == used / 64;
  const int col = is_sums ? c : (int)blockIdx.x * 64 + c;
  const bool live = is_sums ? c < scols : true;
  long long s = 0;
  if (live) {
    if (is_sums) {
      for (int k = k0; k < k1; ++k) s += part_sums[(long)k * scols + col];
    } else {
#pragma unroll 8
      for (int k = k0; k < k1; ++k) s += (long long)part_hist[(long)k * used + col];
    }
  }
  sm[g][c] = s;
  __syncthreads();
  if (g == 0 && live) {
    long long t = sm[0][c];
#pragma unroll
    for (int j = 1; j < 16; ++j) t += sm[j][c];
    (is_sums ? sums : hist)[col] = t;
  }
}

template <typename LT>
void launch_hist(int used, dim3 grid, hipStream_t s, const int16_t* img, const void* lab, long sz, long sy, int H, int W,
                 unsigned total, int n, int hu_lo, int nbins, int img_vec, unsigned* ph, long long* ps) {
  const LT* l = (const LT*)lab;
  if (used <= 8192)
    hipLaunchKernelGGL((lobe_hist_kernel<LT, 8192>), grid, dim3(TPB), 0, s, img, l, sz, sy, H, W, total, n, hu_lo, nbins,
                       img_vec, ph, ps);
  else if (used <= 16384)
    hipLaunchKernelGGL((lobe_hist_kernel<LT, 16384>), grid, dim3(TPB), 0, s, img, l, sz, sy, H, W, total, n, hu_lo, nbins,
                       img_vec, ph, ps);
  else
    hipLaunchKernelGGL((lobe_hist_kernel<LT, 32768>), grid, dim3(TPB), 0, s, img, l, sz, sy, H, W, total, n, hu_lo, nbins,
                       img_vec, ph, ps);
}

}  // namespace

extern "C" int dram_lobe_hist_nblk(long long voxels) {
  long long b = (voxels + (long long)TPB * VPT - 1) / ((long long)TPB * VPT);
  return (int)(b > MAX_WG ? MAX_WG : (b < 1 ? 1 : b));
}

extern "C" int dram_lobe_hist(const void* image, const void* labels, int label_dtype, long long stride_z,
                              long long stride_y, int* part_hist, int64_t* part_sums, int64_t* hist, int64_t* sums, int D,
                              int H, int W, int n_regions, int hu_lo, int nbins, dram_stream_t stream) {
  if (!image || !labels || !part_hist || !part_sums || !hist || !sums || (label_dtype != 1 && label_dtype != 2) || D < 1 ||
      H < 1 || W < 1 || stride_z < 0 || stride_y < 0 || n_regions < 1 || n_regions > 15)
    return DRAM_ERR_BAD_ARG;
  const long long total = (long long)D * H * W;
  const int rows = n_regions + 1;
  if (total >= (1LL << 31) || nbins < 64 || nbins > 2048 || nbins % 64 || rows * nbins > 32768 || hu_lo < -32768 ||
      hu_lo + nbins - 1 > 32767)
    return DRAM_ERR_UNSUPPORTED;
  const int nblk = dram_lobe_hist_nblk(total), used = rows * nbins;
  const double scratch = (double)nblk * (4.0 * used + 16.0 * rows);
  hipStream_t s = (hipStream_t)stream;
  {
    DramProf prof(DRAM_FAM_PREP, 11, 0.0, (double)total * (2.0 + label_dtype) + scratch, s);
    const int img_vec = ((uintptr_t)image & 15) == 0 ? 1 : 0;
    with_label_type(label_dtype, [&](auto t) {
      launch_hist<decltype(t)>(used, dim3(nblk), s, (const int16_t*)image, labels, (long)stride_z, (long)stride_y, H, W,
                               (unsigned)total, n_regions, hu_lo, nbins, img_vec, (unsigned*)part_hist,
                               (long long*)part_sums);
    });
    DRAM_LAUNCH_CHECK();
  }
  DramProf prof(DRAM_FAM_PREP, 12, 0.0, scratch + 8.0 * used + 16.0 * rows, s);
  hipLaunchKernelGGL(lobe_hist_fold_kernel, dim3(used / 64 + 1), dim3(64, 16), 0, s, (const unsigned*)part_hist,
                     (const long long*)part_sums, (long long*)hist, (long long*)sums, nblk, used, 2 * rows);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
