// case_prep.hip -- scan + lobe segmentation -> prepared predict case, the reference's SubtypingInference.get_data
// (dataset.py:57-92) with utils.find_crops (utils.py:53-63):
//   lung = lobe > 0;  dlung = binary_dilation(lung, 3x3x3 full structure, iterations=r);  scan[dlung == 0] = fill;
//   crop of scan / original scan / lung to the padded bounding box of the lung;  ess = (scan < threshold) & lung.
// r iterations of the 26-connected structure with zero border are ONE (2r+1)^3 box dilation clipped to the volume, and
// every lung voxel lies inside the crop box, so voxels outside the crop (or the volume) count as 0: no halo from
// outside the crop is read.
//
// Two kernels.  lung_bbox: one 16-byte-vector pass over the lobes, per-workgroup partial rows {min/max z, y, x, count}
// and a fixed-order fold launch (no atomics, so no memset per call).  case_prepare: the WAVE-BALLOT form -- a 64-voxel
// x-run of the lung is one 64-bit __ballot mask.  A workgroup owns a TZ x TY x (NR * 64) tile of the crop: it ballots the
// lobes of the tile + halo into LDS masks (phase 1), dilates along x by shifts (edge bits from the neighbouring runs)
// and ORs 2r+1 rows (phase 2), and ORs 2r+1 planes while it streams the scan through (phase 3): lane i of a wave
// takes bit i of a mask word that all 64 lanes read from one LDS address (a broadcast).  The dilated volume exists only
// as those masks; the halo re-reads of the 1-byte lobes (neighbouring tiles) are L2 hits.  Outputs leave as coalesced
// vector stores, one x-run per wave instruction.
#include <limits.h>
#include "common.h"

namespace {

constexpr int CP_TZ = 8, CP_TY = 8, CP_NR = 4, CP_RMAX = 3;     // tile: 8 planes x 8 rows x 256 voxels
constexpr int CP_NRH = CP_NR + 2;             // runs of a tile row + one halo run on either side

typedef unsigned long long u64;

// element k of a 16-byte vector held as four words, as "is lung" (lobe > 0: the reference's test, signed for int16)
template <typename LT> __device__ __forceinline__ bool lobe_set(const unsigned (&w)[4], int k);
template <> __device__ __forceinline__ bool lobe_set<uint8_t>(const unsigned (&w)[4], int k) {
  return ((w[k >> 2] >> (8 * (k & 3))) & 0xffu) != 0u;
}
template <> __device__ __forceinline__ bool lobe_set<int16_t>(const unsigned (&w)[4], int k) {
  return (int16_t)(w[k >> 1] >> (16 * (k & 1))) > 0;
}

struct Box {
  int v[7];   // min z, max z, min y, max y, min x, max x (inclusive), count
  __device__ __forceinline__ void init() {
    v[0] = v[2] = v[4] = INT_MAX;
    v[1] = v[3] = v[5] = -1;
    v[6] = 0;
  }
  __device__ __forceinline__ void add(unsigned row, int xa, int xb, unsigned H) {
    const int z = (int)(row / H), y = (int)(row - (unsigned)z * H);
    v[0] = min(v[0], z); v[1] = max(v[1], z);
    v[2] = min(v[2], y); v[3] = max(v[3], y);
    v[4] = min(v[4], xa); v[5] = max(v[5], xb);
  }
  __device__ __forceinline__ void merge(const int* o) {
    v[0] = min(v[0], o[0]); v[1] = max(v[1], o[1]);
    v[2] = min(v[2], o[2]); v[3] = max(v[3], o[3]);
    v[4] = min(v[4], o[4]); v[5] = max(v[5], o[5]);
    v[6] += o[6];
  }
};

// workgroup fold of the 256 threads' boxes; the result is valid in thread 0.  min / max / integer sum: exact in any
// order, the order is fixed anyway.
__device__ __forceinline__ void block_fold(Box& b, int (*sm)[8]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    int t[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) t[k] = __shfl_xor(b.v[k], o, 64);
    b.merge(t);
  }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 7; ++k) sm[threadIdx.x >> 6][k] = b.v[k];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w) b.merge(sm[w]);
}

template <typename LT>
__global__ __launch_bounds__(256) void lung_bbox_kernel(const LT* __restrict__ lobes, int* __restrict__ partial,
                                                        const long n, const unsigned H, const unsigned W) {
  constexpr int N = 16 / (int)sizeof(LT);
  __shared__ int sm[4][8];
  Box b;
  b.init();
  const long nvec = n / N;
  const uint4* __restrict__ lv = reinterpret_cast<const uint4*>(lobes);
  for (long v = blockIdx.x * 256L + threadIdx.x; v < nvec; v += (long)gridDim.x * 256L) {
    const uint4 q = lv[v];
    if (!(q.x | q.y | q.z | q.w)) continue;
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) m |= (lobe_set<LT>(w, k) ? 1u : 0u) << k;
    if (!m) continue;
    b.v[6] += __popc(m);
    const unsigned i0 = (unsigned)(v * N), row = i0 / W, x = i0 - row * W;
    const int first = __ffs(m) - 1, last = 31 - __clz(m);
    if (x + (unsigned)last < W) {            // every set element lies in this row
      b.add(row, (int)x + first, (int)x + last, H);
    } else {                                 // the vector straddles rows: one element at a time
      for (unsigned mm = m; mm; mm &= mm - 1) {
        const unsigned i = i0 + (unsigned)(__ffs(mm) - 1), r = i / W, xx = i - r * W;
        b.add(r, (int)xx, (int)xx, H);
      }
    }
  }
  if (blockIdx.x == 0 && nvec * N + threadIdx.x < n) {     // the last n % N elements
    const long i = nvec * N + threadIdx.x;
    if (lobes[i] > 0) {
      const unsigned r = (unsigned)i / W, xx = (unsigned)i - r * W;
      b.v[6] += 1;
      b.add(r, (int)xx, (int)xx, H);
    }
  }
  block_fold(b, sm);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) partial[blockIdx.x * 8 + k] = b.v[k];
    partial[blockIdx.x * 8 + 7] = 0;
  }
}

// box = {z0, z1, y0, y1, x0, x1, count, 0}, half-open; zeros for an empty lung
__global__ __launch_bounds__(256) void lung_bbox_fold_kernel(const int* __restrict__ partial, int* __restrict__ box,
                                                             const int nblk) {
  __shared__ int sm[4][8];
  Box b;
  b.init();
  for (int r = threadIdx.x; r < nblk; r += 256) b.merge(partial + r * 8);
  block_fold(b, sm);
  if (threadIdx.x == 0) {
    const bool any = b.v[6] > 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      box[2 * a] = any ? b.v[2 * a] : 0;
      box[2 * a + 1] = any ? b.v[2 * a + 1] + 1 : 0;
    }
    box[6] = b.v[6];
    box[7] = 0;
  }
}

struct CaseGeom {
  int H, W;            // volume rows / row length
  int z0, y0, x0;      // crop offset
  int Dc, Hc, Wc;      // crop size
  int nby, nbx;        // tiles along y, x
  int fill, thr;
};

// R = dilation radius: compile-time, so the (plane, row, run) decode of an item index is multiplies and shifts
template <typename LT, int R>
__global__ __launch_bounds__(256) void case_prepare_kernel(const int16_t* __restrict__ scan, const LT* __restrict__ lobes,
                                                           int16_t* __restrict__ image, uint8_t* __restrict__ lung_mask,
                                                           uint8_t* __restrict__ ess_mask, int16_t* __restrict__ original,
                                                           const CaseGeom g) {
  constexpr int PZ = CP_TZ + 2 * R, PY = CP_TY + 2 * R;
  constexpr int N1 = PZ * PY * CP_NRH;         // phase-1 items: one ballot each
  constexpr int U = 8;                         // loads in flight per wave (phases 1 and 3): the kernel is latency-bound
  __shared__ u64 raw[PZ][PY][CP_NRH];          // lung masks of tile + halo; run index shifted by one (halo run first)
  __shared__ u64 xy[PZ][CP_TY][CP_NR];         // x- and y-dilated masks of the tile's rows, every needed plane
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int t = blockIdx.x;
  const int bx = (t % g.nbx) * (CP_NR * 64); t /= g.nbx;
  const int by = (t % g.nby) * CP_TY;
  const int bz = (t / g.nby) * CP_TZ;

  // phase 1: one ballot per (plane, row, run) of tile + halo, U loads issued before the first is used.  Outside the
  // crop box counts as 0 and is not read; of the two halo runs only the R voxels next to the tile are.
  for (int base = wave * U; base < N1; base += 4 * U) {
    LT val[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int it = base + u;
      const int run = it % CP_NRH - 1, q = it / CP_NRH, py = q % PY, pz = q / PY;
      const int z = bz + pz - R, y = by + py - R, x = bx + run * 64 + lane;
      const bool need = (run >= 0 && run < CP_NR) || (run < 0 && lane >= 64 - R) || (run == CP_NR && lane < R);
      val[u] = 0;
      if (it < N1 && need && z >= 0 && z < g.Dc && y >= 0 && y < g.Hc && x >= 0 && x < g.Wc)
        val[u] = lobes[((long)(g.z0 + z) * g.H + (g.y0 + y)) * g.W + (g.x0 + x)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const u64 m = __ballot(val[u] > 0);
      if (base + u < N1 && lane == 0) (&raw[0][0][0])[base + u] = m;      // raw is [pz][py][run + 1] = item order
    }
  }
  __syncthreads();

  // phase 2: x dilation by shifts + the edge bits of the neighbouring runs, OR over 2R+1 rows
  for (int it = threadIdx.x; it < PZ * CP_TY * CP_NR; it += 256) {
    const int run = it % CP_NR, q = it / CP_NR, ty = q % CP_TY, pz = q / CP_TY;
    u64 acc = 0;
#pragma unroll
    for (int dy = 0; dy <= 2 * R; ++dy) {
      const u64* row = raw[pz][ty + dy];
      const u64 L = row[run], m = row[run + 1], Rt = row[run + 2];
      u64 d = m;
#pragma unroll
      for (int s = 1; s <= R; ++s) d |= (m << s) | (m >> s) | (L >> (64 - s)) | (Rt << (64 - s));
      acc |= d;
    }
    xy[pz][ty][run] = acc;
  }
  __syncthreads();

  // phase 3: OR over 2R+1 planes; a wave takes two rows of the tile at a time, one x-run of every output per wave
  // instruction, the U scan loads issued before the first store
  for (int rb = wave * 2; rb < CP_TZ * CP_TY; rb += 8) {
    int sv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = rb + u / CP_NR, run = u % CP_NR;
      const int z = bz + row / CP_TY, y = by + row % CP_TY, x = bx + run * 64 + lane;
      sv[u] = 0;
      if (z < g.Dc && y < g.Hc && x < g.Wc) sv[u] = scan[((long)(g.z0 + z) * g.H + (g.y0 + y)) * g.W + (g.x0 + x)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = rb + u / CP_NR, run = u % CP_NR, tz = row / CP_TY, ty = row % CP_TY;
      const int z = bz + tz, y = by + ty, x = bx + run * 64 + lane;
      u64 dil = 0;
#pragma unroll
      for (int dz = 0; dz <= 2 * R; ++dz) dil |= xy[tz + dz][ty][run];
      const u64 lm = raw[tz + R][ty + R][run + 1];
      if (z < g.Dc && y < g.Hc && x < g.Wc) {
        const int s = sv[u];
        const bool lung = (lm >> lane) & 1, dl = (dil >> lane) & 1;
        const long o = ((long)z * g.Hc + y) * g.Wc + x;
        image[o] = (int16_t)(dl ? s : g.fill);
        lung_mask[o] = lung ? 1 : 0;
        ess_mask[o] = (lung && s < g.thr) ? 1 : 0;
        if (original) original[o] = (int16_t)s;
      }
    }
  }
}

template <typename LT>
void launch_case_prepare(int radius, long long nblk, hipStream_t st, const void* scan, const void* lobes, void* image,
                         uint8_t* lung_mask, uint8_t* ess_mask, void* original, const CaseGeom& g) {
#define CP_LAUNCH(RR)                                                                                              \
  hipLaunchKernelGGL((case_prepare_kernel<LT, RR>), dim3((unsigned)nblk), dim3(256), 0, st, (const int16_t*)scan, \
                     (const LT*)lobes, (int16_t*)image, lung_mask, ess_mask, (int16_t*)original, g)
  switch (radius) {
    case 0: CP_LAUNCH(0); break;
    case 1: CP_LAUNCH(1); break;
    case 2: CP_LAUNCH(2); break;
    default: CP_LAUNCH(3); break;
  }
#undef CP_LAUNCH
}

}  // namespace

extern "C" int dram_lung_bbox_nblk(long long n) {
  long long b = (n + 16383) / 16384;
  return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

extern "C" int dram_lung_bbox(const void* lobes, int lobe_dtype, int* partial, int* box, int D, int H, int W,
                              dram_stream_t stream) {
  if (!lobes || !partial || !box || D < 1 || H < 1 || W < 1 || (lobe_dtype != 1 && lobe_dtype != 2) ||
      ((uintptr_t)lobes & 15))
    return DRAM_ERR_BAD_ARG;
  const long long n = (long long)D * H * W;
  if (n >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  const int nblk = dram_lung_bbox_nblk(n);
  {
    DramProf prof(DRAM_FAM_PREP, 7, 0.0, (double)n * lobe_dtype, (hipStream_t)stream);
    if (lobe_dtype == 1)
      hipLaunchKernelGGL(lung_bbox_kernel<uint8_t>, dim3(nblk), dim3(256), 0, (hipStream_t)stream,
                         (const uint8_t*)lobes, partial, (long)n, (unsigned)H, (unsigned)W);
    else
      hipLaunchKernelGGL(lung_bbox_kernel<int16_t>, dim3(nblk), dim3(256), 0, (hipStream_t)stream,
                         (const int16_t*)lobes, partial, (long)n, (unsigned)H, (unsigned)W);
    DRAM_LAUNCH_CHECK();
  }
  DramProf prof(DRAM_FAM_PREP, 8, 0.0, 32.0 * nblk, (hipStream_t)stream);
  hipLaunchKernelGGL(lung_bbox_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, box, nblk);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_case_prepare(const void* scan, const void* lobes, int lobe_dtype, void* image, uint8_t* lung_mask,
                                 uint8_t* ess_mask, void* original, int D, int H, int W, int z0, int y0, int x0, int Dc,
                                 int Hc, int Wc, int radius, int fill_value, int threshold, dram_stream_t stream) {
  if (!scan || !lobes || !image || !lung_mask || !ess_mask || D < 1 || H < 1 || W < 1 ||
      (lobe_dtype != 1 && lobe_dtype != 2) || radius < 0 || radius > CP_RMAX || fill_value < -32768 ||
      fill_value > 32767 || threshold < -32768 || threshold > 32767)
    return DRAM_ERR_BAD_ARG;
  if (z0 < 0 || y0 < 0 || x0 < 0 || Dc < 1 || Hc < 1 || Wc < 1 || Dc > D - z0 || Hc > H - y0 || Wc > W - x0)
    return DRAM_ERR_BAD_ARG;
  if ((long long)D * H * W >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  CaseGeom g;
  g.H = H; g.W = W;
  g.z0 = z0; g.y0 = y0; g.x0 = x0;
  g.Dc = Dc; g.Hc = Hc; g.Wc = Wc;
  g.nbx = cdiv(Wc, CP_NR * 64);
  g.nby = cdiv(Hc, CP_TY);
  g.fill = fill_value;
  g.thr = threshold;
  const long long nblk = (long long)g.nbx * g.nby * cdiv(Dc, CP_TZ);     // < 2^31: no more tiles than voxels
  const double vox = (double)Dc * Hc * Wc;
  DramProf prof(DRAM_FAM_PREP, 9, 0.0, vox * (2 + lobe_dtype + 2 + 1 + 1 + (original ? 2 : 0)), (hipStream_t)stream);
  if (lobe_dtype == 1)
    launch_case_prepare<uint8_t>(radius, nblk, (hipStream_t)stream, scan, lobes, image, lung_mask, ess_mask, original, g);
  else
    launch_case_prepare<int16_t>(radius, nblk, (hipStream_t)stream, scan, lobes, image, lung_mask, ess_mask, original, g);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
