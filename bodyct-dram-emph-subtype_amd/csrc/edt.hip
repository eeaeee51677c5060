// edt.hip -- the exact 3-D Euclidean distance transform of the lung mask behind the core / peel split of the per-lobe
// report: per lung voxel the squared distance d2 (an integer, in um^2) to the centre of the nearest background voxel of
// the volume at the scan's own anisotropic spacing, and from it
//   zones        0 not lung, 1 peel (d2 <= peel_um^2), 2 core (everything else, +inf included)
//   zone_labels  label r in 1..n -> r + n * (zone - 1), a lung label above n -> 255, not lung -> 0
//   dist_mm      float32(sqrt(double(d2)) / 1000.0), 0 outside the lung, +inf where d2 is
// Background is every voxel of the volume whose label is <= 0; nothing outside the volume is background.
//
// Design.  Three separable passes, x then y then z, all in integers (no result depends on evaluation order):
//   * x: ONE wave per x-row, two sweeps over chunks of 64 voxels.  A chunk's background is one ballot; a lane's nearest
//     background to the left (right) inside the chunk is a clz (ctz) on the ballot's low (high) part, the nearest one
//     outside the chunk is a wave-uniform carry from the chunks swept before.  The forward sweep stores the left
//     distance, the backward sweep reads it back (the same lane wrote it) and stores min(left, right).  2 W / 64
//     iterations per row whatever the row holds.
//   * y, z: min-plus along a strided line, one thread per voxel with x fastest, so that the 64 lanes of a wave read 64
//     consecutive elements of line element j at every step (coalesced; the +-k neighbours of a wave's voxels are the
//     lines the neighbouring waves read, so they come from L2).  best = f[i]; for k = 1 .. K: candidates f[i - k] and
//     f[i + k] cost (s k)^2 more, so the loop ends as soon as (s k)^2 >= best -- exact, because every later candidate
//     is at least that large -- and at the latest at K = min(n - 1, floor(max_um / s)), both known at launch.  A
//     background voxel ends at k = 1, a voxel next to the pleura after a few steps; only voxels whose distance exceeds
//     max_um walk the whole window.
//   * The cap.  With a finite max_um every pass stores +inf for a value above max_um^2.  A background voxel within
//     max_um of a voxel is within floor(max_um / s_a) voxels of it on every axis, so it is inside every window and the
//     partial minimum on the way to it is at most the final one: what is stored is exact or +inf.
//   * Element type of the two work volumes: uint32 when max_um <= 65535 (max_um^2 < 2^32 - 1 = +inf; sums are formed in
//     64 bits before they are compared), else uint64 ((n_a - 1) s_a < 2^25 on every axis keeps every d2 below 2^52).
//   * The z pass is the last one and writes the outputs instead of a third work volume; it reads the label once more
//     (through the view's strides) for zone_labels.
// Workspace: two volumes of D*H*W elements, each rounded up to 256 bytes.  x writes the first (both sweeps), y reads it
// and writes the second, z reads the second: every element that is read was written by the launch before.  No
// atomics, no ticket words, no waiting between workgroups, never synchronises; integer minima: bit-identical from call
// to call.
//
// dram_lobe_zones adds the fissural rind: per lung voxel f2, the squared distance to the nearest SITE (a voxel whose
// label is in 1..n) of another class than the voxel's own.  The answer depends on the voxel's class, so the separable
// passes carry the two nearest sites of distinct classes per element, packed as two uint64 keys (d2 << 3) | class in
// one 16-byte element:
//   * For any query class q the minimum over the classes != q at one element is one of its two kept pairs (the first
//     unless its class is q, then the second); the min-plus over a line is the minimum of those per-element answers plus
//     their costs; so reducing the union of the candidates to its two smallest with distinct classes loses nothing.
//     Exact, ties included: which of two tied classes is kept second changes no answer.
//   * x reads the sites from the labels, y is the same windowed min-plus as above on pairs, both ending at
//     (s k)^2 >= the larger kept distance; the cap argument carries over (a pair above max_um^2 is stored as +inf).
//   * The last launch does the z pass of BOTH transforms: d2 through line_min on the pleural work volume, exactly as
//     edt_z_kernel does (the x and y launches are edt_x_kernel / edt_y_kernel themselves, so zone 1 is dram_lung_zones'
//     zone 1 by construction), and f2 for the voxel's own class only, skipped where no output needs it.
// Five launches, two more work volumes of 16-byte pairs behind the pleural two; the same promises as above.
#include "common.h"

#include <cmath>
#include <limits>

namespace {

constexpr int TPB = 256;                       // 4 waves: 4 x-rows per workgroup in the x pass, 256 voxels in y / z
constexpr long long FULL_UM = 1LL << 26;       // no distance in a supported volume reaches it: sqrt(3) * 2^25 < 2^26

template <typename T> struct Inf;
template <> struct Inf<uint32_t> { static constexpr uint32_t v = 0xffffffffu; };
template <> struct Inf<uint64_t> { static constexpr uint64_t v = ~0ull; };

// x pass: a[row][x] = (sx * distance in voxels to the nearest background voxel of the row)^2 when that distance is
// within Kx voxels, else +inf; 0 for a background voxel.
template <typename LT, typename T>
__global__ __launch_bounds__(TPB) void edt_x_kernel(const LT* __restrict__ lab, long sz, long sy, int H, int W, long rows,
                                                    unsigned long long sx, long long Kx, T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;                                      // the whole wave leaves: ballots below are full waves
  const LT* l = lab + (row / H) * sz + (row % H) * sy;
  T* a = out + row * (long)W;
  const int nch = (W + 63) >> 6;
  long long last = -1;                                          // the last background x of the chunks swept so far
  for (int c = 0; c < nch; ++c) {
    const long long x = (long long)c * 64 + lane;
    const bool in = x < W;
    const bool bg = in && !(l[in ? x : 0] > 0);
    const unsigned long long m = __ballot(bg);
    const unsigned long long lo = m & (~0ull >> (63 - lane));   // background at or left of this lane
    const long long p = lo ? (long long)c * 64 + (63 - __clzll((long long)lo)) : last;
    if (in) {
      const long long d = x - p;
      const unsigned long long e = sx * (unsigned long long)d;
      a[x] = (p >= 0 && d <= Kx) ? (T)(e * e) : Inf<T>::v;
    }
    if (m) last = (long long)c * 64 + (63 - __clzll((long long)m));
  }
  long long next = -1;
  for (int c = nch - 1; c >= 0; --c) {
    const long long x = (long long)c * 64 + lane;
    const bool in = x < W;
    const bool bg = in && !(l[in ? x : 0] > 0);
    const unsigned long long m = __ballot(bg);
    const unsigned long long hi = m >> lane;                    // background at or right of this lane
    const long long q = hi ? x + (__ffsll((long long)hi) - 1) : next;
    if (in && q >= 0 && q - x <= Kx) {
      const unsigned long long e = sx * (unsigned long long)(q - x);
      const T v = (T)(e * e);
      if (v < a[x]) a[x] = v;
    }
    if (m) next = (long long)c * 64 + (__ffsll((long long)m) - 1);
  }
}

// best = min over |k| <= K of in[i + k] + (s k)^2 along the axis whose elements lie `stride` apart; +inf above cap2
template <typename T>
__device__ __forceinline__ unsigned long long line_min(const T* __restrict__ in, long v, int i, int n, long stride,
                                                       unsigned long long s, int K, unsigned long long cap2) {
  const T f0 = in[v];
  unsigned long long best = f0 == Inf<T>::v ? ~0ull : (unsigned long long)f0;
  for (int k = 1; k <= K; ++k) {
    const unsigned long long e = s * (unsigned long long)k, c = e * e;
    if (c >= best) break;
    if (i - k >= 0) {
      const T f = in[v - (long)k * stride];
      if (f != Inf<T>::v) best = min(best, (unsigned long long)f + c);
    }
    if (i + k < n) {
      const T f = in[v + (long)k * stride];
      if (f != Inf<T>::v) best = min(best, (unsigned long long)f + c);
    }
  }
  return best > cap2 ? ~0ull : best;
}

template <typename T>
__global__ __launch_bounds__(TPB) void edt_y_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W,
                                                    unsigned total, unsigned long long s, int K, unsigned long long cap2) {
  const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
  if (v >= total) return;
  const int y = (int)(v / (unsigned)W % (unsigned)H);
  const unsigned long long best = line_min<T>(in, (long)v, y, H, (long)W, s, K, cap2);
  out[v] = best == ~0ull ? Inf<T>::v : (T)best;
}

template <typename LT, typename T>
__global__ __launch_bounds__(TPB) void edt_z_kernel(const T* __restrict__ in, const LT* __restrict__ lab, long sz, long sy,
                                                    int D, int H, int W, unsigned total, unsigned long long s, int K,
                                                    unsigned long long cap2, unsigned long long peel2, int n_regions,
                                                    uint8_t* __restrict__ zones, uint8_t* __restrict__ zone_labels,
                                                    float* __restrict__ dist_mm) {
  const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
  if (v >= total) return;
  const unsigned plane = (unsigned)H * (unsigned)W;
  const int z = (int)(v / plane);
  const unsigned long long d2 = line_min<T>(in, (long)v, z, D, (long)plane, s, K, cap2);
  const int zone = d2 == 0ull ? 0 : (d2 <= peel2 ? 1 : 2);
  zones[v] = (uint8_t)zone;
  if (zone_labels) {
    const unsigned r = v - (unsigned)z * plane;
    const int lb = (int)lab[z * sz + (long)(r / (unsigned)W) * sy + (long)(r % (unsigned)W)];
    zone_labels[v] = (uint8_t)(zone == 0 ? 0 : (lb > n_regions ? 255 : lb + n_regions * (zone - 1)));
  }
  if (dist_mm)
    dist_mm[v] = d2 == ~0ull ? std::numeric_limits<float>::infinity() : (float)(sqrt((double)d2) / 1000.0);
}

long long vol_bytes(long long total, int elem) { return (total * elem + 255) / 256 * 256; }

int window(int n, long long s, long long max_um) {
  const long long k = max_um / s;
  return (int)(k < (long long)(n - 1) ? k : (long long)(n - 1));
}

template <typename LT, typename T>
int run(const void* labels, long sz, long sy, uint8_t* zones, uint8_t* zone_labels, float* dist_mm, void* workspace, int D,
        int H, int W, int sz_um, int sy_um, int sx_um, long long peel_um, long long max_um, int n_regions, hipStream_t s) {
  const long long total = (long long)D * H * W;
  const long rows = (long)D * H;
  T* a = (T*)workspace;
  T* b = (T*)((char*)workspace + vol_bytes(total, (int)sizeof(T)));
  const unsigned long long cap2 = (unsigned long long)max_um * (unsigned long long)max_um;
  const unsigned long long peel2 = (unsigned long long)peel_um * (unsigned long long)peel_um;
  const int Kx = window(W, sx_um, max_um), Ky = window(H, sy_um, max_um), Kz = window(D, sz_um, max_um);
  const unsigned vgrid = (unsigned)((total + TPB - 1) / TPB);
  const double vox = (double)total, e = (double)sizeof(T), lb = (double)sizeof(LT);
  {
    DramProf prof(DRAM_FAM_PREP, 13, 0.0, vox * (2.0 * lb + 3.0 * e), s);
    hipLaunchKernelGGL((edt_x_kernel<LT, T>), dim3((unsigned)((rows + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, s,
                       (const LT*)labels, sz, sy, H, W, rows, (unsigned long long)sx_um, (long long)Kx, a);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 14, 0.0, vox * 2.0 * e, s);
    hipLaunchKernelGGL((edt_y_kernel<T>), dim3(vgrid), dim3(TPB), 0, s, (const T*)a, b, H, W, (unsigned)total,
                       (unsigned long long)sy_um, Ky, cap2);
    DRAM_LAUNCH_CHECK();
  }
  DramProf prof(DRAM_FAM_PREP, 15, 0.0, vox * (e + 1.0 + (zone_labels ? lb + 1.0 : 0.0) + (dist_mm ? 4.0 : 0.0)), s);
  hipLaunchKernelGGL((edt_z_kernel<LT, T>), dim3(vgrid), dim3(TPB), 0, s, (const T*)b, (const LT*)labels, sz, sy, D, H, W,
                     (unsigned)total, (unsigned long long)sz_um, Kz, cap2, peel2, n_regions, zones, zone_labels, dist_mm);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

// the sizes both entry points accept; max_um is clamped to FULL_UM by the callers
int check_sizes(int D, int H, int W, int sz_um, int sy_um, int sx_um) {
  if (D < 1 || H < 1 || W < 1) return DRAM_ERR_BAD_ARG;
  if ((long long)D * H * W >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  const int n[3] = {D, H, W}, sp[3] = {sz_um, sy_um, sx_um};
  for (int i = 0; i < 3; ++i)
    if (sp[i] < 1 || sp[i] > 20000 || (long long)(n[i] - 1) * sp[i] >= (1LL << 25)) return DRAM_ERR_UNSUPPORTED;
  return DRAM_OK;
}

// ------------------------------------------------------------------------------------------------ lobe to lobe
// A kept pair: (squared distance << 3) | class, class 1..5; PAIR_INF (class bits 7) for "none".  Keys order by distance
// first, so the smaller key is the nearer site; a tie between classes goes to the lower class, which no result sees.
constexpr unsigned long long PAIR_INF = ~0ull;

// Insert candidate c into the two smallest keys with distinct classes (k1 <= k2, class(k1) != class(k2) or k2 = inf).
// Invariant: k1 is the minimum of everything inserted, k2 the minimum of everything whose class is not k1's.
// Inserting PAIR_INF changes nothing.
__device__ __forceinline__ void keep_two(unsigned long long& k1, unsigned long long& k2, unsigned long long c) {
  if (((c ^ k1) & 7ull) == 0ull) {
    k1 = min(k1, c);
  } else if (c < k1) {
    k2 = k1;                                                    // the old minimum: its class is not c's
    k1 = c;
  } else {
    k2 = min(k2, c);
  }
}

__device__ __forceinline__ void cap_two(unsigned long long& k1, unsigned long long& k2, unsigned long long cap2) {
  if ((k1 >> 3) > cap2) k1 = PAIR_INF;                          // PAIR_INF >> 3 = 2^61 - 1 is above every cap
  if ((k2 >> 3) > cap2) k2 = PAIR_INF;                          // k2 >= k1: a capped k1 takes k2 with it
}

// the squared distance of the first kept pair whose class is not cv (~0 for none)
__device__ __forceinline__ unsigned long long foreign(const ulonglong2 p, unsigned cv) {
  const unsigned long long k = ((unsigned)(p.x & 7ull) != cv) ? p.x : p.y;
  return k == PAIR_INF ? ~0ull : k >> 3;
}

// x pass: sites are read from the labels themselves (a site is a label in 1..n); out[v] = the two nearest sites of
// distinct classes within the row, within Kx voxels and the cap.
template <typename LT>
__global__ __launch_bounds__(TPB) void lobe_x_kernel(const LT* __restrict__ lab, long sz, long sy, int H, int W,
                                                     unsigned total, unsigned long long s, int K, unsigned long long cap2,
                                                     int n_regions, ulonglong2* __restrict__ out) {
  const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
  if (v >= total) return;
  const unsigned row = v / (unsigned)W;
  const int x = (int)(v - row * (unsigned)W);
  const LT* l = lab + (long)(row / (unsigned)H) * sz + (long)(row % (unsigned)H) * sy;
  const int own = (int)l[x];
  unsigned long long k1 = (own > 0 && own <= n_regions) ? (unsigned long long)own : PAIR_INF, k2 = PAIR_INF;
  for (int k = 1; k <= K; ++k) {
    const unsigned long long e = s * (unsigned long long)k, c = e * e;
    if (c >= (k2 >> 3)) break;                                  // nothing further out can enter the two kept pairs
    if (x - k >= 0) {
      const int lb = (int)l[x - k];
      if (lb > 0 && lb <= n_regions) keep_two(k1, k2, (c << 3) | (unsigned long long)lb);
    }
    if (x + k < W) {
      const int lb = (int)l[x + k];
      if (lb > 0 && lb <= n_regions) keep_two(k1, k2, (c << 3) | (unsigned long long)lb);
    }
  }
  cap_two(k1, k2, cap2);
  out[v] = make_ulonglong2(k1, k2);
}

// y pass: min-plus of the kept pairs along y, reduced to the two smallest with distinct classes again
__global__ __launch_bounds__(TPB) void lobe_y_kernel(const ulonglong2* __restrict__ in, ulonglong2* __restrict__ out, int H,
                                                     int W, unsigned total, unsigned long long s, int K,
                                                     unsigned long long cap2) {
  const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
  if (v >= total) return;
  const int y = (int)(v / (unsigned)W % (unsigned)H);
  const ulonglong2 f0 = in[v];
  unsigned long long k1 = f0.x, k2 = f0.y;
  for (int k = 1; k <= K; ++k) {
    const unsigned long long e = s * (unsigned long long)k, c = e * e;
    if (c >= (k2 >> 3)) break;
    if (y - k >= 0) {
      const ulonglong2 f = in[(long)v - (long)k * W];
      if (f.x != PAIR_INF) keep_two(k1, k2, f.x + (c << 3));
      if (f.y != PAIR_INF) keep_two(k1, k2, f.y + (c << 3));
    }
    if (y + k < H) {
      const ulonglong2 f = in[(long)v + (long)k * W];
      if (f.x != PAIR_INF) keep_two(k1, k2, f.x + (c << 3));
      if (f.y != PAIR_INF) keep_two(k1, k2, f.y + (c << 3));
    }
  }
  cap_two(k1, k2, cap2);
  out[v] = make_ulonglong2(k1, k2);
}

// z pass of both transforms and the outputs.  d2 comes from line_min on the pleural work volume, the very code of
// edt_z_kernel; f2 only asks for the voxel's own class, so its loop ends at (s k)^2 >= the best foreign distance so far,
// and it is skipped outside the lung, and inside the peel when no distance volume is wanted (the peel wins).
template <typename LT, typename T>
__global__ __launch_bounds__(TPB) void lobe_z_kernel(const T* __restrict__ in, const ulonglong2* __restrict__ pairs,
                                                     const LT* __restrict__ lab, long sz, long sy, int D, int H, int W,
                                                     unsigned total, unsigned long long s, int K, unsigned long long cap2,
                                                     unsigned long long peel2, unsigned long long fis2, int n_regions,
                                                     uint8_t* __restrict__ zones, uint8_t* __restrict__ zone_labels,
                                                     float* __restrict__ pleura_mm, float* __restrict__ fissure_mm) {
  const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
  if (v >= total) return;
  const unsigned plane = (unsigned)H * (unsigned)W;
  const int z = (int)(v / plane);
  const unsigned long long d2 = line_min<T>(in, (long)v, z, D, (long)plane, s, K, cap2);
  const unsigned r = v - (unsigned)z * plane;
  const int lb = (int)lab[z * sz + (long)(r / (unsigned)W) * sy + (long)(r % (unsigned)W)];
  const unsigned cv = lb <= 0 ? 0u : (lb > n_regions ? (unsigned)n_regions + 1u : (unsigned)lb);
  const bool lung = d2 != 0ull;
  const bool peel = lung && d2 <= peel2;
  unsigned long long f2 = ~0ull;
  if (lung && (!peel || fissure_mm)) {
    f2 = foreign(pairs[v], cv);
    for (int k = 1; k <= K; ++k) {
      const unsigned long long e = s * (unsigned long long)k, c = e * e;
      if (c >= f2) break;
      if (z - k >= 0) {
        const unsigned long long f = foreign(pairs[(long)v - (long)k * plane], cv);
        if (f != ~0ull) f2 = min(f2, f + c);
      }
      if (z + k < D) {
        const unsigned long long f = foreign(pairs[(long)v + (long)k * plane], cv);
        if (f != ~0ull) f2 = min(f2, f + c);
      }
    }
    if (f2 > cap2) f2 = ~0ull;
  }
  const int zone = !lung ? 0 : (peel ? 1 : (f2 <= fis2 ? 3 : 2));
  zones[v] = (uint8_t)zone;
  if (zone_labels) zone_labels[v] = (uint8_t)(zone == 0 ? 0 : (lb > n_regions ? 255 : lb + n_regions * (zone - 1)));
  if (pleura_mm)
    pleura_mm[v] = d2 == ~0ull ? std::numeric_limits<float>::infinity() : (float)(sqrt((double)d2) / 1000.0);
  if (fissure_mm)
    fissure_mm[v] = !lung ? 0.0f
                          : (f2 == ~0ull ? std::numeric_limits<float>::infinity() : (float)(sqrt((double)f2) / 1000.0));
}

template <typename LT, typename T>
int run_lobe(const void* labels, long sz, long sy, uint8_t* zones, uint8_t* zone_labels, float* pleura_mm, float* fissure_mm,
             void* workspace, int D, int H, int W, int sz_um, int sy_um, int sx_um, long long peel_um, long long fissure_um,
             long long max_um, int n_regions, hipStream_t s) {
  const long long total = (long long)D * H * W;
  const long rows = (long)D * H;
  T* a = (T*)workspace;
  T* b = (T*)((char*)workspace + vol_bytes(total, (int)sizeof(T)));
  ulonglong2* p = (ulonglong2*)((char*)workspace + 2 * vol_bytes(total, (int)sizeof(T)));
  ulonglong2* q = (ulonglong2*)((char*)p + vol_bytes(total, 16));
  const unsigned long long cap2 = (unsigned long long)max_um * (unsigned long long)max_um;
  const unsigned long long peel2 = (unsigned long long)peel_um * (unsigned long long)peel_um;
  const unsigned long long fis2 = (unsigned long long)fissure_um * (unsigned long long)fissure_um;
  const int Kx = window(W, sx_um, max_um), Ky = window(H, sy_um, max_um), Kz = window(D, sz_um, max_um);
  const unsigned vgrid = (unsigned)((total + TPB - 1) / TPB);
  const double vox = (double)total, e = (double)sizeof(T), lb = (double)sizeof(LT);
  {                                                             // the pleural x and y passes: dram_lung_zones' own
    DramProf prof(DRAM_FAM_PREP, 13, 0.0, vox * (2.0 * lb + 3.0 * e), s);
    hipLaunchKernelGGL((edt_x_kernel<LT, T>), dim3((unsigned)((rows + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, s,
                       (const LT*)labels, sz, sy, H, W, rows, (unsigned long long)sx_um, (long long)Kx, a);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 14, 0.0, vox * 2.0 * e, s);
    hipLaunchKernelGGL((edt_y_kernel<T>), dim3(vgrid), dim3(TPB), 0, s, (const T*)a, b, H, W, (unsigned)total,
                       (unsigned long long)sy_um, Ky, cap2);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 22, 0.0, vox * (lb + 16.0), s);
    hipLaunchKernelGGL((lobe_x_kernel<LT>), dim3(vgrid), dim3(TPB), 0, s, (const LT*)labels, sz, sy, H, W, (unsigned)total,
                       (unsigned long long)sx_um, Kx, cap2, n_regions, p);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 23, 0.0, vox * 32.0, s);
    hipLaunchKernelGGL(lobe_y_kernel, dim3(vgrid), dim3(TPB), 0, s, (const ulonglong2*)p, q, H, W, (unsigned)total,
                       (unsigned long long)sy_um, Ky, cap2);
    DRAM_LAUNCH_CHECK();
  }
  DramProf prof(DRAM_FAM_PREP, 24, 0.0,
                vox * (e + 16.0 + lb + 1.0 + (zone_labels ? 1.0 : 0.0) + (pleura_mm ? 4.0 : 0.0) + (fissure_mm ? 4.0 : 0.0)), s);
  hipLaunchKernelGGL((lobe_z_kernel<LT, T>), dim3(vgrid), dim3(TPB), 0, s, (const T*)b, (const ulonglong2*)q,
                     (const LT*)labels, sz, sy, D, H, W, (unsigned)total, (unsigned long long)sz_um, Kz, cap2, peel2, fis2,
                     n_regions, zones, zone_labels, pleura_mm, fissure_mm);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

}  // namespace

extern "C" long long dram_lobe_zones_workspace(int D, int H, int W, long long max_um) {
  if (D < 1 || H < 1 || W < 1 || max_um < 0 || (long long)D * H * W >= (1LL << 31)) return 0;
  const long long total = (long long)D * H * W;
  return 2 * vol_bytes(total, max_um <= 65535 ? 4 : 8) + 2 * vol_bytes(total, 16);
}

extern "C" int dram_lobe_zones(const void* labels, int label_dtype, long long stride_z, long long stride_y, uint8_t* zones,
                               uint8_t* zone_labels, float* pleura_mm, float* fissure_mm_out, void* workspace, int D, int H,
                               int W, int sz_um, int sy_um, int sx_um, long long peel_um, long long fissure_um,
                               long long max_um, int n_regions, dram_stream_t stream) {
  if (!labels || !zones || !workspace || (label_dtype != 1 && label_dtype != 2) || stride_z < 0 || stride_y < 0 ||
      peel_um < 0 || fissure_um < 0 || max_um < peel_um || max_um < fissure_um || n_regions < 1 || n_regions > 5)
    return DRAM_ERR_BAD_ARG;
  const int rc = check_sizes(D, H, W, sz_um, sy_um, sx_um);
  if (rc != DRAM_OK) return rc;
  if (max_um > FULL_UM) max_um = FULL_UM;
  if (peel_um > FULL_UM) peel_um = FULL_UM;
  if (fissure_um > FULL_UM) fissure_um = FULL_UM;
  hipStream_t s = (hipStream_t)stream;
  const long sz = (long)stride_z, sy = (long)stride_y;
  auto go = [&](auto d) {                                          // d: the distance word, 32 bits while max_um^2 fits
    return with_label_type(label_dtype, [&](auto t) {
      return run_lobe<decltype(t), decltype(d)>(labels, sz, sy, zones, zone_labels, pleura_mm, fissure_mm_out, workspace, D,
                                                H, W, sz_um, sy_um, sx_um, peel_um, fissure_um, max_um, n_regions, s);
    });
  };
  return max_um <= 65535 ? go(uint32_t{}) : go(uint64_t{});
}

extern "C" long long dram_lung_zones_workspace(int D, int H, int W, long long max_um) {
  if (D < 1 || H < 1 || W < 1 || max_um < 0 || (long long)D * H * W >= (1LL << 31)) return 0;
  return 2 * vol_bytes((long long)D * H * W, max_um <= 65535 ? 4 : 8);
}

extern "C" int dram_lung_zones(const void* labels, int label_dtype, long long stride_z, long long stride_y, uint8_t* zones,
                               uint8_t* zone_labels, float* dist_mm, void* workspace, int D, int H, int W, int sz_um,
                               int sy_um, int sx_um, long long peel_um, long long max_um, int n_regions,
                               dram_stream_t stream) {
  if (!labels || !zones || !workspace || (label_dtype != 1 && label_dtype != 2) || stride_z < 0 || stride_y < 0 ||
      peel_um < 0 || max_um < peel_um)
    return DRAM_ERR_BAD_ARG;
  if (zone_labels ? (n_regions < 1 || n_regions > 7) : n_regions != 0) return DRAM_ERR_BAD_ARG;
  const int rc = check_sizes(D, H, W, sz_um, sy_um, sx_um);
  if (rc != DRAM_OK) return rc;
  if (max_um > FULL_UM) max_um = FULL_UM;
  if (peel_um > FULL_UM) peel_um = FULL_UM;
  hipStream_t s = (hipStream_t)stream;
  const long sz = (long)stride_z, sy = (long)stride_y;
  auto go = [&](auto d) {                                          // d: the distance word, 32 bits while max_um^2 fits
    return with_label_type(label_dtype, [&](auto t) {
      return run<decltype(t), decltype(d)>(labels, sz, sy, zones, zone_labels, dist_mm, workspace, D, H, W, sz_um, sy_um,
                                           sx_um, peel_um, max_um, n_regions, s);
    });
  };
  return max_um <= 65535 ? go(uint32_t{}) : go(uint64_t{});
}
