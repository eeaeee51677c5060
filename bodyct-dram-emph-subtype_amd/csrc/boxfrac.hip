// boxfrac.hip -- the local low-attenuation fraction of the predict report: at every voxel v the box
// B(v) = [z +- rz] x [y +- ry] x [x +- rx] clipped to the volume is counted,
//   den(v) = #{u in B(v): label(u) > 0},   num(v) = #{u in B(v): label(u) > 0 and image(u) < threshold},
// and where label(v) > 0 the fraction is written in per mille, rounded half up: q = (2000 num + den) / (2 den), 0..1000;
// where label(v) <= 0 the map holds -1.  Voxels outside the volume count in neither.  Integers only: exact, and
// bit-identical from call to call.
//
// Both counts travel in ONE 32-bit word, num << 16 | den: (2 RMAX + 1)^3 = 35 937 < 65 536, so neither half can carry
// into the other; one integer add sums both, and the subtraction of a running sum never borrows because the value that
// leaves is contained in the sum, half by half.
//
// Design (figures: DESIGN.md section 4p).  Two launches and one 32-bit intermediate in the caller's workspace, as the
// Gaussian of gauss.hip.
//   * In-plane pass.  A workgroup of 4 waves owns a TY x TX tile of one plane.  It stages the packed indicator
//     (label > 0 ? 1 | (image < threshold) << 16 : 0; 0 outside the volume, where nothing is read) of the (ny + 2 ry) x
//     (TX + 2 rx) patch in LDS, SB image / label load pairs in flight per thread ahead of their LDS writes.  Then along
//     y first, as a running sum: a wave owns RPW = TY / 4 consecutive output rows, a lane one column of the patch (two
//     for the columns past 64); the first row is the sum of 2 ry + 1 words, each further row adds the entering and
//     subtracts the leaving word -- 2 ry + 1 + 2 (RPW - 1) LDS reads for RPW rows instead of RPW (2 ry + 1).  Then along
//     x out of that second array, 2 rx + 1 reads per output, only for the TY rows that are written (x first would have
//     filtered ny + 2 ry rows).  Lane i reads word i + const of a row in both passes: consecutive lanes, consecutive
//     banks, whatever the row stride.  18 KB + 6 KB = 24 576 B of LDS at any radius: six workgroups per CU.
//   * z pass.  One thread per (y, x) column of a segment of ZSEG planes: the sum of the planes [z0 - rz, z0 + rz] inside
//     the volume, then plane by plane one word enters and one leaves.  D / ZSEG segments x H x W threads fill the chip;
//     a segment re-reads 2 rz + 1 planes, so a plane of the intermediate is read 2 + (2 rz + 1) / ZSEG times, the
//     leaving one out of L2 / MALL.  It reads the voxel's own label, divides once (32-bit unsigned: 2000 num + den <
//     2^27), and writes counts / map / u8, the u8 volume through its own z / y strides.
// Every global read is inside the volume.  1-D grids (< 2^31 workgroups because D*H*W is), no atomics, no scratch, never
// synchronises: capturable.
#include "common.h"

namespace {

constexpr int TX = 64, TY = 16;             // outputs per workgroup of the in-plane pass
constexpr int RMAX = DRAM_BOXFRAC_MAX_RADIUS;   // largest radius: 16
constexpr int TPB = 256, WAVES = TPB / 64, RPW = TY / WAVES;
constexpr int LXMAX = TX + 2 * RMAX, LYMAX = TY + 2 * RMAX;
constexpr int SB = 6;                       // staging load pairs in flight per thread (18 elements per thread at r = 16)
constexpr int ZSEG = 64;                    // planes per thread of the z pass
constexpr int ZPB = 256;                    // threads per workgroup of the z pass

static_assert((2 * RMAX + 1) * (2 * RMAX + 1) * (2 * RMAX + 1) < (1 << 16),
              "num and den of the largest box must each fit 16 bits: they share one 32-bit word");
static_assert((long long)LYMAX * LXMAX < (1 << 16), "the staging index must stay below 2^16 for the magic division");
static_assert(2000LL * (2 * RMAX + 1) * (2 * RMAX + 1) * (2 * RMAX + 1) + (1 << 16) < (1LL << 32),
              "the rounding numerator 2000 num + den must fit 32 bits");

// mid[z][y][x] = packed count of the in-plane window (2 ry + 1) x (2 rx + 1) around (y, x) in plane z
template <typename LT>
__global__ __launch_bounds__(TPB) void boxfrac_plane_kernel(const int16_t* __restrict__ img, const LT* __restrict__ lab,
                                                            long sz, long sy, unsigned* __restrict__ mid, int H, int W,
                                                            int threshold, int ry, int rx, int ntx, int nty,
                                                            unsigned magic) {
  __shared__ unsigned patch[LYMAX * LXMAX];
  __shared__ unsigned cols[TY * LXMAX];
  const int bx = (int)(blockIdx.x % (unsigned)ntx), by = (int)(blockIdx.x / (unsigned)ntx % (unsigned)nty),
            z = (int)(blockIdx.x / (unsigned)ntx / (unsigned)nty);
  const int tx0 = bx * TX, ty0 = by * TY;
  const int ny = min(TY, H - ty0);
  const int LX = TX + 2 * rx, LY = ny + 2 * ry, NE = LY * LX;      // magic = 2^32 / LX + 1: e / LX for e < 2^16
  const int16_t* iplane = img + (size_t)z * H * W;
  const LT* lplane = lab + (long)z * sz;
  const int gy0 = ty0 - ry, gx0 = tx0 - rx;

  // stage: patch[m][i] = indicator of (z, gy0 + m, gx0 + i); indices are clamped for the loads, so every read is inside
  // the volume, and what was clamped counts as 0
  for (int e0 = (int)threadIdx.x; e0 < NE; e0 += SB * TPB) {
    int hu[SB], lb[SB];
    bool in[SB];
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int e = min(e0 + u * TPB, NE - 1);                     // past the end: the last element again, not stored
      const int m = (int)__umulhi((unsigned)e, magic), i = e - m * LX;
      const int gy = gy0 + m, gx = gx0 + i;
      const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);
      hu[u] = (int)iplane[(size_t)cy * W + cx];
      lb[u] = (int)lplane[(long)cy * sy + cx];
      in[u] = cy == gy && cx == gx;
    }
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int e = e0 + u * TPB;
      if (e < NE) patch[e] = (in[u] && lb[u] > 0) ? (1u | (hu[u] < threshold ? 0x10000u : 0u)) : 0u;
    }
  }
  __syncthreads();

  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  // along y, a running sum: cols[j][c] = sum of patch[j .. j + 2 ry][c]
  const int j0 = wv * RPW, j1 = min(ny, j0 + RPW);
  if (j0 < j1) {
    for (int c = lane; c < LX; c += 64) {
      const unsigned* p = patch + j0 * LX + c;
      unsigned s = 0;
      for (int k = 0; k <= 2 * ry; ++k) s += p[k * LX];
      cols[j0 * LX + c] = s;
      for (int j = j0 + 1; j < j1; ++j) {
        s += p[(j - j0 + 2 * ry) * LX] - p[(j - j0 - 1) * LX];     // the leaving word is part of s: no borrow
        cols[j * LX + c] = s;
      }
    }
  }
  __syncthreads();

  // along x: 2 rx + 1 words of the row
  const int x = tx0 + lane;
  if (x >= W) return;                                              // no barrier below
  for (int j = wv; j < ny; j += WAVES) {
    const unsigned* p = cols + j * LX + lane;
    unsigned s = 0;
    for (int k = 0; k <= 2 * rx; ++k) s += p[k];
    mid[((size_t)z * H + (ty0 + j)) * W + x] = s;
  }
}

// item i = (segment, y, x): the planes [seg * ZSEG, min(D, (seg + 1) * ZSEG)) of column (y, x)
template <typename LT>
__global__ __launch_bounds__(ZPB) void boxfrac_z_kernel(const unsigned* __restrict__ mid, const LT* __restrict__ lab,
                                                        long sz, long sy, int* __restrict__ counts,
                                                        int16_t* __restrict__ map, uint8_t* __restrict__ u8, long uz,
                                                        long uy, int D, int H, int W, int rz, unsigned total) {
  const unsigned i = blockIdx.x * (unsigned)ZPB + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % (unsigned)W), y = (int)(i / (unsigned)W % (unsigned)H), seg = (int)(i / (unsigned)W / (unsigned)H);
  const int z0 = seg * ZSEG, z1 = min(D, z0 + ZSEG);
  const size_t plane = (size_t)H * W, off = (size_t)y * W + x;
  const LT* lcol = lab + (long)y * sy + x;
  uint8_t* ucol = u8 ? u8 + (long)y * uy + x : nullptr;

  unsigned s = 0;
  for (int zz = max(0, z0 - rz); zz <= min(D - 1, z0 + rz); ++zz) s += mid[(size_t)zz * plane + off];
#pragma unroll 4
  for (int z = z0; z < z1; ++z) {
    const size_t o = (size_t)z * plane + off;
    const int zin = z + rz + 1, zout = z - rz;
    const unsigned enter = zin < D ? mid[(size_t)zin * plane + off] : 0u;
    const unsigned leave = zout >= 0 ? mid[(size_t)zout * plane + off] : 0u;
    const bool lung = (int)lcol[(long)z * sz] > 0;
    int q = -1;
    if (lung) {                                                    // the voxel itself is in its box: den >= 1
      const unsigned num = s >> 16, den = s & 0xffffu;
      q = (int)((2000u * num + den) / (2u * den));
    }
    if (counts) counts[o] = (int)s;
    map[o] = (int16_t)q;
    if (ucol) ucol[(long)z * uz] = (uint8_t)(q < 0 ? 0 : q * 255 / 1000);
    s += enter - leave;                                            // the leaving word is part of s + enter: no borrow
  }
}

}  // namespace

extern "C" long long dram_boxfrac3d_workspace(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1 || (long long)D * H * W >= (1LL << 31)) return -1;
  return (long long)D * H * W * (long long)sizeof(unsigned);
}

extern "C" int dram_boxfrac3d(const int16_t* image, const void* labels, int label_dtype, long long stride_z,
                              long long stride_y, int threshold, int rz, int ry, int rx, int32_t* counts, int16_t* map,
                              uint8_t* u8, long long u8_stride_z, long long u8_stride_y, void* work, long long work_bytes,
                              int D, int H, int W, dram_stream_t stream) {
  if (!image || !labels || !map || !work || (label_dtype != 1 && label_dtype != 2) || D < 1 || H < 1 || W < 1 ||
      stride_z < 0 || stride_y < 0 || rz < 0 || ry < 0 || rx < 0 || threshold < -32768 || threshold > 32768)
    return DRAM_ERR_BAD_ARG;
  const void* outs[3] = {counts, map, u8};
  for (const void* o : outs)
    if (o && (o == (const void*)image || o == labels || o == work)) return DRAM_ERR_BAD_ARG;
  if (work == (const void*)image || work == labels || (counts && (void*)counts == (void*)map) ||
      (u8 && ((void*)u8 == (void*)map || (void*)u8 == (void*)counts)))
    return DRAM_ERR_BAD_ARG;
  // the u8 window must not overlap itself: rows of W bytes, planes of H rows
  if (u8 && (u8_stride_z < 0 || u8_stride_y < 0 || (H > 1 && u8_stride_y < W) ||
             (D > 1 && u8_stride_z < (long long)(H - 1) * u8_stride_y + W)))
    return DRAM_ERR_BAD_ARG;
  if (((uintptr_t)work & 15) || ((uintptr_t)map & 1) || (counts && ((uintptr_t)counts & 3)) || ((uintptr_t)image & 1) ||
      (label_dtype == 2 && ((uintptr_t)labels & 1)))
    return DRAM_ERR_BAD_ARG;
  if (rz > RMAX || ry > RMAX || rx > RMAX || (long long)D * H * W >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  if (work_bytes < dram_boxfrac3d_workspace(D, H, W)) return DRAM_ERR_BAD_ARG;

  const double n = (double)D * H * W;
  const int ntx = cdiv(W, TX), nty = cdiv(H, TY);
  const unsigned magic = (unsigned)((1ULL << 32) / (unsigned)(TX + 2 * rx)) + 1u;
  hipStream_t s = (hipStream_t)stream;
  unsigned* mid = (unsigned*)work;
  const long sz = (long)stride_z, sy = (long)stride_y;
  {
    DramProf prof(DRAM_FAM_PREP, 29, 0.0, n * (2.0 + label_dtype + 4.0), s);
    const dim3 grid((unsigned)((long long)ntx * nty * D));         // <= D * H * W < 2^31
    with_label_type(label_dtype, [&](auto t) {
      using LT = decltype(t);
      hipLaunchKernelGGL((boxfrac_plane_kernel<LT>), grid, dim3(TPB), 0, s, image, (const LT*)labels, sz, sy, mid, H, W,
                         threshold, ry, rx, ntx, nty, magic);
    });
    DRAM_LAUNCH_CHECK();
  }
  {
    const int nseg = cdiv(D, ZSEG);
    const unsigned total = (unsigned)((long long)nseg * H * W);    // <= D * H * W < 2^31
    const double reads = 2.0 + (2.0 * rz + 1.0) / ZSEG;
    DramProf prof(DRAM_FAM_PREP, 30, 0.0, n * (4.0 * reads + label_dtype + 2.0 + (counts ? 4.0 : 0.0) + (u8 ? 1.0 : 0.0)), s);
    const dim3 grid((unsigned)cdiv(total, ZPB));
    with_label_type(label_dtype, [&](auto t) {
      using LT = decltype(t);
      hipLaunchKernelGGL((boxfrac_z_kernel<LT>), grid, dim3(ZPB), 0, s, mid, (const LT*)labels, sz, sy, counts, map, u8,
                         (long)u8_stride_z, (long)u8_stride_y, D, H, W, rz, total);
    });
    DRAM_LAUNCH_CHECK();
  }
  return DRAM_OK;
}
