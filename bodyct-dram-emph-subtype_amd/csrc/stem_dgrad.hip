// stem_dgrad.hip -- data gradient of Conv3d(1, 64, k=7, s=2, p=3): dx = conv_transpose(dy, w), the gradient of a
// scan-level score with respect to the CT volume (saliency / attribution; the training step does not need it).
//
//   dx[b,d,h,w] = sum_c sum_(kd,kh,kw) dy[b,od,oh,ow,c] * w[c,0,kd,kh,kw],   2*od + kd - 3 == d  (h, w likewise)
//
// A gather per input voxel has ONE output column (C_in = 1): nothing for a matrix core.  So the product is taken the
// other way round, as a scatter GEMM  P[tap][voxel] = sum_c w[c][tap] * dy[voxel][c]  (M = 343 taps, N = dy voxels,
// K = 64, mfma_f32_32x32x2f32 -- the MAC count of the forward), and P is overlap-added into the input patch the voxels
// cover: workgroup = 4x8x8 dy voxels -> the 13x21x21 patch stem_fwd_kernel reads, held in LDS with the same pitch.
//
// Deterministic overlap-add, plain LDS reads and writes (no atomics): taps of different PARITY (kz&1, ky&1, kx&1) land
// on patch cells of different parity (cell = 2*voxel + tap), so the 8 parity classes own disjoint cells.  Each of the 4
// waves owns two classes (A + B = 64 + 27, 48 + 36, 48 + 36, 48 + 36 taps = 91 / 84 rows of its 3 M tiles of 32) over ALL
// 256 voxels: no cell is ever touched by two waves, and a wave's own read - add - write steps are in program order.
// Inside one step no two lanes may meet in a cell.  Two taps of one class meet (through different voxels of the N
// tile, which lies in one z plane) only if they have the SAME kz.  The tap rows are ordered for that (wave_tap): the
// two half-waves of an accumulator element hold an (A, B) pair, and three consecutive elements hold three taps of A
// with three different kz and three of B likewise -- one step = 3 reads in flight, 3 adds, 3 writes, full width.
// Behind B's last tap (pairs of two A taps with different kz, padding) the rows go one by one.
// (ds_add_f32 instead of the read - add - write was measured: 3.6 ms of LDS time per 2x128x256x256)
// Operands come straight from registers: the wave's 96 tap rows x 64 channels of w stay in 96 VGPRs for the whole
// (persistent) workgroup; a lane loads 32 consecutive channels of one dy voxel (K is permuted so that the MFMA k pair kk
// is channels (kk, kk + 32): lanes 0-31 own channels 0-31, lanes 32-63 channels 32-63 -- 128 contiguous bytes per lane).
// Halo: neighbouring patches overlap by 5 cells per axis.  Each workgroup writes its whole patch to the workspace and
// stem_dgrad_fold_kernel sums the <= 2x2x2 patches over a voxel in a fixed order (z, y, x tile ascending; plain adds) -- 2.8 x the
// bytes of dx written and read once more (94 MB per 128x256x256 volume beside the 268 MB of dy), against the 3.3 x MACs a
// halo recompute (7x11x11 dy voxels per 8x16x16 owned cells) would cost.
#include "common.h"

namespace {

constexpr int PZ = 13, PY = 21, PX = 21;
constexpr int PATCH = PZ * PY * PX;      // 5733 values per workgroup patch (dense in the workspace)
constexpr int PXP = 24;                  // x-row pitch in LDS: the four y rows of a half-wave (cell rows 2*ty: offsets 0, 48,
                                         // 96, 144 -> banks 0, 48, 32, 16) and its 8 even x cells fall on 32 different banks
constexpr int PLANE = PY * PXP;          // 504
constexpr int PATCHP = PZ * PLANE;       // 6552 floats
constexpr int ROWS = 96;                 // tap rows per wave: 3 M tiles of 32
constexpr int MAXBLK = 512;              // persistent grid: two workgroups per CU

struct DGeom {
  int B, D, H, W, Do, Ho, Wo;
  int nz, ny, nx, tiles_per_b, nblk;
};

// tap idx of parity class (pz, py, px), kz fastest: consecutive idx differ in kz
__device__ __forceinline__ int class_tap(int pz, int py, int px, int idx) {
  const int nz = pz ? 3 : 4, nx = px ? 3 : 4;
  const int iz = idx % nz, rest = idx / nz;
  return (2 * iz + pz) * 49 + (2 * (rest / nx) + py) * 7 + (2 * (rest % nx) + px);
}

// tap (kz*49 + ky*7 + kx) of row r of wave w, or -1 (padding).  Wave 0 owns the all-even class A (64 taps) and the
// all-odd class B (27); wave a + 1 the class A whose only odd axis is a (48) and the class B whose only even axis is a
// (36).  Accumulator element e of an M tile holds row (e & 3) + 8*(e >> 2) in lanes 0-31 and that row + 4 in lanes
// 32-63: such a PAIR of rows gets two taps that can never meet in a cell -- one of A with one of B (different parity),
// or, once B is used up, two consecutive taps of A (different kz; the 32 voxels of an N tile lie in one z plane).
__device__ __forceinline__ int wave_tap(int w, int r) {
  const int pz = w == 1, py = w == 2, px = w == 3;
  const int nA = (pz ? 3 : 4) * (py ? 3 : 4) * (px ? 3 : 4);
  const int nB = (pz ? 4 : 3) * (py ? 4 : 3) * (px ? 4 : 3);
  const int rr = r & 31, h = (rr >> 2) & 1;
  const int p = 16 * (r >> 5) + (rr & 3) + 4 * (rr >> 3);     // pair index: 16 per M tile
  if (p < nB) return h ? class_tap(pz ^ 1, py ^ 1, px ^ 1, p) : class_tap(pz, py, px, p);
  const int idx = nB + 2 * (p - nB) + h;
  return idx < nA ? class_tap(pz, py, px, idx) : -1;
}

template <typename T>   // T: storage type of dy (float | bf16_t); fp32 arithmetic either way
__global__ __launch_bounds__(256, 2) void stem_dgrad_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                            float* __restrict__ ws, const DGeom g) {
  __shared__ __attribute__((aligned(16))) float patch[PATCHP];
  __shared__ int toff[4 * ROWS];          // patch offset of every wave's tap rows (-1: padding row)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int nB = wave == 0 ? 27 : 36;     // (A, B) pairs of this wave (wave_tap)

  for (int i = tid; i < 4 * ROWS; i += 256) {
    const int t = wave_tap(i / ROWS, i % ROWS);
    toff[i] = t < 0 ? -1 : (t / 49) * PLANE + ((t / 7) % 7) * PXP + t % 7;
  }

  // A[i = tap row][k = channel]: a[mt][kk] is channel kk + 32*lh of tap row 32*mt + li
  float a[3][32];
#pragma unroll
  for (int mt = 0; mt < 3; ++mt) {
    const int t = wave_tap(wave, 32 * mt + li);
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) a[mt][kk] = t >= 0 ? w[(kk + 32 * lh) * 343 + t] : 0.f;
  }

  for (int L = blockIdx.x; L < g.nblk; L += gridDim.x) {
    const int b = L / g.tiles_per_b;
    int r = L - b * g.tiles_per_b;
    const int txi = r % g.nx; r /= g.nx;
    const int tyi = r % g.ny;
    const int tzi = r / g.ny;
    const int z0 = tzi * 4, y0 = tyi * 8, x0 = txi * 8;

    __syncthreads();                      // the previous patch is written out (first pass: toff is complete)
    for (int i = tid; i < PATCHP; i += 256) patch[i] = 0.f;
    __syncthreads();

    // B[k = channel][j = voxel]: N tile nt = voxels (z = nt >> 1, y = 4*(nt & 1) + (li >> 3), x = li & 7)
    float bv[32];
    auto load_b = [&](int nt) {
      const int zo = z0 + (nt >> 1), yo = y0 + 4 * (nt & 1) + (li >> 3), xo = x0 + (li & 7);
      const bool ok = (zo < g.Do) & (yo < g.Ho) & (xo < g.Wo);
      const long o = ((((long)b * g.Do + zo) * g.Ho + yo) * g.Wo + xo) * 64 + 32 * lh;
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          fvec<8> v = fvec<8>{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
          if (ok) v = ldv<T, 8>(dy, o + 8 * q);
#pragma unroll
          for (int j = 0; j < 8; ++j) bv[8 * q + j] = v.v[j];
        }
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float4 v = ok ? ld4<T>(dy, o + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
          bv[4 * q] = v.x; bv[4 * q + 1] = v.y; bv[4 * q + 2] = v.z; bv[4 * q + 3] = v.w;
        }
      }
    };

    load_b(0);
#pragma unroll 1
    for (int nt = 0; nt < 8; ++nt) {
      f32x16 acc[3];
#pragma unroll
      for (int mt = 0; mt < 3; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[mt][e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 32; ++kk)
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
          acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][kk], bv[kk], acc[mt], 0, 0, 0);
      const int vb = (2 * (nt >> 1)) * PLANE + (2 * (4 * (nt & 1) + (li >> 3))) * PXP + 2 * (li & 7);
      if (nt + 1 < 8) load_b(nt + 1);     // in flight under the overlap-add
      // acc[mt][e]: tap row 32*mt + (e & 3) + 8*(e >> 2) + 4*lh, voxel li
#pragma unroll
      for (int mt = 0; mt < 3; ++mt) {
        int o[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] = toff[wave * ROWS + 32 * mt + (e & 3) + 8 * (e >> 2) + 4 * lh];
        // read - add - write in groups of 3 accumulator rows.  Where every pair of the group is an (A, B) pair, the
        // 3 taps of A (consecutive: three different kz) and the 3 of B never meet in a cell, so the group is ONE
        // round trip: 3 reads in flight, 3 writes.  Behind B's last tap (pairs of two A taps, padding) row by row.
#pragma unroll
        for (int g0 = 0; g0 < 16; g0 += 3) {
          const int n = g0 + 3 <= 16 ? 3 : 16 - g0;
          if (16 * mt + g0 + n <= nB) {
            float t[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
              if (j < n) t[j] = patch[vb + o[g0 + j]];
#pragma unroll
            for (int j = 0; j < 3; ++j)
              if (j < n) patch[vb + o[g0 + j]] = t[j] + acc[mt][g0 + j];
          } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
              if (j < n && o[g0 + j] >= 0) {
                patch[vb + o[g0 + j]] += acc[mt][g0 + j];
                __builtin_amdgcn_wave_barrier();
              }
          }
          __builtin_amdgcn_wave_barrier();     // groups in program order
        }
      }
    }
    __syncthreads();
    float* out = ws + (long)L * PATCH;
    for (int i = tid; i < PATCH; i += 256) {
      const int pz = i / (PY * PX), rem = i - pz * (PY * PX);
      out[i] = patch[pz * PLANE + (rem / PX) * PXP + rem % PX];
    }
  }
}

// dx voxel d lies in the patches of the z tiles t with 8t - 3 <= d <= 8t + 9 (y, x: 16t - 3 <= h <= 16t + 17): at most
// two per axis, summed z-major in ascending order.
__global__ __launch_bounds__(256) void stem_dgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ dx,
                                                              const DGeom g, long total) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int xw = (int)(i % g.W);
    long r = i / g.W;
    const int yh = (int)(r % g.H); r /= g.H;
    const int zd = (int)(r % g.D);
    const int b = (int)(r / g.D);
    const int zlo = zd < 2 ? 0 : (zd - 2) / 8, zhi = min(g.nz - 1, (zd + 3) / 8);
    const int ylo = yh < 2 ? 0 : (yh - 2) / 16, yhi = min(g.ny - 1, (yh + 3) / 16);
    const int xlo = xw < 2 ? 0 : (xw - 2) / 16, xhi = min(g.nx - 1, (xw + 3) / 16);
    float s = 0.f;
    for (int tz = zlo; tz <= zhi; ++tz) {
      const int pz = zd + 3 - 8 * tz;
      for (int ty = ylo; ty <= yhi; ++ty) {
        const int py = yh + 3 - 16 * ty;
        for (int tx = xlo; tx <= xhi; ++tx) {
          const int px = xw + 3 - 16 * tx;
          const long tile = (long)b * g.tiles_per_b + ((long)tz * g.ny + ty) * g.nx + tx;
          s += ws[tile * PATCH + (pz * PY + py) * PX + px];
        }
      }
    }
    dx[i] = s;
  }
}

inline int stem_out(int n) { return (n + 6 - 7) / 2 + 1; }

inline DGeom dgeom(int B, int D, int H, int W) {
  DGeom g{};
  g.B = B; g.D = D; g.H = H; g.W = W;
  g.Do = stem_out(D); g.Ho = stem_out(H); g.Wo = stem_out(W);
  g.nz = (g.Do + 3) / 4; g.ny = (g.Ho + 7) / 8; g.nx = (g.Wo + 7) / 8;
  g.tiles_per_b = g.nz * g.ny * g.nx;
  g.nblk = B * g.tiles_per_b;
  return g;
}

}  // namespace

extern "C" size_t dram_stem_bwd_data_workspace(int B, int D, int H, int W) {
  if (B < 1 || D < 1 || H < 1 || W < 1) return 0;
  return (size_t)dgeom(B, D, H, W).nblk * PATCH * sizeof(float);
}

template <typename T>
static int stem_bwd_data_impl(const T* dy, const float* w, float* dx, int B, int D, int H, int W, void* workspace,
                              size_t workspace_bytes, dram_stream_t stream) {
  if (!dy || !w || !dx || B < 1 || D < 1 || H < 1 || W < 1) return DRAM_ERR_BAD_ARG;
  const DGeom g = dgeom(B, D, H, W);
  if (!workspace || workspace_bytes < (size_t)g.nblk * PATCH * sizeof(float)) return DRAM_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const double vo = (double)B * g.Do * g.Ho * g.Wo, vi = (double)B * D * H * W;
  {
    DramProf prof(DRAM_FAM_STEM, 4, 2.0 * (double)g.nblk * 256.0 * 64.0 * 4.0 * ROWS,
                  sizeof(T) * vo * 64.0 + 4.0 * 64.0 * 343.0 + 4.0 * (double)g.nblk * PATCH, s,
                  2.0 * vo * 64.0 * 343.0);
    hipLaunchKernelGGL((stem_dgrad_kernel<T>), dim3(g.nblk < MAXBLK ? g.nblk : MAXBLK), dim3(256), 0, s, dy, w,
                       (float*)workspace, g);
    DRAM_LAUNCH_CHECK();
  }
  {
    const long total = (long)B * D * H * W;
    DramProf prof(DRAM_FAM_STEM, 5, 0.0, 4.0 * (double)g.nblk * PATCH + 4.0 * vi, s);
    hipLaunchKernelGGL(stem_dgrad_fold_kernel, dim3(cdiv(total, 256) < (1 << 20) ? cdiv(total, 256) : (1 << 20)), dim3(256), 0, s,
                       (const float*)workspace, dx, g, total);
    DRAM_LAUNCH_CHECK();
  }
  return DRAM_OK;
}
extern "C" int dram_stem_bwd_data(const float* dy, const float* w, float* dx, int B, int D, int H, int W,
                                  void* workspace, size_t workspace_bytes, dram_stream_t stream) {
  return stem_bwd_data_impl<float>(dy, w, dx, B, D, H, W, workspace, workspace_bytes, stream);
}
extern "C" int dram_stem_bwd_data_bf16(const void* dy, const float* w, float* dx, int B, int D, int H, int W,
                                       void* workspace, size_t workspace_bytes, dram_stream_t stream) {
  return stem_bwd_data_impl<bf16_t>((const bf16_t*)dy, w, dx, B, D, H, W, workspace, workspace_bytes, stream);
}
