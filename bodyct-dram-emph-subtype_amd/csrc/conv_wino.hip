// conv_wino.hip -- Winograd F(2x2x2, 3x3x3) path for the wide stride-1 3x3x3 convolutions
// (forward, data gradient and weight gradient) on the gfx950 fp32 matrix cores.
//
// Same call sites as conv_igemm.hip / conv_wgrad.hip (reference med3d.py:91-100 conv3x3x3 inside
// BasicBlock / Bottleneck, dilation 1/2/4 with padding == dilation; autograd's
// convolution_backward for them).  The direct implicit GEMM already runs at ~0.86 of the fp32
// MFMA peak, so the remaining lever is arithmetic: the 3-D Winograd transform needs 64 instead
// of 216 multiplies per 2x2x2 output tile and channel pair (3.375x fewer MFMA flops).
//
//   U[xi][co][ci] = G w G^T (3-D)                      weight transform, once per step
//   V[xi][t][ci]  = B^T x B (3-D) of the 4x4x4 input tile t            wino_in_kernel<0>
//   M[xi][t][co]  = sum_ci V[xi][t][ci] * U[xi][co][ci]   64 dense GEMMs  wino_gemm_nn_kernel
//   y(tile t)     = A^T M A (3-D) + bias (+ fused epilogue, BN partial sums) wino_out_kernel
// Data gradient: the same pipeline on dy with the tap-flipped, transposed weights.
// Weight gradient: dU[xi][co][ci] = sum_t (A dy A^T)[xi][t][co] * V[xi][t][ci]  (TN GEMMs, split
// over t into slabs), then dw = G^T (sum of slabs) G in a fixed order -> deterministic.
//
// A dilated convolution is d^3 independent dilation-1 convolutions on the residue sub-lattices,
// so the tiles are 2x2x2 blocks of a sub-lattice (voxel step d).  V and M round-trip through HBM
// (8x the activation bytes), which is why the path is planned only for >= 256-channel layers:
// there the GEMMs dominate (layer4: 2.3 GB of transform traffic vs 137 GFLOP per pass).
//
// The GEMMs (wino_gemm_nn_* / wino_gemm_tn_* kernels, run_nn / run_tn) are in wino_gemm.hip, with the 1x1x1
// convolutions that run on them as plain GEMMs; this file keeps the transforms, the tiling and plan functions
// and the dram_wino_* entry points.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "wino_gemm.h"

namespace {

// first OUTPUT voxel of tile t; tile-local positions step by g.d
__device__ __forceinline__ void tile_origin(const WinoGeom& g, int t, int& b, int& z0, int& y0, int& x0) {
  int r = t;
  const int tx = r % g.Tx; r /= g.Tx;
  const int ty = r % g.Ty; r /= g.Ty;
  const int tz = r % g.Tz; r /= g.Tz;
  const int rx = r % g.d; r /= g.d;
  const int ry = r % g.d; r /= g.d;
  const int rz = r % g.d;
  b = r / g.d;
  z0 = g.nz * tz * g.d + rz;
  y0 = g.ny * ty * g.d + ry;
  x0 = g.nx * tx * g.d + rx;
}

// Winograd-domain buffers are blocked by the GEMM M tile: [t / 256][point][t % 256][channel], so the
// 256 x C operand tile of a point is one contiguous run and a workgroup of the transforms writes /
// reads a compact region (all points of its tiles) instead of one 256-B row in each of 64-216 planes.
__device__ __host__ __forceinline__ long wino_index(int t, int npts, int C) {
  return (((long)(t >> 8) * npts) * 256 + (t & 255)) * C;
}

// ---- split-bf16 operand image (math modes "bf16x3" / "bf16", see wino_gemm_nn_bf16_kernel) -------------
// A GEMM operand row of C fp32 channels becomes, per 32-channel block, 32 bf16 "hi" values (64 B) followed
// by 32 bf16 "lo" values (64 B): hi = bf16(v) (round to nearest even), lo = bf16(v - hi), so hi + lo carries
// 16 mantissa bits of v.  Same bytes per row as fp32, so every buffer size and DMA pattern is unchanged.
// Lanes are consecutive channels: the even lane of a pair writes the dword (hi_e, hi_e+1), the odd lane
// (lo_e, lo_e+1); the partner's half arrives by a quad-permute DPP move (no LDS).
__device__ __forceinline__ int split_pos(int lane) {      // dword position inside the lane's 64-channel block
  return (lane >> 5) * 32 + (lane & 1) * 16 + ((lane & 31) >> 1);
}
__device__ __forceinline__ float split_pack(float v, bool odd) {
  const __bf16 h = (__bf16)v;
  const __bf16 l = (__bf16)(v - (float)h);
  const unsigned hb = __builtin_bit_cast(unsigned short, h), lb = __builtin_bit_cast(unsigned short, l);
  const unsigned send = odd ? hb : lb;
  const unsigned recv = (unsigned)__builtin_amdgcn_mov_dpp((int)send, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
  const unsigned lo16 = odd ? recv : hb, hi16 = odd ? lb : recv;
  return __uint_as_float(lo16 | (hi16 << 16));
}

// ---- 1-D transforms (Lavin & Gray): F(2,3) with points {0, 1, -1, inf}, F(4,3) with {0, +-1, +-2, inf} --
// B^T d   (n + 2 -> n + 2)
__device__ __forceinline__ void bt2(float* a) {
  const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
  a[0] = a0 - a2; a[1] = a1 + a2; a[2] = a2 - a1; a[3] = a1 - a3;
}
// (explicit fma chains: with `a * b + c` left to the compiler's contraction, two instantiations of a transform kernel --
// with and without the BatchNorm prologue -- fused differently and their images differed in the last bit)
__device__ __forceinline__ void bt4(float* a) {
  const float d0 = a[0], d1 = a[1], d2 = a[2], d3 = a[3], d4 = a[4], d5 = a[5];
  a[0] = __builtin_fmaf(4.f, d0, __builtin_fmaf(-5.f, d2, d4));
  a[1] = __builtin_fmaf(-4.f, d1 + d2, d3 + d4);
  a[2] = __builtin_fmaf(4.f, d1 - d2, d4 - d3);
  a[3] = __builtin_fmaf(2.f, d3 - d1, d4 - d2);
  a[4] = __builtin_fmaf(2.f, d1 - d3, d4 - d2);
  a[5] = __builtin_fmaf(4.f, d1, __builtin_fmaf(-5.f, d3, d5));
}
// A^T m   (n + 2 -> n)
__device__ __forceinline__ void at2(const float* m, float* r) {
  r[0] = m[0] + m[1] + m[2];
  r[1] = m[1] - m[2] - m[3];
}
__device__ __forceinline__ void at4(const float* m, float* r) {
  const float s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
  r[0] = m[0] + s12 + s34;
  r[1] = d12 + 2.f * d34;
  r[2] = s12 + 4.f * s34;
  r[3] = d12 + 8.f * d34 + m[5];
}
// A y   (n -> n + 2), the transpose of A^T (weight gradient)
__device__ __forceinline__ void a2(const float* y, float* r) {
  r[0] = y[0]; r[1] = y[0] + y[1]; r[2] = y[0] - y[1]; r[3] = -y[1];
}
__device__ __forceinline__ void a4(const float* y, float* r) {
  const float e = y[0] + y[2], o = y[1] + y[3], e4 = y[0] + 4.f * y[2], o4 = 2.f * y[1] + 8.f * y[3];
  r[0] = y[0]; r[1] = e + o; r[2] = e - o; r[3] = e4 + o4; r[4] = e4 - o4; r[5] = y[3];
}
// G g   (3 -> n + 2)
__device__ __forceinline__ void g2(const float* g, float* r) {
  const float h = 0.5f * (g[0] + g[2]);
  r[0] = g[0]; r[1] = h + 0.5f * g[1]; r[2] = h - 0.5f * g[1]; r[3] = g[2];
}
__device__ __forceinline__ void g4z(const float* g, float* r) {
  const float s = (g[0] + g[2]) * (1.f / 6.f), t = g[0] * (1.f / 24.f) + g[2] * (1.f / 6.f);
  r[0] = 0.25f * g[0];
  r[1] = -s - g[1] * (1.f / 6.f);
  r[2] = -s + g[1] * (1.f / 6.f);
  r[3] = t + g[1] * (1.f / 12.f);
  r[4] = t - g[1] * (1.f / 12.f);
  r[5] = g[2];
}
// G^T s   (n + 2 -> 3)
__device__ __forceinline__ void gt2(const float* s, float* r) {
  r[0] = s[0] + 0.5f * (s[1] + s[2]);
  r[1] = 0.5f * (s[1] - s[2]);
  r[2] = 0.5f * (s[1] + s[2]) + s[3];
}
__device__ __forceinline__ void gt4(const float* s, float* r) {
  const float s12 = s[1] + s[2], s34 = s[3] + s[4];
  r[0] = 0.25f * s[0] - s12 * (1.f / 6.f) + s34 * (1.f / 24.f);
  r[1] = (s[2] - s[1]) * (1.f / 6.f) + (s[3] - s[4]) * (1.f / 12.f);
  r[2] = -s12 * (1.f / 6.f) + s34 * (1.f / 6.f) + s[5];
}
template <int NZ> __device__ __forceinline__ void btz(float* a) { if (NZ == 2) bt2(a); else bt4(a); }
template <int NZ> __device__ __forceinline__ void atz(const float* m, float* r) { if (NZ == 2) at2(m, r); else at4(m, r); }
template <int NZ> __device__ __forceinline__ void az(const float* y, float* r) { if (NZ == 2) a2(y, r); else a4(y, r); }
template <int NZ> __device__ __forceinline__ void gz(const float* g, float* r) { if (NZ == 2) g2(g, r); else g4z(g, r); }
template <int NZ> __device__ __forceinline__ void gtz(const float* s, float* r) { if (NZ == 2) gt2(s, r); else gt4(s, r); }

// Matrix entries as compile-time tables (indices are unrolled constants, zero entries vanish).
template <int N> __device__ __forceinline__ constexpr float bt_coef(int r, int c) {   // B^T [N+2][N+2]
  if (N == 2) {
    constexpr float t[4][4] = {{1, 0, -1, 0}, {0, 1, 1, 0}, {0, -1, 1, 0}, {0, 1, 0, -1}};
    return t[r][c];
  }
  constexpr float t[6][6] = {{4, 0, -5, 0, 1, 0}, {0, -4, -4, 1, 1, 0}, {0, 4, -4, -1, 1, 0},
                             {0, -2, -1, 2, 1, 0}, {0, 2, -1, -2, 1, 0}, {0, 4, 0, -5, 0, 1}};
  return t[r][c];
}
template <int N> __device__ __forceinline__ constexpr float at_coef(int o, int i) {   // A^T [N][N+2]
  if (N == 2) {
    constexpr float t[2][4] = {{1, 1, 1, 0}, {0, 1, -1, -1}};
    return t[o][i];
  }
  constexpr float t[4][6] = {{1, 1, 1, 1, 1, 0}, {0, 1, -1, 2, -2, 0}, {0, 1, 1, 4, 4, 0}, {0, 1, -1, 8, -8, 1}};
  return t[o][i];
}
template <int N> __device__ __forceinline__ constexpr float g_coef(int r, int k) {    // G [N+2][3]
  if (N == 2) {
    constexpr float t[4][3] = {{1, 0, 0}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0, 0, 1}};
    return t[r][k];
  }
  constexpr float t[6][3] = {{.25f, 0, 0}, {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                             {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0, 0, 1}};
  return t[r][k];
}

// ------------------------------------------------------------------------------------------
// Tile transforms into the Winograd domain.  One wave per (tile, 64-channel block); lanes are
// consecutive channels (256-B coalesced rows).  out[xi][t][c], xi = (i*NJ + j)*NK + k,
// i < NI = NZ + 2, j < NJ = NY + 2, k < NK = NX + 2.
//   MODE 0:  V = B^T v B over the NI x NJ x NK input tile (zero outside the volume)
//   MODE 1:  A dy A^T over the NZ x NY x NX output-gradient tile (weight gradient)
// All NI*NJ*NK values of a (tile, channel) live in registers (up to 216 at F(4,3)^3; with one wave per
// SIMD the allocator may use the AGPR half of the file).  A form streamed over the z point with the z
// row re-applied to the raw planes (36 live values, 3.7x the loads) measured 2x SLOWER: the kernel is
// bound by vector-memory instructions, not registers.
// Rows t in [T, Tpad) are written as zeros (the TN GEMM contracts over t).
template <int MODE, int NZ, int NY, int NX, bool SPLIT>
__global__ __launch_bounds__(256) void wino_in_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                      const WinoGeom g, const int C) {
  constexpr int NI = NZ + 2, NJ = NY + 2, NK = NX + 2;
  const int lane = threadIdx.x & 63;
  // wave index as a SCALAR: tile origin, bounds tests and row addresses are wave-uniform and run on the SALU (from
  // threadIdx.x >> 6 alone the compiler treats them as divergent: 4 000 VALU instructions of address arithmetic per
  // (tile, 64 channels) in the F(4,3)^3 input transform, more than its loads + transform math)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cblks = C >> 6;
  const long plane0 = 256L * C;           // point stride inside a 256-tile block (see wino_index)
  const long total = (long)g.Tpad * cblks;
  for (long w = blockIdx.x * 4L + wave; w < total; w += gridDim.x * 4L) {
    long plane = plane0;                  // opaque per iteration: otherwise every point offset k * plane becomes a
    asm volatile("" : "+s"(plane));       // 64-bit loop invariant held in registers across the whole loop
    const int t = (int)(w / cblks);
    const int c = (int)(w - (long)t * cblks) * 64 + lane;
    float* o = out + wino_index(t, g.npts, C) + (SPLIT ? c - lane + split_pos(lane) : c);
    float v[NI][NJ][NK];
    if (t >= g.T) {
#pragma unroll
      for (int i = 0; i < NI * NJ * NK; ++i) o[i * plane] = 0.f;
      continue;
    }
    int b, z0, y0, x0;
    tile_origin(g, t, b, z0, y0, x0);
    if (MODE == 0) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int z = z0 + (i - 1) * g.d;
        const bool zo = (z >= 0) & (z < g.D);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int y = y0 + (j - 1) * g.d;
          const bool yo = zo & (y >= 0) & (y < g.H);
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const int x = x0 + (k - 1) * g.d;
            const bool ok = yo & (x >= 0) & (x < g.W);
            const long o = ((((long)b * g.D + z) * g.H + y) * g.W + x) * C + c;
            v[i][j][k] = ok ? in[o] : 0.f;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) btz<NX>(v[i][j]);
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          float col[NJ];
#pragma unroll
          for (int j = 0; j < NJ; ++j) col[j] = v[i][j][k];
          btz<NY>(col);
#pragma unroll
          for (int j = 0; j < NJ; ++j) v[i][j][k] = col[j];
        }
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          float col[NI];
#pragma unroll
          for (int i = 0; i < NI; ++i) col[i] = v[i][j][k];
          btz<NZ>(col);
#pragma unroll
          for (int i = 0; i < NI; ++i) v[i][j][k] = col[i];
        }
    } else {
      float u[NZ][NY][NX];
#pragma unroll
      for (int i = 0; i < NZ; ++i) {
        const int z = z0 + i * g.d;
#pragma unroll
        for (int j = 0; j < NY; ++j) {
          const int y = y0 + j * g.d;
#pragma unroll
          for (int k = 0; k < NX; ++k) {
            const int x = x0 + k * g.d;
            const bool ok = (z < g.D) & (y < g.H) & (x < g.W);
            const long o = ((((long)b * g.D + z) * g.H + y) * g.W + x) * C + c;
            u[i][j][k] = ok ? in[o] : 0.f;
          }
        }
      }
      float p[NZ][NY][NK], q[NZ][NJ][NK];
#pragma unroll
      for (int i = 0; i < NZ; ++i)
#pragma unroll
        for (int j = 0; j < NY; ++j) az<NX>(u[i][j], p[i][j]);
#pragma unroll
      for (int i = 0; i < NZ; ++i)
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          float yy[NY], col[NJ];
#pragma unroll
          for (int j = 0; j < NY; ++j) yy[j] = p[i][j][k];
          az<NY>(yy, col);
#pragma unroll
          for (int j = 0; j < NJ; ++j) q[i][j][k] = col[j];
        }
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          float yy[NZ], col[NI];
#pragma unroll
          for (int i = 0; i < NZ; ++i) yy[i] = q[i][j][k];
          az<NZ>(yy, col);
#pragma unroll
          for (int i = 0; i < NI; ++i) v[i][j][k] = col[i];
        }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < NK; ++k)
          o[((i * NJ + j) * NK + k) * plane] = SPLIT ? split_pack(v[i][j][k], lane & 1) : v[i][j][k];
  }
}

// F(4,3) on all three axes: 216 values per (tile, channel) do not fit beside their temporaries in the 256
// VGPRs of a two-waves-per-SIMD kernel, and with one wave per SIMD (AGPR half of the file) load, compute and
// store phases no longer overlap: 2.7 TB/s where the smaller tilings reach the ~5.3 TB/s of a write-dominated
// HBM stream.  Here a (tile, 64-channel block) is TWO units: unit hx keeps only the x points 3hx .. 3hx + 2
// of every x row as it is loaded (108 live values); both units read the whole tile, the second from L1/L2.
// Addressing: everything about a unit except the lane's channel is WAVE-UNIFORM (tile origin, bounds, row and point
// offsets), so it runs on the scalar unit and the memory instructions are BUFFER loads / stores: a load's per-lane
// offset is ONE v_add (scalar row offset + the lane's channel bytes; a row outside the volume gets an offset beyond
// the descriptor's range and reads 0 in hardware: no select, no mask), a store's lane offset is a constant register
// and its point offset a scalar.  The first form computed 64-bit flat addresses and bounds masks per lane: 4 000 VALU
// instructions per unit, more than its transform arithmetic (~900) -- the kernel was VALU-bound on address math
// (tools/isa_mix.py), not on memory.
// An out-of-volume coordinate contributes 2^30 to the offset instead of its byte offset: windows are < 2^30 bytes
// (wino_size_ok), so a sum with any such term lies beyond the descriptor's range whatever the other terms are -- the
// validity of a row needs no flag and no select, only the two scalar adds of the offset itself (18 scalars per tile;
// with separate flags the scalar state of the unrolled tile spilled into VGPR lanes: 700 v_readlane / v_writelane).
constexpr unsigned WINO_OOB = 0x40000000u;
constexpr int WINO_RSRC_FLAGS = 0x00020000;      // raw buffer, 32-bit data format

// PRO (MODE 0): the input is the PRE-BatchNorm output of the producing convolution and the BatchNorm-apply + ReLU of
// that unit runs here, on the way in (reference med3d.py:121-124 / :153-156: bn, relu, next conv): x -> max(x * scale +
// shift, 0) with bn_apply_kernel's expression, zero outside the volume (the scalar offset says so) -- the activation
// tensor between the two convolutions is never written.
template <int MODE, int HX, bool SPLIT, bool NT, bool PRO = false>
__device__ __forceinline__ void wino_half444(const float* __restrict__ in, float* __restrict__ out, const WinoGeom& g,
                                            const int C, const int cb, const int lane, const int t, const int b,
                                            const int z0, const int y0, const int x0, const float* __restrict__ pscale = nullptr,
                                            const float* __restrict__ pshift = nullptr, const int Cd = 0, const int cofs = 0) {
  // Cd / cofs: the image this source's channels go into has Cd channels per row and they start at channel cofs (a
  // convolution whose input is given as two channel blocks, dram_wino_conv3d_fwd_cat); Cd = 0: the source's own C
  constexpr int NI = 6, NJ = 6, NK = 6;
  float v[NI][NJ][3];
  const int d = g.d;
  // input window: sample b, z planes zb .. zb + nzp - 1
  const int zb = MODE == 0 ? (z0 - d > 0 ? z0 - d : 0) : z0;
  int nzp = (MODE == 0 ? z0 + 4 * d : z0 + 3 * d) + 1 - zb;
  if (nzp > g.D - zb) nzp = g.D - zb;
  if (nzp < 0) nzp = 0;            // a tile of an EMPTY residue sub-lattice (dilation > extent: z0 >= D): nothing in range
  const unsigned row_b = (unsigned)C * 4u, line_b = (unsigned)g.W * row_b, plane_b = (unsigned)g.H * line_b;
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(in) + ((long)b * g.D + zb) * ((long)g.H * g.W * C), 0, (int)(nzp * plane_b), WINO_RSRC_FLAGS);
  const unsigned c4 = (unsigned)(cb + lane) * 4u;
  float psc = 1.f, psh = 0.f;
  if (PRO) { psc = pscale[cb + lane]; psh = pshift[cb + lane]; }
  if (MODE == 0) {
    unsigned yo[NJ], xo[NK];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int y = y0 + (j - 1) * d, x = x0 + (j - 1) * d;
      yo[j] = ((y >= 0) & (y < g.H)) ? (unsigned)y * line_b : WINO_OOB;
      xo[j] = ((x >= 0) & (x < g.W)) ? (unsigned)x * row_b : WINO_OOB;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int z = z0 + (i - 1) * d;
      const unsigned zo = ((z >= 0) & (z < g.D)) ? (unsigned)(z - zb) * plane_b : WINO_OOB;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float row[NK];
        const unsigned zy = zo + yo[j];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const unsigned so = zy + xo[k];
          row[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, (int)(so + c4), 0, 0));
          // Outside the volume the result must be 0, not max(shift, 0).  NO select here: a `cond ? f(x) : 0` per element
          // became 360 v_cndmask on scalar-derived masks, the scheduler then kept every load next to its consumer and
          // the kernel ran with TWO loads in flight (190 s_waitcnt vmcnt in the ISA against 4 in the plain form:
          // 700 us against 477 us on the 2x64x128x128 launch, tools/isa_waits.py).  Arithmetic instead: a scalar 0 / -3e38
          // added to the shift drives max(0 * scale + shift', 0) to 0 for a zero-filled load and leaves shift + 0.0f
          // = shift otherwise (bit-identical to bn_apply_kernel's fma + max).
          // (the 0 / -3e38 term as SCALAR integer arithmetic on the offset's out-of-range bits: written as a float select
          // the compiler moved it to the vector unit again, one v_cndmask per element)
          if (PRO) {
            const unsigned ob = so >> 30;
            const float moff = __builtin_bit_cast(float, (ob < 1u ? ob : 1u) * 0xff61b1e6u);       // 0.0f, or -3.0e38f when out of range
            row[k] = fmaxf(__builtin_fmaf(row[k], psc, psh + moff), 0.f);
          }
        }
        bt4(row);
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) v[i][j][kk] = row[3 * HX + kk];
      }
      // two planes of loads in flight at a time: left alone the scheduler hoists all 216 loads and spills
      if (i & 1) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        float col[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) col[j] = v[i][j][kk];
        bt4(col);
#pragma unroll
        for (int j = 0; j < NJ; ++j) v[i][j][kk] = col[j];
      }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        float col[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) col[i] = v[i][j][kk];
        bt4(col);
#pragma unroll
        for (int i = 0; i < NI; ++i) v[i][j][kk] = col[i];
      }
  } else {
    float p[4][4][3], q2[4][NJ][3];
    unsigned yo[4], xo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int y = y0 + j * d, x = x0 + j * d;
      yo[j] = y < g.H ? (unsigned)y * line_b : WINO_OOB;
      xo[j] = x < g.W ? (unsigned)x * row_b : WINO_OOB;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int z = z0 + i * d;
      const unsigned zo = z < g.D ? (unsigned)(z - zb) * plane_b : WINO_OOB;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float u[4], r[NK];
        const unsigned zy = zo + yo[j];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          u[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, (int)(zy + xo[k] + c4), 0, 0));
        a4(u, r);
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) p[i][j][kk] = r[3 * HX + kk];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        float yy[4], col[NJ];
#pragma unroll
        for (int j = 0; j < 4; ++j) yy[j] = p[i][j][kk];
        a4(yy, col);
#pragma unroll
        for (int j = 0; j < NJ; ++j) q2[i][j][kk] = col[j];
      }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        float yy[4], col[NI];
#pragma unroll
        for (int i = 0; i < 4; ++i) yy[i] = q2[i][j][kk];
        a4(yy, col);
#pragma unroll
        for (int i = 0; i < NI; ++i) v[i][j][kk] = col[i];
      }
  }
  // output: the tile's [point][t % 256][C] block; lane offset constant, point offset scalar
  const int Co = Cd ? Cd : C;
  const unsigned pplane = 256u * (unsigned)Co * 4u;             // bytes between two points of a tile
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out + wino_index(t, g.npts, Co), 0,
                                                                        (int)(216u * pplane), WINO_RSRC_FLAGS);
  const unsigned co4 = (unsigned)(SPLIT ? cofs + cb + split_pos(lane) : cofs + cb + lane) * 4u;
  // the point offset as ONE running scalar (opaque to the optimiser: left alone it precomputes all 108 products
  // point x pplane up front and the scalar file spills into VGPR lanes)
  unsigned so = (unsigned)(3 * HX) * pplane;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        const float val = SPLIT ? split_pack(v[i][j][kk], lane & 1) : v[i][j][kk];
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), rout, (int)co4, (int)so, NT ? 2 : 0);
        so += pplane;
        asm volatile("" : "+s"(so));
      }
      so += 3u * pplane;
      asm volatile("" : "+s"(so));
    }
}

template <int MODE, bool SPLIT, bool NT, bool PRO = false>
__global__ __launch_bounds__(256, 2) void wino_in444_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         const WinoGeom g, const int C,
                                                         const float* __restrict__ pscale = nullptr,
                                                         const float* __restrict__ pshift = nullptr, const int Cd = 0,
                                                         const int cofs = 0) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // scalar: see wino_half444
  const int cblks = C >> 6;
  const long total = (long)g.Tpad * cblks * 2;
  for (long w2 = blockIdx.x * 4L + wave; w2 < total; w2 += gridDim.x * 4L) {
    const int hx = (int)(w2 & 1);          // the two halves of a tile sit in neighbouring waves: shared L1 lines
    const long w = w2 >> 1;
    const int t = (int)(w / cblks);
    const int cb = (int)(w - (long)t * cblks) * 64;
    if (t >= g.T) {                        // padding rows of the GEMM M tile: zeros (the TN GEMM contracts over t)
      const int Co = Cd ? Cd : C;
      const unsigned pplane = 256u * (unsigned)Co * 4u;
      const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out + wino_index(t, g.npts, Co), 0,
                                                                            (int)(216u * pplane), WINO_RSRC_FLAGS);
      const unsigned co4 = (unsigned)(cofs + cb + lane) * 4u;
#pragma unroll
      for (int i = 0; i < 36; ++i)
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
          __builtin_amdgcn_raw_buffer_store_b32(0u, rout, (int)co4, (int)((i * 6 + 3 * hx + kk) * pplane), 0);
      continue;
    }
    int b, z0, y0, x0;
    tile_origin(g, t, b, z0, y0, x0);
    if (hx == 0) wino_half444<MODE, 0, SPLIT, NT, PRO>(in, out, g, C, cb, lane, t, b, z0, y0, x0, pscale, pshift, Cd, cofs);
    else wino_half444<MODE, 1, SPLIT, NT, PRO>(in, out, g, C, cb, lane, t, b, z0, y0, x0, pscale, pshift, Cd, cofs);
  }
}

// ------------------------------------------------------------------------------------------
// Output transform: y(tile) = A^T M A (3-D), + bias, optional fused  += add * (gate > 0)
// (identity-shortcut gradient), per-channel BatchNorm partial sums.  A workgroup owns
// TPB consecutive tiles x 64 channels; stats row = tile block.  One xi_z plane at a time: its
// in-plane A^T . A result is folded into the NZ output planes with the z column of A^T.
// TPB: FOUR tiles per workgroup, one per wave (round 5; 16 before).  On the 16 x 32 x 32 stages 16-tile blocks were 64-256
// workgroups -- an under-filled chip, 2.1-3.3 TB/s -- and on the large grids one tile per wave still streams better than
// four (more workgroups in flight per CU as waves retire at different times): 483 -> 423 us on the 1.8-GB images (5.6 TB/s),
// 59.5 -> 53.0 us on layer1's, 45 -> 30 / 36 -> 17 us on the 256- / 128-channel ones.  Also the number of statistic rows
// (dram_wino_num_stat_rows): 8 192 rows on the largest grids, folded in stages.  -DWINO_TPB=16: A/B build flag.
#ifndef WINO_TPB
#define WINO_TPB 4
#endif
__host__ __device__ inline int wino_tpb(int) { return WINO_TPB; }
__constant__ float c_at4[4][6] = {{1, 1, 1, 1, 1, 0}, {0, 1, -1, 2, -2, 0}, {0, 1, 1, 4, 4, 0}, {0, 1, -1, 8, -8, 1}};   // A^T of F(4,3)

// ADD: 0 plain; 1 `+= add`; 2 `+= add * (gate > 0)` (the shortcut-gradient epilogue) -- compile-time, so that the plane of
// epilogue operands is loaded without a branch in between
// BST (data gradient): the tensor written here is dz of the BatchNorm + ReLU unit in FRONT of this convolution
// (reference med3d.py:121-124 backward); its statistics pass -- g = dz * (y*scale + shift > 0), rows (sum g, sum g*xhat),
// bn.hip colreduce_kernel<1> -- is taken here on the values being stored: one read of that unit's y beside the store
// instead of a pass of its own over dz and y.
struct BnBwdStat { const float* y; const float* mean; const float* invstd; const float* scale; const float* shift; };
// (F(4,3)^3: four workgroups per CU = 128 registers; the statistics form would otherwise take 129 and lose a wave per SIMD)
template <int NZ, int NY, int NX, int ADD = 0, int BST = 0>
__global__ __launch_bounds__(256, (BST && NZ == 4 && NY == 4 && NX == 4) ? 4 : 1) void wino_out_kernel(const float* __restrict__ mh, const float* __restrict__ bias,
                                                       const float* __restrict__ add, const float* __restrict__ gate,
                                                       float* __restrict__ out, float* __restrict__ stats,
                                                       const WinoGeom g, const int N, const BnBwdStat bs) {
  static_assert(!(ADD && BST), "statistics of the unit in front: plain data gradient only");
  constexpr int NI = NZ + 2, NJ = NY + 2, NK = NX + 2;
  __shared__ float red[4][2][64];
  const int lane = threadIdx.x & 63;
  // wave index as a SCALAR: tile origin, bounds tests and row addresses are wave-uniform and run on the SALU (from
  // threadIdx.x >> 6 alone the compiler treats them as divergent: 4 000 VALU instructions of address arithmetic per
  // (tile, 64 channels) in the F(4,3)^3 input transform, more than its loads + transform math)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cblks = N >> 6;
  const int cb = blockIdx.x % cblks, tb = blockIdx.x / cblks;
  const int c = cb * 64 + lane;
  const float bv = bias ? bias[c] : 0.f;
  float s1 = 0.f, s2 = 0.f;
  float bmu = 0.f, bis = 0.f, bsc = 0.f, bsh = 0.f;
  if (BST) { bmu = bs.mean[c]; bis = bs.invstd[c]; bsc = bs.scale[c]; bsh = bs.shift[c]; }
  const int tpb = wino_tpb(g.T);
  for (int q = wave; q < tpb; q += 4) {
    const int t = tb * tpb + q;
    if (t >= g.T) break;
    // the tile's [point][t % 256][N] block of the image: buffer loads, lane offset constant, point offset scalar
    // (wino_half444: no per-lane address arithmetic)
    const unsigned pplane = 256u * (unsigned)N * 4u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(mh) + wino_index(t, g.npts, N), 0, (int)((unsigned)(NI * NJ * NK) * pplane), WINO_RSRC_FLAGS);
    const unsigned c4 = (unsigned)c * 4u;
    float o[NZ][NY][NX];
    constexpr bool ROLLED = NZ == 4 && NY == 4 && NX == 4;
    if (ROLLED) {
      // F(4,3)^3: a rolled loop over the z point keeps one plane of loads (36) in flight per wave and ~140
      // registers; unrolled, the scheduler hoists all 216 loads and the kernel runs one wave per SIMD
#pragma unroll
      for (int a = 0; a < NZ * NY * NX; ++a) (&o[0][0][0])[a] = 0.f;
#pragma unroll 1
      for (int i = 0; i < NI; ++i) {
        float m[NJ][NK], p[NJ][NX], q2[NY][NX];
        const unsigned sp = (unsigned)i * (NJ * NK) * pplane;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int k = 0; k < NK; ++k)
            m[j][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)c4, (int)(sp + (j * NK + k) * pplane),
                                                                                      2));
#pragma unroll
        for (int j = 0; j < NJ; ++j) atz<NX>(m[j], p[j]);
#pragma unroll
        for (int k = 0; k < NX; ++k) {
          float col[NJ], r[NY];
#pragma unroll
          for (int j = 0; j < NJ; ++j) col[j] = p[j][k];
          atz<NY>(col, r);
#pragma unroll
          for (int j = 0; j < NY; ++j) q2[j][k] = r[j];
        }
#pragma unroll
        for (int oz = 0; oz < NZ; ++oz) {
          const float cf = c_at4[oz][i];
#pragma unroll
          for (int j = 0; j < NY; ++j)
#pragma unroll
            for (int k = 0; k < NX; ++k) o[oz][j][k] = __builtin_fmaf(cf, q2[j][k], o[oz][j][k]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < (ROLLED ? 0 : NI); ++i) {
      float m[NJ][NK], p[NJ][NX], q2[NY][NX];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < NK; ++k)
          m[j][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)c4, (int)(((i * NJ + j) * NK + k) * pplane), 0));
#pragma unroll
      for (int j = 0; j < NJ; ++j) atz<NX>(m[j], p[j]);
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        float col[NJ], r[NY];
#pragma unroll
        for (int j = 0; j < NJ; ++j) col[j] = p[j][k];
        atz<NY>(col, r);
#pragma unroll
        for (int j = 0; j < NY; ++j) q2[j][k] = r[j];
      }
#pragma unroll
      for (int oz = 0; oz < NZ; ++oz) {
        const float cf = at_coef<NZ>(oz, i);
        if (cf != 0.f) {
#pragma unroll
          for (int j = 0; j < NY; ++j)
#pragma unroll
            for (int k = 0; k < NX; ++k) {
              if (i == 0 || (i == 1 && oz > 0)) o[oz][j][k] = cf * q2[j][k];     // first contribution to this plane
              else o[oz][j][k] = __builtin_fmaf(cf, q2[j][k], o[oz][j][k]);
            }
        }
      }
    }
    int b, z0, y0, x0;
    tile_origin(g, t, b, z0, y0, x0);
    // output window: sample b, z planes from z0 (descriptors on out / add / gate with the same offsets)
    const unsigned row_b = (unsigned)N * 4u, line_b = (unsigned)g.W * row_b, plane_b = (unsigned)g.H * line_b;
    int nzp = (NZ - 1) * g.d + 1;
    if (nzp > g.D - z0) nzp = g.D - z0;
    if (nzp < 0) nzp = 0;          // (tile of an empty residue sub-lattice: every store below is guarded out as well)
    const long wbase = ((long)b * g.D + z0) * ((long)g.H * g.W * N);
    const int wbytes = (int)((unsigned)nzp * plane_b);
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out + wbase, 0, wbytes, WINO_RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t radd =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(add ? add : out) + wbase, 0, wbytes, WINO_RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rgate =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gate ? gate : out) + wbase, 0, wbytes, WINO_RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rbn =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(BST ? bs.y : out) + wbase, 0, wbytes, WINO_RSRC_FLAGS);
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      const int z = z0 + i * g.d;
      float yv[BST ? NY : 1][BST ? NX : 1];
      if (BST) {                   // the plane of y values, back to back like the shortcut-gradient operands below
#pragma unroll
        for (int j = 0; j < NY; ++j) {
          const int y = y0 + j * g.d;
#pragma unroll
          for (int k = 0; k < NX; ++k) {
            const int x = x0 + k * g.d;
            const bool ok = (z < g.D) & (y < g.H) & (x < g.W);                                               // wave-uniform
            const unsigned so = ok ? (unsigned)(i * g.d) * plane_b + (unsigned)y * line_b + (unsigned)x * row_b : WINO_OOB;
            yv[BST ? j : 0][BST ? k : 0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rbn, (int)c4, (int)so, 0));
          }
        }
      }
      // shortcut-gradient operands of the whole output plane first (up to 2 x NY x NX loads in flight), then the
      // arithmetic and the stores: with each load next to its use the epilogue ran one or two loads at a time -- the
      // three 512-channel data-gradient launches of config 1 took 186 us for 427 MB (2.3 TB/s) where the plain ones of
      // the same size stream at 4.5-5 TB/s, and ResNet-34 / -50 have one such launch per identity block
      float av[ADD ? NY : 1][ADD ? NX : 1], gv[ADD ? NY : 1][ADD ? NX : 1];
      if (ADD) {
#pragma unroll
        for (int j = 0; j < NY; ++j) {
          const int y = y0 + j * g.d;
#pragma unroll
          for (int k = 0; k < NX; ++k) {
            const int x = x0 + k * g.d;
            // NO branch around the loads (a wave-uniform `if` per element keeps each load next to its use: the plane's
            // loads must be issued back to back): an out-of-volume element gets an offset beyond the descriptor's range
            // and reads 0 in hardware (its result is never stored)
            const bool ok = (z < g.D) & (y < g.H) & (x < g.W);                                               // wave-uniform
            const unsigned so = ok ? (unsigned)(i * g.d) * plane_b + (unsigned)y * line_b + (unsigned)x * row_b : WINO_OOB;
            av[ADD ? j : 0][ADD ? k : 0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(radd, (int)c4, (int)so, 0));
            gv[ADD ? j : 0][ADD ? k : 0] = ADD == 2 ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rgate, (int)c4, (int)so, 0)) : 1.f;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NY; ++j) {
        const int y = y0 + j * g.d;
#pragma unroll
        for (int k = 0; k < NX; ++k) {
          const int x = x0 + k * g.d;
          if ((z < g.D) & (y < g.H) & (x < g.W)) {          // wave-uniform
            const int so = (int)((unsigned)(i * g.d) * plane_b + (unsigned)y * line_b + (unsigned)x * row_b);   // scalar
            float v = o[i][j][k] + bv;
            if (ADD) v += gv[ADD ? j : 0][ADD ? k : 0] > 0.f ? av[ADD ? j : 0][ADD ? k : 0] : 0.f;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, (int)c4, so, 0);
            if (BST) {             // (the expressions of colreduce_kernel<1>: mask re-derived with the forward's own fma)
              const float yy = yv[BST ? j : 0][BST ? k : 0];
              const float gg = __builtin_fmaf(yy, bsc, bsh) > 0.f ? v : 0.f;
              s1 += gg;
              s2 += gg * ((yy - bmu) * bis);
            } else {
              s1 += v;
              s2 += v * v;
            }
          }
        }
      }
    }
  }
  if (stats) {
    red[wave][0][lane] = s1;
    red[wave][1][lane] = s2;
    __syncthreads();
    if (threadIdx.x < 128) {
      const int which = threadIdx.x >> 6;
      const float v = red[0][which][lane] + red[1][which][lane] + red[2][which][lane] + red[3][which][lane];
      stats[((long)tb * 2 + which) * N + c] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Weight transform  U = G w G^T (3-D), streamed over the z point (9 + 36 live values).  The launches that cost are
// the 256- and 512-channel layers, bound by writing 216 / 27 x the weight tensor twice (226 MB per direction at
// 512 x 512); one z point per workgroup (6x the workgroups for the 64 x 64 layers) re-reads w six times with 108-byte
// lane strides and measured 42 -> 62 us per launch on average.
//   blockIdx.y == 0: uf[xi][co][ci]               (forward B operand, K = ci contiguous)
//   blockIdx.y == 1: ub[xi][ci][co], taps flipped  (data-gradient B operand, K = co contiguous)
template <int NZ, int NY, int NX>
__global__ __launch_bounds__(256) void wino_weight_kernel(const float* __restrict__ w, float* __restrict__ uf,
                                                          float* __restrict__ ub, const int Cout, const int Cin,
                                                          const int split) {
  constexpr int NI = NZ + 2, NJ = NY + 2, NK = NX + 2;
  const bool bwd = blockIdx.y == 1;
  float* dst = bwd ? ub : uf;
  if (!dst) return;
  const long n = (long)Cout * Cin;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= n) return;
  int co, ci;
  if (!bwd) { ci = (int)(i % Cin); co = (int)(i / Cin); }
  else { co = (int)(i % Cout); ci = (int)(i / Cout); }
  const float* src = w + ((long)co * Cin + ci) * 27;
  const int lane = threadIdx.x & 63;       // == K index mod 64 (K = the contiguous dimension, a multiple of 64)
  const long io = split ? i - lane + split_pos(lane) : i;
  float gw[3][3][3];
#pragma unroll
  for (int a = 0; a < 27; ++a) (&gw[0][0][0])[a] = src[bwd ? 26 - a : a];
#pragma unroll
  for (int a = 0; a < NI; ++a) {
    float r[3][3], p[3][NK], u[NJ][NK];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
        r[ky][kx] = g_coef<NZ>(a, 0) * gw[0][ky][kx] + g_coef<NZ>(a, 1) * gw[1][ky][kx] + g_coef<NZ>(a, 2) * gw[2][ky][kx];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) gz<NX>(r[ky], p[ky]);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const float col[3] = {p[0][k], p[1][k], p[2][k]};
      float rr[NJ];
      gz<NY>(col, rr);
#pragma unroll
      for (int j = 0; j < NJ; ++j) u[j][k] = rr[j];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int k = 0; k < NK; ++k)
        dst[((long)(a * NJ + j) * NK + k) * n + io] = split ? split_pack(u[j][k], lane & 1) : u[j][k];
  }
}

// dw[co][ci][27] = G^T (sum over splits of slab[split][xi][co][ci]) G   (3-D), fixed order.
// One workgroup = 64 (co, ci) elements x 8 point groups (512 threads): every thread sums every 8th of
// the NP points over the splits (coalesced over elements); then wave a transforms z plane a in x and y (G^T . G of a
// 6 x 6 plane -> 3 x 3), waves 0..2 the z columns, and all threads store the 64 x 27 results as ONE contiguous run.
// (The first version left all of G^T . G . G to one wave per workgroup -- 630 flops and 216 LDS reads per lane in
// 128 registers: 48 spilled -- and stored 27 floats per lane 108 bytes apart.)
template <int NZ, int NY, int NX>
__global__ __launch_bounds__(512) void wino_wgrad_out_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                               const int Cout, const int Cin, const int nsplit) {
  constexpr int NI = NZ + 2, NJ = NY + 2, NK = NX + 2, NP = NI * NJ * NK;
  __shared__ float us[NP][64];
  __shared__ float qs[NI][9][64];
  __shared__ float rs[64][28];
  const long n = (long)Cout * Cin;
  const int e = threadIdx.x & 63, gq = threadIdx.x >> 6;
  const long i = blockIdx.x * 64L + e;   // (co, ci), ci fastest
  constexpr int PPT = NP / 8;            // points per thread (NP is a multiple of 8 for every tiling)
  static_assert(NP % 8 == 0 && NI <= 8, "points per group; one wave per z plane");
  float acc[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) acc[j] = 0.f;
  if (i < n)
    for (int sp = 0; sp < nsplit; ++sp) {   // splits in order (deterministic); the PPT loads of a split are independent
#pragma unroll
      for (int j = 0; j < PPT; ++j) acc[j] += slab[((long)sp * NP + gq + 8 * j) * n + i];
    }
#pragma unroll
  for (int j = 0; j < PPT; ++j) us[gq + 8 * j][e] = acc[j];
  __syncthreads();
  if (gq < NI) {                          // plane a = gq: x then y
    const int a = gq;
    float p[NJ][3];
#pragma unroll
    for (int b = 0; b < NJ; ++b) {
      float row[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) row[k] = us[(a * NJ + b) * NK + k][e];
      gtz<NX>(row, p[b]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float col[NJ], rr[3];
#pragma unroll
      for (int b = 0; b < NJ; ++b) col[b] = p[b][k];
      gtz<NY>(col, rr);
      qs[a][0 * 3 + k][e] = rr[0]; qs[a][1 * 3 + k][e] = rr[1]; qs[a][2 * 3 + k][e] = rr[2];
    }
  }
  __syncthreads();
  if (gq < 3) {                           // z columns (j = gq, k = 0..2)
    const int j = gq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float col[NI], rr[3];
#pragma unroll
      for (int a = 0; a < NI; ++a) col[a] = qs[a][j * 3 + k][e];
      gtz<NZ>(col, rr);
      rs[e][0 * 9 + j * 3 + k] = rr[0]; rs[e][1 * 9 + j * 3 + k] = rr[1]; rs[e][2 * 9 + j * 3 + k] = rr[2];
    }
  }
  __syncthreads();
  const long base = blockIdx.x * 64L * 27, lim = n * 27;
  for (int idx = threadIdx.x; idx < 64 * 27; idx += 512)
    if (base + idx < lim) dw[base + idx] = rs[idx / 27][idx % 27];
}

// ------------------------------------------------------------------------------------------
// host side
// instantiated tilings (z, y, x outputs per tile): 2x2x2, 4x2x2, 4x4x2, 4x4x4
#define WINO_TILING_DISPATCH(g_, CALL_)                                 \
  do {                                                                  \
    if ((g_).nz == 4 && (g_).ny == 4 && (g_).nx == 4) { CALL_(4, 4, 4); } \
    else if ((g_).nz == 4 && (g_).ny == 4) { CALL_(4, 4, 2); }          \
    else if ((g_).nz == 4) { CALL_(4, 2, 2); }                          \
    else { CALL_(2, 2, 2); }                                            \
  } while (0)
// Arithmetic of the Winograd-domain GEMMs, DRAM_MATH = "f32" (default: fp32 MFMA) | "bf16x3" (split-bf16
// operands, three bf16 MFMA products per fp32 product, ~2^-16 per product) | "bf16" (bf16 operands, fp32
// accumulation).  Read per call, like the other overrides: tests switch it between cases.
int math_mode() {
  const char* e = tune_env("DRAM_MATH");
  if (!e) return 0;
  if (!strcmp(e, "bf16x3")) return 1;
  if (!strcmp(e, "bf16")) return 2;
  return 0;
}

bool wino_geom_ok(const DramConvDesc* d) {
  if (!d) return false;
  if (d->B < 1 || d->D < 1 || d->H < 1 || d->W < 1) return false;
  if (d->k != 3 || d->stride != 1 || d->dil < 1 || d->pad != d->dil) return false;
  if (d->Do != d->D || d->Ho != d->H || d->Wo != d->W) return false;
  if (d->Cin < 64 || d->Cout < 64 || d->Cin % 64 != 0 || d->Cout % 64 != 0) return false;
  return true;
}

// Tiling (outputs per tile along z, y, x): the cheapest of the instantiated 4x4x4 / 4x4x2 / 4x2x2 / 2x2x2 by
// points x rows (see pick_tiling), among those that leave two GEMM M tiles per point.
long long tiles_for(const DramConvDesc* d, int nz, int ny, int nx) {
  const int dd = d->dil;
  auto tiles = [&](int n, int per) { return (long long)(((n + dd - 1) / dd + per - 1) / per); };
  return (long long)d->B * dd * dd * dd * tiles(d->D, nz) * tiles(d->H, ny) * tiles(d->W, nx);
}

// instantiated tilings: 4x4x4, 4x4x2, 4x2x2, 2x2x2;  DRAM_WINO_TILING = "z,y,x" forces one (tests)
void pick_tiling(const DramConvDesc* d, const int pass, int& nz, int& ny, int& nx) {
  static const int cand[4][3] = {{4, 4, 4}, {4, 4, 2}, {4, 2, 2}, {2, 2, 2}};
  if (const char* e = tune_env("DRAM_WINO_TILING")) {
    int a = 0, b = 0, c = 0;
    if (sscanf(e, "%d,%d,%d", &a, &b, &c) == 3)
      for (int i = 0; i < 4; ++i)
        if (cand[i][0] == a && cand[i][1] == b && cand[i][2] == c) { nz = a; ny = b; nx = c; return; }
  }
  if (math_mode() == 2) { nz = ny = nx = 2; return; }   // bf16 operands: F(4,3) amplifies their 2^-9 rounding 3-17x
  // (pass is kept for per-pass choices; since the 216-value transform runs as two half-tile units --
  // wino_in444_kernel -- F(4,3) on all three axes wins wherever the extents allow it.  Measured, 4x4x4 vs
  // 4x4x2 tiles, fwd / dgrad / wgrad ms: 128->64 @ 2x64x128x128 3.39 / 3.13 / 3.51 vs 3.45 / 3.51 / 3.66;
  // 576->64 @ 2x32x64x64 1.66 / 1.39 / 1.70 vs 1.75 / 1.71 / 1.69; 256->256 dil 2 0.27 / 0.26 / 0.33 vs
  // 0.33 / 0.31 / 0.34.)
  (void)pass;
  // Cost of a tiling = Winograd points x (GEMM rows actually computed = tiles padded to the 256-row M tile, plus
  // the real tiles the transforms touch).  A sub-lattice extent that is not a multiple of 4 no longer rules
  // F(4,3) out on that axis: its edge tiles are simply ragged (zero-filled loads, guarded stores), and e.g. the
  // reference's default 128x224x288 volume (16x28x36 at stride 8: sub-lattice extents 7 and 9 under dilation 4)
  // is cheaper on 4x4x4 tiles with padding (6 tiles x 216 points per lattice) than on 4x2x2 (20 x 96).  A tiling
  // must still leave two GEMM M tiles per point (small volumes keep the finer tiling); ties go to the larger tile.
  long long best = -1;
  int bi = 3;
  for (int i = 0; i < 4; ++i) {
    const long long T = tiles_for(d, cand[i][0], cand[i][1], cand[i][2]);
    const long long Tpad = (T + 255) / 256 * 256;
    if (i < 3 && Tpad < 512) continue;
    const long long cost = (long long)(cand[i][0] + 2) * (cand[i][1] + 2) * (cand[i][2] + 2) * (Tpad + T);
    if (best < 0 || cost < best) { best = cost; bi = i; }
  }
  nz = cand[bi][0]; ny = cand[bi][1]; nx = cand[bi][2];
}

WinoGeom make_geom(const DramConvDesc* d, const int pass = 0) {   // pass: 0 forward, 1 data gradient, 2 weight gradient
  WinoGeom g{};
  g.B = d->B; g.D = d->D; g.H = d->H; g.W = d->W; g.d = d->dil;
  pick_tiling(d, pass, g.nz, g.ny, g.nx);
  g.npts = (g.nz + 2) * (g.ny + 2) * (g.nx + 2);
  auto tiles = [&](int n, int per) { return ((n + g.d - 1) / g.d + per - 1) / per; };
  g.Tz = tiles(g.D, g.nz); g.Ty = tiles(g.H, g.ny); g.Tx = tiles(g.W, g.nx);
  const long long T = (long long)g.B * g.d * g.d * g.d * g.Tz * g.Ty * g.Tx;
  g.T = (int)T;
  g.Tpad = (int)((T + 255) / 256 * 256);
  return g;
}

bool wino_size_ok(const DramConvDesc* d) {   // int32 offsets inside one xi plane of the GEMM operands
  const long long cmax = d->Cin > d->Cout ? d->Cin : d->Cout;
  for (int pass = 0; pass < 2; ++pass) {
    const WinoGeom g = make_geom(d, pass);
    const long long T = (long long)g.B * g.d * g.d * g.d * g.Tz * g.Ty * g.Tx;
    if (!(T > 0 && (T + 255) * cmax < (1LL << 31))) return false;
  }
  // buffer-addressed transforms: a tile's window of input z planes (5 dil + 1 planes), the 216-point block of one tile
  // and its window of output planes each lie below 2^30 bytes (WINO_OOB)
  const long long plane_b = (long long)d->H * d->W * cmax * 4;
  if ((5LL * d->dil + 1) * plane_b >= (1LL << 30) || 216LL * 256 * cmax * 4 >= (1LL << 30)) return false;
  return true;
}


int grid_for(long waves) {
  long b = (waves + 3) / 4;
  return (int)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

// tile transform into the Winograd domain (MODE 0: B^T x B, MODE 1: A dy A^T), fp32 or split-bf16 image.  The fp32
// F(4,3)^3 images are written once and read once: streaming (non-temporal) cache policy on the input transform's
// stores and the output transform's loads.
template <int MODE>
int launch_wino_in(const float* src, float* dst, const WinoGeom& g, const int C, const int math, hipStream_t s,
                   const float* pscale = nullptr, const float* pshift = nullptr, const int Cd = 0, const int cofs = 0) {
  const long units = (long)g.Tpad * (C / 64);
  // (a source that fills a channel range of a wider image: the F(4,3)^3 transform's fp32 form only)
  if (Cd && (math || !(g.nz == 4 && g.ny == 4 && g.nx == 4) || C % 64 || cofs % 64 || cofs + C > Cd)) return DRAM_ERR_UNSUPPORTED;
  if (pscale) {                                  // BatchNorm-apply + ReLU prologue: the F(4,3)^3 input transform only
    if (MODE != 0 || math || !pshift || !(g.nz == 4 && g.ny == 4 && g.nx == 4)) return DRAM_ERR_UNSUPPORTED;
    const double in_elems = (double)g.B * g.D * g.H * g.W * C;
    DramProf prof(DRAM_FAM_WINO_IN, 9444, 0.0, 4.0 * (in_elems + (double)g.npts * g.Tpad * C), s);
    if constexpr (MODE == 0) {
      hipLaunchKernelGGL((wino_in444_kernel<0, false, true, true>), dim3(grid_for(2 * units)), dim3(256), 0, s, src, dst, g, C, pscale, pshift, Cd, cofs);
    }
    DRAM_LAUNCH_CHECK();
    return DRAM_OK;
  }
  // algorithmic bytes: the activation read once + the Winograd-domain image written once
  const double in_elems = (double)g.B * g.D * g.H * g.W * C;
  DramProf prof(DRAM_FAM_WINO_IN, MODE * 1000 + g.nz * 100 + g.ny * 10 + g.nx, 0.0,
                4.0 * (in_elems + (double)g.npts * g.Tpad * C), s);
  if (g.nz == 4 && g.ny == 4 && g.nx == 4) {     // two half-tile units per tile (wino_in444_kernel)
    if (math) hipLaunchKernelGGL((wino_in444_kernel<MODE, true, false>), dim3(grid_for(2 * units)), dim3(256), 0, s, src, dst, g, C, nullptr, nullptr, 0, 0);
    else hipLaunchKernelGGL((wino_in444_kernel<MODE, false, true>), dim3(grid_for(2 * units)), dim3(256), 0, s, src, dst, g, C, nullptr, nullptr, Cd, cofs);
    DRAM_LAUNCH_CHECK();
    return DRAM_OK;
  }
#define W_IN1(NZ_, NY_, NX_)                                                                                       \
  do {                                                                                                             \
    if (math)                                                                                                      \
      hipLaunchKernelGGL((wino_in_kernel<MODE, NZ_, NY_, NX_, true>), dim3(grid_for(units)), dim3(256), 0, s, src, dst, g, C);  \
    else                                                                                                           \
      hipLaunchKernelGGL((wino_in_kernel<MODE, NZ_, NY_, NX_, false>), dim3(grid_for(units)), dim3(256), 0, s, src, dst, g, C); \
  } while (0)
  if (g.nz == 4 && g.ny == 4) W_IN1(4, 4, 2);
  else if (g.nz == 4) W_IN1(4, 2, 2);
  else W_IN1(2, 2, 2);
#undef W_IN1
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

// shared by forward (x, uf) and data gradient (dy, ub): in[..., K] -> out[..., N]
int run_conv(const float* in, const float* U, const float* bias, const float* add, const float* gate, float* out,
             float* stats, float* v_keep, const DramConvDesc* d, int pass, int K, int N, void* ws, size_t ws_bytes,
             hipStream_t s, const float* pscale = nullptr, const float* pshift = nullptr, const float* in1 = nullptr,
             const int C0 = 0, const BnBwdStat bst = BnBwdStat{nullptr, nullptr, nullptr, nullptr, nullptr}) {
  const WinoGeom g = make_geom(d, pass);
  if (bst.y && (add || gate || !stats)) return DRAM_ERR_BAD_ARG;
  const size_t need = (size_t)g.npts * g.Tpad * ((size_t)K + N) * sizeof(float);
  if (!ws || ws_bytes < need) return DRAM_ERR_WORKSPACE;
  float* V = v_keep ? v_keep : (float*)ws;          // kept for the weight gradient when the caller asks
  float* Mh = (float*)ws + (size_t)g.npts * g.Tpad * K;
  const int math = math_mode();
  if (in1) {
    // input given as two channel blocks [in: C0 | in1: K - C0] (pass 0 only): two transforms into one image
    int rc0 = launch_wino_in<0>(in, V, g, C0, math, s, nullptr, nullptr, K, 0);
    if (rc0 == DRAM_OK) rc0 = launch_wino_in<0>(in1, V, g, K - C0, math, s, nullptr, nullptr, K, C0);
    if (rc0 != DRAM_OK) return rc0;
  } else {
    const int rc0 = launch_wino_in<0>(in, V, g, K, math, s, pscale, pshift);
    if (rc0 != DRAM_OK) return rc0;
  }
  const int rc = run_nn(V, U, Mh, g, N, K, s, GemmEpilogue{nullptr, nullptr, nullptr, nullptr}, math,
                        !(pass == 1 && (d->flags & DRAM_CONV_BWD_OVERLAPPED)));
  if (rc != DRAM_OK) return rc;
  const int ntb = (g.T + wino_tpb(g.T) - 1) / wino_tpb(g.T);
  const double out_elems = (double)g.B * g.D * g.H * g.W * N;
  DramProf prof(DRAM_FAM_WINO_OUT, g.nz * 100 + g.ny * 10 + g.nx, 0.0,
                4.0 * ((double)g.npts * g.Tpad * N + out_elems * (1 + (add ? 1 : 0) + (gate ? 1 : 0) + (bst.y ? 1 : 0))), s);
#define W_OUT(NZ_, NY_, NX_)                                                                                              \
  do {                                                                                                                    \
    if (add && gate)                                                                                                      \
      hipLaunchKernelGGL((wino_out_kernel<NZ_, NY_, NX_, 2>), dim3(ntb * (N / 64)), dim3(256), 0, s, Mh, bias, add,          \
                         gate, out, stats, g, N, bst);                                                                    \
    else if (add)                                                                                                         \
      hipLaunchKernelGGL((wino_out_kernel<NZ_, NY_, NX_, 1>), dim3(ntb * (N / 64)), dim3(256), 0, s, Mh, bias, add,          \
                         gate, out, stats, g, N, bst);                                                                    \
    else if (bst.y)                                                                                                       \
      hipLaunchKernelGGL((wino_out_kernel<NZ_, NY_, NX_, 0, 1>), dim3(ntb * (N / 64)), dim3(256), 0, s, Mh, bias, add,       \
                         gate, out, stats, g, N, bst);                                                                    \
    else                                                                                                                  \
      hipLaunchKernelGGL((wino_out_kernel<NZ_, NY_, NX_, 0>), dim3(ntb * (N / 64)), dim3(256), 0, s, Mh, bias, add,          \
                         gate, out, stats, g, N, bst);                                                                    \
  } while (0)
  WINO_TILING_DISPATCH(g, W_OUT);
#undef W_OUT
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
extern "C" int dram_wino_applicable(const DramConvDesc* d) {
  return (wino_geom_ok(d) && wino_size_ok(d)) ? 1 : 0;
}

// Plan: a cost model calibrated on one MI355X (rocprofv3, round 1).  The direct implicit GEMM
// runs at ~135 TFLOP/s; the Winograd pipeline costs, per voxel of the padded tile grid, the
// input transform (36 B x K at ~4.9 TB/s), the 64 GEMMs (16 K N flops at ~118 TFLOP/s, or their
// 32 (K + N) B of operand traffic at ~4.7 TB/s, whichever is larger) and the output transform
// (36 B x N at ~3.4 TB/s).  Forward and data gradient (K and N swapped) are averaged; Winograd is
// planned when it is at least 8 % cheaper.  DRAM_CONV_ALGO: 0/unset auto, 1 always direct,
// 2 Winograd wherever applicable (tests).
// Small volumes underfill the chip: a launch of `wgs` workgroups on `slots` resident slots runs at
// wgs / (rounds * slots) of the steady-state rate.
static double fill(double wgs, double slots) {
  if (wgs < 1.0) wgs = 1.0;
  const double rounds = (double)(long)((wgs + slots - 1.0) / slots);
  return wgs / (rounds * slots);
}
// per voxel of the padded tile grid; pv = Winograd points per output voxel (8 for F(2,3)^3, 6 with F(4,3) along z)
static double wino_cost_per_voxel(double K, double N, double tpad, double npts, double pv) {
  const double nt = (double)(long)((N + 255.0) / 256.0);           // 256-column GEMM tiles (fewer columns: one tile)
  const double gemm = 2.0 * pv * K * N / (118e12 * fill(npts * (tpad / 256.0) * nt, 256.0));
  const double traffic = 4.0 * pv * (K + N) / 4.7e12;
  const double in_rate = npts > 200.0 ? 4.0e12 : 4.9e12;     // the 216-value transform reads its tile twice (half-tile units)
  return (4.0 + 4.0 * pv) * K / in_rate + (gemm > traffic ? gemm : traffic) + (4.0 + 4.0 * pv) * N / 3.4e12;
}
// direct implicit GEMM: 8x8x8 / 4x8x8 output tiles x 64..256 columns, two workgroups per CU
static double direct_rate(const DramConvDesc* d, double N) {
  const double lat = d->dil;
  const double sz = (double)(long)((d->D + lat - 1) / lat), sy = (double)(long)((d->H + lat - 1) / lat),
               sx = (double)(long)((d->W + lat - 1) / lat);
  const double mt = d->B * lat * lat * lat * (double)(long)((sz + 3) / 4) * (double)(long)((sy + 7) / 8) *
                    (double)(long)((sx + 7) / 8);
  return 135e12 * fill(mt * (double)(long)((N + 127.0) / 128.0), 512.0);
}

extern "C" int dram_conv_algo(const DramConvDesc* d) {
  const char* v = tune_env("DRAM_CONV_ALGO");   // read per call: tests switch it between cases
  const int algo = v ? atoi(v) : 0;
  if (algo == 1) return 0;
  if (dram_conv1x1_applicable(d)) return 3;                              // 1x1x1: plain GEMM on the batched-GEMM kernels
  const bool w3 = dram_wino_applicable(d) != 0, w2 = dram_wino2d_applicable(d) != 0;
  if (algo == 2) return w3 ? 1 : 0;
  if (algo == 3) return w2 ? 2 : 0;
  const double vox = d ? (double)d->B * d->D * d->H * d->W : 0.0;
  double best = 1e30;
  int pick = 0;
  if (w3) {
    const WinoGeom g = make_geom(d, 0), gb = make_geom(d, 1);     // forward / data-gradient tilings
    if (g.T >= 128) {
      const double vpad = (double)g.nz * g.ny * g.nx * g.Tpad, pv = g.npts / ((double)g.nz * g.ny * g.nx);
      const double vpadb = (double)gb.nz * gb.ny * gb.nx * gb.Tpad, pvb = gb.npts / ((double)gb.nz * gb.ny * gb.nx);
      const double direct = vox * 54.0 * d->Cin * d->Cout * 0.5 *
                            (1.0 / direct_rate(d, d->Cout) + 1.0 / direct_rate(d, d->Cin));
      const double wino = 0.5 * (vpad * wino_cost_per_voxel(d->Cin, d->Cout, g.Tpad, g.npts, pv) +
                                 vpadb * wino_cost_per_voxel(d->Cout, d->Cin, gb.Tpad, gb.npts, pvb));
      if (wino < 0.92 * direct) { best = wino; pick = 1; }
    }
  }
  if (w2 && d->D >= 12 && vox >= 65536.0) {
    // fused in-plane Winograd: measured ~200 TFLOP/s of direct-conv-equivalent work with 64-column
    // tiles, ~155 with 32-column tiles (forward writes Cout columns, data gradient Cin columns)
    const int zt = (d->D + 15) / 16 * 16;
    const double rf = d->Cout % 64 == 0 ? 200e12 : 155e12, rb = d->Cin % 64 == 0 ? 200e12 : 155e12;
    const double w2d = vox * zt / d->D * 54.0 * d->Cin * d->Cout * 0.5 * (1.0 / rf + 1.0 / rb);
    const double direct = vox * 54.0 * d->Cin * d->Cout / 135e12;
    // the fused kernel needs no workspace (the pipeline: 2 x 3.4-4.5x the activation bytes) and its F(2x2) transforms
    // round 10x less than F(4,3)^3 (1e-6 against 1.1e-5 per layer); rounds 1-3 let it keep a layer unless the pipeline
    // was estimated > 15 % faster.  Round 4: with the streaming Winograd-domain GEMM the pipeline measures 1.89 / 1.80
    // ms against 2.09 / 1.92 fused on 64->64 @ 2x64x128x128 (0.270 / 0.276 against 0.294 / 0.288 at 32x64x64) and
    // hands its transformed input to the weight gradient (1.59 against 1.83 ms).  The cheaper estimate now wins on the
    // LAST decoder stage (D >= 64: its rounding reaches the output un-amplified), not below it: with layer1 / us1 of
    // ResNet-50 on the pipeline the full-size dRAM volumes sit 1.47e-3 from the fp64 oracle (bar 1e-3; 54 BatchNorm
    // layers amplify an early error), with the margin kept there they pass as before.
    // Round 5: the caller may say that its network amplifies a layer's rounding little (DRAM_CONV_ROUNDING_TOLERANT: the
    // BasicBlock ResNets -- full-size outputs 6.0e-5 / 1.9e-4 from the fp64 oracle with every 64->64 layer on F(4,3)^3):
    // the cheaper estimate then wins everywhere (config 1: 39.6 -> 38.5 ms).
    const bool tolerant = (d->flags & DRAM_CONV_ROUNDING_TOLERANT) != 0;
    const double margin = (d->D >= 64 || tolerant) ? 1.0 : 1.15;
    if (w2d < 0.92 * direct && w2d < margin * best) { best = w2d; pick = 2; }
  }
  return pick;
}

constexpr double W2D_WGRAD_RATE = 240e12;   // measured 197-257 TFLOP/s direct-equivalent (round 1)

// Weight-gradient plan (independent of the forward plan: the fused in-plane kernel has no weight
// gradient of its own): 1 = Winograd TN pipeline (dram_wino_conv3d_bwd_weight), 0 = direct.
// Cost per voxel: both tile transforms (36 B x (Cin + Cout) at ~4.9 TB/s) + the 64 TN GEMMs
// (16 Cin Cout flops at ~125 TFLOP/s or their 32 (Cin + Cout) B of operands at ~4.7 TB/s).
extern "C" int dram_conv_wgrad_algo(const DramConvDesc* d) {
  const char* v = tune_env("DRAM_CONV_ALGO");
  const int algo = v ? atoi(v) : 0;
  if (algo == 1) return 0;
  if (dram_conv1x1_applicable(d)) return 3;
  const bool w3 = dram_wino_applicable(d) != 0, w2 = dram_wgrad_w2d_applicable(d) != 0;
  if (algo == 2) return w3 ? 1 : 0;
  if (algo == 3) return w2 ? 2 : 0;
  if (!d) return 0;
  const double vox = (double)d->B * d->D * d->H * d->W;
  const double K = d->Cin, N = d->Cout;
  const double direct = vox * 54.0 * K * N / 125e12;
  double best = 1e30;
  int pick = 0;
  if (w3) {
    const WinoGeom g = make_geom(d);
    if (g.T >= 128) {
      const double vpad = (double)g.nz * g.ny * g.nx * g.Tpad, pv = g.npts / ((double)g.nz * g.ny * g.nx);
      TnPlan tp;
      plan_tn(d, g, tp);
      const double wgs = (double)g.npts * tp.m_tiles * tp.n_tiles * tp.nsplit;
      const double gemm = 2.0 * pv * K * N / (125e12 * fill(wgs, 256.0)), traffic = 4.0 * pv * (K + N) / 4.7e12;
      // (a layer whose FORWARD runs the pipeline hands over its transformed input: only dy is transformed here)
      const double kx = dram_conv_algo(d) == 1 ? 0.0 : K;
      const double wino = vpad * ((4.0 + 4.0 * pv) * (kx + N) / 4.9e12 + (gemm > traffic ? gemm : traffic));
      // the direct weight gradient splits over voxel chunks, so it keeps the chip full down to ~16k voxels
      const double dfill = vox >= 16384.0 ? 1.0 : vox / 16384.0;
      if (wino < 0.85 * direct / dfill) { best = wino; pick = 1; }
    }
  }
  if (w2 && d->D >= 8 && vox >= 65536.0) {
    const double w2d = vox * 54.0 * K * N / W2D_WGRAD_RATE;     // direct-equivalent rate, measured
    // No preference margin here (the forward plan keeps the z-walking kernel at D < 64 for its smaller rounding
    // error, which a weight gradient does not hand on to any other layer): the cheaper estimate wins, the pipeline's
    // including the transform of x that the fused forward kernel did not leave behind.  64->64 @ 2x32x64x64: kernel
    // times are level (0.24 vs 0.26 ms), but on the second stream the pipeline's HBM-bound transforms overlap the
    // matrix-bound data-gradient chain where the z-walking kernel competes with it: config 1 40.95 -> 40.14 ms.
    if (w2d < 0.92 * direct && w2d < best) { best = w2d; pick = 2; }
  }
  return pick;
}

extern "C" int dram_wino_num_points(const DramConvDesc* d) {
  if (!dram_wino_applicable(d)) return DRAM_ERR_UNSUPPORTED;
  return make_geom(d, 0).npts;
}

extern "C" int dram_wino_num_points_bwd(const DramConvDesc* d) {
  if (!dram_wino_applicable(d)) return DRAM_ERR_UNSUPPORTED;
  return make_geom(d, 1).npts;
}

extern "C" int dram_wino_pack_weight(const float* w, float* uf, float* ub, const DramConvDesc* d,
                                     dram_stream_t stream) {
  if (!w || (!uf && !ub)) return DRAM_ERR_BAD_ARG;
  if (!dram_wino_applicable(d)) return DRAM_ERR_UNSUPPORTED;
  const long n = (long)d->Cout * d->Cin;
  const dim3 grid((unsigned)((n + 255) / 256), 2);
  const WinoGeom gf = make_geom(d, 0), gb = make_geom(d, 1);      // uf: forward tiling, ub: data-gradient tiling
  const bool same = gf.nz == gb.nz && gf.ny == gb.ny && gf.nx == gb.nx;
  float *pf = uf, *pb = same ? ub : nullptr;
  DramProf prof(DRAM_FAM_WEIGHT_PACK, 1, 0.0,
                4.0 * (double)n * (27.0 + (uf ? gf.npts : 0) + (ub ? gb.npts : 0)), (hipStream_t)stream);
#define W_WT(NZ_, NY_, NX_)                                                                                            \
  hipLaunchKernelGGL((wino_weight_kernel<NZ_, NY_, NX_>), grid, dim3(256), 0, (hipStream_t)stream, w, pf, pb, d->Cout, \
                     d->Cin, math_mode() ? 1 : 0)
  if (pf || pb) WINO_TILING_DISPATCH(gf, W_WT);
  if (!same && ub) {
    pf = nullptr;
    pb = ub;
    WINO_TILING_DISPATCH(gb, W_WT);
  }
#undef W_WT
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

extern "C" int dram_wino_num_stat_rows(const DramConvDesc* d) {
  if (!dram_wino_applicable(d)) return DRAM_ERR_UNSUPPORTED;
  const WinoGeom g = make_geom(d);
  return (g.T + wino_tpb(g.T) - 1) / wino_tpb(g.T);
}

/* pass: 0 forward, 1 data gradient, 2 weight gradient */
extern "C" size_t dram_wino_workspace(const DramConvDesc* d, int pass) {
  if (!dram_wino_applicable(d) || pass < 0 || pass > 2) return 0;
  const WinoGeom g = make_geom(d, pass);
  size_t n = (size_t)g.npts * g.Tpad * ((size_t)d->Cin + d->Cout);
  if (pass == 2) {
    TnPlan p;
    if (!plan_tn(d, g, p)) return 0;
    n += (size_t)p.nsplit * g.npts * d->Cout * d->Cin;
  }
  return n * sizeof(float);
}

extern "C" int dram_wino_conv3d_fwd(const float* x, const float* uf, const float* bias, float* y, float* stats_partial,
                                    float* v_keep, const DramConvDesc* d, void* workspace, size_t workspace_bytes,
                                    dram_stream_t stream) {
  if (!x || !uf || !y) return DRAM_ERR_BAD_ARG;
  if (!dram_wino_applicable(d)) return DRAM_ERR_UNSUPPORTED;
  return run_conv(x, uf, bias, nullptr, nullptr, y, stats_partial, v_keep, d, 0, d->Cin, d->Cout, workspace,
                  workspace_bytes, (hipStream_t)stream);
}

extern "C" int dram_wino_prologue_supported(const DramConvDesc* d) {
  if (!dram_wino_applicable(d) || math_mode()) return 0;
  const WinoGeom g = make_geom(d, 0);
  return (g.nz == 4 && g.ny == 4 && g.nx == 4) ? 1 : 0;
}

extern "C" int dram_wino_conv3d_fwd_bn(const float* x_pre, const float* pscale, const float* pshift, const float* uf,
                                       const float* bias, float* y, float* stats_partial, float* v_keep,
                                       const DramConvDesc* d, void* workspace, size_t workspace_bytes, dram_stream_t stream) {
  if (!x_pre || !pscale || !pshift || !uf || !y) return DRAM_ERR_BAD_ARG;
  if (!dram_wino_prologue_supported(d)) return DRAM_ERR_UNSUPPORTED;
  return run_conv(x_pre, uf, bias, nullptr, nullptr, y, stats_partial, v_keep, d, 0, d->Cin, d->Cout, workspace,
                  workspace_bytes, (hipStream_t)stream, pscale, pshift);
}

extern "C" int dram_wino_conv3d_fwd_cat(const float* x0, int C0, const float* x1, int C1, const float* uf, const float* bias,
                                        float* y, float* stats_partial, float* v_keep, const DramConvDesc* d,
                                        void* workspace, size_t workspace_bytes, dram_stream_t stream) {
  if (!x0 || !x1 || !uf || !y || !d || C0 < 64 || C1 < 64 || (C0 % 64) || (C1 % 64) || C0 + C1 != d->Cin)
    return DRAM_ERR_BAD_ARG;
  if (!dram_wino_prologue_supported(d)) return DRAM_ERR_UNSUPPORTED;        // (F(4,3)^3 tiles, fp32 images)
  return run_conv(x0, uf, bias, nullptr, nullptr, y, stats_partial, v_keep, d, 0, d->Cin, d->Cout, workspace,
                  workspace_bytes, (hipStream_t)stream, nullptr, nullptr, x1, C0);
}

extern "C" size_t dram_wino_v_elems(const DramConvDesc* d) {
  if (!dram_wino_applicable(d)) return 0;
  const WinoGeom g = make_geom(d);
  return (size_t)g.npts * g.Tpad * (size_t)d->Cin;
}

extern "C" int dram_wino_conv3d_bwd_data(const float* dy, const float* ub, float* dx, const float* add,
                                         const float* gate, const DramConvDesc* d, void* workspace,
                                         size_t workspace_bytes, dram_stream_t stream) {
  if (!dy || !ub || !dx || (gate && !add)) return DRAM_ERR_BAD_ARG;
  if (!dram_wino_applicable(d)) return DRAM_ERR_UNSUPPORTED;
  return run_conv(dy, ub, nullptr, add, gate, dx, nullptr, nullptr, d, 1, d->Cout, d->Cin, workspace, workspace_bytes,
                  (hipStream_t)stream);
}

extern "C" int dram_wino_num_stat_rows_bwd(const DramConvDesc* d) {
  if (!dram_wino_applicable(d)) return 0;
  const WinoGeom g = make_geom(d, 1);
  return (g.T + wino_tpb(g.T) - 1) / wino_tpb(g.T);
}

extern "C" int dram_wino_conv3d_bwd_data_bn(const float* dy, const float* ub, float* dx, const float* bn_y,
                                            const float* bn_mean, const float* bn_invstd, const float* bn_scale,
                                            const float* bn_shift, float* stats_partial, const DramConvDesc* d,
                                            void* workspace, size_t workspace_bytes, dram_stream_t stream) {
  if (!dy || !ub || !dx || !bn_y || !bn_mean || !bn_invstd || !bn_scale || !bn_shift || !stats_partial)
    return DRAM_ERR_BAD_ARG;
  if (!dram_wino_applicable(d) || d->Cin % 64) return DRAM_ERR_UNSUPPORTED;
  return run_conv(dy, ub, nullptr, nullptr, nullptr, dx, stats_partial, nullptr, d, 1, d->Cout, d->Cin, workspace,
                  workspace_bytes, (hipStream_t)stream, nullptr, nullptr, nullptr, 0,
                  BnBwdStat{bn_y, bn_mean, bn_invstd, bn_scale, bn_shift});
}

extern "C" int dram_wino_conv3d_bwd_weight(const float* x, const float* v_cache, const float* dy, float* dw,
                                           const DramConvDesc* d, void* workspace, size_t workspace_bytes,
                                           dram_stream_t stream) {
  if ((!x && !v_cache) || !dy || !dw) return DRAM_ERR_BAD_ARG;
  if (!dram_wino_applicable(d)) return DRAM_ERR_UNSUPPORTED;
  const WinoGeom g = make_geom(d);
  TnPlan p;
  if (!plan_tn(d, g, p)) return DRAM_ERR_UNSUPPORTED;
  const size_t need = dram_wino_workspace(d, 2);
  if (!workspace || workspace_bytes < need) return DRAM_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* V = (float*)workspace;                               // [64][Tpad][Cin]
  float* Dh = V + (size_t)g.npts * g.Tpad * d->Cin;           // [npts][Tpad][Cout]
  float* slab = Dh + (size_t)g.npts * g.Tpad * d->Cout;       // [nsplit][npts][Cout][Cin]
  const int math = math_mode();      // the cached V is in the image of the mode it was written in: same mode here
  if (v_cache) V = const_cast<float*>(v_cache);
  else {
    const int rc0 = launch_wino_in<0>(x, V, g, d->Cin, math, s);
    if (rc0 != DRAM_OK) return rc0;
  }
  { const int rc1 = launch_wino_in<1>(dy, Dh, g, d->Cout, math, s); if (rc1 != DRAM_OK) return rc1; }
  const int rc = run_tn(Dh, V, slab, g, p, d->Cout, d->Cin, math, s);
  if (rc != DRAM_OK) return rc;
  const long n = (long)d->Cout * d->Cin;
  DramProf prof(DRAM_FAM_WINO_WGRAD_OUT, 1, 0.0, 4.0 * (double)n * ((double)g.npts * p.nsplit + 27.0), s);
#define W_WGO(NZ_, NY_, NX_)                                                                                         \
  hipLaunchKernelGGL((wino_wgrad_out_kernel<NZ_, NY_, NX_>), dim3((unsigned)((n + 63) / 64)), dim3(512), 0, s, slab, dw, \
                     d->Cout, d->Cin, p.nsplit)
  WINO_TILING_DISPATCH(g, W_WGO);
#undef W_WGO
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
