// gauss.hip -- the separable 3-D Gaussian filter: the GaussianSmooth augmentation (zero border,
// fp32 volume) and the Gaussian pre-filter of the scan side of the predict report (edge replication, int16 scan).
//   f[z,y,x] = sum_k wz[k] sum_j wy[j] sum_i wx[i] * in[z+k, y+j, x+i], along x, then y, then z, in fp32; per axis a
//   symmetric tap of radius 0..16 given by its half w[0..r]; `out` is a box of f (the whole volume: the box at 0).
//
// One value along one axis is ((w[0] c + w[1] (l1 + r1)) + w[2] (l2 + r2)) + ...: `line()` below, one multiply, then
// one add and one explicit fused multiply-add per distance.  All three passes call it, so the order of the fp32
// operations of an output voxel depends on the taps alone: a box is the crop of the whole result, the int16 output is
// rintf of the float32 one, and two calls agree, bit for bit.  A radius of 0 passes the value through.
//
// Design (figures: DESIGN.md section 4n).  Two launches and one fp32 intermediate in the caller's workspace.
//   * In-plane pass.  A workgroup of 4 waves owns a TY x TX tile of one source plane.  It stages the (ny + 2 ry) x
//     (TX + 2 rx) patch in LDS as fp32, applying the border rule while staging (the only place the rule exists in the
//     plane: indices clamped, or zeros for what lies outside the volume; every global read is inside the volume), SB
//     loads in flight per thread ahead of their LDS writes.  A wave then filters whole rows: along x out of the patch
//     into a second LDS array of (ny + 2 ry) x TX, along y out of that into the intermediate.  Lane i of a wave reads
//     word i + const of a row in both passes: consecutive lanes, consecutive banks, whatever the row stride.
//     18 KB + 12 KB of LDS at any radius: five workgroups per CU.
//     The planes written are those the z pass reads, [max(0, z0 - rz), min(D, z0 + Do + rz)), rows and columns of the
//     box only.
//   * z pass.  One thread per output (per four along x where Wo % 4 == 0 and `out` is aligned for the vector store;
//     else element by element, which is also the tail form: nothing depends on Wo or on the alignment of `out`).  It
//     sums 2 rz + 1 planes of the intermediate; the plane index is clamped to the volume (a replicated plane filters
//     to a replicated plane: exact), or the plane counts as zeros.  Neighbouring outputs re-read planes through L2 / MALL.
// 1-D grids (< 2^31 workgroups because D*H*W is), no atomics, no scratch, never synchronises: capturable.
#include "common.h"

namespace {

constexpr int TX = 64, TY = 16;             // outputs per workgroup of the in-plane pass; a wave filters rows of TX
constexpr int RMAX = 16;                    // largest radius: DramGaussTaps holds RMAX + 1 weights per axis
constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int LXMAX = TX + 2 * RMAX, LYMAX = TY + 2 * RMAX;
constexpr int SB = 6;                       // staging loads in flight per thread (18 elements per thread at r = 16)
constexpr int ZPB = 256;                    // threads per workgroup of the z pass

static_assert(sizeof(DramGaussTaps) == 3 * 4 + 3 * (RMAX + 1) * 4, "DramGaussTaps: 17 weights per axis");
static_assert((long long)LYMAX * LXMAX < (1 << 16), "the staging index must stay below 2^16 for the magic division");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float ld(const int16_t* p, size_t i) { return (float)p[i]; }
__device__ __forceinline__ float ld(const float* p, size_t i) { return p[i]; }

// the value along one axis: centre c, at(k) the sample at signed distance k.  The ONE accumulation order.
// The weights are read where they are used, by the loop counter: scalar loads from the kernel arguments.  (Unrolled to
// RMAX with a uniform exit and the weights loaded once into scalar registers, the in-plane pass took twice as long.)
template <class F>
__device__ __forceinline__ float line(const float* w, int r, float c, F at) {
  if (r == 0) return c;
  float acc = w[0] * c;
  for (int k = 1; k <= r; ++k) acc = __fmaf_rn(w[k], at(-k) + at(k), acc);
  return acc;
}

__device__ __forceinline__ int16_t to_i16(float v) {
  return (int16_t)(int)fminf(fmaxf(rintf(v), -32768.0f), 32767.0f);
}

// mid[p][j][i] = (x then y filter of plane zlo + p)[y0 + j][x0 + i], p < np, j < Ho, i < Wo
template <typename T, bool ZERO>
__global__ __launch_bounds__(TPB) void gauss_plane_kernel(const T* __restrict__ in, float* __restrict__ mid, int H,
                                                          int W, int zlo, int y0, int x0, int Ho, int Wo, int ntx,
                                                          int nty, unsigned magic, DramGaussTaps t) {
  __shared__ float patch[LYMAX * LXMAX];
  __shared__ float rows[LYMAX * TX];
  const int ry = t.radius[1], rx = t.radius[2];
  const int bx = (int)(blockIdx.x % (unsigned)ntx), by = (int)(blockIdx.x / (unsigned)ntx % (unsigned)nty),
            bz = (int)(blockIdx.x / (unsigned)ntx / (unsigned)nty);
  const int tx0 = bx * TX, ty0 = by * TY;                          // the tile's origin inside the box
  const int ny = min(TY, Ho - ty0);
  const int LX = TX + 2 * rx, LY = ny + 2 * ry, NE = LY * LX;      // magic = 2^32 / LX + 1: e / LX for e < 2^16
  const T* plane = in + (size_t)(zlo + bz) * H * W;
  const int gy0 = y0 + ty0 - ry, gx0 = x0 + tx0 - rx;

  // stage: patch[m][i] = in[zlo + bz][gy0 + m][gx0 + i] under the border rule, every read inside the volume
  for (int e0 = (int)threadIdx.x; e0 < NE; e0 += SB * TPB) {
    float v[SB];
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int e = min(e0 + u * TPB, NE - 1);                     // past the end: the last element again, not stored
      const int m = (int)__umulhi((unsigned)e, magic), i = e - m * LX;
      const int gy = gy0 + m, gx = gx0 + i;
      const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);
      const float s = ld(plane, (size_t)cy * W + cx);
      v[u] = (ZERO && (cy != gy || cx != gx)) ? 0.0f : s;
    }
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int e = e0 + u * TPB;
      if (e < NE) patch[e] = v[u];
    }
  }
  __syncthreads();

  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  for (int m = wv; m < LY; m += WAVES) {
    const float* p = patch + m * LX + rx + lane;
    rows[m * TX + lane] = line(t.w[2], rx, p[0], [&](int k) { return p[k]; });
  }
  __syncthreads();

  const int x = tx0 + lane;
  if (x >= Wo) return;                                             // no barrier below
  for (int j = wv; j < ny; j += WAVES) {
    const float* p = rows + (j + ry) * TX + lane;
    mid[((size_t)bz * Ho + (ty0 + j)) * Wo + x] = line(t.w[1], ry, p[0], [&](int k) { return p[k * TX]; });
  }
}

template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&a)[V]) {
  if constexpr (V == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    a[0] = q.x, a[1] = q.y, a[2] = q.z, a[3] = q.w;
  } else {
    a[0] = p[0];
  }
}

template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&a)[V]) {
  if constexpr (V == 4) {
    f32x4 q = {a[0], a[1], a[2], a[3]};
    *reinterpret_cast<f32x4*>(p) = q;
  } else {
    p[0] = a[0];
  }
}

template <int V>
__device__ __forceinline__ void store_v(int16_t* p, const float (&a)[V]) {
  if constexpr (V == 4) {
    s16x4 q = {to_i16(a[0]), to_i16(a[1]), to_i16(a[2]), to_i16(a[3])};
    *reinterpret_cast<s16x4*>(p) = q;
  } else {
    p[0] = to_i16(a[0]);
  }
}

// out[z][y][x .. x + V) = z filter of mid; nq = Wo / V outputs groups per row, total = Do * Ho * nq
template <typename OutT, int V, bool ZERO>
__global__ __launch_bounds__(ZPB) void gauss_z_kernel(const float* __restrict__ mid, OutT* __restrict__ out, int D,
                                                      int zlo, int z0, int Ho, int nq, unsigned total,
                                                      DramGaussTaps t) {
  const unsigned i = blockIdx.x * (unsigned)ZPB + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % (unsigned)nq), y = (int)(i / (unsigned)nq % (unsigned)Ho), z = (int)(i / (unsigned)nq / (unsigned)Ho);
  const size_t plane = (size_t)Ho * nq * V, off = ((size_t)y * nq + q) * V;
  const int rz = t.radius[0], zc = z0 + z;

  float c[V], acc[V];
  load_v<V>(mid + (size_t)(zc - zlo) * plane + off, c);
  float lo[V], hi[V];
  auto fetch = [&](int zz, float (&a)[V]) {                       // plane zz of the volume under the border rule
    const int cz = min(max(zz, 0), D - 1);
    load_v<V>(mid + (size_t)(cz - zlo) * plane + off, a);
    if (ZERO && cz != zz) {
#pragma unroll
      for (int u = 0; u < V; ++u) a[u] = 0.0f;
    }
  };
  if (rz == 0) {
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = c[u];
  } else {
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = t.w[0][0] * c[u];
    for (int k = 1; k <= rz; ++k) {
      fetch(zc - k, lo);
      fetch(zc + k, hi);
#pragma unroll
      for (int u = 0; u < V; ++u) acc[u] = __fmaf_rn(t.w[0][k], lo[u] + hi[u], acc[u]);   // line()'s order
    }
  }
  store_v<V>(out + (size_t)z * plane + off, acc);
}

template <typename T>
void launch_plane(bool zero, dim3 grid, hipStream_t s, const T* in, float* mid, int H, int W, int zlo, int y0, int x0,
                  int Ho, int Wo, int ntx, int nty, unsigned magic, const DramGaussTaps& t) {
  if (zero)
    hipLaunchKernelGGL((gauss_plane_kernel<T, true>), grid, dim3(TPB), 0, s, in, mid, H, W, zlo, y0, x0, Ho, Wo, ntx, nty,
                       magic, t);
  else
    hipLaunchKernelGGL((gauss_plane_kernel<T, false>), grid, dim3(TPB), 0, s, in, mid, H, W, zlo, y0, x0, Ho, Wo, ntx,
                       nty, magic, t);
}

template <typename OutT, int V>
void launch_z(bool zero, hipStream_t s, const float* mid, OutT* out, int D, int zlo, int z0, int Do, int Ho, int Wo,
              const DramGaussTaps& t) {
  const int nq = Wo / V;
  const unsigned total = (unsigned)((long long)Do * Ho * nq);      // < 2^31
  const dim3 grid((unsigned)cdiv(total, ZPB));
  if (zero)
    hipLaunchKernelGGL((gauss_z_kernel<OutT, V, true>), grid, dim3(ZPB), 0, s, mid, out, D, zlo, z0, Ho, nq, total, t);
  else
    hipLaunchKernelGGL((gauss_z_kernel<OutT, V, false>), grid, dim3(ZPB), 0, s, mid, out, D, zlo, z0, Ho, nq, total, t);
}

template <typename OutT>
void launch_z_any(bool zero, hipStream_t s, const float* mid, OutT* out, int D, int zlo, int z0, int Do, int Ho, int Wo,
                  const DramGaussTaps& t) {
  const bool vec = Wo % 4 == 0 && ((uintptr_t)out & (4 * sizeof(OutT) - 1)) == 0;   // mid is 16-byte aligned (checked)
  if (vec)
    launch_z<OutT, 4>(zero, s, mid, out, D, zlo, z0, Do, Ho, Wo, t);
  else
    launch_z<OutT, 1>(zero, s, mid, out, D, zlo, z0, Do, Ho, Wo, t);
}

}  // namespace

extern "C" long long dram_gauss3d_workspace(int D, int z0, int Do, int Ho, int Wo, int rz) {
  if (D < 1 || Do < 1 || Ho < 1 || Wo < 1 || z0 < 0 || (long long)z0 + Do > D || rz < 0 || rz > RMAX) return -1;
  const long long np = (long long)min(D, z0 + Do + rz) - max(0, z0 - rz);
  return np * Ho * Wo * (long long)sizeof(float);
}

extern "C" int dram_gauss3d(const void* in, int in_type, void* out, int out_type, int D, int H, int W, int z0, int y0,
                            int x0, int Do, int Ho, int Wo, const DramGaussTaps* taps, int border, void* work,
                            long long work_bytes, dram_stream_t stream) {
  if (!in || !out || !taps || !work || in == out || work == in || work == out || D < 1 || H < 1 || W < 1 || Do < 1 ||
      Ho < 1 || Wo < 1 || z0 < 0 || y0 < 0 || x0 < 0 || (long long)z0 + Do > D || (long long)y0 + Ho > H ||
      (long long)x0 + Wo > W)
    return DRAM_ERR_BAD_ARG;
  if (!((in_type == 2 && (out_type == 2 || out_type == 4)) || (in_type == 4 && out_type == 4))) return DRAM_ERR_BAD_ARG;
  if (border != DRAM_GAUSS_NEAREST && border != DRAM_GAUSS_ZERO) return DRAM_ERR_BAD_ARG;
  for (int a = 0; a < 3; ++a)
    if (taps->radius[a] < 0 || taps->radius[a] > RMAX) return DRAM_ERR_BAD_ARG;
  if ((long long)D * H * W >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  const DramGaussTaps t = *taps;                                   // by value into the kernel arguments
  const int rz = t.radius[0], rx = t.radius[2];
  const long long need = dram_gauss3d_workspace(D, z0, Do, Ho, Wo, rz);
  if (need < 0 || work_bytes < need || ((uintptr_t)work & 15)) return DRAM_ERR_BAD_ARG;

  const int zlo = max(0, z0 - rz), np = min(D, z0 + Do + rz) - zlo;
  const int ntx = cdiv(Wo, TX), nty = cdiv(Ho, TY);
  const dim3 grid((unsigned)((long long)ntx * nty * np));         // <= np * Ho * Wo < 2^31
  const unsigned magic = (unsigned)((1ULL << 32) / (unsigned)(TX + 2 * rx)) + 1u;
  const bool zero = border == DRAM_GAUSS_ZERO;
  hipStream_t s = (hipStream_t)stream;
  float* mid = (float*)work;
  const double nmid = (double)np * Ho * Wo, nout = (double)Do * Ho * Wo;
  {
    DramProf prof(DRAM_FAM_PREP, 26, 0.0, nmid * (in_type + 4.0), s);
    if (in_type == 2)
      launch_plane<int16_t>(zero, grid, s, (const int16_t*)in, mid, H, W, zlo, y0, x0, Ho, Wo, ntx, nty, magic, t);
    else
      launch_plane<float>(zero, grid, s, (const float*)in, mid, H, W, zlo, y0, x0, Ho, Wo, ntx, nty, magic, t);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 27, 0.0, nmid * 4.0 + nout * out_type, s);
    if (out_type == 2)
      launch_z_any<int16_t>(zero, s, mid, (int16_t*)out, D, zlo, z0, Do, Ho, Wo, t);
    else
      launch_z_any<float>(zero, s, mid, (float*)out, D, zlo, z0, Do, Ho, Wo, t);
    DRAM_LAUNCH_CHECK();
  }
  return DRAM_OK;
}
