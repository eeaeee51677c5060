// bilateral.hip -- the bilateral noise filter in front of the scan side of the predict report: an
// edge-preserving weighted mean of an int16 volume in exact integer fixed point, its taps optionally confined to a
// label volume (`within`: the lung).  With the host tables T_a[0..r_a] (spatial, per axis, 256 = 1.0) and R[0..L-1]
// (range, 256 = 1.0, R[L-1] = 0):
//   S(dz,dy,dx) = (T_z[|dz|] T_y[|dy|] T_x[|dx|] + 2^15) >> 16          (256 at the centre; S = 0: no such tap)
//   d_i = v_i - v_c,  w_i = S_i R[min(|d_i|, L-1)],  num = sum w_i d_i,  den = sum w_i
//   out_c = v_c + floor((2 num + den) / (2 den))                         (the quotient rounded half up)
// over the taps inside the volume and inside `within`; a centre outside `within` keeps its value.  Integers only, so the
// kernel is held to the numpy yardstick bit for bit.
//
// Design (figures: DESIGN.md section 4o).
//   * One launch.  A workgroup owns TX x TY x TZ outputs and stages them with the halo of the radii as int32 in LDS;
//     a tap outside the volume or outside `within` is stored as SENT = 2^30: its |d| is far above L - 1, clamps to it,
//     reads R[L-1] = 0 and weighs nothing, so the inner loop has neither a bounds nor a mask branch.  Every global
//     address is clamped into the volume while staging: no border value is read, none outside the volume either.
//   * R lives in LDS as the symmetric table Rs[1023 + d] = R[|d|] for d = -1024..1023, 0 from |d| = L - 1 on (uint16,
//     4 KB), gathered per tap by the signed difference: no |d| is formed.  The three spatial tables stay in the kernel
//     arguments and S is formed on the scalar unit from the loop counters, the same in every lane.
//   * Sums: w <= 2^16, and |d| <= L - 2 <= 1022 wherever w != 0, so d is clamped to +-(L - 1) first (one v_med3_i32:
//     the table read is R[min(|d|, L - 1)] as defined) and every product fits 24-bit multiplies.  The x radius is a
//     template argument: the 2 rx + 1 taps of a tile row are unrolled, independent of one another, and their w d add up
//     in int32 (11 * 2^16 * 1022 < 2^30); a row's sum then goes into the 64-bit num (|num| < 2^37), one 64-bit add per
//     row, none per tap.  den < 2^27 is a 32-bit sum.  A row is skipped when its largest S, the one at dx = 0, is 0; a tap
//     with S = 0 in a row that counts is multiplied by 0.  The final quotient |q| < 1024 is taken in fp64 -- a = 2 num
//     + den and b = 2 den are exact doubles, and a / b lies at least 1 / b >= 2^-28 from the next integer it does not
//     equal, far more than the division's rounding error -- and then checked against a - q b in integers all the same.
//   * A thread owns one (x, y) column of the tile and walks its TZ planes; the 32 lanes of a half-wave read 32
//     consecutive dwords of a tile row.  LDS: 4 (TZ + 2 rz)(TY + 2 ry)(TX + 2 rx) + 4096 bytes, 58 KB at radius 5: two
//     workgroups per CU.
// A 1-D grid of ceil(W/TX) * ceil(H/TY) * ceil(D/TZ) workgroups (< 2^31 because D*H*W is), no atomics, no scratch,
// never synchronises: bit-identical from call to call and capturable.
#include "common.h"

namespace {

constexpr int TX = 32, TY = 8, TZ = 8;      // outputs per workgroup; TX x TY threads, each walks TZ planes
constexpr int TPB = TX * TY;
constexpr int RMAX = DRAM_BILAT_MAX_RADIUS, LMAX = DRAM_BILAT_RANGE_LEN;
constexpr int SENT = 1 << 30;               // a tap that does not count: |SENT - v| >= 2^30 - 2^15 > LMAX
constexpr int SU = 4;                       // staging rows in flight per wave

struct BilatArgs {                          // by value in the kernel arguments: 2136 bytes
  uint16_t R[LMAX];
  int T[3][RMAX + 1];
  int r[3];
  int L;
};

template <int WT>
__device__ __forceinline__ bool inside(const void* within, size_t off) {
  if constexpr (WT == 1) return static_cast<const uint8_t*>(within)[off] != 0;
  if constexpr (WT == 2) return static_cast<const int16_t*>(within)[off] != 0;
  return true;
}

template <int WT, int RX>   // WT 0: no `within`, 1: uint8, 2: int16; RX: the x radius
__global__ __launch_bounds__(TPB) void bilateral3d_kernel(const int16_t* __restrict__ in, int16_t* __restrict__ out,
                                                          const void* __restrict__ within, long long wsz, long long wsy,
                                                          int D, int H, int W, int ntx, int nty, const BilatArgs a) {
  __shared__ uint16_t Rs[2 * LMAX];                                // Rs[LMAX - 1 + d] = R[|d|], 0 from |d| = L - 1 on
  extern __shared__ __attribute__((aligned(16))) int tile[];
  const int rz = a.r[0], ry = a.r[1], L1 = a.L - 1;
  constexpr int rx = RX, LX = TX + 2 * RX;
  const int LY = TY + 2 * ry, LZ = TZ + 2 * rz;

  const int bx = (int)(blockIdx.x % (unsigned)ntx), by = (int)(blockIdx.x / (unsigned)ntx % (unsigned)nty),
            bz = (int)(blockIdx.x / (unsigned)ntx / (unsigned)nty);
  const int x0 = bx * TX, y0 = by * TY, z0 = bz * TZ;
  const size_t HW = (size_t)H * W;

  for (int i = threadIdx.x; i < 2 * LMAX; i += TPB) {
    const int k = abs(i - (LMAX - 1));
    Rs[i] = k <= L1 ? a.R[min(k, LMAX - 1)] : (uint16_t)0;
  }

  // stage: tile[l][m][i] = in[z0 - rz + l][y0 - ry + m][x0 - rx + i] inside the volume and `within`, SENT elsewhere; a
  // wave takes whole rows (LX <= 42 lanes of it), SU rows' loads ahead of their LDS writes; addresses are clamped
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nrows = LZ * LY;
  const int gx = x0 - rx + lane, cx = min(max(gx, 0), W - 1);
  const bool xin = gx >= 0 && gx < W;
  for (int row0 = wave; row0 < nrows; row0 += SU * (TPB / 64)) {
    int v[SU];
    bool ok[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int row = min(row0 + u * (TPB / 64), nrows - 1);          // past the end: the last row again, not stored
      const int l = row / LY, m = row - l * LY;
      const int gz = z0 - rz + l, gy = y0 - ry + m;
      const int cz = min(max(gz, 0), D - 1), cy = min(max(gy, 0), H - 1);
      v[u] = in[(size_t)cz * HW + (size_t)cy * W + cx];
      ok[u] = inside<WT>(within, (size_t)cz * (size_t)wsz + (size_t)cy * (size_t)wsy + cx) && xin && gz == cz && gy == cy;
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int row = row0 + u * (TPB / 64);
      if (row < nrows && lane < LX) tile[row * LX + lane] = ok[u] ? v[u] : SENT;
    }
  }
  __syncthreads();

  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;                                   // no barrier below
  const int nz = min(TZ, D - z0);
  int tx_tab[RX + 1];
#pragma unroll
  for (int k = 0; k <= RX; ++k) tx_tab[k] = a.T[2][k];
  const int plane = LY * LX;
  for (int t = 0; t < nz; ++t) {
    const int centre = (t + rz) * plane + (ty + ry) * LX + tx + rx;
    const size_t o = (size_t)(z0 + t) * HW + (size_t)y * W + x;
    const int c = tile[centre];
    if (c == SENT) {                                              // outside `within`: the voxel as it is
      out[o] = in[o];
      continue;
    }
    long long num = 0;
    int den = 0;
    for (int dz = -rz; dz <= rz; ++dz) {
      const int tz = a.T[0][abs(dz)];
      for (int dy = -ry; dy <= ry; ++dy) {
        const int tzy = tz * a.T[1][abs(dy)];                     // <= 2^16; wave-uniform, as every S below
        if (((tzy * 256 + (1 << 15)) >> 16) == 0) continue;
        const int* p = tile + centre + dz * plane + dy * LX;
        int rowsum = 0;
#pragma unroll
        for (int dx = -RX; dx <= RX; ++dx) {
          const int S = (tzy * tx_tab[dx < 0 ? -dx : dx] + (1 << 15)) >> 16;
          const int d = min(max(p[dx] - c, -L1), L1);               // v_med3_i32; exact where w != 0
          const int w = __mul24(S, (int)Rs[LMAX - 1 + d]);          // <= 2^16
          rowsum += __mul24(w, d);
          den += w;
        }
        num += rowsum;
      }
    }
    const long long A = 2 * num + den, B = 2LL * den;             // den >= 2^16: the centre tap
    long long q = (long long)floor((double)A / (double)B);
    const long long rem = A - q * B;
    q += rem < 0 ? -1 : (rem >= B ? 1 : 0);
    out[o] = (int16_t)(c + (int)q);
  }
}

template <int WT, int RX>
void launch_rx(dim3 grid, size_t lds, hipStream_t s, const int16_t* in, int16_t* out, const void* within, long long wsz,
            long long wsy, int D, int H, int W, int ntx, int nty, const BilatArgs& a) {
  hipLaunchKernelGGL((bilateral3d_kernel<WT, RX>), grid, dim3(TPB), lds, s, in, out, within, wsz, wsy, D, H, W, ntx, nty, a);
}

template <int WT>
void launch(dim3 grid, size_t lds, hipStream_t s, const int16_t* in, int16_t* out, const void* within, long long wsz,
            long long wsy, int D, int H, int W, int ntx, int nty, const BilatArgs& a) {
  switch (a.r[2]) {
    case 0: launch_rx<WT, 0>(grid, lds, s, in, out, within, wsz, wsy, D, H, W, ntx, nty, a); break;
    case 1: launch_rx<WT, 1>(grid, lds, s, in, out, within, wsz, wsy, D, H, W, ntx, nty, a); break;
    case 2: launch_rx<WT, 2>(grid, lds, s, in, out, within, wsz, wsy, D, H, W, ntx, nty, a); break;
    case 3: launch_rx<WT, 3>(grid, lds, s, in, out, within, wsz, wsy, D, H, W, ntx, nty, a); break;
    case 4: launch_rx<WT, 4>(grid, lds, s, in, out, within, wsz, wsy, D, H, W, ntx, nty, a); break;
    default: launch_rx<WT, 5>(grid, lds, s, in, out, within, wsz, wsy, D, H, W, ntx, nty, a); break;
  }
}

}  // namespace

extern "C" int dram_bilateral3d(const int16_t* in, int16_t* out, const void* within, int within_type,
                                long long within_sz, long long within_sy, int D, int H, int W, const DramBilateral* tab,
                                dram_stream_t stream) {
  if (!in || !out || !tab || in == out || D < 1 || H < 1 || W < 1) return DRAM_ERR_BAD_ARG;
  if (within && ((within_type != 1 && within_type != 2) || within_sz < 0 || within_sy < 0)) return DRAM_ERR_BAD_ARG;
  if (tab->range_len < 1 || tab->range_len > LMAX || tab->range[tab->range_len - 1] != 0 ||
      tab->range[0] != 256)
    return DRAM_ERR_BAD_ARG;
  BilatArgs a;
  for (int k = 0; k < 3; ++k) {
    const int r = tab->radius[k];
    if (r < 0 || r > RMAX || tab->spatial[k][0] != 256) return DRAM_ERR_BAD_ARG;
    a.r[k] = r;
    for (int i = 0; i <= RMAX; ++i) {
      const int v = i <= r ? tab->spatial[k][i] : 0;
      if (v < 0 || v > 256) return DRAM_ERR_BAD_ARG;
      a.T[k][i] = v;
    }
  }
  a.L = tab->range_len;
  for (int i = 0; i < LMAX; ++i) {
    const int v = i < a.L ? tab->range[i] : 0;
    if (v < 0 || v > 256) return DRAM_ERR_BAD_ARG;
    a.R[i] = (uint16_t)v;
  }
  const long long total = (long long)D * H * W;
  if (total >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  const int ntx = cdiv(W, TX), nty = cdiv(H, TY), ntz = cdiv(D, TZ);
  const dim3 grid((unsigned)((long long)ntx * nty * ntz));        // <= D*H*W < 2^31
  const size_t lds = sizeof(int) * (size_t)(TZ + 2 * a.r[0]) * (TY + 2 * a.r[1]) * (TX + 2 * a.r[2]);   // <= 54432
  hipStream_t s = (hipStream_t)stream;
  DramProf prof(DRAM_FAM_PREP, 28, 0.0, (double)total * (4.0 + (within ? within_type : 0)), s);
  if (!within)
    launch<0>(grid, lds, s, in, out, nullptr, 0, 0, D, H, W, ntx, nty, a);
  else if (within_type == 1)
    launch<1>(grid, lds, s, in, out, within, within_sz, within_sy, D, H, W, ntx, nty, a);
  else
    launch<2>(grid, lds, s, in, out, within, within_sz, within_sy, D, H, W, ntx, nty, a);
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
