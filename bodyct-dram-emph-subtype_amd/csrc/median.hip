// median.hip -- the 3-D median noise filter in front of the scan side of the predict report:
//   out[z,y,x] = median of in over the (2rz+1)(2ry+1)(2rx+1) window centred on the voxel, every radius 0 or 1, indices
//   clamped to the volume (edge replication: scipy.ndimage.median_filter(mode='nearest')), int16 in and out.
// The sample count N is 3, 9 or 27, always odd: the median is a SELECTION (rank N/2 + 1), never a mean of two, so the
// result is one of the inputs and the kernel is held to the definition bit for bit.
//
// Design (figures: DESIGN.md section 4l).
//   * Selection network, no sort.  "Forgetful selection": the minimum of any K = N'/2 + 2 of the N' samples still in play
//     has K - 1 >= N'/2 + 1 samples at or above it, so it is not above the median, and the maximum is not below it; drop
//     both, and the median of the remaining N' - 2 is the same value.  Start with K = N/2 + 2 samples (15 of 27), find
//     min and max (pair the set's ends: floor(K/2) exchanges, then one chain through the lower half for the min and one
//     through the upper half for the max: ceil(3K/2) - 2 exchanges), forget them, take in the next sample, and so on down
//     to a median of 3: 153 exchanges for 27 samples, 20 for 9, 3 for 3.  Only min / max, fully unrolled with compile-time
//     indices: everything stays in registers, and the 0/1 principle proves the network (tools/median_net_check.cpp
//     runs all 2^N inputs of each size on the host).
//   * Two outputs per register.  A thread owns the x-pair (x, x + 1), x even within its tile, and runs ONE network on
//     packed int16 pairs (v_pk_min_i16 / v_pk_max_i16 are signed: -32768 and 32767 order correctly): an exchange is two
//     instructions for two voxels.  The low half of every register is a sample of x's window, the high half the sample
//     one voxel to the right, which is x + 1's.
//   * Reuse through LDS.  A workgroup stages its tile with the halo, indices clamped while staging (the only place edge
//     replication exists), as int16 rows of TX + 2; tile column i holds x0 - 1 + i, so the pair's left neighbours
//     (x - 1, x) and its right ones (x + 1, x + 2) are the aligned dwords p and p + 1 of the row and the centre pair
//     (x, x + 1) is one byte permute of the two.  33 dwords per row: consecutive lanes, consecutive banks.  A thread walks
//     the TZ planes of its tile and reads the (2rz+1)(2ry+1) rows of each window again, 2 dwords per row (keeping two
//     planes in registers instead would save at most the 18 us by which 3x3x1 exceeds 1x3x3, of 255: not built).
//     Staging issues its loads SB at a time ahead of the LDS writes: one element at a time, every workgroup waited
//     out a memory latency per element (10 us of every size).
//   * Tails: a pair whose second voxel is outside the volume, or whose output address is not 4-byte aligned (odd W, or
//     an `out` that starts on an odd element), stores int16 by int16; nothing depends on W being even or a multiple of TX.
// One launch, a 1-D grid of ceil(W/TX) * ceil(H/TY) * ceil(D/TZ) workgroups (< 2^31 because D*H*W is), no atomics, no
// scratch, never synchronises: bit-identical from call to call and capturable.
#include "common.h"

namespace {

constexpr int TX = 64, TY = 8, TZ = 8;      // outputs per workgroup; TX / 2 x TY threads, each walks TZ planes
constexpr int LX = TX + 2;                  // staged row: tile columns x0 - 1 .. x0 + TX, 33 dwords
constexpr int TPB = (TX / 2) * TY;
constexpr int SB = 13;                      // staging loads in flight per thread (26 elements per thread at 3x3x3)

typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 med_min(s16x2 a, s16x2 b) { return __builtin_elementwise_min(a, b); }   // v_pk_min_i16
__device__ __forceinline__ s16x2 med_max(s16x2 a, s16x2 b) { return __builtin_elementwise_max(a, b); }   // v_pk_max_i16

}  // namespace
#define MED_FN __device__ __forceinline__
#include "median_net.h"
namespace {

template <int RZ, int RY, int RX>
__global__ __launch_bounds__(TPB) void median3d_kernel(const int16_t* __restrict__ in, int16_t* __restrict__ out, int D,
                                                       int H, int W, int ntx, int nty) {
  constexpr int LY = TY + 2 * RY, LZ = TZ + 2 * RZ;
  constexpr int N = (2 * RZ + 1) * (2 * RY + 1) * (2 * RX + 1);
  __shared__ __attribute__((aligned(4))) int16_t tile[LZ * LY * LX];

  const int bx = (int)(blockIdx.x % (unsigned)ntx), by = (int)(blockIdx.x / (unsigned)ntx % (unsigned)nty),
            bz = (int)(blockIdx.x / (unsigned)ntx / (unsigned)nty);
  const int x0 = bx * TX, y0 = by * TY, z0 = bz * TZ;
  const size_t HW = (size_t)H * W;

  // stage: tile[l][m][i] = in[clamp(z0 - RZ + l)][clamp(y0 - RY + m)][clamp(x0 - 1 + i)], every read inside the volume
  // in batches of SB loads ahead of their LDS writes: one at a time, a workgroup waits out a memory latency per element
  constexpr int NE = LZ * LY * LX, IT = (NE + TPB - 1) / TPB;
#pragma unroll
  for (int k0 = 0; k0 < IT; k0 += SB) {
    int16_t r[SB];
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int e = min((int)threadIdx.x + (k0 + u) * TPB, NE - 1);     // past the end: the last element again, not stored
      const int i = e % LX, m = e / LX % LY, l = e / (LX * LY);
      const int z = min(max(z0 - RZ + l, 0), D - 1), y = min(max(y0 - RY + m, 0), H - 1), x = min(max(x0 - 1 + i, 0), W - 1);
      r[u] = in[(size_t)z * HW + (size_t)y * W + x];
    }
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int e = (int)threadIdx.x + (k0 + u) * TPB;
      if (k0 + u < IT && e < NE) tile[e] = r[u];
    }
  }
  __syncthreads();

  const int p = threadIdx.x % (TX / 2), ty = threadIdx.x / (TX / 2);
  const int x = x0 + 2 * p, y = y0 + ty;
  if (x >= W || y >= H) return;                                   // no barrier below
  const unsigned* rows = reinterpret_cast<const unsigned*>(tile);   // LX is even: every row starts on a dword
  const int odd_base = (int)(((uintptr_t)out >> 1) & 1);
  const int nz = min(TZ, D - z0);
  for (int t = 0; t < nz; ++t) {
    s16x2 v[N];
#pragma unroll
    for (int dz = 0; dz <= 2 * RZ; ++dz) {
#pragma unroll
      for (int dy = 0; dy <= 2 * RY; ++dy) {
        const int row = ((t + dz) * LY + (ty + dy)) * (LX / 2) + p;
        const unsigned a = rows[row], b = rows[row + 1];          // (x - 1, x), (x + 1, x + 2)
        const unsigned c = __builtin_amdgcn_alignbit(b, a, 16);   // (x, x + 1)
        const int k = (dz * (2 * RY + 1) + dy) * (2 * RX + 1);
        if constexpr (RX == 1) {
          v[k] = __builtin_bit_cast(s16x2, a);
          v[k + 1] = __builtin_bit_cast(s16x2, c);
          v[k + 2] = __builtin_bit_cast(s16x2, b);
        } else {
          v[k] = __builtin_bit_cast(s16x2, c);
        }
      }
    }
    const s16x2 med = median_net::select_median<0>(v);
    const size_t o = (size_t)(z0 + t) * HW + (size_t)y * W + x;
    if (x + 1 < W && (((int)(o & 1) ^ odd_base) == 0)) {
      *reinterpret_cast<unsigned*>(out + o) = __builtin_bit_cast(unsigned, med);
    } else {
      out[o] = med.x;
      if (x + 1 < W) out[o + 1] = med.y;
    }
  }
}

template <int RZ, int RY, int RX>
void launch(dim3 grid, hipStream_t s, const int16_t* in, int16_t* out, int D, int H, int W, int ntx, int nty) {
  hipLaunchKernelGGL((median3d_kernel<RZ, RY, RX>), grid, dim3(TPB), 0, s, in, out, D, H, W, ntx, nty);
}

}  // namespace

extern "C" int dram_median3d(const int16_t* in, int16_t* out, int D, int H, int W, int rz, int ry, int rx,
                             dram_stream_t stream) {
  if (!in || !out || in == out || D < 1 || H < 1 || W < 1 || (rz | ry | rx) < 0 || rz > 1 || ry > 1 || rx > 1 ||
      rz + ry + rx == 0)
    return DRAM_ERR_BAD_ARG;
  const long long total = (long long)D * H * W;
  if (total >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  const int ntx = cdiv(W, TX), nty = cdiv(H, TY), ntz = cdiv(D, TZ);
  const dim3 grid((unsigned)((long long)ntx * nty * ntz));        // <= D*H*W < 2^31
  hipStream_t s = (hipStream_t)stream;
  DramProf prof(DRAM_FAM_PREP, 21, 0.0, 4.0 * (double)total, s);
  switch (rz * 4 + ry * 2 + rx) {
    case 1: launch<0, 0, 1>(grid, s, in, out, D, H, W, ntx, nty); break;
    case 2: launch<0, 1, 0>(grid, s, in, out, D, H, W, ntx, nty); break;
    case 3: launch<0, 1, 1>(grid, s, in, out, D, H, W, ntx, nty); break;
    case 4: launch<1, 0, 0>(grid, s, in, out, D, H, W, ntx, nty); break;
    case 5: launch<1, 0, 1>(grid, s, in, out, D, H, W, ntx, nty); break;
    case 6: launch<1, 1, 0>(grid, s, in, out, D, H, W, ntx, nty); break;
    default: launch<1, 1, 1>(grid, s, in, out, D, H, W, ntx, nty); break;
  }
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}
