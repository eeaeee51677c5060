// ccl_shapes.hip -- one row per connected component of a labelled volume: size, bounding box, centroid sums, exposed
// faces and zone counts, behind the cluster shapes of the predict report.  The input is what
// dram_label_components (ccl.hip) writes: components[v] = the linear index of the smallest voxel of v's component, -1 on
// background.  A voxel v with c = components[v] counts in component c only when 0 <= c < D*H*W and components[c] == c,
// so no int32 content can index out of bounds; a root is a voxel with components[v] == v.
//
// dram_component_rank numbers the roots in ascending linear index (three launches):
//   1 count   a workgroup owns RANK_TILE consecutive voxels and writes its number of roots to blk[b]
//   2 scan    ONE workgroup turns blk into exclusive offsets in index order, blk[nblk] and count[0] get the total
//   3 assign  the workgroup of launch 1 again: ballots give the rank inside a wave, a 64-entry scan in LDS the offsets of
//             its (iteration, wave) pairs in voxel order; rank[v] = blk[b] + those, written at roots only
// dram_component_shapes fills the rows (two launches):
//   4 init    every root writes its whole row: root, class, the identities of the sums / minima / maxima; rows from
//             count[1] up to capacity are zeroed, count is written
//   5 accum   one wave per x-row, chunks of 64 voxels.  A SEGMENT is a maximal stretch of equal `components` value inside
//             a chunk.  Length, bounding box and the three coordinate sums of a segment are closed forms of its ends; the
//             z / y faces and the zone counts are ballots of the chunk masked to the segment's lanes and counted; the x
//             faces exist only at the ends of a run, so a cut at a chunk boundary looks at the voxel across it (a carry
//             from the chunk before, one load for the chunk after).  The LAST lane of a segment issues the segment's
//             atomics: never one per voxel.  A chunk without foreground is left after its first load.
//             A large component would still put every wave of the chip on one row (one solid component over 300 x 350 x
//             450: 137 ms; the two lungs as two components: 58 ms), so a workgroup (16 x-rows) keeps up to 16 HOME rows
//             in LDS, claimed by segments of 16 voxels or more, adds their segments there with LDS atomics and flushes
//             each home row once (the same volumes: 0.90 and 1.57 ms).  Everything else goes to
//             the row in memory; minima and maxima first look at it with a relaxed load and skip the atomic when it
//             cannot change the value (a stale value is only ever further from the result: it costs an atomic, never
//             correctness).
// Integer atomics only (64-bit add, min, max): independent of arrival order, bit-identical from call to call.  No waiting
// between workgroups, no ticket word, never synchronises, capturable.
// Workspace: int32 rank [D*H*W] and int32 blk [nblk + 1], each rounded up to 256 bytes; needs no clearing.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int COLS = 18;
constexpr int RANK_ITERS = 16;
constexpr int RANK_TILE = TPB * RANK_ITERS;   // voxels per workgroup of the rank launches
constexpr int SCAN_TPB = 1024;
constexpr int ROWS_PER_WAVE = 4;              // x-rows per wave of the accumulate launch
constexpr unsigned long long MIN_ID = 0x7fffffffffffffffull;   // identity of the minima, as int64

long long vol_bytes(long long n, int elem) { return (n * elem + 255) / 256 * 256; }
long long rank_blocks(long long total) { return (total + RANK_TILE - 1) / RANK_TILE; }

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// ---------------------------------------------------------------------------------------------------- 1 count
__global__ __launch_bounds__(TPB) void rank_count_kernel(const int* __restrict__ comp, unsigned total,
                                                         int* __restrict__ blk) {
  __shared__ int wsum[WAVES];
  const unsigned base = blockIdx.x * (unsigned)RANK_TILE + threadIdx.x;
  int n = 0;
#pragma unroll
  for (int i = 0; i < RANK_ITERS; ++i) {
    const unsigned v = base + (unsigned)(i * TPB);
    n += (v < total && comp[v] == (int)v) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < WAVES; ++w) s += wsum[w];
    blk[blockIdx.x] = s;
  }
}

// ---------------------------------------------------------------------------------------------------- 2 scan
__global__ __launch_bounds__(SCAN_TPB) void rank_scan_kernel(int* __restrict__ blk, int nblk,
                                                             long long* __restrict__ count) {
  __shared__ int wtot[SCAN_TPB / 64];
  __shared__ int carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int t0 = 0; t0 < nblk; t0 += SCAN_TPB) {
    const int i = t0 + (int)threadIdx.x;
    const int n = i < nblk ? blk[i] : 0;
    const int inc = wave_incl_scan(n, lane);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int off = carry_s;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    if (i < nblk) blk[i] = off + inc - n;
    __syncthreads();                                            // every thread has read carry_s and wtot
    if (threadIdx.x == SCAN_TPB - 1) carry_s = off + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    blk[nblk] = carry_s;
    count[0] = (long long)carry_s;
  }
}

// ---------------------------------------------------------------------------------------------------- 3 assign
__global__ __launch_bounds__(TPB) void rank_assign_kernel(const int* __restrict__ comp, unsigned total,
                                                          const int* __restrict__ blk, int* __restrict__ rank) {
  __shared__ int wc[RANK_ITERS * WAVES];                        // roots of (iteration, wave), in voxel order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned base = blockIdx.x * (unsigned)RANK_TILE + threadIdx.x;
  unsigned flags = 0;
  int pre[RANK_ITERS];
#pragma unroll
  for (int i = 0; i < RANK_ITERS; ++i) {
    const unsigned v = base + (unsigned)(i * TPB);
    const bool root = v < total && comp[v] == (int)v;
    const unsigned long long m = __ballot(root);
    pre[i] = __popcll(m & ((1ull << lane) - 1ull));
    if (root) flags |= 1u << i;
    if (lane == 0) wc[i * WAVES + wave] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < 64) {                                       // RANK_ITERS * WAVES == 64: one wave scans them
    const int n = wc[threadIdx.x];
    const int inc = wave_incl_scan(n, lane);
    wc[threadIdx.x] = inc - n;
  }
  __syncthreads();
  if (!flags) return;
  const int off = blk[blockIdx.x];
#pragma unroll
  for (int i = 0; i < RANK_ITERS; ++i)
    if (flags & (1u << i)) rank[base + (unsigned)(i * TPB)] = off + wc[i * WAVES + wave] + pre[i];
}
static_assert(RANK_ITERS * WAVES == 64, "rank_assign_kernel scans its wave counts with one wave");

// ---------------------------------------------------------------------------------------------------- 4 init
template <typename LT>
__global__ __launch_bounds__(TPB) void shapes_init_kernel(const int* __restrict__ comp, const LT* __restrict__ lab,
                                                          long sz, long sy, const int* __restrict__ rank,
                                                          const int* __restrict__ blk_total, long long* __restrict__ rows,
                                                          long long capacity, long long* __restrict__ count, int H, int W,
                                                          unsigned total) {
  const long long n = (long long)blk_total[0];
  const long long filled = n < capacity ? n : capacity;
  const unsigned long long tid = blockIdx.x * (unsigned long long)TPB + threadIdx.x;
  if (tid == 0) {
    count[0] = n;
    count[1] = filled;
  }
  const unsigned long long stride = (unsigned long long)gridDim.x * TPB;
  for (unsigned long long i = (unsigned long long)filled * COLS + tid; i < (unsigned long long)capacity * COLS; i += stride)
    rows[i] = 0;
  if (tid >= total) return;
  const unsigned v = (unsigned)tid;
  if (comp[v] != (int)v) return;
  const long long r = (long long)rank[v];
  if (r >= capacity) return;
  long long cls = 0;
  if (lab) {
    const unsigned x = v % (unsigned)W, q = v / (unsigned)W;
    cls = (long long)lab[(long)(q / (unsigned)H) * sz + (long)(q % (unsigned)H) * sy + (long)x];
  }
  long long* p = rows + r * COLS;
  p[0] = (long long)v;
  p[1] = cls;
#pragma unroll
  for (int c = 2; c < COLS; ++c) p[c] = (c == 3 || c == 5 || c == 7) ? (long long)MIN_ID : 0;
}

// ---------------------------------------------------------------------------------------------------- 5 accum
__device__ __forceinline__ unsigned long long row_peek(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// PEEK (rows in memory): look before a minimum / maximum and skip the atomic that cannot change the value
template <bool PEEK> __device__ __forceinline__ void row_min(unsigned long long* p, unsigned long long v) {
  if (!PEEK || row_peek(p) > v) atomicMin(p, v);
}
template <bool PEEK> __device__ __forceinline__ void row_max(unsigned long long* p, unsigned long long v) {
  if (!PEEK || row_peek(p) < v) atomicMax(p, v);
}
__device__ __forceinline__ void row_add(unsigned long long* p, unsigned long long v) {
  if (v) atomicAdd(p, v);
}

struct Segment {                // what one x-run segment adds to its row: columns 2..17
  unsigned long long len, z, y, xs, xe, fz, fy, fx, n1, n2, n3;
};
template <bool PEEK> __device__ __forceinline__ void segment_flush(unsigned long long* p, const Segment& g) {
  atomicAdd(p + 2, g.len);
  row_min<PEEK>(p + 3, g.z);
  row_max<PEEK>(p + 4, g.z + 1);
  row_min<PEEK>(p + 5, g.y);
  row_max<PEEK>(p + 6, g.y + 1);
  row_min<PEEK>(p + 7, g.xs);
  row_max<PEEK>(p + 8, g.xe + 1);
  row_add(p + 9, g.z * g.len);
  row_add(p + 10, g.y * g.len);
  row_add(p + 11, (g.xs + g.xe) * g.len / 2);                   // xs + ... + xe; (xs + xe) * len is even
  row_add(p + 12, g.fz);
  row_add(p + 13, g.fy);
  row_add(p + 14, g.fx);
  row_add(p + 15, g.n1);
  row_add(p + 16, g.n2);
  row_add(p + 17, g.n3);
}

// Home rows: the workgroup keeps up to HOMES rows in LDS.  A segment of at least CLAIM_LEN voxels -- the mark of a large
// component -- may claim a free slot for its component (open addressing, PROBES linear probes, one compare-and-swap on
// the slot's key); every later segment of that component in the workgroup adds to the slot, and the slots are flushed
// to the rows once at the end.  A component without a slot adds to its row in memory directly.  Which components get
// slots changes where the additions happen, never their sum.
constexpr int HOMES = 16, PROBES = 4, CLAIM_LEN = 16, NO_HOME = -1;

__device__ __forceinline__ int home_slot(int* keys, int c, int len) {
  const unsigned h = ((unsigned)c * 2654435761u) >> 28;
#pragma unroll
  for (int p = 0; p < PROBES; ++p) {
    const int i = (int)((h + (unsigned)p) & (unsigned)(HOMES - 1));
    int k = __hip_atomic_load(keys + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == NO_HOME) {
      if (len < CLAIM_LEN) return -1;
      k = atomicCAS(keys + i, NO_HOME, c);
      if (k == NO_HOME) return i;
    }
    if (k == c) return i;
  }
  return -1;
}
static_assert((HOMES & (HOMES - 1)) == 0 && HOMES == 16 && HOMES * (COLS - 2) == TPB, "home_slot hashes to 4 bits; the "
              "flush gives every (slot, column) one thread");

__global__ __launch_bounds__(TPB) void shapes_accum_kernel(const int* __restrict__ comp, const uint8_t* __restrict__ zones,
                                                           const int* __restrict__ rank,
                                                           unsigned long long* __restrict__ rows, long long capacity,
                                                           int D, int H, int W, long nrows, unsigned total) {
  __shared__ unsigned long long acc[HOMES * COLS];
  __shared__ int keys[HOMES];
  const int lane = threadIdx.x & 63;
  const long row_first = ((long)blockIdx.x * WAVES + (threadIdx.x >> 6)) * ROWS_PER_WAVE;
  const long plane = (long)H * W;
  const int nch = (W + 63) >> 6;
  const unsigned long long le = ~0ull >> (63 - lane);           // this lane and the ones left of it
  for (int i = threadIdx.x; i < HOMES * COLS; i += TPB) {
    const int col = i % COLS;
    acc[i] = (col == 3 || col == 5 || col == 7) ? MIN_ID : 0ull;
  }
  if (threadIdx.x < HOMES) keys[threadIdx.x] = NO_HOME;
  __syncthreads();
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const long row = row_first + k;
    if (row >= nrows) break;                                    // the whole wave leaves: ballots below are full waves
    const int z = (int)(row / H), y = (int)(row % H);
    const long base = row * (long)W;
    int carry = -1;                                             // value left of the chunk (unused at x == 0)
    for (int ch = 0; ch < nch; ++ch) {
      const int x = ch * 64 + lane;
      const bool in = x < W;
      const long v = base + x;
      const int c = in ? comp[v] : -1;
      const int left_of_chunk = carry;
      carry = __shfl(c, 63, 64);
      if (!__ballot(c >= 0)) continue;                          // no foreground in the chunk (wave-uniform)
      const int prev = __shfl_up(c, 1, 64), next = __shfl_down(c, 1, 64);
      const bool start = in && (lane == 0 || prev != c);
      const bool last = in && (lane == 63 || x + 1 == W || next != c);
      const unsigned long long m = __ballot(start) & le;        // never 0 for a lane inside the row: lane 0 starts
      const int s = in ? 63 - __clzll((long long)m) : lane;     // first lane of this lane's segment
      const unsigned long long seg = (le >> s) << s;
      // faces normal to z and to y, zone membership: one ballot each, counted over the segment by its last lane
      const unsigned long long bz0 = __ballot(in && (z == 0 || comp[v - plane] != c));
      const unsigned long long bz1 = __ballot(in && (z + 1 == D || comp[v + plane] != c));
      const unsigned long long by0 = __ballot(in && (y == 0 || comp[v - W] != c));
      const unsigned long long by1 = __ballot(in && (y + 1 == H || comp[v + W] != c));
      unsigned long long n1 = 0, n2 = 0, n3 = 0;
      if (zones) {
        const int zn = in ? (int)zones[v] : 0;
        n1 = __ballot(zn == 1);
        n2 = __ballot(zn == 2);
        n3 = __ballot(zn == 3);
      }
      if (last && c >= 0 && (unsigned)c < total && comp[c] == c) {
        const long long r = (long long)rank[c];
        if (r < capacity) {
          Segment g;
          g.len = (unsigned long long)(lane - s + 1);
          g.z = (unsigned long long)z;
          g.y = (unsigned long long)y;
          g.xs = (unsigned long long)(ch * 64 + s);
          g.xe = (unsigned long long)x;
          g.fz = (unsigned long long)(__popcll(bz0 & seg) + __popcll(bz1 & seg));
          g.fy = (unsigned long long)(__popcll(by0 & seg) + __popcll(by1 & seg));
          // an x face only at the end of a run: a cut at a chunk boundary looks at the voxel across it
          g.fx = (unsigned long long)(((s > 0 || g.xs == 0 || left_of_chunk != c) ? 1 : 0) +
                                      ((lane < 63 || x + 1 == W || comp[v + 1] != c) ? 1 : 0));
          g.n1 = (unsigned long long)__popcll(n1 & seg);
          g.n2 = (unsigned long long)__popcll(n2 & seg);
          g.n3 = (unsigned long long)__popcll(n3 & seg);
          const int slot = home_slot(keys, c, (int)g.len);
          if (slot >= 0) segment_flush<false>(acc + slot * COLS, g);
          else segment_flush<true>(rows + r * COLS, g);
        }
      }
    }
  }
  __syncthreads();
  const int slot = threadIdx.x / (COLS - 2), t = 2 + threadIdx.x % (COLS - 2);
  const int c = keys[slot];
  if (c != NO_HOME) {                                           // claimed by a counted segment: a root within capacity
    unsigned long long* p = rows + (long long)rank[c] * COLS + t;
    const unsigned long long a = acc[slot * COLS + t];
    if (t == 3 || t == 5 || t == 7) row_min<true>(p, a);
    else if (t == 4 || t == 6 || t == 8) row_max<true>(p, a);
    else row_add(p, a);
  }
}

template <typename LT>
void launch_init(const int* comp, const void* labels, long sz, long sy, const int* rank, const int* blk_total,
                 long long* rows, long long capacity, long long* count, int H, int W, unsigned total, hipStream_t s) {
  hipLaunchKernelGGL((shapes_init_kernel<LT>), dim3((total + TPB - 1) / TPB), dim3(TPB), 0, s, comp, (const LT*)labels, sz,
                     sy, rank, blk_total, rows, capacity, count, H, W, total);
}

}  // namespace

extern "C" long long dram_component_shapes_workspace(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1 || (long long)D * H * W >= (1LL << 31)) return 0;
  const long long total = (long long)D * H * W;
  return vol_bytes(total, 4) + vol_bytes(rank_blocks(total) + 1, 4);
}

extern "C" int dram_component_rank(const int32_t* components, void* work, int64_t* count, int D, int H, int W,
                                   dram_stream_t stream) {
  if (!components || !work || !count || D < 1 || H < 1 || W < 1) return DRAM_ERR_BAD_ARG;
  const long long total = (long long)D * H * W;
  if (total >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int* rank = (int*)work;
  int* blk = (int*)((char*)work + vol_bytes(total, 4));
  const int nblk = (int)rank_blocks(total);
  {
    DramProf prof(DRAM_FAM_PREP, 21, 0.0, (double)total * 4.0, s);
    hipLaunchKernelGGL(rank_count_kernel, dim3(nblk), dim3(TPB), 0, s, (const int*)components, (unsigned)total, blk);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 22, 0.0, (double)nblk * 8.0, s);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, s, blk, nblk, (long long*)count);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 23, 0.0, (double)total * 4.0, s);
    hipLaunchKernelGGL(rank_assign_kernel, dim3(nblk), dim3(TPB), 0, s, (const int*)components, (unsigned)total,
                       (const int*)blk, rank);
    DRAM_LAUNCH_CHECK();
  }
  return DRAM_OK;
}

extern "C" int dram_component_shapes(const int32_t* components, const void* labels, int lab_elem, long long stride_z,
                                     long long stride_y, const uint8_t* zones, const void* work, int64_t* rows,
                                     long long capacity, int64_t* count, int D, int H, int W, dram_stream_t stream) {
  if (!components || !work || !count || capacity < 0 || (capacity > 0 && !rows) || D < 1 || H < 1 || W < 1 ||
      stride_z < 0 || stride_y < 0 || (labels && lab_elem != 1 && lab_elem != 2))
    return DRAM_ERR_BAD_ARG;
  const long long total = (long long)D * H * W;
  if (total >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int* rank = (const int*)work;
  const int* blk = (const int*)((const char*)work + vol_bytes(total, 4));
  const int* blk_total = blk + rank_blocks(total);
  {
    DramProf prof(DRAM_FAM_PREP, 24, 0.0, (double)total * 4.0 + (double)capacity * COLS * 8.0, s);
    if (labels && lab_elem == 2)
      launch_init<int16_t>((const int*)components, labels, (long)stride_z, (long)stride_y, rank, blk_total,
                           (long long*)rows, capacity, (long long*)count, H, W, (unsigned)total, s);
    else
      launch_init<uint8_t>((const int*)components, labels, (long)stride_z, (long)stride_y, rank, blk_total,
                           (long long*)rows, capacity, (long long*)count, H, W, (unsigned)total, s);
    DRAM_LAUNCH_CHECK();
  }
  if (capacity > 0) {
    const long nrows = (long)D * H;
    const long per_wg = (long)WAVES * ROWS_PER_WAVE;
    DramProf prof(DRAM_FAM_PREP, 25, 0.0, (double)total * (zones ? 5.0 : 4.0), s);
    hipLaunchKernelGGL(shapes_accum_kernel, dim3((unsigned)((nrows + per_wg - 1) / per_wg)), dim3(TPB), 0, s,
                       (const int*)components, zones, rank, (unsigned long long*)rows, capacity, D, H, W, nrows,
                       (unsigned)total);
    DRAM_LAUNCH_CHECK();
  }
  return DRAM_OK;
}
