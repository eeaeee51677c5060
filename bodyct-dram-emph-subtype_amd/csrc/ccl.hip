// ccl.hip -- connected-component labelling of a 3-D key volume, behind the LAA cluster analysis of the predict report
// (INTEGRATION.md B8).  A key is a non-negative integer per voxel, 0 is background; two voxels are connected when they
// are neighbours (6: faces, 26: faces, edges, corners) and carry the same non-zero key.  Outputs
//   components      int32 per voxel: the linear index (z * H + y) * W + x of the smallest voxel of its component, -1 on
//                   background -- canonical, so it does not depend on scheduling
//   cluster_voxels  int32 per voxel (optional): the size of its component, 0 on background
//   table           int64 [n_regions + 1][35]: per row (key r in 1..n -> row r, a key above n -> row 0) columns 0..31 the
//                   components with 2^k <= size < 2^(k+1), 32 their number, 33 the sum of their sizes, 34 the largest
// The key is the label volume itself (image == NULL) or the LAA key of an image: label > 0 and hu < threshold, carrying
// the label (by_lobe) or 1.
//
// Design.  Label-equivalence union-find on ONE parent array, which is `components` itself: parent[v] <= v always, a
// root has parent[v] == v, background holds -1.  Five launches, the launch boundaries are the only phase boundaries:
//   1 init      one wave per x-row, chunks of 64 voxels: forms the key (stored as int16 in the workspace: the merge
//               reads up to 13 neighbours of it), and gives every foreground voxel the START OF ITS X-RUN as parent: a
//               ballot of the lanes whose key differs from their left neighbour's, a clz on its low part, and a
//               wave-uniform carry for a run that began in an earlier chunk.  A run ends where the key changes, not
//               only at background.  Also clears the per-voxel size counters and the table.
//   2 merge     one thread per voxel unions with its already-visited neighbours of the same key in the preceding rows:
//               (y-1) and (z-1) for 6, (z, y-1), (z-1, y-1), (z-1, y), (z-1, y+1) at x-1, x, x+1 for 26.  All voxels
//               of a run already share a parent, so a pair of runs needs one union: with a = key[row][x-1], b =
//               key[row][x], c = key[row][x+1] equal to the voxel's own key,
//                 b: union when the voxel starts its run or !a (else the thread to the left sees the same two runs);
//                 !b: union with x-1 when a and the voxel starts its run (else the voxel to the left lies under x-1),
//                     and with x+1 when c (no voxel to the left touches that run) -- 26 only.
//               Lock-free min-root union: find both roots; atomicMin the smaller root into the larger one's slot; when
//               the old value shows that the slot was no longer a root, go on from that old value (the slot now points
//               at min(old, smaller root), and the pair (old, smaller root) is what is still owed).  Parent values only
//               ever decrease and always name a voxel of the same component, so ANY value ever read from a slot is a
//               valid ancestor: a stale read costs steps, never correctness.  Every loop advances on the thread's own
//               reads and ends because the larger of its two indices strictly decreases: no waiting on another
//               thread, no flags, no tickets.  The parent reads of this launch are relaxed agent-scope atomic loads
//               (the XCD L2s are not coherent and L1 is never refreshed; a plain load could be served stale for ever
//               from L1 -- still correct by the argument above, but the atomic form bounds the extra steps).
//   3 compress  components[v] = find(v), in place.  The roots are final after launch 2; a slot another thread of this
//               launch has already overwritten holds the root, an ancestor as good as any.  The LAST voxel of every
//               x-run adds the run's length to sizes[root] with ONE integer atomic per run (a per-voxel add would
//               serialise a large component on one address).  The run's start is the voxel's own slot as launch 1 wrote
//               it: a slot that is no run start is never a root, so launch 2 never wrote it, and in launch 3 only its
//               own thread does, after reading it.
//   4 table     every root (components[v] == v) counts into a table in LDS (64-bit integer adds / max), the workgroup's
//               non-zero entries go to the int64 table with integer atomics.  At most 2048 workgroups, their threads
//               striding over the volume: with one workgroup per 256 voxels the clearing and flushing of 184 000 LDS
//               tables was 1.3 ms of a 1.8 ms call at 300 x 350 x 450.
//   5 sizes     optional: cluster_voxels[v] = sizes[components[v]].
// Integer atomics only: every result is bit-identical from call to call.  Never synchronises; capturable.
// Workspace: int32 sizes [D*H*W] and int16 key [D*H*W], each rounded up to 256 bytes; needs no clearing.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int COLS = 35;
constexpr int MAX_ROWS = 16;
constexpr unsigned TABLE_WG = 2048;   // workgroups of the table launch (8 per CU): each clears and flushes an LDS table

long long vol_bytes(long long total, int elem) { return (total * elem + 255) / 256 * 256; }

// ---------------------------------------------------------------------------------------------------- 1 init
template <typename LT>
__global__ __launch_bounds__(TPB) void ccl_init_kernel(const LT* __restrict__ lab, long sz, long sy,
                                                       const int16_t* __restrict__ img, int threshold, int by_lobe, int H,
                                                       int W, long rows, int* __restrict__ parent, int* __restrict__ sizes,
                                                       int16_t* __restrict__ key, unsigned long long* __restrict__ table,
                                                       int table_elems) {
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < table_elems; i += TPB) table[i] = 0ull;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;                                      // the whole wave leaves: ballots below are full waves
  const LT* l = lab + (row / H) * sz + (row % H) * sy;
  const long base = row * (long)W;
  const int nch = (W + 63) >> 6;
  int carry_key = 0;                                            // key of the voxel left of the chunk (0 at the row start)
  int carry_start = 0;                                          // x where the run of that voxel began
  for (int c = 0; c < nch; ++c) {
    const int x = c * 64 + lane;
    const bool in = x < W;
    int k = 0;
    if (in) {
      const int lb = (int)l[x];
      if (lb > 0) k = img ? ((int)img[base + x] < threshold ? (by_lobe ? lb : 1) : 0) : lb;
    }
    int left = __shfl_up(k, 1, 64);
    if (lane == 0) left = carry_key;
    const bool start = k != 0 && (x == 0 || k != left);
    const unsigned long long m = __ballot(start);
    const unsigned long long lo = m & (~0ull >> (63 - lane));   // run starts at or left of this lane
    const int s = lo ? c * 64 + (63 - __clzll((long long)lo)) : carry_start;
    if (in) {
      parent[base + x] = k ? (int)(base + s) : -1;
      sizes[base + x] = 0;
      key[base + x] = (int16_t)k;
    }
    carry_key = __shfl(k, 63, 64);
    carry_start = __shfl(s, 63, 64);
  }
}

// ---------------------------------------------------------------------------------------------------- 2 merge
__device__ __forceinline__ int parent_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above v: parent values strictly decrease along the walk, so it ends
__device__ __forceinline__ int find_root(const int* parent, int v) {
  int p = parent_load(parent + v);
  while (p != v) {
    v = p;
    p = parent_load(parent + v);
  }
  return v;
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
  a = find_root(parent, a);
  b = find_root(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }               // a is the larger
    const int old = atomicMin(parent + a, b);
    if (old == a) break;                                        // a was a root and now hangs under b
    a = find_root(parent, old);                                 // old < a: a had a parent already; (old, b) is still owed
    b = find_root(parent, b);
  }
}

// the voxel v (key k, `start`: first of its x-run) against the row whose voxel x has index u0 (r: that row's keys)
template <bool DIAG>
__device__ __forceinline__ void merge_row(int* parent, const int16_t* __restrict__ key, int v, int u0, int x, int W, int k,
                                          bool start) {
  const bool a = x > 0 && (int)key[u0 - 1] == k;
  const bool b = (int)key[u0] == k;
  if (b) {
    if (start || !a) unite(parent, v, u0);
  } else if (DIAG) {
    if (a && start) unite(parent, v, u0 - 1);
    if (x + 1 < W && (int)key[u0 + 1] == k) unite(parent, v, u0 + 1);
  }
}

template <bool DIAG>
__global__ __launch_bounds__(TPB) void ccl_merge_kernel(int* parent, const int16_t* __restrict__ key, int H, int W,
                                                        unsigned total) {
  const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
  if (v >= total) return;
  const int k = (int)key[v];
  if (k == 0) return;
  const int x = (int)(v % (unsigned)W);
  const unsigned r = v / (unsigned)W;
  const int y = (int)(r % (unsigned)H);
  const bool has_z = r >= (unsigned)H;                          // z > 0
  const bool start = x == 0 || (int)key[v - 1] != k;
  const int plane = H * W;
  if (y > 0) merge_row<DIAG>(parent, key, (int)v, (int)v - W, x, W, k, start);
  if (has_z) {
    if (DIAG && y > 0) merge_row<DIAG>(parent, key, (int)v, (int)v - plane - W, x, W, k, start);
    merge_row<DIAG>(parent, key, (int)v, (int)v - plane, x, W, k, start);
    if (DIAG && y + 1 < H) merge_row<DIAG>(parent, key, (int)v, (int)v - plane + W, x, W, k, start);
  }
}

// ---------------------------------------------------------------------------------------------------- 3 compress
__global__ __launch_bounds__(TPB) void ccl_compress_kernel(int* parent, const int16_t* __restrict__ key,
                                                           int* __restrict__ sizes, int W, unsigned total) {
  const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
  if (v >= total) return;
  const int k = (int)key[v];
  if (k == 0) return;
  const int x = (int)(v % (unsigned)W);
  const bool start = x == 0 || (int)key[v - 1] != k;
  const bool last = x + 1 == W || (int)key[v + 1] != k;
  // plain loads.  The own slot: written by launches 1 / 2 only, and in this launch by this thread alone.  The walk:
  // roots are final, and a slot holds what launch 2 left or the root a thread of this launch stored -- both ancestors.
  const int own = parent[v];
  int root = (int)v, p = own;
  while (p != root) {
    root = p;
    p = parent[root];
  }
  parent[v] = root;
  if (last) atomicAdd(sizes + root, (int)v - (start ? (int)v : own) + 1);
}

// ---------------------------------------------------------------------------------------------------- 4 table
__global__ __launch_bounds__(TPB) void ccl_table_kernel(const int* __restrict__ comp, const int16_t* __restrict__ key,
                                                        const int* __restrict__ sizes, int n_regions, unsigned total,
                                                        unsigned long long* __restrict__ table) {
  __shared__ unsigned long long t[MAX_ROWS * COLS];
  const int used = (n_regions + 1) * COLS;
  for (int i = threadIdx.x; i < used; i += TPB) t[i] = 0ull;
  __syncthreads();
  // 64-bit index: v + stride may pass 2^32 before the bound is tested
  const unsigned long long stride = (unsigned long long)gridDim.x * TPB;
  for (unsigned long long v = blockIdx.x * (unsigned long long)TPB + threadIdx.x; v < total; v += stride) {
    if (comp[v] != (int)v) continue;
    const int k = (int)key[v];
    const unsigned s = (unsigned)sizes[v];
    unsigned long long* row = t + (k <= n_regions ? k : 0) * COLS;
    atomicAdd(row + (s ? 31 - __clz((int)s) : 0), 1ull);        // a root holds at least its own run: s >= 1
    atomicAdd(row + 32, 1ull);
    atomicAdd(row + 33, (unsigned long long)s);
    atomicMax(row + 34, (unsigned long long)s);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < used; i += TPB) {
    const unsigned long long c = t[i];
    if (c) {
      if (i % COLS == 34) atomicMax(table + i, c);
      else atomicAdd(table + i, c);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- 5 sizes
__global__ __launch_bounds__(TPB) void ccl_gather_kernel(const int* __restrict__ comp, const int* __restrict__ sizes,
                                                         int* __restrict__ out, unsigned total) {
  const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
  if (v >= total) return;
  const int c = comp[v];
  out[v] = c >= 0 ? sizes[c] : 0;
}

template <typename LT>
int run(const void* labels, long sz, long sy, const int16_t* image, int threshold, int by_lobe, int connectivity,
        int n_regions, int* components, int* cluster_voxels, unsigned long long* table, void* work, int D, int H, int W,
        hipStream_t s) {
  const long long total = (long long)D * H * W;
  const long rows = (long)D * H;
  int* sizes = (int*)work;
  int16_t* key = (int16_t*)((char*)work + vol_bytes(total, 4));
  const unsigned vgrid = (unsigned)((total + TPB - 1) / TPB);
  const double vox = (double)total;
  {
    DramProf prof(DRAM_FAM_PREP, 16, 0.0, vox * ((double)sizeof(LT) + (image ? 2.0 : 0.0) + 10.0), s);
    hipLaunchKernelGGL((ccl_init_kernel<LT>), dim3((unsigned)((rows + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, s,
                       (const LT*)labels, sz, sy, image, threshold, by_lobe, H, W, rows, components, sizes, key, table,
                       (n_regions + 1) * COLS);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 17, 0.0, vox * 6.0, s);
    if (connectivity == 26)
      hipLaunchKernelGGL((ccl_merge_kernel<true>), dim3(vgrid), dim3(TPB), 0, s, components, (const int16_t*)key, H, W,
                         (unsigned)total);
    else
      hipLaunchKernelGGL((ccl_merge_kernel<false>), dim3(vgrid), dim3(TPB), 0, s, components, (const int16_t*)key, H, W,
                         (unsigned)total);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 18, 0.0, vox * 10.0, s);
    hipLaunchKernelGGL(ccl_compress_kernel, dim3(vgrid), dim3(TPB), 0, s, components, (const int16_t*)key, sizes, W,
                       (unsigned)total);
    DRAM_LAUNCH_CHECK();
  }
  {
    DramProf prof(DRAM_FAM_PREP, 19, 0.0, vox * 4.0, s);
    hipLaunchKernelGGL(ccl_table_kernel, dim3(vgrid < TABLE_WG ? vgrid : TABLE_WG), dim3(TPB), 0, s,
                       (const int*)components, (const int16_t*)key,
                       (const int*)sizes, n_regions, (unsigned)total, table);
    DRAM_LAUNCH_CHECK();
  }
  if (cluster_voxels) {
    DramProf prof(DRAM_FAM_PREP, 20, 0.0, vox * 12.0, s);
    hipLaunchKernelGGL(ccl_gather_kernel, dim3(vgrid), dim3(TPB), 0, s, (const int*)components, (const int*)sizes,
                       cluster_voxels, (unsigned)total);
    DRAM_LAUNCH_CHECK();
  }
  return DRAM_OK;
}

}  // namespace

extern "C" size_t dram_label_components_workspace(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1 || (long long)D * H * W >= (1LL << 31)) return 0;
  const long long total = (long long)D * H * W;
  return (size_t)(vol_bytes(total, 4) + vol_bytes(total, 2));
}

extern "C" int dram_label_components(const void* key_or_labels, int lab_elem, long long stride_z, long long stride_y,
                                     const int16_t* image, int threshold, int by_lobe, int connectivity, int n_regions,
                                     int32_t* components, int32_t* cluster_voxels, int64_t* table, void* work, int D, int H,
                                     int W, dram_stream_t stream) {
  if (!key_or_labels || !components || !table || !work || (lab_elem != 1 && lab_elem != 2) || stride_z < 0 ||
      stride_y < 0 || D < 1 || H < 1 || W < 1 || (connectivity != 6 && connectivity != 26) || n_regions < 1 ||
      n_regions > MAX_ROWS - 1 || threshold < -32768 || threshold > 32768)
    return DRAM_ERR_BAD_ARG;
  if ((long long)D * H * W >= (1LL << 31)) return DRAM_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  return with_label_type(lab_elem, [&](auto t) {
    return run<decltype(t)>(key_or_labels, (long)stride_z, (long)stride_y, image, threshold, by_lobe ? 1 : 0, connectivity,
                            n_regions, (int*)components, (int*)cluster_voxels, (unsigned long long*)table, work, D, H, W, s);
  });
}
