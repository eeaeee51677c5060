// wino_gemm.hip -- the batched GEMMs on the gfx950 matrix cores behind the Winograd pipeline of conv_wino.hip
// (64-216 dense GEMMs per convolution, one per Winograd point) and, as plain GEMMs with one "point", the
// 1x1x1 convolutions of the Bottleneck blocks.
//
//   NN  Y[xi][m][n] = sum_k A[xi][m][k] * Bw[xi][n][k]          forward and data gradient     run_nn
//   TN  slab[split][xi][m][n] = sum_t Ah[xi][t][m] * Bh[xi][t][n]   weight gradient           run_tn
//
// GEMM kernels: 512 threads (8 waves as 4(M) x 2(N)), tile 256 x (64*NJ) x 32, operands staged by
// LDS-DMA (global_load_lds_dwordx4), double-buffered, one barrier per K-step; NN form reads both
// operands with the ds_read_b128 k-permutation trick of conv_igemm.hip, TN form reads [t][c] rows
// with ds_read_b32 (lanes = consecutive channels).  Opt-in bf16 matrix-core forms of both (DRAM_MATH,
// split-bf16 operand images, see split_pack in conv_wino.hip / wino_gemm_nn_bf16_kernel / wino_gemm_tn_bf16_kernel).
// The fp32 TN GEMM has a streaming form (64 x 128, HBM-bound) and a persistent form (short K) beside its one-tile kernels.
// Written once and shared: the NN tile decode and operand DMA with its swizzle (one-tile, persistent and bf16 kernels),
// the lane roles and the fp32 k-group loop (one-tile and persistent kernels), the TN tile / split decode (generic and
// bf16 kernels).  The LDS-turn epilogue is still written twice, in the one-tile and in the persistent kernel: see the
// note in front of the persistent kernel's copy before changing either.
#include <stdlib.h>
#include "wino_gemm.h"

namespace {

template <int MI, int NJ>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[MI][NJ]) {
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][nj][e] = 0.f;
}

// ------------------------------------------------------------------------------------------
// NN batched GEMM:  Y[xi][m][n] = sum_k A[xi][m][k] * Bw[xi][n][k]     (M = Tpad, K % 32 == 0)
// Shared pieces of the one-tile, persistent and bf16 kernels (the bf16 kernel computes its own lane roles).

// Tile idx of a launch (n tiles fastest, then m tiles, then points) -> its operand and result blocks.
struct NnTile { const float* Ab; const float* Bb; float* Yb; int mt, nt; };
template <int NJ>
__device__ __forceinline__ NnTile nn_tile(const int idx, const float* A, const float* Bw, float* Y, const int N,
                                          const int K, const int m_tiles, const int n_tiles, const int nblk,
                                          const int npts) {
  constexpr int BN = 64 * NJ;
  const int L = xcd_remap(idx, nblk);
  NnTile t;
  t.nt = L % n_tiles;
  const int r0 = L / n_tiles;
  t.mt = r0 % m_tiles;
  const int xi = r0 / m_tiles;
  t.Ab = A + (((long)t.mt * npts + xi) * 256) * K;
  t.Bb = Bw + ((long)xi * N + (long)t.nt * BN) * K;
  t.Yb = Y + (((long)t.mt * npts + xi) * 256) * N + t.nt * BN;
  return t;
}

// A lane's place among the 8 waves (wave = wn * 4 + wm, wave tile 64 x 32 NJ) and its read offsets inside a stage
// (A rows first, then B rows, 32 floats each; rsw undoes the DMA's slot swizzle).
template <int NJ>
struct NnLane {
  int tid, lane, wave, li, lh, wm, wn, rsw, a_row, b_row;
  __device__ __forceinline__ NnLane() {
    tid = threadIdx.x;
    lane = tid & 63;
    wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    li = lane & 31; lh = lane >> 5;
    wm = wave & 3; wn = wave >> 2;
    rsw = (li >> 1) & 7;
    a_row = (wm * 64 + li) * 32;
    b_row = 256 * 32 + (wn * NJ * 32 + li) * 32;
  }
};

// Operand DMA of one 32-wide k step into a stage (256 A rows, then 64 NJ B rows).
// DMA pieces (8 rows x 128 B each): A rows 32*wave + 8j + sub, B rows 8*NJ*wave + 8jj + sub.
// 16-B slot swizzle slot ^ ((row >> 1) & 7) applied on the source address.
template <int NJ>
struct NnDma {
  int wave, aoff[4], boff[NJ];
  __device__ __forceinline__ NnDma(const int lane, const int wave_, const int K) : wave(wave_) {
    const int sub = lane >> 3, pslot = lane & 7;
    const int s_even = pslot ^ (lane >> 4), s_odd = s_even ^ 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) aoff[j] = (32 * wave + 8 * j + sub) * K + ((j & 1) ? s_odd : s_even) * 4;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      const int nrow = 8 * NJ * wave + 8 * jj + sub;
      boff[jj] = nrow * K + (pslot ^ ((nrow >> 1) & 7)) * 4;
    }
  }
  __device__ __forceinline__ void issue(const float* Ab, const float* Bb, const int it, float* stage) const {
    float* as = stage + 32 * wave * 32;
    float* bs = stage + 256 * 32 + 8 * NJ * wave * 32;
    const float* ag = Ab + it * 32;
    const float* bg = Bb + it * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ag + aoff[j]),
                                       (__attribute__((address_space(3))) void*)(as + j * 8 * 32), 16, 0, 0);
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bg + boff[jj]),
                                       (__attribute__((address_space(3))) void*)(bs + jj * 8 * 32), 16, 0, 0);
  }
};

// The four k-groups of a landed fp32 stage: 4 x 4 x NJ x 2 MFMAs.
template <int NJ>
__device__ __forceinline__ void nn_kgroups(const float* st, const NnLane<NJ>& ln, f32x16 (&acc)[2][NJ]) {
  // operand fragments double-buffered in registers: the reads of k-group gk + 1 are issued in front of the
  // MFMAs of gk (left to the scheduler they came one MFMA before their use)
  f32x4 a0[2], a1[2], bf[2][NJ];
  auto frag = [&](int gk, int buf) __attribute__((always_inline)) {
    const int so = ((2 * gk + ln.lh) ^ ln.rsw) * 4;
    a0[buf] = *reinterpret_cast<const f32x4*>(st + ln.a_row + so);
    a1[buf] = *reinterpret_cast<const f32x4*>(st + ln.a_row + 32 * 32 + so);
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) bf[buf][nj] = *reinterpret_cast<const f32x4*>(st + ln.b_row + nj * 32 * 32 + so);
  };
  frag(0, 0);
#pragma unroll
  for (int gk = 0; gk < 4; ++gk) {
    if (gk + 1 < 4) frag(gk + 1, (gk + 1) & 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) {
        acc[0][nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[gk & 1][e], bf[gk & 1][nj][e], acc[0][nj], 0, 0, 0);
        acc[1][nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[gk & 1][e], bf[gk & 1][nj][e], acc[1][nj], 0, 0, 0);
      }
    }
    // pin the order inside the region: the (2 + NJ) fragment reads of the next group first, then the MFMAs
    if (gk + 1 < 4) __builtin_amdgcn_sched_group_barrier(0x100, 2 + NJ, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 8 * NJ, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One 256 x 64 NJ tile per workgroup, two stages in one LDS array.  Optional fused epilogue (GemmEpilogue).
template <int NJ>
__global__ __launch_bounds__(512) void wino_gemm_nn_kernel(const float* __restrict__ A, const float* __restrict__ Bw,
                                                           float* __restrict__ Y, const int Mpad, const int N,
                                                           const int K, const int m_tiles, const int n_tiles,
                                                           const int nblk, const int npts, const GemmEpilogue ep) {
  constexpr int STAGE = (256 + 64 * NJ) * 32;
  __shared__ __attribute__((aligned(1024))) float lds[2 * STAGE];
  const NnLane<NJ> ln;
  const NnTile t = nn_tile<NJ>(blockIdx.x, A, Bw, Y, N, K, m_tiles, n_tiles, nblk, npts);
  const NnDma<NJ> dma(ln.lane, ln.wave, K);
  const int niter = K / 32;
  f32x16 acc[2][NJ];
  zero_acc(acc);

  dma.issue(t.Ab, t.Bb, 0, lds);
  for (int it = 0; it < niter; ++it) {
    __syncthreads();   // tile `it` has landed; stage (it+1)&1 is free again
    if (it + 1 < niter) dma.issue(t.Ab, t.Bb, it + 1, lds + ((it + 1) & 1) * STAGE);
    nn_kgroups<NJ>(lds + (it & 1) * STAGE, ln, acc);
  }

  constexpr int BN = 64 * NJ;
  const bool fused = ep.bias || ep.add || ep.stats;       // uniform
  // Store through LDS (every Winograd-domain GEMM of the pipeline, and the 1x1x1 convolutions with their fused
  // epilogues): the 32x32 accumulator layout gives a lane ONE column, so direct stores are 32 dword stores per
  // accumulator in 128-B pieces -- 64 vector-memory instructions per wave behind only 128 MFMAs when K = 64 -- and
  // the shortcut-gradient epilogue adds two dword loads per element (ResNet-50's 1024->256 data gradient: 186 us
  // against 81 us for the forward of the same layer).  Each wave turns 32 rows x 64 (32) columns at a time through
  // a private LDS region (row pitch + 8 floats: the two row groups of a write land in different bank halves) and
  // moves 16 B per lane: a quarter of the memory instructions, whole 256-B (128-B) row pieces.
  constexpr int CW = NJ >= 2 ? 64 : 32;                 // columns per round
  constexpr int NR = NJ >= 2 ? NJ / 2 : 1;              // column rounds
  constexpr int P = CW + 8;
  constexpr int Q = CW / 4;                             // 4-column groups per row
  __syncthreads();                                      // every wave is done with the last operand stage
  float* reg = lds + ln.wave * (32 * P);
  const int cq = ln.lane % Q, rs = ln.lane / Q;
  float s1[NR][4], s2[NR][4];
#pragma unroll
  for (int cr = 0; cr < NR; ++cr)
#pragma unroll
    for (int j = 0; j < 4; ++j) { s1[cr][j] = 0.f; s2[cr][j] = 0.f; }
#pragma unroll
  for (int cr = 0; cr < NR; ++cr) {
    const int col = t.nt * BN + ln.wn * NJ * 32 + cr * CW + 4 * cq;          // column of Y (and of bias)
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (ep.bias) bv = *reinterpret_cast<const f32x4*>(ep.bias + col);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int e = 0; e < 16; ++e)
#pragma unroll
        for (int j = 0; j < CW / 32; ++j)
          reg[((e & 3) + 8 * (e >> 2) + 4 * ln.lh) * P + j * 32 + ln.li] = acc[mi][cr * (CW / 32) + j][e];
#pragma unroll
      for (int r = 0; r < 32 / (64 / Q); ++r) {
        const int row = r * (64 / Q) + rs;
        f32x4 v = *reinterpret_cast<const f32x4*>(reg + row * P + 4 * cq);
        float* o = t.Yb + (long)(ln.wm * 64 + mi * 32 + row) * N + ln.wn * NJ * 32 + cr * CW + 4 * cq;
        if (fused) {
          v += bv;
          if (ep.add) {
            const long oo = o - Y;
            const f32x4 av = *reinterpret_cast<const f32x4*>(ep.add + oo);
            if (ep.gate) {
              const f32x4 gv = *reinterpret_cast<const f32x4*>(ep.gate + oo);
#pragma unroll
              for (int j = 0; j < 4; ++j) v[j] += gv[j] > 0.f ? av[j] : 0.f;
            } else {
              v += av;
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) { s1[cr][j] += v[j]; s2[cr][j] += v[j] * v[j]; }
        }
        *reinterpret_cast<f32x4*>(o) = v;
      }
    }
  }
  if (ep.stats) {
#pragma unroll
    for (int cr = 0; cr < NR; ++cr)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int o = Q; o < 64; o <<= 1) {
          s1[cr][j] += __shfl_xor(s1[cr][j], o, 64);
          s2[cr][j] += __shfl_xor(s2[cr][j], o, 64);
        }
    __syncthreads();                                    // every wave is done with its turn region
    float* red = lds;  // [8 waves][2][32 * NJ]
    if (rs == 0) {
#pragma unroll
      for (int cr = 0; cr < NR; ++cr)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          red[(ln.wave * 2 + 0) * 32 * NJ + cr * CW + 4 * cq + j] = s1[cr][j];
          red[(ln.wave * 2 + 1) * 32 * NJ + cr * CW + 4 * cq + j] = s2[cr][j];
        }
    }
    __syncthreads();
    if (ln.tid < 2 * BN) {
      const int which = ln.tid / BN, cc = ln.tid - which * BN;       // column within the workgroup's BN
      const int cwn = cc / (32 * NJ), c2 = cc - cwn * 32 * NJ;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) v += red[((cwn * 4 + w) * 2 + which) * 32 * NJ + c2];   // wave = wn * 4 + wm
      ep.stats[((long)t.mt * 2 + which) * N + t.nt * BN + cc] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Persistent form of wino_gemm_nn_kernel (round 5) for the matrix-bound launches.  A workgroup of the one-tile kernel
// lives for K / 32 = 4-16 main-loop iterations: it starts with a cold pipeline (the first 48-64 KB stage is a full
// memory round trip with nothing to compute), ends with an epilogue during which the matrix pipe idles, and the
// launch runs in whole rounds of 256 workgroups -- the 128- / 256-channel stages of the network (432 / 864 tiles) sat
// at 0.48 / 0.68 of the pipe where the 512-channel ones (1 728 tiles) reach 0.76.  Here gridDim.x <= 256 workgroups
// (one per CU) walk the tiles b, b + gridDim.x, ...; the FIRST stage of a workgroup's next tile is issued under the
// last k-group of the current one, so it lands during that k-group and the epilogue, and the next tile's MFMAs start
// right behind the epilogue's stores.  Needs an even number of iterations (the stage parity is then the same for
// every tile; K is a multiple of 64 everywhere in the network) and the two stages as separate LDS objects: the
// epilogue turns its accumulators through stage 1 (16 rows per wave at a time, 37 KB) while the prefetch fills
// stage 0, and the wait-count pass must be able to tell the two apart (wait-count traps) --
// which is why the shared pieces take stage POINTERS and never an index into one array.
// Accumulation order, epilogue arithmetic and results are those of the one-tile kernel, bit for bit (tested).
template <int NJ>
__global__ __launch_bounds__(512) void wino_gemm_nn_pers_kernel(const float* __restrict__ A, const float* __restrict__ Bw,
                                                                float* __restrict__ Y, const int Mpad, const int N,
                                                                const int K, const int m_tiles, const int n_tiles,
                                                                const int nblk, const int npts, const GemmEpilogue ep) {
  constexpr int STAGE = (256 + 64 * NJ) * 32;
  // (NJ = 1: 2 x 40 KB would let two persistent workgroups share a CU and leave others empty -- pad past half the LDS)
  __shared__ __attribute__((aligned(1024))) float s0[STAGE];
  __shared__ __attribute__((aligned(1024))) float s1[STAGE + (NJ == 1 ? 1024 : 0)];
  const NnLane<NJ> ln;
  const NnDma<NJ> dma(ln.lane, ln.wave, K);
  constexpr int BN = 64 * NJ;
  const int niter = K / 32;                                  // even (host-checked)
  const bool fused = ep.bias || ep.add || ep.stats;          // uniform
  f32x16 acc[2][NJ];

  int idx = blockIdx.x;
  NnTile cur = nn_tile<NJ>(idx, A, Bw, Y, N, K, m_tiles, n_tiles, nblk, npts);
  dma.issue(cur.Ab, cur.Bb, 0, s0);
  for (;;) {
    const int nxt = idx + gridDim.x;
    const bool more = nxt < nblk;                             // uniform
    NnTile nx = cur;
    if (more) nx = nn_tile<NJ>(nxt, A, Bw, Y, N, K, m_tiles, n_tiles, nblk, npts);
    zero_acc(acc);
    for (int it = 0; it < niter; it += 2) {
      __syncthreads();                 // stage 0 (iteration it) has landed; stage 1 is free
      dma.issue(cur.Ab, cur.Bb, it + 1, s1);
      nn_kgroups<NJ>(s0, ln, acc);
      __syncthreads();                 // stage 1 has landed; stage 0 is free
      if (it + 2 < niter) dma.issue(cur.Ab, cur.Bb, it + 2, s0);
      else if (more) dma.issue(nx.Ab, nx.Bb, 0, s0);         // the NEXT tile's first stage: lands under the epilogue
      nn_kgroups<NJ>(s1, ln, acc);
    }

    // epilogue through LDS (stage 1's space; the prefetch owns stage 0): per wave 16 rows x CW columns at a time.
    // The one-tile kernel's epilogue with 16 instead of 32 rows per turn (region row (e & 3) + 8 * ((e >> 2) & 1) +
    // 4 * lh; a lane meets its rows in the same ascending order, so the statistics are the same bits).  Kept as a copy:
    // as a shared function -- even the statistics fold alone -- it compiled to another order of DMA issues, LDS reads
    // and waits in this kernel's main loop and epilogue, which no measurement has covered yet.
    constexpr int CW = NJ >= 2 ? 64 : 32;                 // columns per round
    constexpr int NR = NJ >= 2 ? NJ / 2 : 1;              // column rounds
    constexpr int P = CW + 8;
    constexpr int Q = CW / 4;                             // 4-column groups per row
    __syncthreads();                                      // every wave is done with the last operand stage
    float* reg = s1 + ln.wave * (16 * P);
    const int cq = ln.lane % Q, rs = ln.lane / Q;
    float s1v[NR][4], s2v[NR][4];
#pragma unroll
    for (int cr = 0; cr < NR; ++cr)
#pragma unroll
      for (int j = 0; j < 4; ++j) { s1v[cr][j] = 0.f; s2v[cr][j] = 0.f; }
#pragma unroll
    for (int cr = 0; cr < NR; ++cr) {
      const int col = cur.nt * BN + ln.wn * NJ * 32 + cr * CW + 4 * cq;          // column of Y (and of bias)
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (ep.bias) bv = *reinterpret_cast<const f32x4*>(ep.bias + col);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {                     // accumulator rows 16 h .. 16 h + 15 of the 32-row block
#pragma unroll
          for (int e = 8 * h; e < 8 * h + 8; ++e)
#pragma unroll
            for (int j = 0; j < CW / 32; ++j)
              reg[((e & 3) + 8 * ((e >> 2) & 1) + 4 * ln.lh) * P + j * 32 + ln.li] = acc[mi][cr * (CW / 32) + j][e];
#pragma unroll
          for (int r = 0; r < 16 / (64 / Q); ++r) {
            const int row = r * (64 / Q) + rs;
            f32x4 v = *reinterpret_cast<const f32x4*>(reg + row * P + 4 * cq);
            float* o = cur.Yb + (long)(ln.wm * 64 + mi * 32 + 16 * h + row) * N + ln.wn * NJ * 32 + cr * CW + 4 * cq;
            if (fused) {
              v += bv;
              if (ep.add) {
                const long oo = o - Y;
                const f32x4 av = *reinterpret_cast<const f32x4*>(ep.add + oo);
                if (ep.gate) {
                  const f32x4 gv = *reinterpret_cast<const f32x4*>(ep.gate + oo);
#pragma unroll
                  for (int j = 0; j < 4; ++j) v[j] += gv[j] > 0.f ? av[j] : 0.f;
                } else {
                  v += av;
                }
              }
#pragma unroll
              for (int j = 0; j < 4; ++j) { s1v[cr][j] += v[j]; s2v[cr][j] += v[j] * v[j]; }
            }
            *reinterpret_cast<f32x4*>(o) = v;
          }
        }
      }
    }
    if (ep.stats) {
#pragma unroll
      for (int cr = 0; cr < NR; ++cr)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int o = Q; o < 64; o <<= 1) {
            s1v[cr][j] += __shfl_xor(s1v[cr][j], o, 64);
            s2v[cr][j] += __shfl_xor(s2v[cr][j], o, 64);
          }
      __syncthreads();                                    // every wave is done with its turn region
      float* red = s1;  // [8 waves][2][32 * NJ]
      if (rs == 0) {
#pragma unroll
        for (int cr = 0; cr < NR; ++cr)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            red[(ln.wave * 2 + 0) * 32 * NJ + cr * CW + 4 * cq + j] = s1v[cr][j];
            red[(ln.wave * 2 + 1) * 32 * NJ + cr * CW + 4 * cq + j] = s2v[cr][j];
          }
      }
      __syncthreads();
      if (ln.tid < 2 * BN) {
        const int which = ln.tid / BN, cc = ln.tid - which * BN;       // column within the workgroup's BN
        const int cwn = cc / (32 * NJ), c2 = cc - cwn * 32 * NJ;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) v += red[((cwn * 4 + w) * 2 + which) * 32 * NJ + c2];   // wave = wn * 4 + wm
        ep.stats[((long)cur.mt * 2 + which) * N + cur.nt * BN + cc] = v;
      }
    }
    if (!more) break;
    idx = nxt;
    cur = nx;
  }
}
// ------------------------------------------------------------------------------------------
// Streaming form of the NN batched GEMM for the launches that are HBM-bound whatever the tile: few channels on both
// sides (K <= 128 and N <= 128 -- the 128->64 decoder convolution on 2 x 64 x 128 x 128 voxels moves 5.4 GB through
// each of its GEMMs for 116 GFLOP).  wino_gemm_nn_kernel gives such a launch one or two 40-48 KB stages in flight per
// CU and a cold pipeline every K / 32 = 2-4 iterations (a workgroup lives for one 256-row tile): 3.5-3.8 TB/s.  Here a
// workgroup is PERSISTENT: it owns a contiguous run of (point, 64-row tile) items, keeps the point's whole B operand in
// REGISTERS (64 per lane, re-read from a 32-KB LDS image only when the point changes), and streams 64 x K A tiles
// through a ring of S LDS stages filled by LDS-DMA S - 1 items ahead (2-3 x 16-32 KB in flight per CU the whole time;
// counted s_waitcnt vmcnt + one barrier per item).  Results leave through a wave-private LDS turn (16 B per lane).
// LDS rows are K floats; 16-B slot s of row r lives at slot (s & ~15) | ((s ^ r) & 15) (applied on the DMA source
// side and on the reads: the 16 lanes of a ds_read_b128 group hit 16 different 16-B columns).
// Cache policy of the streaming GEMM's once-read A stream (aux of global_load_lds: 2 = non-temporal); A/B build flag
// (DRAM_EXTRA_HIPCC_FLAGS under DRAM_TUNING=1).  Measured, config 1: 765 -> 743-754 us (64->64 @ 64x128x128), 1 260 ->
// 1 227-1 245: kept.  Non-temporal STORES of the result (gated by image size or not) and non-temporal operand loads in the
// TN GEMMs: no effect beyond the run-to-run drift inside one process (the second run of a pair is ~2 % faster whatever
// it runs); not kept.
#ifndef DRAM_STREAM_NT
#define DRAM_STREAM_NT 2
#endif
// DB ("direct B", round 5): the point's B fragments are loaded from global memory straight into the registers that hold
// them (16 KB per point, L2-resident, once per 100-200 items) instead of through a 16-KB LDS image, and the ring is three
// stages deep: 68 KB of LDS, so TWO workgroups share a CU -- one's MFMAs and LDS turn run under the other's waits and
// stores (one workgroup per CU = one wave per SIMD leaves every wait of a wave exposed).  64 -> 64 launches only.
// KH = 2 (K = 128, DB only): an item is one 64-wide k-HALF of a 64-row tile -- 16-KB stages like the K = 64 forms, so the
// ring still fits twice on a CU; the accumulators run over the two halves of a tile in k order (bit-identical to the
// whole-row form) and the turn + store follow the second half.
template <int NJ, int KT, int S, bool DB = false, int KH = 1>
__global__ __launch_bounds__(256, DB ? 2 : 1) void wino_gemm_nn_stream_kernel(const float* __restrict__ A,
                                                                    const float* __restrict__ Bw, float* __restrict__ Y,
                                                                    const int npts, const int m64, const int per_wg,
                                                                    const int total) {
  constexpr int N = 64 * NJ;
  constexpr int STG = 64 * KT;                     // floats per A stage
  constexpr int SPR = KT / 4;                      // 16-B slots per row
  constexpr int RPI = 64 / SPR;                    // rows per DMA instruction (1 KB)
  constexpr int IPW = 64 / RPI / 4;                // A DMA instructions per wave and stage
  constexpr int BPW = N / RPI / 4;                 // B DMA instructions per wave
  constexpr int KG = KT / 8;                       // k-groups (one ds_read_b128 per lane each)
  constexpr int P = DB ? 40 : 32 * NJ + 8;         // DB: the turn takes one 32-column block at a time (20 KB whatever NJ)
  constexpr int KS = KT * KH;                      // row length of A and B in memory (K)
  static_assert(S == 3 || S == 4, "ring depth");
  static_assert(KH == 1 || (KH == 2 && DB && S == 3), "k halves: direct-B form, three stages");
  // separate LDS objects per stage (the wait-count pass tells DMA targets apart by object)
  __shared__ __attribute__((aligned(1024))) float st0[STG], st1[STG], st2[STG], st3[S == 4 ? STG : 64];
  __shared__ __attribute__((aligned(1024))) float bt[DB ? 64 : N * KT];
  __shared__ __attribute__((aligned(16))) float turn[4 * 32 * P];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int i0 = blockIdx.x * per_wg;
  const int n = (i0 + per_wg <= total ? per_wg : total - i0);
  if (n <= 0) return;

  // per-lane DMA source offsets (floats) inside a 64 x KT (A) / N x KT (B) tile
  int aoff[IPW], boff[BPW];
#pragma unroll
  for (int j = 0; j < IPW; ++j) {
    const int row = RPI * (wave + 4 * j) + lane / SPR, ph = lane % SPR;
    aoff[j] = row * KS + ((ph & ~15) | ((ph ^ row) & 15)) * 4;
  }
#pragma unroll
  for (int j = 0; j < BPW; ++j) {
    const int row = RPI * (wave + 4 * j) + lane / SPR, ph = lane % SPR;
    boff[j] = row * KT + ((ph & ~15) | ((ph ^ row) & 15)) * 4;
  }
  auto a_src = [&](int item) __attribute__((always_inline)) {
    const int ti = item / KH, h = item - ti * KH;
    const int xi = ti / m64, t = ti - xi * m64;
    return A + (((long)(t >> 2) * npts + xi) * 256 + (t & 3) * 64) * KS + h * KT;
  };
  auto issue_a = [&](int item, float* stage) __attribute__((always_inline)) {
    const float* src = a_src(item);
#pragma unroll
    for (int j = 0; j < IPW; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + aoff[j]),
                                       (__attribute__((address_space(3))) void*)(stage + (wave + 4 * j) * 256), 16, 0,
                                       DRAM_STREAM_NT);
  };
  auto stage_of = [&](int k) __attribute__((always_inline)) -> float* {
    return k == 0 ? st0 : (k == 1 ? st1 : (k == 2 ? st2 : st3));
  };

  const int r0 = 32 * (wave & 1), c0 = 32 * NJ * (wave >> 1);
  const int arow = r0 + li;
  f32x4 bfr[NJ][KG * KH];
  auto load_b = [&](int xi) __attribute__((always_inline)) {
    if (DB) {
      const float* srcd = Bw + (long)xi * N * KS;
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int kg = 0; kg < KG * KH; ++kg)
          bfr[nj][kg] = *reinterpret_cast<const f32x4*>(srcd + (c0 + nj * 32 + li) * KS + (2 * kg + lh) * 4);
      __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): the counted waits below start from an empty queue
      asm volatile("" ::: "memory");
      return;
    }
    __syncthreads();                               // (no wave still reads the previous point's image)
    const float* src = Bw + (long)xi * N * KT;
#pragma unroll
    for (int j = 0; j < BPW; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + boff[j]),
                                       (__attribute__((address_space(3))) void*)(bt + (wave + 4 * j) * 256), 16, 0, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
    asm volatile("" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      const int brow = c0 + nj * 32 + li;
#pragma unroll
      for (int kg = 0; kg < KG; ++kg) {
        const int sl = 2 * kg + lh;
        bfr[nj][kg] = *reinterpret_cast<const f32x4*>(bt + brow * KT + ((sl & ~15) | ((sl ^ brow) & 15)) * 4);
      }
    }
  };

  int xi_cur = i0 / KH / m64;
  // prologue: S - 1 stages ahead (the B load below waits for them too: once per point)
#pragma unroll
  for (int k = 0; k < S - 1; ++k)
    if (k < n) issue_a(i0 + k, stage_of(k));
  load_b(xi_cur);

  float* reg = turn + wave * (32 * P);
  constexpr int Q = 8 * NJ;                        // 4-column groups per row of the wave's 32 NJ columns
  const int cq = lane % Q, rs = lane / Q;

  constexpr int U = S * KH;                        // unroll: stage k % S and k half k % KH are compile-time
  f32x16 acc[NJ];
  for (int itb = 0; itb < n; itb += U) {
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int it = itb + k;
      const int h = k % KH;                        // (i0 and itb are multiples of KH)
      if (it < n) {                                // uniform
        const int item = i0 + it;
        const int ti = item / KH;
        const int xi = ti / m64, t = ti - xi * m64;
        if (h == 0 && xi != xi_cur) {              // next point: its B operand (rare: a run spans 1-3 points)
          xi_cur = xi;
          load_b(xi);                              // (its vmcnt(0) also covers the stages in flight)
        }
        // stage `it` has landed for this wave when at most the S - 2 younger stages are outstanding (loads complete
        // in order; stores in between only make the wait stricter); in the tail nothing younger was issued
        if (it + S - 2 < n) __builtin_amdgcn_s_waitcnt(0x0F70 | ((IPW * (S - 2)) & 15) | (((IPW * (S - 2)) >> 4) << 14));
        else __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();              // ... and for every wave; all waves are done with stage it - 1
        if (it + S - 1 < n) issue_a(item + S - 1, stage_of((k + S - 1) % S));
        const float* stg = stage_of(k % S);
        if (h == 0) {
#pragma unroll
          for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[nj][e] = 0.f;
        }
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) {
          const int sl = 2 * kg + lh;
          const f32x4 af = *reinterpret_cast<const f32x4*>(stg + arow * KT + ((sl & ~15) | ((sl ^ arow) & 15)) * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
              acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bfr[nj][h * KG + kg][e], acc[nj], 0, 0, 0);
        }
        if (h != KH - 1) continue;                 // (compile-time: the second half of the tile follows)
        // turn through the wave's private LDS region, 16 B per lane
        float* yb = Y + (((long)(t >> 2) * npts + xi) * 256 + (t & 3) * 64 + r0) * N + c0;
        if (DB) {
          const int cq8 = lane & 7, rs8 = lane >> 3;
#pragma unroll
          for (int nj = 0; nj < NJ; ++nj) {
#pragma unroll
            for (int e = 0; e < 16; ++e) reg[((e & 3) + 8 * (e >> 2) + 4 * lh) * P + li] = acc[nj][e];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = r * 8 + rs8;
              *reinterpret_cast<f32x4*>(yb + (long)row * N + nj * 32 + 4 * cq8) =
                  *reinterpret_cast<const f32x4*>(reg + row * P + 4 * cq8);
            }
          }
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) reg[((e & 3) + 8 * (e >> 2) + 4 * lh) * P + nj * 32 + li] = acc[nj][e];
#pragma unroll
          for (int r = 0; r < Q / 2; ++r) {
            const int row = r * (64 / Q) + rs;
            *reinterpret_cast<f32x4*>(yb + (long)row * N + 4 * cq) = *reinterpret_cast<const f32x4*>(reg + row * P + 4 * cq);
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// The same NN batched GEMM on the bf16 matrix cores, operands in the split-bf16 image (split_pack):
//   NT = 3 ("bf16x3"):  a*b ~= ah*bh + ah*bl + al*bh   -- fp32 accumulation, the dropped al*bl term and the
//                       split residues are <= 2^-16 relative per product (fp32 MFMA: 2^-24)
//   NT = 1 ("bf16"):    a*b ~= ah*bh                    -- bf16 operands, fp32 accumulation (autocast-like)
// v_mfma_f32_32x32x16_bf16 runs 32 cycles for 16 k (the fp32 32x32x2 form: 64 cycles for 2 k), so three
// products per k cost 96 cycles where the fp32 kernel spends 512.  Tile, DMA pattern, swizzle and epilogue
// are those of wino_gemm_nn_kernel (the image has the same bytes per row); per 32-channel stage a lane-half
// reads hi slot 2j + lh and lo slot 4 + 2j + lh (8 channels each) for the two k16 steps j.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <int NJ, int NT>
__global__ __launch_bounds__(512) void wino_gemm_nn_bf16_kernel(const float* __restrict__ A, const float* __restrict__ Bw,
                                                                float* __restrict__ Y, const int Mpad, const int N,
                                                                const int K, const int m_tiles, const int n_tiles,
                                                                const int nblk, const int npts) {
  constexpr int STAGE = (256 + 64 * NJ) * 32;
  __shared__ __attribute__((aligned(1024))) float lds[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const NnTile t = nn_tile<NJ>(blockIdx.x, A, Bw, Y, N, K, m_tiles, n_tiles, nblk, npts);
  const NnDma<NJ> dma(lane, wave, K);
  const int niter = K / 32;
  f32x16 acc[2][NJ];
  zero_acc(acc);

  // (NnLane's values, computed here: taken from an NnLane at the top, the main loop of the one-product forms with
  // NJ >= 2 came out with its LDS reads and MFMAs in another order)
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave & 3, wn = wave >> 2;
  const int rsw = (li >> 1) & 7;
  const int a_row = (wm * 64 + li) * 32;
  const int b_row = 256 * 32 + (wn * NJ * 32 + li) * 32;

  dma.issue(t.Ab, t.Bb, 0, lds);
  for (int it = 0; it < niter; ++it) {
    __syncthreads();
    if (it + 1 < niter) dma.issue(t.Ab, t.Bb, it + 1, lds + ((it + 1) & 1) * STAGE);
    const float* st = lds + (it & 1) * STAGE;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int sh = ((2 * j + lh) ^ rsw) * 4, sl = ((4 + 2 * j + lh) ^ rsw) * 4;
      bf16x8 ah[2], al[2], bh[NJ], bl[NJ];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        ah[mi] = *reinterpret_cast<const bf16x8*>(st + a_row + mi * 32 * 32 + sh);
        if (NT > 1) al[mi] = *reinterpret_cast<const bf16x8*>(st + a_row + mi * 32 * 32 + sl);
      }
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) {
        bh[nj] = *reinterpret_cast<const bf16x8*>(st + b_row + nj * 32 * 32 + sh);
        if (NT > 1) bl[nj] = *reinterpret_cast<const bf16x8*>(st + b_row + nj * 32 * 32 + sl);
      }
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          if (NT > 1) {
            acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh[nj], acc[mi][nj], 0, 0, 0);
            acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl[nj], acc[mi][nj], 0, 0, 0);
          }
          acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh[nj], acc[mi][nj], 0, 0, 0);
        }
    }
  }

#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      float* o = t.Yb + (long)row * N + wn * NJ * 32 + li;
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) o[nj * 32] = acc[mi][nj][e];
    }
}

// ------------------------------------------------------------------------------------------
// TN batched GEMM (weight gradient):
//   slab[split][xi][m][n] = sum_{t in split} Ah[xi][t][m] * Bh[xi][t][n]
// 8 waves as WMW (M) x 8/WMW (N), wave tile 32*MI x 32*NJ; M % (WMW*32*MI) == 0, N may be ragged
// (the DMA column is clamped into the row, the extra columns are never stored).
// Shared by the fp32 and the bf16 kernel: the workgroup's tile and split.
struct TnTile {
  int nt, mt, split, xi;
  int t0, t1;          // the split's rows of t
  // first of the 32 operand rows of k step `it`, in one 256-tile block: [tt / 256][xi][tt % 256 ..]
  __device__ __forceinline__ long row(const int it, const int npts) const {
    const int tt = t0 + it * 32;
    return ((long)(tt >> 8) * npts + xi) * 256 + (tt & 255);
  }
};
// (item L of a launch: n tiles fastest, then m tiles, splits, points)
__device__ __forceinline__ TnTile tn_item(int L, const int m_tiles, const int n_tiles, const int nsplit, const int kper,
                                          const int Tpad) {
  TnTile t;
  t.nt = L % n_tiles; L /= n_tiles;
  t.mt = L % m_tiles; L /= m_tiles;
  t.split = L % nsplit;
  t.xi = L / nsplit;
  t.t0 = t.split * kper;
  t.t1 = (t.t0 + kper < Tpad) ? t.t0 + kper : Tpad;
  return t;
}
__device__ __forceinline__ TnTile tn_tile(const int bid, const int nblk, const int m_tiles, const int n_tiles,
                                          const int nsplit, const int kper, const int Tpad) {
  return tn_item(xcd_remap(bid, nblk), m_tiles, n_tiles, nsplit, kper, Tpad);
}
template <int WMW, int MI, int NJ>
__global__ __launch_bounds__(512) void wino_gemm_tn_kernel(const float* __restrict__ Ah, const float* __restrict__ Bh,
                                                           float* __restrict__ slab, const int Tpad, const int M,
                                                           const int N, const int m_tiles, const int n_tiles,
                                                           const int nsplit, const int kper, const int nblk,
                                                           const int npts) {
  constexpr int WNW = 8 / WMW;
  constexpr int BM = WMW * 32 * MI, BN = WNW * 32 * NJ;
  static_assert(BM % 64 == 0 && BM <= 256 && BN % 64 == 0 && BN <= 256, "one DMA piece = 256 floats");
  constexpr int STAGE = 32 * (BM + BN);
  constexpr int AQ = BM / 4, ARPP = 64 / AQ, APW = BM / 64;   // 16-B slots per row, rows per piece, pieces per wave
  constexpr int BQ = BN / 4, BRPP = 64 / BQ, BPW = BN / 64;
  __shared__ __attribute__((aligned(1024))) float lds[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const TnTile t = tn_tile(blockIdx.x, nblk, m_tiles, n_tiles, nsplit, kper, Tpad);
  int bcol = t.nt * BN + (lane % BQ) * 4;
  if (bcol > N - 4) bcol = N - 4;
  const float* Ab = Ah + (long)(lane / AQ) * M + t.mt * BM + (lane % AQ) * 4;
  const float* Bb = Bh + (long)(lane / BQ) * N + bcol;

  auto issue = [&](int it, int stage) __attribute__((always_inline)) {
    float* as = lds + stage * STAGE;
    float* bs = as + 32 * BM;
    const long row = t.row(it, npts);
    const float* ag = Ab + row * M;
    const float* bg = Bb + row * N;
#pragma unroll
    for (int j = 0; j < APW; ++j) {
      const int p = APW * wave + j;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ag + (long)(p * ARPP) * M),
                                       (__attribute__((address_space(3))) void*)(as + p * 256), 16, 0, 0);
    }
#pragma unroll
    for (int jj = 0; jj < BPW; ++jj) {
      const int p = BPW * wave + jj;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bg + (long)(p * BRPP) * N),
                                       (__attribute__((address_space(3))) void*)(bs + p * 256), 16, 0, 0);
    }
  };

  f32x16 acc[MI][NJ];
  zero_acc(acc);

  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave % WMW, wn = wave / WMW;
  const int niter = (t.t1 - t.t0) / 32;

  if (niter > 0) issue(0, 0);
  for (int it = 0; it < niter; ++it) {
    __syncthreads();
    if (it + 1 < niter) issue(it + 1, (it + 1) & 1);
    const float* as = lds + (it & 1) * STAGE + wm * 32 * MI + li;
    const float* bs = lds + (it & 1) * STAGE + 32 * BM + wn * 32 * NJ + li;
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
      const int kr = 2 * kk + lh;
      float af[MI], bf[NJ];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) af[mi] = as[kr * BM + mi * 32];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) bf[nj] = bs[kr * BN + nj * 32];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
          acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mi], bf[nj], acc[mi][nj], 0, 0, 0);
    }
  }

  float* sb = slab + (((long)t.split * npts + t.xi) * M + t.mt * BM) * N + t.nt * BN;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * 32 * MI + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      float* o = sb + (long)row * N + wn * 32 * NJ + li;
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
        if (t.nt * BN + wn * 32 * NJ + nj * 32 + li < N) o[nj * 32] = acc[mi][nj][e];
    }
}

// ------------------------------------------------------------------------------------------
// TN GEMM for a 64 x 64 result per point (the 64->64 layers on the pipeline): wino_gemm_tn_kernel's smallest tile with
// M = 64 is 64 x 128, so half its B loads and MFMAs were padding and a workgroup kept 16 KB of real bytes in flight
// per stage (3.6 GB in 1.22 ms: 3.0 TB/s).  Here: 64 x 64, K steps of 64 rows (2 x 16 KB per stage, two stages,
// two workgroups per CU); the eight waves are (row half, column half, K half) -- the two K halves of a 32 x 32
// block meet through LDS at the end, added in a fixed order.
__global__ __launch_bounds__(512, 2) void wino_gemm_tn64_kernel(const float* __restrict__ Ah, const float* __restrict__ Bh,
                                                                float* __restrict__ slab, const int Tpad, const int nsplit,
                                                                const int kper, const int nblk, const int npts) {
  constexpr int M = 64, N = 64, KS = 64;
  constexpr int STAGE = KS * (M + N);                 // floats
  __shared__ __attribute__((aligned(1024))) float lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int L = xcd_remap(blockIdx.x, nblk);
  const int split = L % nsplit;
  const int xi = L / nsplit;
  const int t0 = split * kper;
  const int t1 = (t0 + kper < Tpad) ? t0 + kper : Tpad;
  // DMA: a piece = 4 rows x 64 floats (1 KB); a stage = 16 pieces of A + 16 of B, two of each per wave
  const int prow = lane >> 4, pcol = (lane & 15) * 4;
  auto issue = [&](int it, int stage) __attribute__((always_inline)) {
    float* as = lds + stage * STAGE;
    float* bs = as + KS * M;
    const int tt = t0 + it * KS;            // 64 rows of one 256-tile block: [tt / 256][xi][tt % 256 ..]
    const long row = ((long)(tt >> 8) * npts + xi) * 256 + (tt & 255);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = 2 * wave + j;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Ah + (row + p * 4 + prow) * M + pcol),
                                       (__attribute__((address_space(3))) void*)(as + p * 256), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Bh + (row + p * 4 + prow) * N + pcol),
                                       (__attribute__((address_space(3))) void*)(bs + p * 256), 16, 0, 0);
    }
  };
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave & 1, wn = (wave >> 1) & 1, kh = wave >> 2;
  const int niter = (t1 - t0) / KS;
  if (niter > 0) issue(0, 0);
  for (int it = 0; it < niter; ++it) {
    __syncthreads();
    if (it + 1 < niter) issue(it + 1, (it + 1) & 1);
    const float* as = lds + (it & 1) * STAGE + (kh * 32) * M + wm * 32 + li;
    const float* bs = lds + (it & 1) * STAGE + KS * M + (kh * 32) * N + wn * 32 + li;
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
      const int kr = 2 * kk + lh;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[kr * M], bs[kr * N], acc, 0, 0, 0);
    }
  }
  // K halves: kh = 1 hands its block over through LDS, kh = 0 adds (fixed order) and stores
  __syncthreads();
  float* ex = lds + (wave & 3) * 1024;
  if (kh == 1) {
#pragma unroll
    for (int e = 0; e < 16; ++e) ex[e * 64 + lane] = acc[e];
  }
  __syncthreads();
  if (kh == 0) {
    float* sb = slab + (((long)split * npts + xi) * M) * N;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      sb[(long)row * N + wn * 32 + li] = acc[e] + ex[e * 64 + lane];
    }
  }
}

// ------------------------------------------------------------------------------------------
// Persistent form of wino_gemm_tn_kernel for the short-K launches (kper / 32 = 4 k steps: the 128- and 256-channel
// layers at 16 x 32 x 32, where the one-tile kernel's cold first stage and its store epilogue are as long as its main
// loop; measured on config 1's shapes, one-tile -> persistent: 256 -> 256 167 -> 155 us, 128 -> 256 90 -> 83, 128 -> 128
// 45.8 -> 42.7).  A workgroup walks a contiguous run of per_wg items (tn_item order, the runs dealt out XCD by XCD); the FIRST
// stage of its next item is issued under the last k step of the current one, so it is in flight during that step and
// the accumulator stores.  Needs an even number of k steps, the same for every item (host-checked), and the two
// stages as separate LDS objects (the wait-count pass tells DMA targets apart by object only).  Every item is computed
// exactly as wino_gemm_tn_kernel computes it: same rows per MFMA, same order, same bits (tested).
template <int WMW, int MI, int NJ>
__global__ __launch_bounds__(512) void wino_gemm_tn_pers_kernel(const float* __restrict__ Ah, const float* __restrict__ Bh,
                                                                float* __restrict__ slab, const int Tpad, const int M,
                                                                const int N, const int m_tiles, const int n_tiles,
                                                                const int nsplit, const int kper, const int nblk,
                                                                const int npts, const int per_wg) {
  constexpr int WNW = 8 / WMW;
  constexpr int BM = WMW * 32 * MI, BN = WNW * 32 * NJ;
  static_assert(BM % 64 == 0 && BM <= 256 && BN % 64 == 0 && BN <= 256, "one DMA piece = 256 floats");
  constexpr int AQ = BM / 4, ARPP = 64 / AQ, APW = BM / 64;   // 16-B slots per row, rows per piece, pieces per wave
  constexpr int BQ = BN / 4, BRPP = 64 / BQ, BPW = BN / 64;
  // (A and B rows of a stage apart as well: in one object the reads of the B rows were guarded by a vmcnt(0) against the
  // DMA just issued into the OTHER stage, seen in the ISA of the forms with NJ >= 2)
  __shared__ __attribute__((aligned(1024))) float a0[32 * BM], a1[32 * BM];
  __shared__ __attribute__((aligned(1024))) float b0[32 * BN], b1[32 * BN];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave % WMW, wn = wave / WMW;
  const int first = xcd_remap(blockIdx.x, gridDim.x) * per_wg;
  const int last = first + per_wg < nblk ? first + per_wg : nblk;
  if (first >= last) return;
  const int niter = kper / 32;                               // even, every split whole (host-checked)

  // a lane's DMA sources of an item (the B column clamped into the row: ragged N)
  auto a_src = [&](const TnTile& t) __attribute__((always_inline)) {
    return Ah + (long)(lane / AQ) * M + t.mt * BM + (lane % AQ) * 4;
  };
  auto b_src = [&](const TnTile& t) __attribute__((always_inline)) {
    int bcol = t.nt * BN + (lane % BQ) * 4;
    if (bcol > N - 4) bcol = N - 4;
    return Bh + (long)(lane / BQ) * N + bcol;
  };
  auto issue = [&](const TnTile& t, const float* Ab, const float* Bb, int it, float* as, float* bs)
      __attribute__((always_inline)) {
    const long row = t.row(it, npts);
    const float* ag = Ab + row * M;
    const float* bg = Bb + row * N;
#pragma unroll
    for (int j = 0; j < APW; ++j) {
      const int p = APW * wave + j;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ag + (long)(p * ARPP) * M),
                                       (__attribute__((address_space(3))) void*)(as + p * 256), 16, 0, 0);
    }
#pragma unroll
    for (int jj = 0; jj < BPW; ++jj) {
      const int p = BPW * wave + jj;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bg + (long)(p * BRPP) * N),
                                       (__attribute__((address_space(3))) void*)(bs + p * 256), 16, 0, 0);
    }
  };
  f32x16 acc[MI][NJ];
  // the 32 rows of a landed stage, two per MFMA (lane half lh takes row 2 kk + lh), in increasing order
  auto kstep = [&](const float* sa, const float* sb) __attribute__((always_inline)) {
    const float* as = sa + wm * 32 * MI + li;
    const float* bs = sb + wn * 32 * NJ + li;
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
      const int kr = 2 * kk + lh;
      float af[MI], bf[NJ];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) af[mi] = as[kr * BM + mi * 32];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) bf[nj] = bs[kr * BN + nj * 32];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
          acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mi], bf[nj], acc[mi][nj], 0, 0, 0);
    }
  };

  int idx = first;
  TnTile cur = tn_item(idx, m_tiles, n_tiles, nsplit, kper, Tpad);
  const float* Ab = a_src(cur);
  const float* Bb = b_src(cur);
  issue(cur, Ab, Bb, 0, a0, b0);
  for (;;) {
    const bool more = idx + 1 < last;                         // uniform
    TnTile nx = cur;
    if (more) nx = tn_item(idx + 1, m_tiles, n_tiles, nsplit, kper, Tpad);
    const float* nAb = a_src(nx);
    const float* nBb = b_src(nx);
    zero_acc(acc);
    for (int it = 0; it < niter; it += 2) {
      __syncthreads();                 // stage 0 (k step it) has landed; stage 1 is free
      issue(cur, Ab, Bb, it + 1, a1, b1);
      kstep(a0, b0);
      __syncthreads();                 // stage 1 has landed; stage 0 is free
      if (it + 2 < niter) issue(cur, Ab, Bb, it + 2, a0, b0);
      else if (more) issue(nx, nAb, nBb, 0, a0, b0);             // the NEXT item's first stage: lands under the stores
      kstep(a1, b1);
    }
    float* sb = slab + (((long)cur.split * npts + cur.xi) * M + cur.mt * BM) * N + cur.nt * BN;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wm * 32 * MI + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        float* o = sb + (long)row * N + wn * 32 * NJ + li;
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
          if (cur.nt * BN + wn * 32 * NJ + nj * 32 + li < N) o[nj * 32] = acc[mi][nj][e];
      }
    if (!more) break;
    ++idx;
    cur = nx;
    Ab = nAb;
    Bb = nBb;
  }
}

// ------------------------------------------------------------------------------------------
// Streaming form of wino_gemm_tn_kernel<2, 1, 1> for the HBM-bound 64 x 128 launches of the pipeline (the 128 -> 64
// decoder convolution on 2 x 64 x 128 x 128 voxels moves 5.4 GB through this GEMM).  The one-tile kernel keeps ONE 24-KB
// stage per workgroup in flight (its per-step __syncthreads() is a vmcnt(0) wait) and fills the chip in 1.125 rounds of
// workgroups: 4.3 TB/s.  Here a (point, split) chain streams through a ring of S stages of 16 rows (12 KB), filled by
// LDS-DMA S - 1 stages ahead, with a counted s_waitcnt vmcnt and one s_barrier per stage; 256 threads, <= 128 VGPRs and
// 36 KB of LDS, so four workgroups share a CU and the 864 chains of a 216-point launch are resident at once.  Every
// stage -- its A rows and its B rows apart -- is an LDS object of its own: the wait-count pass tells DMA targets apart by
// object only (with A and B rows in one object the B reads were guarded by a vmcnt(0), seen in the ISA).
// Four waves as 2 (M) x 2 (N), wave tile 32 x 64: every result sums the rows of its split in increasing order, two per
// MFMA, lane half lh taking row 2 kk + lh -- the order of wino_gemm_tn_kernel (stage boundaries are multiples of two
// rows): bit-identical to it (tested).
// The same ring in the order of wino_gemm_tn64_kernel (64 x 64, one accumulator per k half) was built and measured
// too: 664 -> 668 us and 87.4 -> 87.2 us on the two 64 -> 64 shapes of config 1 -- that kernel already moves 5.4 TB/s --
// so those launches stay where they were.
template <int S>
__global__ __launch_bounds__(256, 4) void wino_gemm_tn_stream_kernel(const float* __restrict__ Ah, const float* __restrict__ Bh,
                                                                     float* __restrict__ slab, const int Tpad,
                                                                     const int nsplit, const int kper, const int nchains,
                                                                     const int npts) {
  constexpr int M = 64, N = 128, R = 16;
  constexpr int IPW = 3;                           // DMA instructions (1 KB) per wave and stage
  static_assert(S == 3 || S == 4, "ring depth");
  __shared__ __attribute__((aligned(1024))) float sa0[R * M], sa1[R * M], sa2[R * M], sa3[S == 4 ? R * M : 64];
  __shared__ __attribute__((aligned(1024))) float sb0[R * N], sb1[R * N], sb2[R * N], sb3[S == 4 ? R * N : 64];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  // DMA: wave w moves stage rows 4 w .. 4 w + 3 of both operands (A: one piece of 4 rows x 64; B: two of 2 rows x 128)
  const int a_lane = (lane >> 4) * M + (lane & 15) * 4;
  const int b_lane = (lane >> 5) * N + (lane & 31) * 4;
  auto a_of = [&](int k) __attribute__((always_inline)) -> float* {
    return k == 0 ? sa0 : (k == 1 ? sa1 : (k == 2 ? sa2 : sa3));
  };
  auto b_of = [&](int k) __attribute__((always_inline)) -> float* {
    return k == 0 ? sb0 : (k == 1 ? sb1 : (k == 2 ? sb2 : sb3));
  };

  for (int c = blockIdx.x; c < nchains; c += gridDim.x) {
    const int L = xcd_remap(c, nchains);
    const int split = L % nsplit, xi = L / nsplit;
    const int t0 = split * kper;
    const int t1 = (t0 + kper < Tpad) ? t0 + kper : Tpad;
    const int n = t1 > t0 ? (t1 - t0) / R : 0;     // stages of the chain
    auto issue = [&](int s, float* sa, float* sb) __attribute__((always_inline)) {
      // first of the wave's four rows, in one 256-tile block: [g / 256][xi][g % 256 ..]
      const int g = t0 + R * s + 4 * wave;
      const long row = ((long)(g >> 8) * npts + xi) * 256 + (g & 255);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Ah + row * M + a_lane),
                                       (__attribute__((address_space(3))) void*)(sa + wave * 256), 16, 0, 0);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Bh + (row + 2 * j) * N + b_lane),
                                         (__attribute__((address_space(3))) void*)(sb + (2 * wave + j) * 256), 16, 0, 0);
    };
    // the previous chain's stores have retired (the counted waits start from an empty queue) and every wave is done
    // with its last stages
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // S - 1 stages ahead.  In front of them stage 0's rows go into the LAST ring slot as well (12 KB per chain, retired
    // by the first counted wait, overwritten by the first look-ahead): the wait-count pass then meets a DMA into every
    // stage object before the main loop -- with one met first INSIDE the loop it guarded the reads behind the loop header
    // with a vmcnt(0), once per S stages (seen in the ISA)
    if (n > 0) issue(0, a_of(S - 1), b_of(S - 1));
#pragma unroll
    for (int k = 0; k < S - 1; ++k)
      if (k < n) issue(k, a_of(k), b_of(k));

    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;

    // one stage (k = it % S at compile time).  full: every stage up to it + S - 1 exists, so the wait is the counted
    // one and the look-ahead issue unconditional
    auto stage = [&](const int k, const int it, const bool full) __attribute__((always_inline)) {
      // stage `it` has landed for this wave when at most the S - 2 younger stages are outstanding (loads complete in
      // order); in the tail nothing younger was issued
      if (full || it + S - 2 < n) __builtin_amdgcn_s_waitcnt(0x0F70 | (IPW * (S - 2)));
      else __builtin_amdgcn_s_waitcnt(0x0F70);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();                  // ... and for every wave; all waves are done with stage it - 1
      if (full || it + S - 1 < n) issue(it + S - 1, a_of((k + S - 1) % S), b_of((k + S - 1) % S));
      const float* as = a_of(k) + wm * 32 + li;
      const float* bs = b_of(k) + wn * 64 + li;
#pragma unroll
      for (int kk = 0; kk < R / 2; ++kk) {
        const int kr = 2 * kk + lh;
        const float af = as[kr * M], b0 = bs[kr * N], b1 = bs[kr * N + 32];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, b1, acc[1], 0, 0, 0);
      }
    };
    // Main loop: whole groups of S stages whose look-ahead issues all exist, without a condition inside -- with the
    // conditional form alone the wait-count pass follows the path "stage issued, the next one not, loop again" (which
    // never runs) and guards the first reads behind the loop header with a vmcnt(0), once per S stages.  The tail loop
    // is that conditional form.
    int itb = 0;
    for (; itb + 2 * S - 2 < n; itb += S) {
#pragma unroll
      for (int k = 0; k < S; ++k) stage(k, itb + k, true);
    }
    for (; itb < n; itb += S) {
#pragma unroll
      for (int k = 0; k < S; ++k)
        if (itb + k < n) stage(k, itb + k, false);   // uniform
    }

    float* sb = slab + (((long)split * npts + xi) * M) * N;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      float* o = sb + (long)row * N + wn * 64 + li;
      o[0] = acc[0][e];
      o[32] = acc[1][e];
    }
  }
}

// ------------------------------------------------------------------------------------------
// TN batched GEMM on the bf16 matrix cores (weight gradient in the "bf16x3" / "bf16" math modes): both
// operands are split-bf16 images [t][channel] and the contraction runs over the ROW index t, so an MFMA
// operand (8 consecutive t of one channel per lane) is a transposed read of the LDS image:
// ds_read_b64_tr_b16 hands a 16-lane group the 4 rows x 16 columns block it addresses, column-major.
// The image keeps the DMA's lane-linear rows; to spread the 4 rows of a block over the banks the 64-B
// chunks (= the hi or the lo half of one 32-channel block) are XOR-swizzled by (row & 3) inside each
// 256-B window, applied on the source address of the DMA and on the read address.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

template <int WMW, int MI, int NJ, int NT>
__global__ __launch_bounds__(512) void wino_gemm_tn_bf16_kernel(const float* __restrict__ Ah, const float* __restrict__ Bh,
                                                                float* __restrict__ slab, const int Tpad, const int M,
                                                                const int N, const int m_tiles, const int n_tiles,
                                                                const int nsplit, const int kper, const int nblk,
                                                                const int npts) {
  constexpr int WNW = 8 / WMW;
  constexpr int BM = WMW * 32 * MI, BN = WNW * 32 * NJ;
  static_assert(BM % 64 == 0 && BM <= 256 && BN % 64 == 0 && BN <= 256, "one DMA piece = 256 floats");
  constexpr int STAGE = 32 * (BM + BN);
  constexpr int AQ = BM / 4, ARPP = 64 / AQ, APW = BM / 64;
  constexpr int BQ = BN / 4, BRPP = 64 / BQ, BPW = BN / 64;
  __shared__ __attribute__((aligned(1024))) float lds[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const TnTile t = tn_tile(blockIdx.x, nblk, m_tiles, n_tiles, nsplit, kper, Tpad);

  // DMA source columns: the piece j of a wave covers stage rows (APW * wave + j) * ARPP + lane / AQ, whose
  // low two bits are (j * ARPP + lane / AQ) & 3 (APW * ARPP == 4).
  int acol[APW], bcol[BPW];
#pragma unroll
  for (int j = 0; j < APW; ++j) {
    const int r3 = (j * ARPP + lane / AQ) & 3, slot = lane % AQ;
    acol[j] = t.mt * BM + ((((slot >> 2) ^ r3) << 2) | (slot & 3)) * 4;
  }
#pragma unroll
  for (int j = 0; j < BPW; ++j) {
    const int r3 = (j * BRPP + lane / BQ) & 3, slot = lane % BQ;
    int c = t.nt * BN + ((((slot >> 2) ^ r3) << 2) | (slot & 3)) * 4;
    bcol[j] = c > N - 4 ? N - 4 : c;
  }
  const float* Ab = Ah + (long)(lane / AQ) * M;
  const float* Bb = Bh + (long)(lane / BQ) * N;

  auto issue = [&](int it, int stage) __attribute__((always_inline)) {
    float* as = lds + stage * STAGE;
    float* bs = as + 32 * BM;
    const long row = t.row(it, npts);
    const float* ag = Ab + row * M;
    const float* bg = Bb + row * N;
#pragma unroll
    for (int j = 0; j < APW; ++j) {
      const int p = APW * wave + j;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ag + (long)(p * ARPP) * M + acol[j]),
                                       (__attribute__((address_space(3))) void*)(as + p * 256), 16, 0, 0);
    }
#pragma unroll
    for (int jj = 0; jj < BPW; ++jj) {
      const int p = BPW * wave + jj;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bg + (long)(p * BRPP) * N + bcol[jj]),
                                       (__attribute__((address_space(3))) void*)(bs + p * 256), 16, 0, 0);
    }
  };

  f32x16 acc[MI][NJ];
  zero_acc(acc);

  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave % WMW, wn = wave / WMW;
  const int niter = (t.t1 - t.t0) / 32;

  // transposed-read addresses (bytes inside a stage): 16-lane group g4 = (k half, column half), lane 4q + p
  // of the group addresses row q, columns 4p .. 4p + 3 of its block
  const int g4 = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
  const int rrow = (g4 >> 1) * 8 + q;
  const int cbyte = (g4 & 1) * 32 + p4 * 8;
  int a_hi[MI], a_lo[MI], b_hi[NJ], b_lo[NJ];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int ch = 2 * (wm * MI + mi);
    a_hi[mi] = rrow * BM * 4 + ((ch ^ q) * 64) + cbyte;
    a_lo[mi] = rrow * BM * 4 + (((ch + 1) ^ q) * 64) + cbyte;
  }
#pragma unroll
  for (int nj = 0; nj < NJ; ++nj) {
    const int ch = 2 * (wn * NJ + nj);
    b_hi[nj] = 32 * BM * 4 + rrow * BN * 4 + ((ch ^ q) * 64) + cbyte;
    b_lo[nj] = 32 * BM * 4 + rrow * BN * 4 + (((ch + 1) ^ q) * 64) + cbyte;
  }
  auto frag = [&](const char* st, int off, int rstride) __attribute__((always_inline)) {
    const s16x4 r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(st + off));
    const s16x4 r1 =
        __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(st + off + 4 * rstride));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(r0, r1, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  if (niter > 0) issue(0, 0);
  for (int it = 0; it < niter; ++it) {
    __syncthreads();
    if (it + 1 < niter) issue(it + 1, (it + 1) & 1);
    const char* st = reinterpret_cast<const char*>(lds + (it & 1) * STAGE);
#pragma unroll
    for (int s16 = 0; s16 < 2; ++s16) {
      bf16x8 ah[MI], al[MI], bh[NJ], bl[NJ];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        ah[mi] = frag(st, a_hi[mi] + s16 * 16 * BM * 4, BM * 4);
        if (NT > 1) al[mi] = frag(st, a_lo[mi] + s16 * 16 * BM * 4, BM * 4);
      }
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) {
        bh[nj] = frag(st, b_hi[nj] + s16 * 16 * BN * 4, BN * 4);
        if (NT > 1) bl[nj] = frag(st, b_lo[nj] + s16 * 16 * BN * 4, BN * 4);
      }
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          if (NT > 1) {
            acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh[nj], acc[mi][nj], 0, 0, 0);
            acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl[nj], acc[mi][nj], 0, 0, 0);
          }
          acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh[nj], acc[mi][nj], 0, 0, 0);
        }
    }
  }

  float* sb = slab + (((long)t.split * npts + t.xi) * M + t.mt * BM) * N + t.nt * BN;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * 32 * MI + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      float* o = sb + (long)row * N + wn * 32 * NJ + li;
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
        if (t.nt * BN + wn * 32 * NJ + nj * 32 + li < N) o[nj * 32] = acc[mi][nj][e];
    }
}

// dw = sum of the split-K slabs.  64 results x 4 slab groups per workgroup: a thread sums its group's slabs (k = kg,
// kg + 4, ...) in eight interleaved partial sums (eight loads in flight), the four groups meet through LDS in a fixed
// order -- with up to 256 slabs (the 1x1x1 weight gradients of ResNet-50's 32x64x64 stages) one thread per result and
// four loads in flight was a chain of 64 memory latencies.
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ slab, float* __restrict__ out, const long n,
                                                       const int nsplit) {
  __shared__ float part[4][64];
  const int r = threadIdx.x & 63, kg = threadIdx.x >> 6;
  for (long i0 = blockIdx.x * 64L; i0 < n; i0 += (long)gridDim.x * 64L) {      // (uniform: every thread reaches the barriers)
    const long i = i0 + r;
    const bool live = i < n;
    float p[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = 0.f;
    if (live) {
      int k = kg;
      for (; k + 28 < nsplit; k += 32) {
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] += slab[(long)(k + 4 * j) * n + i];
      }
      for (int j = 0; k < nsplit; k += 4, ++j) p[j] += slab[(long)k * n + i];
    }
    part[kg][r] = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
    __syncthreads();
    if (kg == 0 && live) out[i] = (part[0][r] + part[1][r]) + (part[2][r] + part[3][r]);
    __syncthreads();
  }
}
}  // namespace

// ------------------------------------------------------------------------------------------
// host side

// wgrad: M = Cout, N = Cin.  Tile = the largest (BM, BN) that divides M and wastes < 13 % of N;
// split over t so that >= ~512 workgroups are in flight.
bool plan_tn(const DramConvDesc* d, const WinoGeom& g, TnPlan& p) {
  const int M = d->Cout, N = d->Cin;
  p.bm = M % 256 == 0 ? 256 : (M % 128 == 0 ? 128 : 64);
  const int ncand = p.bm == 256 ? 3 : 2;             // 64-column tiles only exist for BM = 256
  const int cand[3] = {256, 128, 64};
  p.bn = 0;
  int best_pad = 1 << 30;
  for (int i = 0; i < ncand; ++i) {
    const int padded = (N + cand[i] - 1) / cand[i] * cand[i];
    if (padded * 100 <= N * 113) { p.bn = cand[i]; break; }
    if (padded < best_pad) { best_pad = padded; p.bn = cand[i]; }
  }
  p.m_tiles = M / p.bm;
  p.n_tiles = (N + p.bn - 1) / p.bn;
  // whole rounds of 256 workgroups (one per CU), as in run_nn: half-width tiles when they waste less of the last round
  if (p.bn >= 128 && (p.bn > 128 || p.bm == 256)) {
    const long w1 = (long)g.npts * p.m_tiles * p.n_tiles;
    const int hb = p.bn / 2, hn = (N + hb - 1) / hb;
    const long w2 = (long)g.npts * p.m_tiles * hn;
    if (w1 >= 512 && (double)((w2 + 255) / 256) * 0.5 * 1.03 < (double)((w1 + 255) / 256)) {
      p.bn = hb;
      p.n_tiles = hn;
    }
  }
  const int base = g.npts * p.m_tiles * p.n_tiles;
  const int k32 = g.Tpad / 32;
  int ns = 1;
  // (1x1x1, one point: a 64 x 256 weight gradient over 131 072 voxels is ONE output tile -- 64 splits left three
  // quarters of the chip idle, 168 MB in 147 us; up to 256 splits of >= 256 rows, one round of workgroups: a second
  // round's worth of splits only added slab traffic to the matrix-bound 256 <-> 1024 shapes)
  while (base * ns < (g.npts == 1 ? 256 : 512) && ns * 2 <= k32 / 4 && ns < (g.npts == 1 ? 256 : 16)) ns *= 2;
  p.nsplit = ns;
  p.kper = ((k32 + ns - 1) / ns) * 32;
  return true;
}

int run_nn(const float* A, const float* U, float* Y, const WinoGeom& g, int N, int K, hipStream_t s,
           const GemmEpilogue ep, const int math, const bool alone) {
  // N tile = 64 * nj columns.  One workgroup per CU (64-128 KB of LDS), so a launch runs in whole rounds of 256
  // workgroups: 864 workgroups of 256 columns (layer4, 216 points) take 4 rounds with the last 3/8 full, 1728 of
  // 128 columns take 7 (measured 0.747 -> 0.706 ms).  Pick the width with the least rounds x width x per-column
  // cost (narrower tiles re-read the M operand more often: +3 % / +10 %, measured).
  const int m_tiles = g.Tpad / 256;
  int nj = 1;
  double best = 1e30;
  for (int c = 4; c >= 1; c >>= 1) {
    if (N % (64 * c) != 0) continue;
    const long wgs = (long)g.npts * m_tiles * (N / (64 * c));
    const double cost = (double)((wgs + 255) / 256) * c * (c == 4 ? 1.0 : (c == 2 ? 1.03 : 1.10));
    if (cost < best) { best = cost; nj = c; }
  }
  const int n_tiles = N / (64 * nj);
  const int nblk = g.npts * m_tiles * n_tiles;
  // executed: 2*M*N*K per point; algorithmic bytes: A, U read once, Y written once
  DramProf prof(DRAM_FAM_WINO_GEMM_NN, nj, 2.0 * g.npts * (double)g.Tpad * N * K,
                4.0 * g.npts * ((double)g.Tpad * (K + N) + (double)N * K), s,
                g.npts > 1 ? 2.0 * g.B * g.D * g.H * g.W * (double)N * K * 27.0 : -1.0);
  if (math) {      // split-bf16 operand images (Winograd pipeline only; no fused epilogue there)
#define WNB(NJ_, NT_)                                                                                                  \
  hipLaunchKernelGGL((wino_gemm_nn_bf16_kernel<NJ_, NT_>), dim3(nblk), dim3(512), 0, s, A, U, Y, g.Tpad, N, K, m_tiles, \
                     n_tiles, nblk, g.npts)
    if (math == 1) { if (nj == 4) WNB(4, 3); else if (nj == 2) WNB(2, 3); else WNB(1, 3); }
    else { if (nj == 4) WNB(4, 1); else if (nj == 2) WNB(2, 1); else WNB(1, 1); }
#undef WNB
    DRAM_LAUNCH_CHECK();
    return DRAM_OK;
  }
#define WNN(NJ_)                                                                                                   \
  hipLaunchKernelGGL((wino_gemm_nn_kernel<NJ_>), dim3(nblk), dim3(512), 0, s, A, U, Y, g.Tpad, N, K, m_tiles, n_tiles, \
                     nblk, g.npts, ep)
  // HBM-bound shapes of the pipeline (no epilogue, whole K in one stage): the persistent streaming form
  const char* se = tune_env("DRAM_NN_STREAM");           // 0 off, 1 from 4 096 items on (default), 2 always (tests)
  const int stream_on = se ? atoi(se) : 1;
  const bool fused = ep.bias || ep.add || ep.gate || ep.stats;
  if (stream_on && !fused && g.npts > 1 && g.Tpad % 256 == 0 &&
      ((N == 64 && (K == 128 || K == 64)) || (N == 128 && K == 64))) {
    const int m64 = g.Tpad / 64;
    const long total = (long)g.npts * m64;
    if (total < (1L << 31) && (total >= 4096 || stream_on == 2)) {
      const int wgs = stream_on == 2 ? 8 : 256;                      // one persistent workgroup per CU (tests: 8 in all,
                                                                     // so that small cases run the ring too)
      const int per_wg = (int)((total + wgs - 1) / wgs);
      const int grid = (int)((total + per_wg - 1) / per_wg);
#define WNS(NJ_, KT_, S_)                                                                                          \
  hipLaunchKernelGGL((wino_gemm_nn_stream_kernel<NJ_, KT_, S_>), dim3(grid), dim3(256), 0, s, A, U, Y, g.npts, m64, \
                     per_wg, (int)total)
      const char* sde = tune_env("DRAM_NN_STREAM_DB");                  // A/B switch (read per call: the tests flip it)
      // bit 0: 64 -> 64, bit 1: 64 -> 128, bit 2: 128 -> 64 (k halves); not beside another stream's kernels (two of
      // these workgroups fill a CU's LDS: config 1's eager two-stream step lost in backward what it won in forward)
      const int sdb = sde ? atoi(sde) : (alone ? 7 : 0);
      // two workgroups per CU (the direct-B form, 68 KB of LDS each)
      const int wgs2 = stream_on == 2 ? 8 : 512;
      const int per2 = (int)((total + wgs2 - 1) / wgs2);
      const int grid2 = (int)((total + per2 - 1) / per2);
      if (N == 64 && K == 128 && (sdb & 4)) {
        // items are k-halves of tiles: an even number per workgroup, so that every run starts on a first half
        const long total2 = 2 * total;
        if (total2 < (1L << 31)) {
          const int perk = 2 * (int)((total + wgs2 - 1) / wgs2);
          const int gridk = (int)((total2 + perk - 1) / perk);
          hipLaunchKernelGGL((wino_gemm_nn_stream_kernel<1, 64, 3, true, 2>), dim3(gridk), dim3(256), 0, s, A, U, Y, g.npts,
                             m64, perk, (int)total2);
        } else WNS(1, 128, 3);
      }
      else if (N == 64 && K == 128) WNS(1, 128, 3);
      else if (N == 64 && (sdb & 1))
        hipLaunchKernelGGL((wino_gemm_nn_stream_kernel<1, 64, 3, true>), dim3(grid2), dim3(256), 0, s, A, U, Y, g.npts, m64,
                           per2, (int)total);
      else if (N == 128 && (sdb & 2))
        hipLaunchKernelGGL((wino_gemm_nn_stream_kernel<2, 64, 3, true>), dim3(grid2), dim3(256), 0, s, A, U, Y, g.npts, m64,
                           per2, (int)total);
      else if (N == 64) WNS(1, 64, 4);
      else WNS(2, 64, 4);
#undef WNS
      DRAM_LAUNCH_CHECK();
      return DRAM_OK;
    }
  }
  // matrix-bound launches: the persistent form (the next tile's first stage prefetched under the epilogue), when the
  // main loop has an even number of iterations; DRAM_NN_PERSIST=0 (DRAM_TUNING=1): the one-tile kernel (A/B, tests)
  const char* pe = tune_env("DRAM_NN_PERSIST");          // (read per call: the tests switch it between cases)
  const int persist = pe ? atoi(pe) : 1;
  // (256-column tiles: accumulators + state spill.  Fused epilogues -- the 1x1x1 convolutions of the Bottleneck blocks --
  // keep the one-tile kernel: their bias / shortcut-gradient loads wait on vmcnt, which the prefetch DMA shares, so the
  // epilogue serialises behind the prefetch it was meant to hide: ResNet-50 fp32 38.8 -> 45.6 ms with it, measured)
  if (persist && !fused && nj <= 2 && (K / 32) % 2 == 0) {
    // every workgroup the same number of tiles where that costs no round: 432 tiles -> 216 workgroups x 2 (the other
    // 40 CUs stay free for the second stream's kernels) instead of 176 x 2 + 80 x 1
    const int rounds = (nblk + 255) / 256;
    int grid = ((nblk + rounds - 1) / rounds + 7) / 8 * 8;
    if (grid > 256) grid = 256;
    if (grid > nblk) grid = nblk;
#define WNP(NJ_)                                                                                                   \
  hipLaunchKernelGGL((wino_gemm_nn_pers_kernel<NJ_>), dim3(grid), dim3(512), 0, s, A, U, Y, g.Tpad, N, K, m_tiles, \
                     n_tiles, nblk, g.npts, ep)
    if (nj == 2) WNP(2);
    else WNP(1);
#undef WNP
    DRAM_LAUNCH_CHECK();
    return DRAM_OK;
  }
  if (nj == 4) WNN(4);
  else if (nj == 2) WNN(2);
  else WNN(1);
#undef WNN
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

// The TN GEMM of both weight gradients in the (bm, bn) form of the plan.  math 1 / 2: operands are split-bf16 images
// (the Winograd pipeline under DRAM_MATH; the 1x1x1 weight gradient reads the activations themselves and passes 0).
int run_tn(const float* Ah, const float* Bh, float* slab, const WinoGeom& g, const TnPlan& p, const int M, const int N,
           const int math, hipStream_t s) {
  const int nblk = g.npts * p.nsplit * p.m_tiles * p.n_tiles;
  DramProf prof(DRAM_FAM_WINO_GEMM_TN, p.bm * 1000 + p.bn, 2.0 * g.npts * (double)g.Tpad * M * N,
                4.0 * g.npts * ((double)g.Tpad * (M + N) + (double)p.nsplit * M * N), s,
                g.npts > 1 ? 2.0 * g.B * g.D * g.H * g.W * (double)M * N * 27.0 : -1.0);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(512), 0, s, Ah, Bh, slab, g.Tpad, M, N, p.m_tiles, p.n_tiles, p.nsplit,
                       p.kper, nblk, g.npts);
  };
#define WTN(WM_, MI_, NJ_)                                             \
  launch(math == 1   ? wino_gemm_tn_bf16_kernel<WM_, MI_, NJ_, 3>      \
         : math == 2 ? wino_gemm_tn_bf16_kernel<WM_, MI_, NJ_, 1>      \
                     : wino_gemm_tn_kernel<WM_, MI_, NJ_>)
  // fp32: the streaming and the persistent form, bit-identical to the one-tile kernels below (which stay the reference).
  // The switch is run_nn's, one for the streaming GEMMs of both sides: DRAM_NN_STREAM=0 under DRAM_TUNING=1 = the one-tile
  // kernels; 1 = by shape (default); 2 = wherever legal and on 8 workgroups, so that small test cases run ring
  // wrap-around, short tails and several items per workgroup (read per call, the tests flip it)
  const char* te = tune_env("DRAM_NN_STREAM");
  const int tn_stream = te ? atoi(te) : 1;
  if (math == 0 && tn_stream) {
    // the 64 x 64 launches of the pipeline stay on wino_gemm_tn64_kernel (another order of sums than any form here)
    const bool t64 = g.npts > 1 && M == 64 && N == 64 && p.kper % 64 == 0 && g.Tpad % 64 == 0;
    // HBM-bound 64 x 128 launches of the pipeline: the streaming form, one (point, split) chain per workgroup
    if (g.npts > 1 && M == 64 && N == 128 && p.bm == 64 && p.bn == 128) {
      const int nchains = g.npts * p.nsplit;
      const int grid = tn_stream == 2 && nchains > 8 ? 8 : nchains;
      hipLaunchKernelGGL((wino_gemm_tn_stream_kernel<3>), dim3(grid), dim3(256), 0, s, Ah, Bh, slab, g.Tpad, p.nsplit, p.kper,
                         nchains, g.npts);
      DRAM_LAUNCH_CHECK();
      return DRAM_OK;
    }
    // short K (4 k steps per item: the 128- and 256-channel layers at 16 x 32 x 32; measured with 8 steps, 256 -> 512: 284
    // -> 281 us, inside the run-to-run spread, so those and the 16-step launches of the 512-channel layers, at 0.88 of
    // the pipe, keep the one-tile kernel): persistent workgroups over whole items, as run_nn sizes its persistent grid --
    // at most the resident slots (two workgroups per CU up to 64 KB of stages), every workgroup the same number of items
    // where that costs no round
    const int niter = p.kper / 32;
    const bool whole = niter % 2 == 0 && (long)p.kper * p.nsplit == g.Tpad;
    if (!t64 && whole && (tn_stream == 2 || (g.npts > 1 && niter <= 4))) {
      const int slots = 256 * (p.bm + p.bn <= 256 ? 2 : 1);
      const int rounds = (nblk + slots - 1) / slots;
      int grid = ((nblk + rounds - 1) / rounds + 7) / 8 * 8;
      if (grid > slots) grid = slots;
      if (tn_stream == 2) grid = 8;
      if (grid > nblk) grid = nblk;
      const int per_wg = (nblk + grid - 1) / grid;
      grid = (nblk + per_wg - 1) / per_wg;
      if (per_wg > 1 || tn_stream == 2) {
#define WTP(WM_, MI_, NJ_)                                                                                              \
  hipLaunchKernelGGL((wino_gemm_tn_pers_kernel<WM_, MI_, NJ_>), dim3(grid), dim3(512), 0, s, Ah, Bh, slab, g.Tpad, M, N, \
                     p.m_tiles, p.n_tiles, p.nsplit, p.kper, nblk, g.npts, per_wg)
        if (p.bm == 256 && p.bn == 256) WTP(4, 2, 4);
        else if (p.bm == 256 && p.bn == 128) WTP(4, 2, 2);
        else if (p.bm == 256 && p.bn == 64) WTP(4, 2, 1);
        else if (p.bm == 128 && p.bn == 256) WTP(2, 2, 2);
        else if (p.bm == 128 && p.bn == 128) WTP(2, 2, 1);
        else if (p.bm == 64 && p.bn == 256) WTP(2, 1, 2);
        else if (p.bm == 64 && p.bn == 128) WTP(2, 1, 1);
        else return DRAM_ERR_UNSUPPORTED;
#undef WTP
        DRAM_LAUNCH_CHECK();
        return DRAM_OK;
      }
    }
  }
  // (the 64 x 64 kernel sums in another order than the generic 64 x 128 form: pipeline only, so that a 64 -> 64
  // 1x1x1 weight gradient keeps its bits)
  if (math == 0 && g.npts > 1 && M == 64 && N == 64 && p.kper % 64 == 0 && g.Tpad % 64 == 0)
    hipLaunchKernelGGL(wino_gemm_tn64_kernel, dim3(g.npts * p.nsplit), dim3(512), 0, s, Ah, Bh, slab, g.Tpad, p.nsplit,
                       p.kper, g.npts * p.nsplit, g.npts);
  else if (p.bm == 256 && p.bn == 256) WTN(4, 2, 4);
  else if (p.bm == 256 && p.bn == 128) WTN(4, 2, 2);
  else if (p.bm == 256 && p.bn == 64) WTN(4, 2, 1);
  else if (p.bm == 128 && p.bn == 256) WTN(2, 2, 2);
  else if (p.bm == 128 && p.bn == 128) WTN(2, 2, 1);
  else if (p.bm == 64 && p.bn == 256) WTN(2, 1, 2);
  else if (p.bm == 64 && p.bn == 128) WTN(2, 1, 1);
  else return DRAM_ERR_UNSUPPORTED;
#undef WTN
  DRAM_LAUNCH_CHECK();
  return DRAM_OK;
}

// ------------------------------------------------------------------------------------------
// 1x1x1 convolutions (Bottleneck conv1 / conv3, reference med3d.py:152-157) as plain GEMMs on the
// batched-GEMM kernels above (one "point", M = voxels): no transform, no packing beyond the transposed
// copy for the data gradient.  Geometry for the kernels: Tpad = M, npts = 1 (the blocked index is t*C).
namespace {
bool c1_ok(const DramConvDesc* d) {
  if (!d || d->k != 1 || d->stride != 1 || d->pad != 0) return false;
  if (d->B < 1 || d->D < 1 || d->H < 1 || d->W < 1) return false;
  if (d->Do != d->D || d->Ho != d->H || d->Wo != d->W) return false;
  if (d->Cin < 64 || d->Cout < 64 || d->Cin % 64 != 0 || d->Cout % 64 != 0) return false;
  const long long M = (long long)d->B * d->D * d->H * d->W;
  const long long cmax = d->Cin > d->Cout ? d->Cin : d->Cout;
  return M % 256 == 0 && M * cmax < (1LL << 31);
}
WinoGeom c1_geom(const DramConvDesc* d) {
  WinoGeom g{};
  g.B = d->B; g.D = d->D; g.H = d->H; g.W = d->W; g.d = 1;
  g.nz = g.ny = g.nx = 1;
  g.npts = 1;
  g.T = g.Tpad = d->B * d->D * d->H * d->W;
  return g;
}
}  // namespace

extern "C" int dram_conv1x1_applicable(const DramConvDesc* d) { return c1_ok(d) ? 1 : 0; }

extern "C" int dram_conv1x1_num_stat_rows(const DramConvDesc* d) {
  if (!c1_ok(d)) return DRAM_ERR_UNSUPPORTED;
  return c1_geom(d).Tpad / 256;
}

/* w2d: the reference weight [Cout][Cin][1][1][1] itself (= GEMM B operand, K = Cin contiguous) */
extern "C" int dram_conv1x1_fwd(const float* x, const float* w2d, const float* bias, float* y, float* stats_partial,
                                const DramConvDesc* d, dram_stream_t stream) {
  if (!x || !w2d || !y) return DRAM_ERR_BAD_ARG;
  if (!c1_ok(d)) return DRAM_ERR_UNSUPPORTED;
  return run_nn(x, w2d, y, c1_geom(d), d->Cout, d->Cin, (hipStream_t)stream,
                GemmEpilogue{bias, nullptr, nullptr, stats_partial});
}

/* wt: transposed weight [Cin][Cout] (dram_pack_conv_weight's wb with taps = 1) */
extern "C" int dram_conv1x1_bwd_data(const float* dy, const float* wt, float* dx, const float* add, const float* gate,
                                     const DramConvDesc* d, dram_stream_t stream) {
  if (!dy || !wt || !dx || (gate && !add)) return DRAM_ERR_BAD_ARG;
  if (!c1_ok(d)) return DRAM_ERR_UNSUPPORTED;
  return run_nn(dy, wt, dx, c1_geom(d), d->Cin, d->Cout, (hipStream_t)stream, GemmEpilogue{nullptr, add, gate, nullptr});
}

extern "C" size_t dram_conv1x1_bwd_weight_workspace(const DramConvDesc* d) {
  if (!c1_ok(d)) return 0;
  TnPlan p;
  plan_tn(d, c1_geom(d), p);
  return (size_t)p.nsplit * d->Cout * d->Cin * sizeof(float);
}

extern "C" int dram_conv1x1_bwd_weight(const float* x, const float* dy, float* dw, const DramConvDesc* d, void* workspace,
                                       size_t workspace_bytes, dram_stream_t stream) {
  if (!x || !dy || !dw) return DRAM_ERR_BAD_ARG;
  if (!c1_ok(d)) return DRAM_ERR_UNSUPPORTED;
  const WinoGeom g = c1_geom(d);
  TnPlan p;
  plan_tn(d, g, p);
  const size_t need = (size_t)p.nsplit * d->Cout * d->Cin * sizeof(float);
  if (p.nsplit > 1 && (!workspace || workspace_bytes < need)) return DRAM_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* slab = p.nsplit > 1 ? (float*)workspace : dw;      // one split: the GEMM writes dw[co][ci] directly
  // (fp32 whatever DRAM_MATH says: the operands are the activations, not split images)
  const int rc = run_tn(dy, x, slab, g, p, d->Cout, d->Cin, 0, s);
  if (rc != DRAM_OK) return rc;
  if (p.nsplit > 1) {
    const long n = (long)d->Cout * d->Cin;
    const int grid = (int)((n + 63) / 64 > 4096 ? 4096 : (n + 63) / 64);
    DramProf prof(DRAM_FAM_WINO_WGRAD_OUT, 0, 0.0, 4.0 * (double)n * (p.nsplit + 1), s);
    hipLaunchKernelGGL(slab_sum_kernel, dim3(grid), dim3(256), 0, s, slab, dw, n, p.nsplit);
    DRAM_LAUNCH_CHECK();
  }
  return DRAM_OK;
}
