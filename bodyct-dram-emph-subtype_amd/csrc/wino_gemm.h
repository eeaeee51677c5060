// wino_gemm.h -- what conv_wino.hip calls in wino_gemm.hip: the batched NN / TN GEMM launchers of the Winograd
// pipeline and the types they take.  Internal to the library (not part of the C ABI in dram_hip.h).
#pragma once
#include "common.h"

// Tile: NZ x NY x 2 outputs, (NZ + 2) x (NY + 2) x 4 inputs / Winograd points.  NZ, NY = 2 (F(2,3)) or
// 4 (F(4,3): 6 instead of 8 products per 4 outputs of that axis -> 25 % fewer GEMM flops and
// Winograd-domain bytes per axis; used when the sub-lattice extent of the axis is a multiple of 4).
// Measured rel-L2 vs fp64 on a 256-channel layer: 6.6e-7 (2,2), 1.7e-6 (4,2); torch fp32 direct 3.6e-7.
struct WinoGeom {
  int B, D, H, W;  // voxel grid (input and output grids coincide: stride 1, pad == dil)
  int d;           // dilation
  int nz, ny, nx;  // outputs per tile along z, y, x (2 or 4); points = (nz + 2) * (ny + 2) * (nx + 2)
  int npts;
  int Tz, Ty, Tx;  // tiles per residue sub-lattice axis
  int T;           // B * d^3 * Tz * Ty * Tx
  int Tpad;        // T rounded up to the GEMM M tile (256)
};

// Optional fused epilogue of the NN GEMM (the 1x1x1 convolutions of the Bottleneck blocks run it as a plain
// GEMM, npts = 1): bias, += add * (gate > 0) (identity-shortcut gradient), per-M-tile BatchNorm sums.
struct GemmEpilogue {
  const float* bias;
  const float* add;
  const float* gate;
  float* stats;      // [m_tiles][2][N]
};

// NN batched GEMM  Y[xi][m][n] = sum_k A[xi][m][k] * U[xi][n][k]  (M = g.Tpad, K % 32 == 0), in the form the shape and
// the tuning switches select.  math: 0 fp32, 1 / 2 split-bf16 operand images.  alone: no other stream's kernels are
// expected beside this launch.
int run_nn(const float* A, const float* U, float* Y, const WinoGeom& g, int N, int K, hipStream_t s,
           const GemmEpilogue ep = GemmEpilogue{nullptr, nullptr, nullptr, nullptr}, const int math = 0,
           const bool alone = true);

// Weight gradient (M = Cout, N = Cin): tile and split-K plan, and the TN batched GEMM
// slab[split][xi][m][n] = sum_{t in split} Ah[xi][t][m] * Bh[xi][t][n] launched by it.
struct TnPlan { int bm, bn, m_tiles, n_tiles, nsplit, kper; };
bool plan_tn(const DramConvDesc* d, const WinoGeom& g, TnPlan& p);
int run_tn(const float* Ah, const float* Bh, float* slab, const WinoGeom& g, const TnPlan& p, int M, int N, int math,
           hipStream_t s);
