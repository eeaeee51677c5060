/* dram_hip.h -- C ABI of libdram_hip.so (MI355X / gfx950 hand-written HIP kernels).
 *
 * The reference has no FFI of its own: its hot path is torch-op call sites inside
 * med3d.py / models.py / metrics.py.  Each entry point below
 * replaces the cuDNN/ATen kernels behind one family of those call sites; the
 * reference file:line each one stands in for is cited on the declaration.
 *
 * Conventions
 *  - Activations are NDHWC ("channels-last-3D") contiguous float32:
 *      x[b][z][y][x][c], element offset ((((b*D+z)*H+y)*W+x)*C+c).
 *    The reference uses NCDHW; for C == 1 (network input, lung masks, regression
 *    dRAM maps) the two layouts are the same bytes.
 *  - Convolution weights cross the ABI in the reference's own layout
 *    [Cout][Cin][kD][kH][kW] (state_dict contract); packed copies
 *    are produced by dram_pack_conv_weight.
 *  - Every function enqueues on `stream` and never synchronises, allocates or frees.
 *    The caller owns all buffers including workspaces.
 *  - Return value: 0 on success, DRAM_ERR_* (<0) on a rejected argument, or a
 *    positive hipError_t from the launch.  Nothing is thrown across the ABI.
 */
#ifndef DRAM_HIP_H
#define DRAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dram_stream_t; /* hipStream_t */

#define DRAM_OK 0
#define DRAM_ERR_BAD_ARG (-1)
#define DRAM_ERR_UNSUPPORTED (-2)
#define DRAM_ERR_WORKSPACE (-3)

#define DRAM_ABI_VERSION 7
int dram_version(void);
/* static string: "gfx950" build tag */
const char* dram_build_info(void);
/* sha1 (first 16 hex digits) of the dram_hip.h this library was compiled against; the host binding
 * compares it with the header it reads its signatures from and refuses a mismatching library. */
const char* dram_abi_hash(void);
/* Identity of the hipGraph capture `stream` is recording into (hipStreamGetCaptureInfo): 0 when the stream is not
 * capturing, otherwise a number unique to that capture.  The host side keys everything a captured launch bakes a
 * pointer of (scratch buffers, device work lists) by it, so that no other capture and no eager call can take over or
 * free such memory while the graph lives.  Does not enqueue anything. */
unsigned long long dram_stream_capture_id(dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Kernel timeline (measurement only; off by default, no cost when off).
 * Between dram_profile_start and dram_profile_stop every kernel launch of the library is bracketed by
 * two hipEvents recorded on the stream it is launched on, tagged with its kernel family, the MFMA
 * FLOPs it EXECUTES (products really issued -- a Winograd kernel issues fewer than the direct
 * convolution it replaces) and the ALGORITHMIC HBM bytes it has to move (each operand read once,
 * each result written once).  bench.py builds its roofline table from these records; rocprofv3
 * --kernel-trace --stats of the same command must agree (profiles/).
 *   dram_profile_start(max_records): allocate the event pool, clear the log, switch recording on.
 *   dram_profile_stop(): recording off (the log stays readable).
 *   dram_profile_read(out, max): waits for the recorded events (the ONE entry point of the library
 *     that synchronises), fills out[i].ms, returns the number of records (<= max).
 * Launches beyond max_records are not recorded (dram_profile_dropped() counts them). */
enum {
  DRAM_FAM_CONV_WINO2D = 0, /* fused in-plane Winograd conv, fwd + dgrad          (mfma) */
  DRAM_FAM_WINO_IN,         /* 3-D Winograd input / gradient tile transforms      (hbm)  */
  DRAM_FAM_WINO_GEMM_NN,    /* Winograd-domain GEMMs fwd + dgrad, 1x1x1 GEMMs     (mfma) */
  DRAM_FAM_WINO_OUT,        /* 3-D Winograd output transforms (+ epilogues)       (hbm)  */
  DRAM_FAM_WINO_GEMM_TN,    /* Winograd-domain weight-gradient GEMMs              (mfma) */
  DRAM_FAM_WINO_WGRAD_OUT,  /* slab sum + G^T dU G                                (hbm)  */
  DRAM_FAM_WEIGHT_PACK,     /* weight repacking / weight transforms               (hbm)  */
  DRAM_FAM_WGRAD_W2D,       /* in-plane Winograd weight gradient (+ reduce)       (mfma) */
  DRAM_FAM_CONV_IGEMM,      /* direct implicit-GEMM conv, fwd + dgrad             (mfma) */
  DRAM_FAM_CONV_WGRAD,      /* direct weight gradient (+ reduce)                  (mfma) */
  DRAM_FAM_STEM,            /* 7x7x7 stem conv fwd + wgrad + dgrad (variants 4, 5) (mfma) */
  DRAM_FAM_BN,              /* BN apply / backward / statistics folds / add       (hbm)  */
  DRAM_FAM_POOL_UP,         /* max-pool, upsample+concat, up-projection           (hbm)  */
  DRAM_FAM_HEAD_LOSS,       /* heads, dRAM losses                                 (hbm)  */
  DRAM_FAM_OPTIM,           /* fused Adam / SGD                                   (hbm)  */
  DRAM_FAM_PREP,            /* input transforms                                   (hbm)  */
  DRAM_FAM_CONV_BF16,       /* bf16-storage direct conv, fwd + dgrad (bf16 MFMA)  (mfma) */
  DRAM_FAM_WGRAD_BF16,      /* bf16-storage weight gradient (+ reduce)            (mfma) */
  DRAM_FAM_COUNT
};
typedef struct DramProfRecord {
  int32_t family;      /* DRAM_FAM_* */
  int32_t variant;     /* kernel variant within the family (template instance id; informational) */
  double mfma_flops;   /* executed MFMA FLOPs of this launch (0 for non-matrix kernels) */
  double alg_flops;    /* direct-convolution FLOPs (2*M*N*K) the launch stands for; for the 3-D Winograd
                          pipeline they are booked on the GEMM launch; 0 elsewhere */
  double hbm_bytes;    /* algorithmic HBM bytes of this launch */
  float ms;            /* hipEventElapsedTime(start, end) */
  float pad_;
} DramProfRecord;
const char* dram_profile_family_name(int family);
/* 1 when the family's roof is the matrix pipe, 0 when it is HBM bandwidth */
int dram_profile_family_is_mfma(int family);
int dram_profile_start(int max_records);
int dram_profile_stop(void);
int dram_profile_dropped(void);
int dram_profile_read(DramProfRecord* out, int max_records);

/* ------------------------------------------------------------------------- */
/* Convolution geometry (isotropic stride / padding / dilation, cubic kernel). */
typedef struct DramConvDesc {
  int32_t B;             /* batch */
  int32_t D, H, W, Cin;  /* input  (forward sense) */
  int32_t Do, Ho, Wo, Cout; /* output (forward sense) */
  int32_t k;             /* kernel edge: 1 or 3 (7 only via dram_stem_*) */
  int32_t stride, pad, dil;
  int32_t flags;         /* DRAM_CONV_* plan hints; 0 = none */
} DramConvDesc;
/* The caller's network hands a layer's rounding error on with little amplification (the BasicBlock ResNets: 22 / 38
 * BatchNorm layers; measured at full size with every 64->64 layer on F(4,3)^3 tiles: outputs 6.0e-5 / 1.9e-4 from the
 * fp64 oracle against a bar of 1e-3).  The plan then lets the cheaper estimate win on every layer; without the flag the
 * fused in-plane kernels (F(2x2): a tenth of the rounding error) keep the layers below the last decoder stage unless
 * the 3-D pipeline is estimated > 15 % faster -- ResNet-50's 54 BatchNorm layers amplify an early error ~100 x.
 * Results under either plan are within the 1e-3 bar; only the plan differs. */
#define DRAM_CONV_ROUNDING_TOLERANT 1
/* Per-call hint for a DATA GRADIENT (dram_wino_conv3d_bwd_data[_bn]): the caller runs weight-gradient kernels on another
 * stream at the same time.  The HBM-bound Winograd-domain GEMMs then keep the form with ONE workgroup per CU (100 KB of
 * LDS, room for the other stream's workgroups beside it) instead of the two-workgroups-per-CU form, which is 8-15 %
 * faster on a device of its own and takes the overlap away when it is not (measured).  Results are
 * bit-identical either way. */
#define DRAM_CONV_BWD_OVERLAPPED 2

/* Repack [Cout][Cin][k^3] -> wf[tap][Cout][Cin] (forward B-operand, K=Cin contiguous)
 * and wb[tap][Cin][Cout] (data-gradient B-operand).  Either output may be NULL. */
int dram_pack_conv_weight(const float* w, float* wf, float* wb, int Cout, int Cin, int taps,
                          dram_stream_t stream);

/* Forward 3x3x3 / 1x1x1 convolution as an LDS-tiled fp32-MFMA implicit GEMM.
 * Replaces nn.Conv3d at med3d.py:91-100 (conv3x3x3), :152-157 (Bottleneck), :67/:76
 * (decoder, with bias), :226/:325 (us3).
 *   x  [B,D,H,W,Cin]   wf packed [k^3][Cout][Cin]   bias [Cout] or NULL
 *   y  [B,Do,Ho,Wo,Cout] (pre-BatchNorm output)
 *   stats_partial: NULL, or [dram_conv_num_mtiles(desc)][2][Cout] -- per-M-tile
 *     sum(y) and sum(y*y) per channel (BatchNorm batch statistics, fused epilogue). */
int dram_conv3d_fwd(const float* x, const float* wf, const float* bias, float* y,
                    float* stats_partial, const DramConvDesc* desc, dram_stream_t stream);

/* Data gradient: dx[B,D,H,W,Cin] = conv^T(dy[B,Do,Ho,Wo,Cout], w); wb packed [k^3][Cin][Cout].
 * Optional fused epilogue: dx += add * (gate > 0)   (gate NULL => dx += add); both
 * shaped like dx.  This is the identity-shortcut gradient of med3d.py:141-142/:181-182.
 * Replaces autograd's convolution_backward (input) for the call sites above. */
int dram_conv3d_bwd_data(const float* dy, const float* wb, float* dx, const float* add,
                         const float* gate, const DramConvDesc* desc, dram_stream_t stream);

/* Weight gradient.  dw is written in the reference layout [Cout][Cin][k^3].
 * workspace: split-K slabs, size from dram_conv3d_bwd_weight_workspace().
 * Deterministic (slab + ordered reduce, no float atomics). */
size_t dram_conv3d_bwd_weight_workspace(const DramConvDesc* desc);
int dram_conv3d_bwd_weight(const float* x, const float* dy, float* dw, const DramConvDesc* desc,
                           void* workspace, size_t workspace_bytes, dram_stream_t stream);

/* number of M tiles (rows of stats_partial) dram_conv3d_fwd produces for desc */
int dram_conv_num_mtiles(const DramConvDesc* desc);

/* ------------------------------------------------------------------------- */
/* 3-D Winograd pipeline (F(2,3) or F(4,3) per axis) for stride-1 3x3x3 convolutions with pad == dil and
 * Cin, Cout multiples of 64 (the BasicBlock / Bottleneck conv3x3x3 sites, med3d.py:91-100,
 * and their autograd gradients): 64 instead of 216 multiplies per 2x2x2 output tile and
 * channel pair with F(2,3), 216 instead of 1728 per 4x4x4 tile with F(4,3).  Same tensors and layouts as dram_conv3d_*; the packed weights are the
 * transformed ones and every pass needs a caller-owned workspace.
 *   dram_wino_applicable: 1 when the geometry is supported.
 *   dram_conv_wgrad_algo: plan for the WEIGHT gradient of desc, decided separately from
 *                         dram_conv_algo: 0 direct (dram_conv3d_bwd_weight), 1 this pipeline,
 *                         2 in-plane Winograd z-walking kernel (dram_wgrad_w2d).
 *   dram_wino_num_points: P = Winograd points of desc's tiling (outputs per tile along z, y, x: the
 *                         largest of 4x4x4 / 4x4x2 / 4x2x2 / 2x2x2 whose F(4,3) axes divide the
 *                         dilation sub-lattice extent and that leaves >= 512 tiles):
 *                         216, 144, 96 or 64.
 *   dram_wino_num_points_bwd: Pb = points of the DATA-GRADIENT tiling of desc (the plan may tile that
 *                         pass on its own; forward and weight gradient share the cached V and so
 *                         one tiling).  Today Pb == P.
 *   dram_wino_pack_weight: w [Cout][Cin][27] -> uf [P][Cout][Cin], ub [Pb][Cin][Cout]
 *                         (taps flipped, data-gradient operand); either may be NULL.
 *   dram_wino_workspace(desc, pass): bytes for pass 0 forward, 1 data gradient, 2 weight
 *                         gradient (0 when unsupported).
 *   dram_wino_num_stat_rows: rows of stats_partial written by dram_wino_conv3d_fwd.
 *   v_keep / v_cache: optional [dram_wino_v_elems(desc)] floats; the forward pass leaves the
 *                         transformed input there and the weight gradient reuses it instead of
 *                         transforming x again (x may then be NULL).
 * Deterministic (no atomics; the weight gradient sums its slabs in a fixed order).
 * Arithmetic of the Winograd-domain GEMMs: fp32 MFMA by default.  The environment variable
 * DRAM_MATH = "bf16x3" | "bf16" (opt-in, read per call) switches uf / ub / V and the transformed
 * gradients to a split-bf16 image of the same size (hi = bf16(v), lo = bf16(v - hi) per 32-channel
 * block) and the GEMMs to v_mfma_f32_32x32x16_bf16: three products hi*hi + hi*lo + lo*hi per fp32
 * product ("bf16x3", ~2^-16 per product) or hi*hi alone ("bf16", F(2,3) tiles only).  Weights packed
 * and V cached under one mode must be consumed under the same mode. */
int dram_wino_applicable(const DramConvDesc* desc);
int dram_conv_wgrad_algo(const DramConvDesc* desc);
int dram_wino_num_points(const DramConvDesc* desc);
int dram_wino_num_points_bwd(const DramConvDesc* desc);
int dram_wino_pack_weight(const float* w, float* uf, float* ub, const DramConvDesc* desc, dram_stream_t stream);
size_t dram_wino_workspace(const DramConvDesc* desc, int pass);
int dram_wino_num_stat_rows(const DramConvDesc* desc);
size_t dram_wino_v_elems(const DramConvDesc* desc);
int dram_wino_conv3d_fwd(const float* x, const float* uf, const float* bias, float* y,
                         float* stats_partial, float* v_keep, const DramConvDesc* desc, void* workspace,
                         size_t workspace_bytes, dram_stream_t stream);
/* The same convolution reading the PRE-BatchNorm output x_pre of the producing unit: BatchNorm-apply + ReLU
 * (max(x*pscale + pshift, 0), zero padding outside the volume) run inside the input transform (med3d.py:121-124: bn,
 * relu, next conv) -- the activation tensor in between is never written.  F(4,3)^3 tilings, fp32 math only
 * (dram_wino_prologue_supported). */
int dram_wino_prologue_supported(const DramConvDesc* d);
/* The same forward convolution on an input given as TWO channel blocks, x0 [B,D,H,W,C0] | x1 [B,D,H,W,C1] with
 * C0 + C1 = desc->Cin (both multiples of 64): crop_concat_5d feeding conv_blocks[0] of a decoder block (reference
 * med3d.py:39-48, :87) WITHOUT the concatenated tensor -- each source's input transform writes its channel range of the
 * Winograd-domain image; output, statistics and the kept image are bit-identical to dram_wino_conv3d_fwd on the
 * concatenation.  Where dram_wino_prologue_supported(desc) (F(4,3)^3 tiles). */
int dram_wino_conv3d_fwd_cat(const float* x0, int C0, const float* x1, int C1, const float* uf, const float* bias, float* y,
                             float* stats_partial, float* v_keep, const DramConvDesc* desc, void* workspace,
                             size_t workspace_bytes, dram_stream_t stream);
int dram_wino_conv3d_fwd_bn(const float* x_pre, const float* pscale, const float* pshift, const float* uf, const float* bias,
                            float* y, float* stats_partial, float* v_keep, const DramConvDesc* d, void* workspace,
                            size_t workspace_bytes, dram_stream_t stream);
int dram_wino_conv3d_bwd_data(const float* dy, const float* ub, float* dx, const float* add,
                              const float* gate, const DramConvDesc* desc, void* workspace,
                              size_t workspace_bytes, dram_stream_t stream);
/* The data gradient that also takes the BatchNorm-backward statistics of the unit IN FRONT of this convolution
 * (med3d.py:121-124 / :153-161 backward: conv <- relu <- bn): dx is that unit's dz, and with its pre-BatchNorm output
 * bn_y [B,D,H,W,Cin], its batch mean / invstd and the fused scale / shift of its forward pass the output transform
 * writes, per tile block, the rows (sum g, sum g * xhat) with g = dx * (bn_y*scale + shift > 0),
 * xhat = (bn_y - mean) * invstd -- what dram_bn_bwd_reduce (relu = 1, z = NULL) produces in a pass of its own over dx
 * and bn_y.  stats_partial: [dram_wino_num_stat_rows_bwd(desc)][2][Cin] floats, to be folded with
 * dram_fold_partials.  dx is bit-identical to dram_wino_conv3d_bwd_data(add = gate = NULL). */
int dram_wino_num_stat_rows_bwd(const DramConvDesc* desc);
int dram_wino_conv3d_bwd_data_bn(const float* dy, const float* ub, float* dx, const float* bn_y, const float* bn_mean,
                                 const float* bn_invstd, const float* bn_scale, const float* bn_shift,
                                 float* stats_partial, const DramConvDesc* desc, void* workspace, size_t workspace_bytes,
                                 dram_stream_t stream);
int dram_wino_conv3d_bwd_weight(const float* x, const float* v_cache, const float* dy, float* dw,
                                const DramConvDesc* desc, void* workspace, size_t workspace_bytes,
                                dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Fused in-plane Winograd F(2x2, 3x3) x direct-z kernel for narrow (<= 128-channel) stride-1
 * 3x3x3 convolutions with pad == dil == 1, Cin and Cout multiples of 32 (layer1 and decoder
 * conv sites, med3d.py:91-100, :67/:76): forward and data gradient in one kernel each, 2.25x
 * fewer MFMA products than the direct implicit GEMM, nothing extra in HBM.  Weight gradient
 * stays on dram_conv3d_bwd_weight.
 *   dram_wino2d_pack_weight: w [Cout][Cin][27] -> uf [16][3][Cout][Cin], ub [16][3][Cin][Cout]
 *                         (taps flipped); either may be NULL.
 *   stats_partial rows: dram_wino2d_num_stat_rows(desc). */
int dram_wino2d_applicable(const DramConvDesc* desc);
int dram_wino2d_num_stat_rows(const DramConvDesc* desc);
int dram_wino2d_pack_weight(const float* w, float* uf, float* ub, int Cout, int Cin, dram_stream_t stream);
int dram_wino2d_conv3d_fwd(const float* x, const float* uf, const float* bias, float* y,
                           float* stats_partial, const DramConvDesc* desc, dram_stream_t stream);
int dram_wino2d_conv3d_bwd_data(const float* dy, const float* ub, float* dx, const float* add,
                                const float* gate, const DramConvDesc* desc, dram_stream_t stream);

/* Weight gradient of the same narrow layers through the in-plane Winograd domain (z-walking,
 * 48 instead of 108 MFMA products per 2x2 tile); dw in the reference layout [Cout][Cin][27];
 * workspace = column slabs, summed in a fixed order (deterministic). */
int dram_wgrad_w2d_applicable(const DramConvDesc* desc);
size_t dram_wgrad_w2d_workspace(const DramConvDesc* desc);
int dram_wgrad_w2d(const float* x, const float* dy, float* dw, const DramConvDesc* desc, void* workspace,
                   size_t workspace_bytes, dram_stream_t stream);

/* 1x1x1 stride-1 convolutions (Bottleneck conv1 / conv3, med3d.py:152-157) as plain GEMMs on the
 * batched-GEMM kernels of the Winograd pipeline (M = voxels, a multiple of 256; Cin, Cout multiples of
 * 64), with the same fused epilogues as dram_conv3d_*.  w2d is the reference weight [Cout][Cin][1][1][1]
 * as it is; wt its transpose [Cin][Cout] (dram_pack_conv_weight's wb with taps = 1).
 * stats_partial rows: dram_conv1x1_num_stat_rows(desc).  Weight gradient: split over voxels into slabs
 * (workspace), summed in a fixed order. */
int dram_conv1x1_applicable(const DramConvDesc* desc);
int dram_conv1x1_num_stat_rows(const DramConvDesc* desc);
int dram_conv1x1_fwd(const float* x, const float* w2d, const float* bias, float* y, float* stats_partial,
                     const DramConvDesc* desc, dram_stream_t stream);
int dram_conv1x1_bwd_data(const float* dy, const float* wt, float* dx, const float* add, const float* gate,
                          const DramConvDesc* desc, dram_stream_t stream);
size_t dram_conv1x1_bwd_weight_workspace(const DramConvDesc* desc);
int dram_conv1x1_bwd_weight(const float* x, const float* dy, float* dw, const DramConvDesc* desc, void* workspace,
                            size_t workspace_bytes, dram_stream_t stream);

/* The library's plan for one convolution: 0 direct implicit GEMM (dram_conv3d_*), 1 Winograd
 * F(2x2x2,3x3x3) pipeline (dram_wino_*), 2 fused in-plane Winograd (dram_wino2d_*), 3 1x1x1 GEMM
 * (dram_conv1x1_*; dram_conv_wgrad_algo likewise).
 * env DRAM_CONV_ALGO: 1 = always direct, 2 / 3 = path 1 / 2 wherever applicable (tests). */
int dram_conv_algo(const DramConvDesc* desc);

/* ------------------------------------------------------------------------- */
/* Stem: Conv3d(1,64,k=7,s=2,p=3,bias=False)  (med3d.py:196-202 / :296-302).
 *   x [B,D,H,W] (C=1), w [64][1][7][7][7], y [B,Do,Ho,Wo,64], Do=(D+6-7)/2+1 ...
 *   stats_partial [dram_stem_num_tiles][2][64] or NULL. */
int dram_stem_num_tiles(int B, int Do, int Ho, int Wo);
int dram_stem_fwd(const float* x, const float* w, float* y, float* stats_partial, int B, int D, int H,
                  int W, dram_stream_t stream);
size_t dram_stem_bwd_weight_workspace(int B, int D, int H, int W);
int dram_stem_bwd_weight(const float* x, const float* dy, float* dw, int B, int D, int H, int W,
                         void* workspace, size_t workspace_bytes, dram_stream_t stream);
/* Data gradient (the transposed convolution): dx[b,d,h,w] = sum_c sum_k dy[b,od,oh,ow,c] * w[c,0,kd,kh,kw] over
 * 2*od + kd - 3 == d (h, w likewise), dx [B,D,H,W] fp32.  Two launches: the scatter GEMM taps x voxels (K = 64) of
 * every 4x8x8 block of dy voxels, overlap-added into that block's 13x21x21 input patch (workspace), and a fold of
 * the overlapping patches in a fixed order -- deterministic, no atomics.  Any D, H, W >= 1. */
size_t dram_stem_bwd_data_workspace(int B, int D, int H, int W);
int dram_stem_bwd_data(const float* dy, const float* w, float* dx, int B, int D, int H, int W, void* workspace,
                       size_t workspace_bytes, dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* BatchNorm3d (+ReLU, + residual) -- med3d.py:121-124,133-142,153-182,203-204,227-228.
 *
 * dram_reduce_partials: sums[r][c] (double) = sum_p partial[p][r][c], r < R.
 *   Used for the BN statistics, BN-backward sums and bias gradients.  In DDP the
 *   caller all-reduces `sums` (SyncBatchNorm, train.py:101) before finalising.
 *   Two-stage for many partials: scratch = dram_reduce_partials_stages(nparts)*R*C doubles
 *   (may be NULL when stages == 1).  Fixed summation order (deterministic).
 *   has_tail != 0: also writes sums[R*C] = tail (the caller's buffer then has R*C+1 doubles): the
 *   rank's element count rides behind the sums so that ONE all-reduce gives global sums AND the
 *   global count (ranks may hold different batch sizes -- torch SyncBatchNorm semantics). */
int dram_reduce_partials_stages(int nparts);
/* The same fold in ONE launch (S = dram_fold_partials_stages(nparts) stage rows; for S > 1 the last block of a column
 * group to finish folds them, fixed order): scratch = S*R*C doubles, followed for S > 1 by DRAM_FOLD_TICKET_DOUBLES
 * doubles of per-call ticket words which the call zeroes itself (a memset on `stream`: launches in flight together on
 * other streams, or a graph replay beside an eager step, never share a counter); sums_f32: optional float copy of the sums
 * ([R][C]; with f32_row1 != NULL and R == 2, row 1 goes there instead: two separately allocated [C] tensors).
 * dram_bn_fold_finalize: fold of the [nparts][2][C] convolution-epilogue partials + dram_bn_finalize on the result
 * (host-side count) in that launch -- the single-process training forward. */
#define DRAM_FOLD_TICKET_DOUBLES 256
int dram_fold_partials_stages(int nparts);
int dram_fold_partials(const float* partial, double* sums, double* scratch, float* sums_f32, float* f32_row1, int nparts,
                       int R, int C, double tail, int has_tail, dram_stream_t stream);
int dram_bn_fold_finalize(const float* partial, double* sums, double* scratch, int nparts, int C, double count,
                          const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                          float eps, int update_running, float* mean, float* invstd, float* scale, float* shift,
                          dram_stream_t stream);
int dram_reduce_partials(const float* partial, double* sums, double* scratch, int nparts, int R, int C,
                         double tail, int has_tail, dram_stream_t stream);

/* training: mean/var from sums[2][C] over `count` elements per channel;
 * eval (sums == NULL): running stats.  Writes mean, invstd, scale = gamma*invstd,
 * shift = beta - mean*scale; when update_running != 0 also
 * running = (1-momentum)*running + momentum*{mean, unbiased var}. */
/* count_dev (device pointer, may be NULL): when given the element count is read from device memory
 * (the all-reduced tail of dram_reduce_partials) and `count` is ignored -- no host round trip. */
int dram_bn_finalize(const double* sums, double count, const double* count_dev, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps,
                     int update_running, float* mean, float* invstd, float* scale, float* shift,
                     int C, dram_stream_t stream);

/* z = act(y*scale[c] + shift[c] + residual).  residual: NULL, or a tensor
 * [B,Dr,Hr,Wr,Cr] sampled at (z*rs, y*rs, x*rs) with channels >= Cr reading 0 --
 * identity shortcut (rs=1, same shape) or shortcut type A (med3d.py:103-112, strided
 * subsample + zero channel pad).  relu != 0 => max(0,.) */
int dram_bn_apply(const float* y, const float* scale, const float* shift, const float* residual,
                  int Dr, int Hr, int Wr, int Cr, int rs, float* z, int B, int D, int H, int W, int C,
                  int relu, dram_stream_t stream);

/* Backward, phase 1: g = dz * (z > 0) (relu != 0) ; partial[p][0][c] = sum g,
 * partial[p][1][c] = sum g * xhat, xhat = (y-mean)*invstd.  nparts from dram_colsum_nparts.
 * The ReLU mask comes from the saved output z, or -- z == NULL, for a BatchNorm without residual --
 * is re-derived from y as fma(y, scale, shift) > 0 with the forward's scale / shift vectors
 * (bitwise the forward's decision; saves one tensor read in each phase). */
int dram_colsum_nparts(long long rows, int C);
int dram_bn_bwd_reduce(const float* dz, const float* z, const float* y, const float* mean,
                       const float* invstd, const float* scale, const float* shift, float* partial,
                       long long rows, int C, int relu, dram_stream_t stream);
/* phase 2: dy = gamma*invstd*(g - sums[0]/count - xhat*sums[1]/count).
 * colsum_partial: NULL, or [dram_bn_bwd_apply_nparts(rows, C)][C] -- per-workgroup column sums of dy (the
 * bias gradient of the convolution in front, med3d.py:67/:76/:226, without a pass of its own); nparts < 1
 * => unsupported for this C (C / 4 must divide 256), use dram_colsum.  count_dev: as in dram_bn_finalize. */
int dram_bn_bwd_apply_nparts(long long rows, int C);
int dram_bn_bwd_apply(const float* dz, const float* z, const float* y, const float* mean,
                      const float* invstd, const float* gamma, const float* scale, const float* shift,
                      const double* sums, double count, const double* count_dev, float* dy,
                      float* colsum_partial, long long rows, int C, int relu, dram_stream_t stream);
/* phase 2 of a BatchNorm that ran on its RUNNING statistics (eval mode): dy = scale * g, scale = gamma *
 * invstd_running as dram_bn_finalize(sums == NULL) returns it; no batch-mean terms, so it needs no phase 1 (that one,
 * with the running mean / invstd, gives the parameter gradients where they are wanted).  The ReLU mask comes from z,
 * and then y is not read and may be NULL, or (z == NULL) from fma(y, scale, shift) > 0.  colsum_partial as above. */
int dram_bn_bwd_apply_eval(const float* dz, const float* z, const float* y, const float* scale, const float* shift,
                           float* dy, float* colsum_partial, long long rows, int C, int relu, dram_stream_t stream);
/* partial[p][0][c] = sum_rows a[row][c]  (conv-bias gradient) */
int dram_colsum(const float* a, float* partial, long long rows, int C, dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* MaxPool3d(k=3,s=2,p=1) -- med3d.py:206/:275.  argmax: uint8 tap index (first max
 * wins, scan order kd,kh,kw like ATen).  Backward is a gather (deterministic);
 * dx = maxpool^T(dy) (+ add if not NULL).  add: voxel-major like dx with add_stride floats per voxel
 * (add_stride == C: a tensor shaped like dx; larger: a channel slice of a wider tensor, e.g. the skip half
 * of the decoder's concat gradient read in place). */
int dram_maxpool_fwd(const float* x, float* y, uint8_t* argmax, int B, int D, int H, int W, int C,
                     dram_stream_t stream);
/* Stem: BatchNorm-apply + ReLU + max-pool in one pass over the pre-BN tensor y (med3d.py:272-275): writes z =
 * relu(y*scale + shift) (full resolution: skip connection, ReLU mask), the pooled tensor and the taps -- bit-identical to
 * dram_bn_apply followed by dram_maxpool_fwd, one read of the tensor less. */
int dram_bn_maxpool_fwd(const float* y, const float* scale, const float* shift, float* z, float* pooled, uint8_t* argmax,
                        int B, int D, int H, int W, int C, dram_stream_t stream);
int dram_maxpool_bwd(const float* dy, const uint8_t* argmax, const float* add, int add_stride, float* dx,
                     int B, int D, int H, int W, int C, dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* dRAM up-projection inside the decoder: nn.Upsample(x2, trilinear, align_corners=True)
 * + crop_concat_5d -- med3d.py:83-87, :39-48.
 *   src  [B,Ds,Hs,Ws,Cu]  -> upsampled to (2Ds,2Hs,2Ws)
 *   skip [B,Dk,Hk,Wk,Ck]  centre-cropped to the upsampled size
 *   cat  [B,2Ds,2Hs,2Ws,Cu+Ck]  (upsampled channels FIRST)
 * skip == NULL with Ck == 0 (Dk, Hk, Wk >= the up-sampled extents): the up-sampled tensor alone -- the convolution
 * behind it takes the skip tensor as a second source (dram_wino_conv3d_fwd_cat) and `cat` is never built. */
int dram_upcat_fwd(const float* src, const float* skip, float* cat, int B, int Ds, int Hs, int Ws, int Cu,
                   int Dk, int Hk, int Wk, int Ck, dram_stream_t stream);
/* dsrc = upsample^T(dcat[..., :Cu]);  dskip (full skip shape, zero outside the crop)
 * = dcat[..., Cu:].  Either output may be NULL. */
int dram_upcat_bwd(const float* dcat, float* dsrc, float* dskip, int B, int Ds, int Hs, int Ws, int Cu,
                   int Dk, int Hk, int Wk, int Ck, dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* First decoder convolution of us1 WITHOUT the up-sampled tensor (csrc/upmix.hip) -- med3d.py:83-87 with
 * conv_blocks[0] (med3d.py:67): conv(concat(up(a), s)) = sum_t up(W_up[t] . a) shifted by tap t + conv_s(s).
 * The channel mixing W_up[t] . a is a plain GEMM at the LOW resolution (the 1x1x1 entry points, Cout = 27 Co);
 * what these entry points add is the tap/trilinear gather, separable per axis, and the weight split / merge.
 *
 * dram_upmix_axis_fwd:  In[outer][Ni][m][3][C] (float, or bf16 when in_bf16) -> Out[outer][2 Ni][m][C] (float):
 *   Out[o][v][m][c] = sum_k [0 <= u = v+k-1 < 2Ni] (w0(u) In[o][i0(u)][m][k][c] + w1(u) In[o][i1(u)][m][k][c]),
 *   (i0, i1, w0, w1)(u) = PyTorch's align_corners source index of destination u, scale (Ni-1)/(2Ni-1).
 *   Three calls: X (outer = B Ds Hs, Ni = Ws, m = 9), Y (outer = B Ds, Ni = Hs, m = 2Ws 3), Z = ..._final.
 * dram_upmix_axis_fwd_final: the same pass, + base (NULL, or the skip convolution's output; may alias out), stored
 *   as float / bf16, with BatchNorm partial sums of the stored values: stats [dram_upmix_stat_rows(nvox)][2][C]
 *   (NULL: none), nvox = outer 2Ni m, C <= 128.
 * dram_upmix_axis_bwd: the exact transpose, G[outer][2Ni][m][C] -> H[outer][Ni][m][3][C] (gather form, no atomics).
 * dram_upmix_split_weight: w [Co][Cu+Cs][27] -> wlo [27 Co][Cu] (row t Co + co) and ws [Co][Cs][27];
 * dram_upmix_merge_wgrad: the inverse, for the two weight gradients. */
int dram_upmix_stat_rows(long long nvox);
int dram_upmix_axis_fwd(const void* in, int in_bf16, float* out, long long outer, int Ni, int m, int C,
                        dram_stream_t stream);
int dram_upmix_axis_fwd_final(const float* in, const void* base, void* out, int out_bf16, float* stats, long long outer,
                              int Ni, int m, int C, dram_stream_t stream);
int dram_upmix_axis_bwd(const void* g, int g_bf16, void* h, int h_bf16, long long outer, int Ni, int m, int C,
                        dram_stream_t stream);
int dram_upmix_split_weight(const float* w, float* wlo, float* ws, int Co, int Cu, int Cs, dram_stream_t stream);
int dram_upmix_merge_wgrad(const float* dwlo, const float* dws, float* dw, int Co, int Cu, int Cs, dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Heads -- med3d.py:283-284 (cls) / :382-387 (reg).
 *   x [B,D,H,W,32]; w [NO][32], bias [NO]  (fcs.0 and fcs.1 stacked: NO = 6+3 or 1+1)
 *   dense [B][NO][D*H*W]  (planar == the reference's NCDHW per head)
 *   sigmoid != 0: dense = sigmoid(.) and pooled sums are lung-weighted:
 *     lungs: NULL (=> ones) or the FULL-RES mask [B,Dl,Hl,Wl], sampled nearest
 *     (F.interpolate(mode='nearest'), med3d.py:386).
 *   partial [B][nblk][NO+1]: per-block sum(dense*L) per output, and sum(L) last. */
int dram_head_nblk(long long voxels_per_sample);
int dram_head_fwd(const float* x, const float* w, const float* bias, const float* lungs, int Dl, int Hl,
                  int Wl, float* dense, float* partial, int B, int D, int H, int W, int NO, int sigmoid,
                  dram_stream_t stream);
/* backward: dpre[c] = (gdense[b][c][v] + gpool[b][c]*L[v]) * (sigmoid ? s(1-s) : 1)
 *   gdense may be NULL.  dx [B,D,H,W,32] = sum_c w[c][:] dpre[c];
 *   wpartial [B*nparts][NO][33]: per-block sum dpre[c]*x[k] (k<32) and sum dpre[c] (k=32);
 *   nparts = dram_head_bwd_nparts(D*H*W) blocks per sample. */
int dram_head_bwd_nparts(long long voxels_per_sample);
int dram_head_bwd(const float* x, const float* w, const float* dense, const float* gdense,
                  const float* gpool, const float* lungs, int Dl, int Hl, int Wl, float* dx,
                  float* wpartial, int B, int D, int H, int W, int NO, int sigmoid, dram_stream_t stream);

/* Class-activation maps at the target layer (get_target_layer(), med3d.py:267,366: the us3 output x the heads read).
 *   G[b][v][k] = sum_c w[c][k] * dpre[b][c][v], dpre exactly as dram_head_bwd defines it (gdense may be NULL; lungs as
 *   for the heads), with s = sigmoid(bias[c] + w[c] . x) recomputed from x -- G is formed in registers, never stored.
 *   out [B][D*H*W] float; r(t) = relu != 0 ? max(t, 0) : t.
 * dram_cam_point (one pass over x):  DRAM_CAM_HIRESCAM  out = r(sum_k G * x)
 *                                    DRAM_CAM_LAYERCAM  out = r(sum_k max(G, 0) * x)
 * DRAM_CAM_GRADCAM, out = r(sum_k alpha[b][k] * x), alpha[b][k] = (1/V) sum_v G[b][v][k], is two passes:
 *   dram_cam_sum      partial [nblk][B][NO], nblk = dram_cam_nblk(D*H*W): per-block sums of dpre (x is read only when
 *                     sigmoid != 0); the caller folds them with dram_fold_partials (R*C = B*NO: samples stay apart)
 *   dram_cam_combine  sums [B][NO] (double): alpha = (sum_c w[c][k] * sums[b][c]) / (D*H*W) in double, then the map.
 * Fixed summation order, no atomics: bit-identical from call to call.  B*D*H*W*32 < 2^31 (DRAM_ERR_UNSUPPORTED). */
#define DRAM_CAM_GRADCAM 0
#define DRAM_CAM_HIRESCAM 1
#define DRAM_CAM_LAYERCAM 2
int dram_cam_nblk(long long voxels_per_sample);
int dram_cam_point(const float* x, const float* w, const float* bias, const float* gdense, const float* gpool,
                   const float* lungs, int Dl, int Hl, int Wl, float* out, int B, int D, int H, int W, int NO,
                   int sigmoid, int method, int relu, dram_stream_t stream);
int dram_cam_sum(const float* x, const float* w, const float* bias, const float* gdense, const float* gpool,
                 const float* lungs, int Dl, int Hl, int Wl, float* partial, int B, int D, int H, int W, int NO,
                 int sigmoid, dram_stream_t stream);
int dram_cam_combine(const float* x, const float* w, const double* sums, float* out, int B, int D, int H, int W,
                     int NO, int relu, dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* dRAM segmentation losses -- models.py:523-531 + metrics.py:10-37, label prep
 * models.py:567-570.  cle/pse: [B,1,D,H,W] dense maps; lungs/ems: full-res masks
 * [B,Dl,Hl,Wl] sampled nearest; binary[b] in {0,1} multiplies ems; smoothness = the
 * in-mask weight of metrics.py:10,24 (0.85 at the models.py:529 call site).
 *   partial [nblk][6]: sum t, A1, A0, I, S1, S2 (see csrc/loss.hip). */
int dram_segloss_nblk(long long voxels_total);
int dram_segloss_fwd(const float* cle, const float* pse, const float* lungs, const float* ems,
                     const float* binary, int Dl, int Hl, int Wl, float* partial, int B, int D, int H,
                     int W, float smoothness, dram_stream_t stream);
/* coef[8] (device): c_dice_a, c_dice_b, c_bce1, c_bce0, -, -, -, - (see loss.hip) */
int dram_segloss_bwd(const float* cle, const float* pse, const float* lungs, const float* ems,
                     const float* binary, int Dl, int Hl, int Wl, const float* coef, float* gcle,
                     float* gpse, int B, int D, int H, int W, float smoothness, dram_stream_t stream);

/* The O(B) tail of the regression train loss (models.py:549-574) in ONE launch: the fp64 fold of the seg-loss
 * block sums, dice + balanced BCE (metrics.py:10-37), the two interval losses (models.py:512-521) with the band
 * of each label looked up in *_bands [n][2] (models.py:492-510), loss = cle + pse + 2 mul + seg.
 *   out [5]: loss, loss_cle, loss_pse, mul_loss, seg_loss;  coef [8]: dram_segloss_bwd's input for d loss;
 *   greg [2][B]: d loss / d reg_outs.  A label outside its band table makes the loss NaN. */
int dram_regloss_tail(const float* partial, int nblk, const float* reg_cle, const float* reg_pse,
                      const long long* cle_labels, const long long* pse_labels, const float* cle_w,
                      const float* pse_w, const float* cle_bands, int n_cle, const float* pse_bands, int n_pse,
                      int B, double voxels_total, double smooth, double beta, double gamma, float* out,
                      float* coef, float* greg, dram_stream_t stream);

/* Predict-time up-projection (models.py:438-441): out = trilinear(dense -> Do,Ho,Wo,
 * align_corners) * ess; partial [B][nblk] per-block sums of out. */
int dram_upproject_nblk(long long voxels_per_sample);
int dram_upproject(const float* dense, const float* ess, float* out, float* partial, int B, int D, int H,
                   int W, int Do, int Ho, int Wo, dram_stream_t stream);

/* Predict-time up-projection of BOTH heads with a per-region table (csrc/regions.hip; the reference has no regional
 * code: with every lung label <= n_regions the table reduces to its per-lung number, models.py:438-441).
 *   cle, pse: the two heads' dense maps [D,H,W] of sample b at cle / pse + b * dense_batch_stride (elements): two
 *     channel views of one tensor need no copy.  ess, labels [B][Do][Ho][Wo] bytes (ess: non-zero = 1.0f).
 *   out_cle, out_pse [B][Do][Ho][Wo] = trilinear(dense -> Do,Ho,Wo, align_corners) * ess, bit for bit what
 *     dram_upproject stores; both NULL: the table only.
 *   table [B][n_regions + 1][4] double, row r = { sum out_cle, sum out_pse, #(ess != 0), #voxels } over the voxels with
 *     labels == r; row 0 also collects every label above n_regions.  partial [B][nblk][n_regions + 1][4] float scratch,
 *     nblk = dram_region_nblk(Do*Ho*Wo) (every row is written: no memset); a second launch folds it per sample in index
 *     order in double.  No atomics: bit-identical from call to call.  The counts are exact.
 * n_regions 1..15, dense_batch_stride >= D*H*W, sizes >= 1, exactly one of out_cle / out_pse NULL: DRAM_ERR_BAD_ARG;
 * Do*Ho*Wo or D*H*W >= 2^31, B > 65535: DRAM_ERR_UNSUPPORTED.
 * dram_prep_labels: out [Do,Ho,Wo] bytes = clamp(labels[zidx[zo]][ys][xs], 0, 255), ys / xs = min(floor(dst * in/out),
 *   in - 1) as dram_prep_mask; labels of label_dtype 1 (uint8) or 2 (int16) is a [D,H,W] view read through its element
 *   strides (x stride 1, strides >= 0), e.g. the lung crop of the lobe volume: never copied or converted. */
int dram_region_nblk(long long voxels_per_sample);
int dram_upproject_regions(const float* cle, const float* pse, long long dense_batch_stride, const uint8_t* ess,
                           const uint8_t* labels, float* out_cle, float* out_pse, float* partial, double* table, int B,
                           int D, int H, int W, int Do, int Ho, int Wo, int n_regions, dram_stream_t stream);
int dram_prep_labels(const void* labels, int label_dtype, long long stride_z, long long stride_y, const int* zidx,
                     uint8_t* out, int D, int H, int W, int Do, int Ho, int Wo, dram_stream_t stream);

/* Validation / test activation-map volumes (_draw_predictions, models.py:192-234 / :455-493), csrc/heat.hip.
 *   dense: head outputs of one head, C channels [d,h,w] (innermost three dimensions contiguous) at
 *     dense + b * stride_b + c * stride_c (strides in ELEMENTS, multiples of 4; dense 16-byte aligned; w % 4 == 0),
 *     so both heads read the engine's one [B,n0+n1,d,h,w] tensor through its channel views without a copy.
 *   up_c = F.interpolate(dense[b,c], size=(D,H,W)=(2d,2h,2w), mode='trilinear'), align_corners=False: source
 *     coordinate max(k/2 - 0.25, 0), weights {0.25, 0.75} ({1, 0} at k = 0), far tap clamped to n - 1.  The
 *     up-sampled channels are never stored; both passes recompute them from dense.
 *   DRAM_HEAT_CLASSSUM (C >= 2): dp = sum_{c>=1} max(up_c, 0);  v = dp / (peak[b] + 1e-7f) * lung
 *   DRAM_HEAT_PLAIN    (C == 1): v = up_0 * lung
 *   lung [B][D][H][W] bytes (bool / uint8), non-zero = 1.0f, 8-byte aligned.
 * dram_heat_peak: partial [B][nblk], nblk = dram_heat_nblk(D*H*W): per-block maxima of dp over the WHOLE volume, before
 *   the lung mask; the caller folds them (max over nblk) into peak [B].
 * dram_heat_volume: out_f32 = v (unclamped) and / or out_u8 = trunc(255 * clamp(v, 0, 1)), either may be NULL, each
 *   [B][D][H][W] -- or, with zsel [B][nz] int32 (output-grid z indices in [0, D), per sample, repeats allowed; the
 *   caller checks the range), [B][nz][H][W]: those slices of the full result, bit for bit.  nz is ignored without zsel.
 *   Every output element is written.  peak is read in CLASSSUM only.
 * No atomics, fixed order: bit-identical from call to call.  D*H*W >= 2^31: DRAM_ERR_UNSUPPORTED; an output grid that
 * is not exactly twice the dense grid, a channel count the mode does not take, zsel with nz <= 0: DRAM_ERR_BAD_ARG. */
#define DRAM_HEAT_CLASSSUM 0
#define DRAM_HEAT_PLAIN 1
int dram_heat_nblk(long long voxels_per_sample);
int dram_heat_peak(const float* dense, long long stride_b, long long stride_c, int C, float* partial, int B, int d,
                   int h, int w, int D, int H, int W, dram_stream_t stream);
int dram_heat_volume(const float* dense, long long stride_b, long long stride_c, int C, const uint8_t* lung,
                     const float* peak, const int* zsel, int nz, float* out_f32, uint8_t* out_u8, int mode, int B,
                     int d, int h, int w, int D, int H, int W, dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Multi-tensor optimizers -- torch.optim.Adam at models.py:385-387 / :689-691 and the
 * SGD arguments of train.py:25,27.  table: device array of DramTensorRef[ntensors];
 * chunks: device array of DramChunkRef[nchunks] (tensor index + element offset). */
typedef struct DramTensorRef {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} DramTensorRef;
typedef struct DramChunkRef {
  int32_t tensor;
  int32_t pad;
  int64_t offset;
} DramChunkRef;
#define DRAM_OPT_CHUNK 16384
/* Work list of dram_pack_conv_weight_bf16_multi: weight [Cout][Cin][taps] (fp32) -> its bf16 packed copies wf
 * [taps][Cout][Cin] / wb [taps reversed][Cin][Cout] at ELEMENT offsets off_f / off_b of one flat bf16 buffer (-1: not
 * wanted); chunks enumerate the tiles of each weight: offset = 0 .. dram_pack_conv_weight_bf16_tiles(...) - 1. */
typedef struct DramPackRef {
  const float* w;
  int64_t off_f;
  int64_t off_b;
  int32_t Cout, Cin, taps, pad;
} DramPackRef;
int dram_adam_multi(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float lr,
                    float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                    float bias_corr2, float grad_scale, dram_stream_t stream);
/* Same update with every hyper-parameter and the step count in DEVICE memory:
 *   hyper = float[7] {lr, beta1, beta2, eps, weight_decay, grad_scale, step}
 * step is incremented on the device first and the bias corrections 1 - beta^step are computed in the
 * kernel (double), so a hipGraph captured around a train step stays valid across steps and lr changes
 * (the host only rewrites hyper[0] when the scheduler moves lr). */
int dram_adam_multi_dev(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float* hyper,
                        dram_stream_t stream);
int dram_sgd_multi(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float lr,
                   float momentum, float weight_decay, int first_step, float grad_scale,
                   dram_stream_t stream);

/* Gradient clipping on the same work list (Lightning's --gradient_clip_val / --gradient_clip_algorithm, which the
 * reference's Trainer.add_argparse_args puts on its command line, train.py:46,100).  clip = float[4] in device memory:
 *   clip[0] in   max_norm
 *   clip[1] in   clip_value; NEGATIVE selects norm mode in the launches below, >= 0 value mode
 *   clip[2] out  total_norm = (float)(|grad_scale| * sqrt(sum g^2)), squares and sums in double
 *   clip[3] out  coef = min(1, max_norm / (total_norm + 1e-6f)) in fp32 (torch.nn.utils.clip_grad_norm_)
 * dram_grad_norm_multi: reads every gradient of the table once (4 B/element; p, m, v are not touched and may be NULL),
 *   writes one double per chunk into partials[nchunks] and folds them in a second, one-block launch: a fixed summation
 *   order that depends on the element index only -- not on the order the blocks ran in, and not on whether a gradient is
 *   16- or only 4-byte aligned.  grad_scale: host value, or hyper[5] when hyper (dram_adam_multi_dev's block) is given.
 * dram_*_clip: the three updates with gg = (g * grad_scale) * clip[3]  (norm mode)  or
 *   gg = clamp(g * grad_scale, -clip[1], clip[1]) (value mode; a NaN stays a NaN) in place of g * grad_scale; everything
 *   behind that is the code of the plain entry points.  No gradient is written.
 * dram_grad_scale_multi: g = g * clip[3] or clamp(g, -clip[1], clip[1]) IN PLACE (8 B/element) -- the drop-in
 *   clip_grad_norm_ / clip_grad_value_ for callers who look at the gradients afterwards. */
int dram_grad_norm_multi(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, double* partials,
                         float* clip, float grad_scale, const float* hyper, dram_stream_t stream);
int dram_grad_scale_multi(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, const float* clip,
                          dram_stream_t stream);
int dram_adam_multi_clip(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float lr,
                         float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                         float bias_corr2, float grad_scale, const float* clip, dram_stream_t stream);
int dram_adam_multi_dev_clip(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float* hyper,
                             const float* clip, dram_stream_t stream);
int dram_sgd_multi_clip(const DramTensorRef* table, const DramChunkRef* chunks, int nchunks, float lr,
                        float momentum, float weight_decay, int first_step, float grad_scale, const float* clip,
                        dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Deterministic input transforms of the reference data module (models.py:59-63):
 * IntensityWindow (functional.py:13-26), Standardize (intensity_transforms.py:108-111),
 * Interpolate(align_corners, only_in_plane) for images / masks (spatial_transforms.py:55-98).
 *   scan [D,H,W] raw HU as float32; zidx [Do] int32 = torch.linspace(0, D-1, Do).long();
 *   dram_window_stats -> partial [nblk][2] (sum w, sum w^2 of the windowed values);
 *   mean_invstd [2] (device) = {mean, 1/std(unbiased)} of the windowed volume;
 *   dram_prep_image -> out [Do,Ho,Wo]; dram_prep_mask -> nearest-resized mask. */
int dram_window_stats_nblk(long long n);
int dram_window_stats(const float* scan, float* partial, long long n, float lo, float hi, dram_stream_t stream);
int dram_prep_image(const float* scan, const int* zidx, const float* mean_invstd, float* out, int D, int H, int W,
                    int Do, int Ho, int Wo, float lo, float hi, dram_stream_t stream);
int dram_prep_mask(const float* mask, const int* zidx, float* out, int D, int H, int W, int Do, int Ho, int Wo,
                   dram_stream_t stream);

/* One archive case -> one training sample straight from the int16 data (csrc/sample_prep.hip; dataset.py:147-155 with
 * the transforms above): two launches, no float32 copy of a full-size volume.
 *   dram_sample_stats_i16: scan [n] int16 (any 2-byte-aligned base, any n >= 2); c = clamp(x, lo, hi) - lo per voxel;
 *     partial [dram_sample_stats_nblk(n)][2] int64, row b = {sum c, sum c^2} over block b's share (every row is written:
 *     no memset).  Integer sums, no atomics: exact, bit-identical from call to call.  The windowed value of the reference
 *     is c / (hi - lo), so with S1, S2 the column sums: mean = S1 / n / (hi - lo),
 *     var (unbiased) = (S2 - S1^2 / n) / (n - 1) / (hi - lo)^2 -- the caller's float64 glue on [nblk][2].
 *   dram_prep_sample_i16: one pass over the output grid.  scan [D,H,W] int16; lung [D,H,W] of lung_dtype 1 (uint8 / bool)
 *     or 2 (int16); zidx [Do] and mean_invstd [2] as for dram_prep_image.  Per output voxel:
 *       out_image = (bilinear(window(scan[zidx[z]]))(y, x) - mean) * invstd, dram_prep_image's arithmetic on the (exactly)
 *         converted taps;
 *       out_lung  = lung[nn] > 0 (signed for int16), nn the nearest source voxel of dram_prep_mask;
 *       out_em    = scan[nn] < em_threshold && lung[nn] > 0
 *     -- the masks equal thresholding at full size and resizing afterwards (dataset.py:149, spatial_transforms.py:77-97).
 *     out_image (float), out_lung, out_em (bytes 0 / 1): dense [Do,Ho,Wo] blocks at any base, e.g. one slot of a batch.
 * Neither call synchronises; both can be captured.
 * A null pointer, a size < 1, n < 2, hi <= lo, hi - lo > 4095, lo or hi outside -65536..65536, lung_dtype not 1 / 2:
 * DRAM_ERR_BAD_ARG.  n, D*H*W or Do*Ho*Wo >= 2^31: DRAM_ERR_UNSUPPORTED. */
int dram_sample_stats_nblk(long long n);
int dram_sample_stats_i16(const int16_t* scan, long long* partial, long long n, int lo, int hi, dram_stream_t stream);
int dram_prep_sample_i16(const int16_t* scan, const void* lung, int lung_dtype, const int* zidx, const float* mean_invstd,
                         float* out_image, uint8_t* out_lung, uint8_t* out_em, int D, int H, int W, int Do, int Ho, int Wo,
                         int lo, int hi, int em_threshold, dram_stream_t stream);

/* Predict post-processing (processor.py:111-129, :143): src [D,H,W] resized (trilinear, align_corners=True) to
 * the lung-crop size (rd,rh,rw) and pasted at offset (oz,oy,ox) into a zero volume of the original grid
 * [Do,Ho,Wo]; out_f32 and/or out_u8 (= utils.windowing(., (0,1) -> (0,255)) truncated to uint8). */
int dram_resample_paste(const float* src, float* out_f32, uint8_t* out_u8, int D, int H, int W, int rd, int rh, int rw,
                        int oz, int oy, int ox, int Do, int Ho, int Wo, dram_stream_t stream);

/* Scan + lobe segmentation -> prepared predict case (dataset.py:57-92 SubtypingInference.get_data with
 * utils.py:53-63 find_crops), csrc/case_prep.hip.  scan [D,H,W] int16 HU; lobes [D,H,W] of lobe_dtype 1 (uint8) or
 * 2 (int16), 16-byte aligned for dram_lung_bbox; lung = lobes > 0.  D*H*W < 2^31 (DRAM_ERR_UNSUPPORTED).
 *   dram_lung_bbox: partial [dram_lung_bbox_nblk(D*H*W)][8] int32 scratch (every row is written: no memset), then a
 *     fixed-order fold -> box [8] int32 (device) = {z0, z1, y0, y1, x0, x1, voxel count, 0}, half-open; all 0 for
 *     an empty lung.  No atomics: bit-identical from call to call.
 *   dram_case_prepare over the crop box [Dc,Hc,Wc] at offset (z0,y0,x0), which must lie inside the volume AND hold
 *     every lung voxel (the padded bounding box does; lobes outside it are not read, so the dilation needs no halo
 *     from outside the crop):
 *       image [Dc,Hc,Wc] int16 = scan where the (2*radius+1)^3 box dilation of the lung, clipped to the volume,
 *         is set (= `radius` iterations of scipy's binary_dilation with the full 3x3x3 structure), else fill_value;
 *       lung_mask, ess_mask [Dc,Hc,Wc] uint8 0/1, ess = scan < threshold && lung;
 *       original (optional, may be NULL) int16 = the plain crop of scan.
 *     radius 0..3; fill_value and threshold within int16.  The dilated volume is never written. */
int dram_lung_bbox_nblk(long long n);
int dram_lung_bbox(const void* lobes, int lobe_dtype, int* partial, int* box, int D, int H, int W,
                   dram_stream_t stream);
int dram_case_prepare(const void* scan, const void* lobes, int lobe_dtype, void* image, uint8_t* lung_mask,
                      uint8_t* ess_mask, void* original, int D, int H, int W, int z0, int y0, int x0, int Dc, int Hc,
                      int Wc, int radius, int fill_value, int threshold, dram_stream_t stream);

/* Per-lobe CT histogram of a prepared case (csrc/densito.hip): ONE pass over image [D,H,W] int16 HU (contiguous) and
 * labels [D,H,W] of label_dtype 1 (uint8) or 2 (int16), read in place through stride_z / stride_y (in elements, >= 0;
 * x stride 1), e.g. dram_case_prepare's image and the lung crop of the lobe volume.
 *   hist [n_regions + 1][nbins] int64: voxels per row and 1-HU bin, bin = clamp(hu, hu_lo, hu_lo + nbins - 1) - hu_lo
 *     (the two end bins collect the tails);
 *   sums [n_regions + 1][2] int64 = { voxel count, sum of the raw (unclamped) HU values }.
 *   Rows: label r in 1..n_regions -> row r; label <= 0 (signed for int16) is not lung and is counted nowhere; a label
 *     above n_regions -> row 0 (lung that belongs to no region; no background there).  Sum over the rows = lobes > 0.
 *   part_hist [nblk][n_regions + 1][nbins] int32 and part_sums [nblk][n_regions + 1][2] int64 scratch, nblk =
 *     dram_lobe_hist_nblk(D*H*W): every workgroup writes all of its rows (no memset), a second launch folds them in
 *     index order.  No global atomics, no ticket word, never synchronises, capturable; integer counts: bit-identical
 *     from call to call.
 * Null operand, label_dtype not 1 / 2, a size < 1, a negative stride, n_regions outside 1..15: DRAM_ERR_BAD_ARG.
 * Supported: D*H*W < 2^31; nbins a multiple of 64 in 64..2048 with (n_regions + 1) * nbins <= 32768 (the counters of
 * a workgroup live in LDS, 128 KiB at most); -32768 <= hu_lo and hu_lo + nbins - 1 <= 32767.  Anything else:
 * DRAM_ERR_UNSUPPORTED. */
int dram_lobe_hist_nblk(long long voxels);
int dram_lobe_hist(const void* image, const void* labels, int label_dtype, long long stride_z, long long stride_y,
                   int* part_hist, int64_t* part_sums, int64_t* hist, int64_t* sums, int D, int H, int W, int n_regions,
                   int hu_lo, int nbins, dram_stream_t stream);

/* Core / peel zones of the lung from an exact 3-D Euclidean distance transform (csrc/edt.hip).  labels [D,H,W] of
 * label_dtype 1 (uint8) or 2 (int16), read in place through stride_z / stride_y (in elements, >= 0; x stride 1) like
 * dram_lobe_hist's; lung = label > 0 (signed for int16), background = every other voxel of the volume, and nothing
 * outside the volume is background.  All distance arithmetic is in integers: s*_um the spacing in whole micrometres,
 *   d2(v) = min over background voxels u of sum_a (s_a (v_a - u_a))^2   [um^2, to the centre of the voxel u],
 * +inf when the volume holds no background or none within max_um (d2 > max_um^2).  max_um >= 2^26 is the full
 * transform: no distance in a supported volume reaches it.
 *   zones [D,H,W] uint8: 0 not lung, 1 peel (d2 <= peel_um^2, equality included), 2 core (+inf included);
 *   zone_labels [D,H,W] uint8, optional (NULL, and then n_regions = 0): 0 not lung; a lung voxel with label r in
 *     1..n_regions -> r + n_regions * (zone - 1), so 1..n is the peel and n+1..2n the core of region r; a lung label
 *     above n_regions -> 255 (row 0 of dram_lobe_hist / dram_upproject_regions called with 2 n regions);
 *   dist_mm [D,H,W] float32, optional (NULL): float(sqrt(double(d2)) / 1000.0), 0 outside the lung, +inf with d2;
 *   workspace: dram_lung_zones_workspace(D, H, W, max_um) bytes (two work volumes of uint32 when max_um <= 65535, else
 *     of uint64; 0 for sizes the call refuses), 256-byte aligned, owned by the caller; needs no clearing.
 * Three launches (x, y, z passes); every output element and every workspace element that is read is written by them.
 * No global atomics, no ticket word, no waiting between workgroups, never synchronises, capturable; integer minima:
 * bit-identical from call to call.
 * Null labels / zones / workspace, label_dtype not 1 / 2, a size < 1, a negative stride, peel_um < 0, max_um < peel_um,
 * n_regions outside 1..7 with zone_labels (2 n <= 15) or non-zero without: DRAM_ERR_BAD_ARG.  Supported: D*H*W < 2^31,
 * 1 <= s_a <= 20000 and (n_a - 1) * s_a < 2^25 on every axis (every d2 is then below 2^53: exact in int64 and in
 * double).  Anything else: DRAM_ERR_UNSUPPORTED. */
long long dram_lung_zones_workspace(int D, int H, int W, long long max_um);
int dram_lung_zones(const void* labels, int label_dtype, long long stride_z, long long stride_y, uint8_t* zones,
                    uint8_t* zone_labels, float* dist_mm, void* workspace, int D, int H, int W, int sz_um, int sy_um,
                    int sx_um, long long peel_um, long long max_um, int n_regions, dram_stream_t stream);

/* Peel / core / fissural rind of the lobes from two exact distance transforms (csrc/edt.hip; definitions:
 * INTEGRATION.md B7).  labels, strides, spacings, d2, peel_um, max_um and the supported sizes are dram_lung_zones'.
 * With n = n_regions in 1..5 (3 n <= 15), the class of a voxel is its label for a label in 1..n, n + 1 for a lung label
 * above n and 0 for a label <= 0; a SITE is a voxel of class 1..n (a lung voxel that belongs to no region makes no
 * fissure), and per lung voxel
 *   f2(v) = min over sites u with class(u) != class(v) of sum_a (s_a (v_a - u_a))^2   [um^2, to the centre of u],
 * +inf when there is no such site or none within max_um (f2 > max_um^2); a voxel beside a foreign one has f2 = s_a^2.
 *   zones [D,H,W] uint8: 0 not lung, 1 peel (d2 <= peel_um^2: bit for bit dram_lung_zones' zone 1 -- the peel wins),
 *     3 fissural rind (not peel and f2 <= fissure_um^2, equality included), 2 core (the rest, +inf included); zones
 *     2 and 3 together are dram_lung_zones' zone 2;
 *   zone_labels [D,H,W] uint8, optional (NULL): 0 not lung; class r in 1..n -> r + n * (zone - 1), so 1..n is the peel,
 *     n+1..2n the core and 2n+1..3n the fissural rind of region r; class n + 1 -> 255 (row 0 of dram_lobe_hist /
 *     dram_upproject_regions called with 3 n regions);
 *   pleura_mm, fissure_mm_out [D,H,W] float32, optional (NULL): float(sqrt(double(d2 | f2)) / 1000.0), 0 outside the
 *     lung, +inf with the squared distance;
 *   workspace: dram_lobe_zones_workspace(D, H, W, max_um) bytes (dram_lung_zones' two work volumes, then two of 16-byte
 *     elements: the two nearest sites of distinct classes as (d2 << 3) | class; 0 for sizes the call refuses), 256-byte
 *     aligned, owned by the caller; needs no clearing.
 * Five launches (the pleural x and y passes -- dram_lung_zones' own kernels --, the x and y passes of the pairs, one z
 * pass of both with the outputs); every output element and every workspace element that is read is written by them.
 * No global atomics, no ticket word, no waiting between workgroups, never synchronises, capturable; integer minima:
 * bit-identical from call to call.
 * Null labels / zones / workspace, label_dtype not 1 / 2, a size < 1, a negative stride, peel_um < 0, fissure_um < 0,
 * max_um below either width, n_regions outside 1..5: DRAM_ERR_BAD_ARG.  Sizes and spacings outside dram_lung_zones'
 * support: DRAM_ERR_UNSUPPORTED. */
long long dram_lobe_zones_workspace(int D, int H, int W, long long max_um);
int dram_lobe_zones(const void* labels, int label_dtype, long long stride_z, long long stride_y, uint8_t* zones,
                    uint8_t* zone_labels, float* pleura_mm, float* fissure_mm_out, void* workspace, int D, int H, int W,
                    int sz_um, int sy_um, int sx_um, long long peel_um, long long fissure_um, long long max_um,
                    int n_regions, dram_stream_t stream);

/* Connected-component labelling of a 3-D key volume and the per-row cluster table of the LAA cluster analysis
 * (csrc/ccl.hip; definitions: INTEGRATION.md B8).  A key is a non-negative integer per voxel, 0 is background; two
 * voxels are connected when they are neighbours under `connectivity` (6: faces; 26: faces, edges, corners) and carry the
 * same non-zero key.  key_or_labels [D,H,W] of lab_elem 1 (uint8) or 2 (int16) bytes per element, read in place through
 * stride_z / stride_y (in elements, >= 0; x stride 1) like dram_lobe_hist's labels.
 *   image == NULL: the first argument is the key itself (a value <= 0 is background; threshold, by_lobe are ignored);
 *   image [D,H,W] int16 HU, contiguous: the first argument holds lobe labels and the key is the LAA key: label > 0 and
 *     hu < threshold (strict, as dram_lobe_hist's counts below a threshold) -> the label (by_lobe != 0) or 1.
 *   components [D,H,W] int32: the linear index (z*H + y)*W + x of the smallest voxel of the voxel's component, -1 on
 *     background (canonical: independent of scheduling);
 *   cluster_voxels [D,H,W] int32, optional (NULL): the size of the voxel's component, 0 on background;
 *   table [n_regions + 1][35] int64, a component in the row of its key (key r in 1..n_regions -> row r, a key above
 *     n_regions -> row 0): columns 0..31 the components with 2^k <= size < 2^(k+1), 32 the number of components, 33 the
 *     number of foreground voxels, 34 the largest size (0 for an empty row);
 *   work: dram_label_components_workspace(D, H, W) bytes (int32 sizes + int16 key per voxel, each rounded up to 256
 *     bytes; 0 for sizes the call refuses), 256-byte aligned, owned by the caller; needs no clearing.
 * Four launches (init, merge, compress, table) and a fifth with cluster_voxels; every output element is written.
 * Lock-free union-find: integer atomics only, no waiting between threads or workgroups, never synchronises,
 * capturable; bit-identical from call to call.
 * Null key_or_labels / components / table / work, lab_elem not 1 / 2, a size < 1, a negative stride, connectivity not
 * 6 / 26, n_regions outside 1..15, threshold outside -32768..32768: DRAM_ERR_BAD_ARG.  D*H*W >= 2^31:
 * DRAM_ERR_UNSUPPORTED. */
size_t dram_label_components_workspace(int D, int H, int W);
int dram_label_components(const void* key_or_labels, int lab_elem, long long stride_z, long long stride_y,
                          const int16_t* image, int threshold, int by_lobe, int connectivity, int n_regions,
                          int32_t* components, int32_t* cluster_voxels, int64_t* table, void* work, int D, int H, int W,
                          dram_stream_t stream);

/* Per-component table of a labelled volume: one row per connected component, behind the cluster shapes of the predict
 * report (csrc/ccl_shapes.hip; definitions: INTEGRATION.md B8).
 *   components [D,H,W] int32, contiguous, only read: what dram_label_components writes, the linear index of the
 *     component's smallest voxel, -1 on background.  A voxel v with c = components[v] counts in component c only when
 *     0 <= c < D*H*W and components[c] == c; any other voxel is background, so no int32 content indexes out of bounds.
 *   A root is a voxel with components[v] == v; roots are ranked in ascending linear index.
 *   dram_component_rank: work (dram_component_shapes_workspace(D, H, W) bytes, 256-byte aligned, owned by the caller,
 *     needs no clearing) receives the rank of every root at the root's slot of an int32 volume -- no other slot is ever
 *     read -- and count[0] the number of components.  Three launches: root count per workgroup, one ordered scan of
 *     the workgroup counts by a single workgroup, rank assignment.
 *   dram_component_shapes: after dram_component_rank on the same components and work.
 *     labels (optional, NULL) [D,H,W] of lab_elem 1 (uint8) or 2 (int16) bytes per element, read in place through
 *       stride_z / stride_y (in elements, >= 0; x stride 1) like dram_lobe_hist's labels;
 *     zones (optional, NULL) [D,H,W] uint8, contiguous: the zones output of dram_lung_zones / dram_lobe_zones;
 *     rows [capacity][18] int64, row r the component of rank r:
 *       0 root (the component's id in components), 1 class (labels at the root, raw value, sign-extended for int16; 0
 *       without labels), 2 voxels, 3..8 z0, z1, y0, y1, x0, x1 (bounding box, half-open like dram_lung_bbox),
 *       9..11 sum of z, of y, of x over the voxels, 12..14 exposed faces normal to z, to y, to x (a voxel face whose
 *       neighbour along the axis lies outside the volume or holds another value in components; two components that
 *       touch each count the shared face), 15..17 voxels with zones == 1, == 2, == 3 (any other zone value counts
 *       nowhere; 0 without zones);
 *     count [2] int64: count[0] the number of components, count[1] = min(count[0], capacity) the rows filled; rows
 *       count[1]..capacity are zeros; a component of rank >= capacity is dropped.  Every output element is written.
 *     Two launches (row init, accumulate).  One wave per x-row in chunks of 64 voxels: everything that shares a row is
 *     reduced in the wave first, the last lane of each x-run segment of equal value issues the segment's atomics, and a
 *     workgroup adds the segments of its large components in LDS before it touches their rows (never one atomic per
 *     voxel; a single giant component does not serialise the chip on one row).
 * Integer atomics only (64-bit add, min, max): independent of arrival order, bit-identical from call to call.  No
 * waiting between workgroups, no ticket word, never synchronises, capturable.  With D*H*W < 2^31 every coordinate sum
 * is below 2^31 * 2^31 = 2^62: no column can overflow int64.
 * Null components / work / count, null rows with capacity > 0, capacity < 0, a size < 1, a negative stride, lab_elem
 * not 1 / 2 with labels: DRAM_ERR_BAD_ARG.  D*H*W >= 2^31: DRAM_ERR_UNSUPPORTED (the workspace function returns 0). */
long long dram_component_shapes_workspace(int D, int H, int W);
int dram_component_rank(const int32_t* components, void* work, int64_t* count, int D, int H, int W,
                        dram_stream_t stream);
int dram_component_shapes(const int32_t* components, const void* labels, int lab_elem, long long stride_z,
                          long long stride_y, const uint8_t* zones, const void* work, int64_t* rows, long long capacity,
                          int64_t* count, int D, int H, int W, dram_stream_t stream);

/* 3-D median filter of an int16 volume (csrc/median.hip; definitions: INTEGRATION.md B9): out[z,y,x] = the median of
 * the (2rz+1)(2ry+1)(2rx+1) values of `in` in the window centred on the voxel, each radius 0 or 1 (3, 9 or 27 samples;
 * (1,1,1) is the 3x3x3 filter, (0,1,1) the in-plane 3x3 one), indices clamped to the volume (edges replicated:
 * scipy.ndimage.median_filter(mode='nearest')).  in, out [D,H,W] contiguous, out != in; `in` is only read.
 * One launch, every output element written; a min / max selection network on integers: exact, no atomics, no
 * workspace, never synchronises, capturable; bit-identical from call to call.
 * Null pointer, a size < 1, a radius other than 0 / 1, all three radii 0, out == in: DRAM_ERR_BAD_ARG.
 * D*H*W >= 2^31: DRAM_ERR_UNSUPPORTED. */
int dram_median3d(const int16_t* in, int16_t* out, int D, int H, int W, int rz, int ry, int rx, dram_stream_t stream);

/* Separable 3-D Gaussian (any symmetric tap) filter (csrc/gauss.hip; definitions: INTEGRATION.md B11):
 *   f[z,y,x] = sum_k wz[k] sum_j wy[j] sum_i wx[i] * in[z+k, y+j, x+i],  evaluated along x, then y, then z, in fp32.
 * taps (host pointer, read during the call): per axis a in (z, y, x) order the radius r_a in 0..16 and the symmetric half
 *   w[a][0..r_a] (w[a][k] weighs the two voxels at distance k); radius 0 leaves the axis untouched (w[a][0] is not read).
 * in [D,H,W] contiguous, in_type 2 (int16) or 4 (float32), only read.  out: the box [z0,z0+Do) x [y0,y0+Ho) x
 *   [x0,x0+Wo) of f as a contiguous [Do,Ho,Wo] array (the whole volume: origin 0, extents D, H, W); out_type 4
 *   (float32, from either source) or 2 (int16, from an int16 source: rintf of the same fp32 value, clamped to
 *   -32768..32767).  Every output element is written.
 * border: source indices outside the VOLUME (not the box) are clamped (DRAM_GAUSS_NEAREST: edge replication,
 *   scipy.ndimage mode='nearest') or read as 0 (DRAM_GAUSS_ZERO: conv1d(padding='same'), scipy mode='constant').
 * Along one axis the value is ((w[0] c + w[1] (l1 + r1)) + w[2] (l2 + r2)) + ..., each `+ w (l + r)` one fused
 *   multiply-add: the order of the fp32 operations of an output voxel depends on the taps alone -- not on the tile, the
 *   box, the output type or the call.  So a box equals the crop of the whole result, the int16 output equals rintf of the
 *   float32 one, and two calls agree, all bit for bit.
 * Two launches: the in-plane pass (x then y out of LDS, the border rule applied while staging) writes the planes
 *   [max(0, z0-rz), min(D, z0+Do+rz)) of the box's rows and columns as fp32 into `work`; the z pass sums 2 rz + 1 of
 *   them per output.  work: dram_gauss3d_workspace(D, z0, Do, Ho, Wo, rz) bytes, 16-byte aligned; work_bytes its size.
 *   1-D grids, no atomics, never synchronises, capturable.
 * Null pointer, a size < 1, a radius outside 0..16, a box that leaves the volume, a type pair other than (2,2), (2,4),
 *   (4,4), a border other than the two, out == in, work not 16-byte aligned or work_bytes too small: DRAM_ERR_BAD_ARG
 *   (the workspace function returns -1).  D*H*W >= 2^31: DRAM_ERR_UNSUPPORTED. */
#define DRAM_GAUSS_NEAREST 0
#define DRAM_GAUSS_ZERO 1
typedef struct DramGaussTaps {
  int32_t radius[3];
  float w[3][17];
} DramGaussTaps;
long long dram_gauss3d_workspace(int D, int z0, int Do, int Ho, int Wo, int rz);
int dram_gauss3d(const void* in, int in_type, void* out, int out_type, int D, int H, int W, int z0, int y0, int x0,
                 int Do, int Ho, int Wo, const DramGaussTaps* taps, int border, void* work, long long work_bytes,
                 dram_stream_t stream);

/* Bilateral filter of an int16 volume in exact integer fixed point, optionally confined to a label volume
 * (csrc/bilateral.hip; definitions: INTEGRATION.md B12).  tab (host pointer, read during the call, handed to the kernel
 * by value): per axis a in (z, y, x) order the radius r_a in 0..5 and the spatial table spatial[a][0..r_a] (values
 * 0..256, spatial[a][0] = 256); range_len = L in 2..1024 and range[0..L-1] (values 0..256, range[0] = 256, range[L-1] = 0).
 *   S(dz,dy,dx) = (spatial[0][|dz|] * spatial[1][|dy|] * spatial[2][|dx|] + 2^15) >> 16; a tap with S = 0 does not exist.
 *   Per centre c, over the taps i inside the volume and (with `within`) at voxels where within != 0:
 *     d_i = v_i - v_c,  w_i = S_i * range[min(|d_i|, L-1)],  num = sum w_i d_i (64-bit),  den = sum w_i;
 *     out_c = v_c + floor((2 num + den) / (2 den));  with `within` and within_c == 0: out_c = v_c.
 * in, out [D,H,W] contiguous, any 2-byte alignment, out != in; `in` is only read.  within: NULL, or [D,H,W] of
 * within_type 1 (uint8) or 2 (int16), read in place through within_sz / within_sy (in elements, >= 0; x stride 1).
 * One launch, every output element written; integers only: exact, no atomics, no workspace, never synchronises,
 * capturable; bit-identical from call to call.
 * Null in / out / tab, out == in, a size < 1, a radius outside 0..5, a table entry outside 0..256, spatial[a][0] != 256,
 * L outside 2..1024, range[0] != 256, range[L-1] != 0, within with a type other than 1 / 2 or a negative stride: DRAM_ERR_BAD_ARG.
 * D*H*W >= 2^31: DRAM_ERR_UNSUPPORTED. */
#define DRAM_BILAT_MAX_RADIUS 5
#define DRAM_BILAT_RANGE_LEN 1024
typedef struct DramBilateral {
  int32_t radius[3];
  int32_t spatial[3][6];
  int32_t range_len;
  int32_t range[1024];
} DramBilateral;
int dram_bilateral3d(const int16_t* in, int16_t* out, const void* within, int within_type, long long within_sz,
                     long long within_sy, int D, int H, int W, const DramBilateral* tab, dram_stream_t stream);

/* Local low-attenuation fraction: an exact 3-D box count over the lung (csrc/boxfrac.hip; definitions: INTEGRATION.md
 * B13).  image [D,H,W] int16 HU, contiguous; labels [D,H,W] of label_dtype 1 (uint8) or 2 (int16), read in place through
 * stride_z / stride_y (in elements, >= 0; x stride 1) like dram_lobe_hist's; lung = label > 0 (signed for int16).
 * Per voxel v, with the box B(v) = [z-rz, z+rz] x [y-ry, y+ry] x [x-rx, x+rx] clipped to the volume (voxels outside the
 * volume count nowhere), each radius in 0..16:
 *   den(v) = #{u in B(v): label(u) > 0},   num(v) = #{u in B(v): label(u) > 0 and image(u) < threshold}  (strict).
 *   counts [D,H,W] int32 (or NULL) = num << 16 | den: (2*16+1)^3 = 35 937 < 65 536, both fit their half (the word is
 *     unsigned in meaning: num = (c >> 16) & 0xffff, which exceeds 32 767 in the largest boxes).
 *   map [D,H,W] int16: where label(v) > 0 (then den >= 1) q = (2000 num + den) / (2 den), the fraction num / den in per
 *     mille rounded half up, 0..1000; where label(v) <= 0: -1.
 *   u8 (or NULL): (q * 255) / 1000, 0 where q = -1, one byte per voxel written at u8[z * u8_stride_z + y * u8_stride_y +
 *     x]: u8 points at the first voxel of a [D,H,W] window of a larger volume (strides in bytes, >= 0, rows and planes
 *     of the window disjoint); nothing outside the window is touched.
 * Every element of counts / map / the u8 window is written; the inputs are only read.  Two launches: the in-plane pass
 * writes the packed (2ry+1) x (2rx+1) counts of every plane into `work` (dram_boxfrac3d_workspace(D, H, W) = 4 D H W
 * bytes, 16-byte aligned; work_bytes its size), the z pass walks z with a running sum.  Integers only: exact; 1-D grids,
 * no atomics, never synchronises, capturable; bit-identical from call to call.
 * Null image / labels / map / work, label_dtype not 1 / 2, a size < 1, a negative stride, a negative radius, a threshold
 * outside -32768..32768, outputs that alias an input, the workspace or each other, a u8 window that overlaps itself, a
 * misaligned pointer, work_bytes too small: DRAM_ERR_BAD_ARG.  A radius above 16, D*H*W >= 2^31: DRAM_ERR_UNSUPPORTED
 * (the workspace function returns -1). */
#define DRAM_BOXFRAC_MAX_RADIUS 16
long long dram_boxfrac3d_workspace(int D, int H, int W);
int dram_boxfrac3d(const int16_t* image, const void* labels, int label_dtype, long long stride_z, long long stride_y,
                   int threshold, int rz, int ry, int rx, int32_t* counts, int16_t* map, uint8_t* u8,
                   long long u8_stride_z, long long u8_stride_y, void* work, long long work_bytes, int D, int H, int W,
                   dram_stream_t stream);

/* Train-time augmentations (models.py:66-74) with GIVEN parameters, fused into one gather pass:
 * GaussianAddictive (intensity_transforms.py:145-177; noise [D,H,W] supplied by the caller, minmax[2] = volume
 * {min, max} on the device, e.g. folded from dram_minmax partials [nblk][2]), BoxMaskOut (:180-237), Flip
 * (spatial_transforms.py:100-131), CropAndResize (:133-197, functional.py:68-94: affine_grid + grid_sample;
 * image trilinear / align_corners=True, mask nearest / align_corners=False, zero padding).
 * flags: bit 0 noise, 1 boxes, 2 flip, 3 crop-resize; boxes[b] = {z0,z1,y0,y1,x0,x1} half-open, pre-flip grid;
 * flip_axes: bit 0 z, 1 y, 2 x; box_lo/box_hi: bounding box / size per axis (z, y, x).  x != out. */
typedef struct DramAugment {
  int32_t flags;
  int32_t n_boxes;
  int32_t boxes[10][6];
  int32_t flip_axes;
  float sigma;
  float box_lo[3];
  float box_hi[3];
} DramAugment;
int dram_minmax_nblk(long long n);
int dram_minmax(const float* x, float* partial, long long n, dram_stream_t stream);
int dram_augment_image(const float* x, const float* noise, const float* minmax, float* out, int D, int H, int W,
                       const DramAugment* aug, dram_stream_t stream);
int dram_augment_mask(const float* mask, float* out, int D, int H, int W, const DramAugment* aug,
                      dram_stream_t stream);

/* out[i] = a[i] + b[i]  (gradient accumulation where two consumers meet) */
int dram_add(const float* a, const float* b, float* out, long long n, dram_stream_t stream);

/* ------------------------------------------------------------------------- */
/* bf16 STORAGE path -- the reference's `--precision bf16` (train.py:46: Lightning wraps the step in
 * torch.autocast(bfloat16); BASELINE configs[2], [4]).  Activation-sized tensors (x, y, z, dy, dx, residuals,
 * concat buffers) are bf16 NDHWC (`void*`, 2 bytes per element, same offsets); everything else keeps the types of
 * the fp32 entry points: BatchNorm statistics / scale / shift, biases, the dense head outputs and every weight
 * GRADIENT are fp32, statistic folds are double.  Arithmetic: products of bf16 operands accumulated in fp32
 * (v_mfma_f32_32x32x16_bf16), element-wise math in fp32, one rounding (to nearest even) on store.
 * The *_bf16 element-wise entry points take exactly the arguments of their fp32 namesakes. */
long long dram_pack_conv_weight_bf16_tiles(int Cout, int Cin, int taps);
int dram_pack_conv_weight_bf16_multi(const DramPackRef* table, const DramChunkRef* chunks, int nchunks, void* flat,
                                     double total_elems, dram_stream_t stream);
int dram_cast_f32_to_bf16(const float* src, void* dst, long long n, dram_stream_t stream);
int dram_cast_bf16_to_f32(const void* src, float* dst, long long n, dram_stream_t stream);
/* The stride-2 3x3x3 convolution (k 3, stride 2, pad 1, even extents, Cin % 8 == 0) as a stride-1 convolution of the
 * space-to-depth tensor: x8[b][z][y][x][p][c] = x[b][2z + pz][2y + py][2x + px][c], p = 4 pz + 2 py + px (8 Cin
 * channels at half the extents), with the embedded weights w3 [Cout][8 Cin][3][3][3] (dram_s2_embed_weight: 27 of
 * 216 (parity, offset) slots per (co, ci) carry a tap, the rest are zero).  dram_d2s_bf16 is the inverse permutation
 * with the data gradient's optional `+= add * (gate > 0)`; dram_s2_extract_wgrad picks the 27 taps out of the
 * gradient of w3.  The host runs forward / data gradient / weight gradient of the derived stride-1 geometry on the
 * bf16 convolution entry points below. */
int dram_s2d_bf16(const void* x, void* x8, int B, int D, int H, int W, int C, dram_stream_t stream);
int dram_d2s_bf16(const void* dx8, const void* add, const void* gate, void* dx, int B, int D, int H, int W, int C,
                  dram_stream_t stream);
int dram_s2_embed_weight(const float* w, float* w3, int Cout, int Cin, dram_stream_t stream);
int dram_s2_extract_wgrad(const float* dw3, float* dw, int Cout, int Cin, dram_stream_t stream);
/* 1 when the bf16 direct kernels take this geometry: 3x3x3, stride 1, pad == dilation, Cin % 32 == Cout % 32 == 0
 * (everything else is run by the host on the fp32 kernels around cast passes) */
int dram_conv_bf16_supported(const DramConvDesc* d);
int dram_conv_bf16_num_stat_rows(const DramConvDesc* d);
/* w [Cout][Cin][k^3] fp32 -> wf [taps][Cout][Cin] bf16 (forward operand), wb [taps][Cin][Cout] bf16 with the taps
 * flipped (data-gradient operand); either may be NULL */
int dram_pack_conv_weight_bf16(const float* w, void* wf, void* wb, int Cout, int Cin, int taps, dram_stream_t stream);
/* nn.Conv3d forward (med3d.py:11,121,123,...) / its data gradient / its weight gradient on bf16 tensors.
 * stats_partial [dram_conv_bf16_num_stat_rows][2][Cout] fp32: per-tile sums of y and y^2 (of the ROUNDED values the
 * BatchNorm pass reads back), or NULL.  bwd_data: dx = conv_transpose(dy) (+ add * (gate > 0), both bf16, optional). */
int dram_conv3d_fwd_bf16(const void* x, const void* wf, const float* bias, void* y, float* stats_partial,
                         const DramConvDesc* d, dram_stream_t stream);
int dram_conv3d_bwd_data_bf16(const void* dy, const void* wb, void* dx, const void* add, const void* gate,
                              const DramConvDesc* d, dram_stream_t stream);
size_t dram_conv3d_bwd_weight_bf16_workspace(const DramConvDesc* d);
int dram_conv3d_bwd_weight_bf16(const void* x, const void* dy, float* dw, const DramConvDesc* d, void* workspace,
                                size_t workspace_bytes, dram_stream_t stream);
int dram_stem_fwd_bf16(const float* x, const float* w, void* y, float* stats_partial, int B, int D, int H, int W,
                       dram_stream_t stream);
int dram_stem_bwd_weight_bf16(const float* x, const void* dy, float* dw, int B, int D, int H, int W, void* workspace,
                              size_t workspace_bytes, dram_stream_t stream);
/* dy in bf16, widened on load; fp32 MFMA arithmetic, dx fp32 (same workspace) */
int dram_stem_bwd_data_bf16(const void* dy, const float* w, float* dx, int B, int D, int H, int W, void* workspace,
                            size_t workspace_bytes, dram_stream_t stream);
/* the same two on the bf16 matrix cores (input rounded to bf16 on its way into LDS, weights rounded per launch;
 * same tile geometry, statistic rows and workspace as the fp32-MFMA forms above) */
int dram_stem_fwd_bf16mm(const float* x, const float* w, void* y, float* stats_partial, int B, int D, int H, int W,
                         dram_stream_t stream);
int dram_stem_bwd_weight_bf16mm(const float* x, const void* dy, float* dw, int B, int D, int H, int W, void* workspace,
                                size_t workspace_bytes, dram_stream_t stream);
/* workgroups dram_stem_fwd_bf16mm launches for ntile = dram_stem_num_tiles(...) tiles (persistent: each walks
 * ceil(ntile / blocks) tiles at most) */
int dram_stem_fwd_blocks(int ntile);
int dram_bn_apply_bf16(const void* y, const float* scale, const float* shift, const void* residual, int Dr, int Hr,
                       int Wr, int Cr, int rs, void* z, int B, int D, int H, int W, int C, int relu,
                       dram_stream_t stream);
int dram_bn_bwd_reduce_bf16(const void* dz, const void* z, const void* y, const float* mean, const float* invstd,
                            const float* scale, const float* shift, float* partial, long long rows, int C, int relu,
                            dram_stream_t stream);
int dram_bn_bwd_apply_bf16(const void* dz, const void* z, const void* y, const float* mean, const float* invstd,
                           const float* gamma, const float* scale, const float* shift, const double* sums, double count,
                           const double* count_dev, void* dy, float* colsum_partial, long long rows, int C, int relu,
                           dram_stream_t stream);
int dram_bn_bwd_apply_eval_bf16(const void* dz, const void* z, const void* y, const float* scale, const float* shift,
                                void* dy, float* colsum_partial, long long rows, int C, int relu, dram_stream_t stream);
int dram_colsum_bf16(const void* a, float* partial, long long rows, int C, dram_stream_t stream);
int dram_maxpool_fwd_bf16(const void* x, void* y, uint8_t* argmax, int B, int D, int H, int W, int C,
                          dram_stream_t stream);
int dram_bn_maxpool_fwd_bf16(const void* y, const float* scale, const float* shift, void* z, void* pooled, uint8_t* argmax,
                             int B, int D, int H, int W, int C, dram_stream_t stream);
int dram_maxpool_bwd_bf16(const void* dy, const uint8_t* argmax, const void* add, int add_stride, void* dx, int B, int D,
                          int H, int W, int C, dram_stream_t stream);
int dram_upcat_fwd_bf16(const void* src, const void* skip, void* cat, int B, int Ds, int Hs, int Ws, int Cu, int Dk,
                        int Hk, int Wk, int Ck, dram_stream_t stream);
int dram_upcat_bwd_bf16(const void* dcat, void* dsrc, void* dskip, int B, int Ds, int Hs, int Ws, int Cu, int Dk, int Hk,
                        int Wk, int Ck, dram_stream_t stream);
int dram_head_fwd_bf16(const void* x, const float* w, const float* bias, const float* lungs, int Dl, int Hl, int Wl,
                       float* dense, float* partial, int B, int D, int H, int W, int NO, int sigmoid,
                       dram_stream_t stream);
int dram_head_bwd_bf16(const void* x, const float* w, const float* dense, const float* gdense, const float* gpool,
                       const float* lungs, int Dl, int Hl, int Wl, void* dx, float* wpartial, int B, int D, int H, int W,
                       int NO, int sigmoid, dram_stream_t stream);
int dram_cam_point_bf16(const void* x, const float* w, const float* bias, const float* gdense, const float* gpool,
                        const float* lungs, int Dl, int Hl, int Wl, float* out, int B, int D, int H, int W, int NO,
                        int sigmoid, int method, int relu, dram_stream_t stream);
int dram_cam_sum_bf16(const void* x, const float* w, const float* bias, const float* gdense, const float* gpool,
                      const float* lungs, int Dl, int Hl, int Wl, float* partial, int B, int D, int H, int W, int NO,
                      int sigmoid, dram_stream_t stream);
int dram_cam_combine_bf16(const void* x, const float* w, const double* sums, float* out, int B, int D, int H, int W,
                          int NO, int relu, dram_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRAM_HIP_H */
