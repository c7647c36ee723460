/*
 * include/slak_hip.h -- C ABI of libslak_hip.so, the MI355X (gfx950) drop-in for the two native
 * boundaries of VITA-Group/SLaK's training hot path.  Plain pointers and sizes only: no torch
 * types, no C++ in the signatures.  All pointers are DEVICE pointers unless a name ends in _host.
 * Every entry point returns a slak_status_t (0 == ok) and never calls exit()
 * (the reference exits the process on failure: forward_fp32.cu:173-192).
 * Work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream).  The
 * reference launches on the null stream (cutlass/include/cutlass/convolution/device/convolution.h:243);
 * callers here pass PyTorch's current stream.
 *
 * Boundary 1 -- depthwise conv, replaces pybind module `_depthwise_conv2d_implicit_gemm_C`
 *   (cutlass/examples/19_large_depthwise_conv2d_torch_extension/frontend.h:3-10, frontend.cpp:3-16):
 *     forward_fp32/fp16(x, w)            -> slak_dwconv2d_forward
 *     backward_data_fp32/fp16(dy, w)     -> slak_dwconv2d_backward_data
 *     backward_filter_fp32/fp16(dy,x,w)  -> slak_dwconv2d_backward_filter
 *   Semantics fixed by the reference kernels (forward_fp32.cu:135-144, :227, :235): NCHW contiguous,
 *   weight (C,1,kh,kw), stride 1, dilation 1, padding (kh/2, kw/2), groups == C, cross-correlation,
 *   output shape == input shape, so kh and kw must be odd (the reference silently mis-sizes even
 *   kernels; here that is SLAK_ERR_INVALID_ARG).  bf16 is added (the reference raises TypeError:
 *   depthwise_conv2d_implicit_gemm.py:63).  The filter gradient is always fp32
 *   (backward_filter_fp16.cu:187).
 *
 * Boundary 2 -- dynamic-sparsity step, replaces the per-tensor torch loops of
 *   sparse_core.Masking.apply_mask (sparse_core.py:316-333), .truncate_weights (:335-357),
 *   funcs.magnitude_prune (funcs.py:107-114) and funcs.gradient_growth (funcs.py:196-205).
 *   Masks stay fp32 0/1 tensors owned by the caller (Masking.masks, read by model_sema.py:83-89).
 *   Ties at the cut are broken by LOWEST FLAT INDEX (== torch.sort(stable=True)); the reference's
 *   unstable torch.sort is arbitrary there.
 */
#ifndef SLAK_HIP_H
#define SLAK_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SLAK_OK = 0,
    SLAK_ERR_INVALID_ARG = 1,   /* null pointer, non-positive dim, even kernel, bad dtype enum */
    SLAK_ERR_UNSUPPORTED = 2,   /* dtype combination / size outside what the kernels cover     */
    SLAK_ERR_WORKSPACE = 3,     /* workspace missing or smaller than *_workspace_bytes()       */
    SLAK_ERR_LAUNCH = 4,        /* HIP launch/runtime error; see slak_last_hip_error()         */
    SLAK_ERR_NO_DEVICE = 5
} slak_status_t;

typedef enum { SLAK_F32 = 0, SLAK_F16 = 1, SLAK_BF16 = 2, SLAK_I64 = 3 /* slak_ema_update only */ } slak_dtype_t;

/* conv algorithm selector: AUTO picks per dtype/shape; DIRECT = fp32-exact VALU kernels (any dtype);
 * MFMA = banded-Toeplitz matrix-core kernels (f16/bf16 inputs; fp32 inputs through the two-term split below).  AUTO runs 16-bit tensors on
 * the matrix cores for every kernel with a 5-tap side and, with the rows taken five at a time, for every odd kh <= kw <= 63 kernel on maps
 * up to 64 wide (the square 3 .. 31 kernels of test_correctness.py:16-20, the 51 x 51 of --Decom False); everything else (maps beyond 128,
 * kernels with more rows than columns and no 5-tap side, fp32 unless allowed below) runs the exact VALU kernels. */
typedef enum { SLAK_ALGO_AUTO = 0, SLAK_ALGO_DIRECT = 1, SLAK_ALGO_MFMA = 2 } slak_algo_t;

const char* slak_status_string(int status);
const char* slak_last_hip_error(void);      /* text of the last HIP error seen by this library */
/* ABI version: bumped whenever an entry point's argument list or meaning changes (round 5: 5).  A host module compiled against this header
 * (slak_amd/pybind, *.cpp) records the value it saw and refuses to load on a library that reports another one: a stale module would call raw-pointer
 * entry points with a changed argument list -- silent corruption, not an error. */
#define SLAK_ABI_VERSION 10
int slak_version(void);                     /* == SLAK_ABI_VERSION of the header the library was built from */
int slak_device_info(int* cu_count, int* lds_bytes_per_cu, char* arch_name, size_t arch_name_len);
int slak_set_conv_algo(int algo);           /* process-wide override of the AUTO choice */
/* fp32 tensors on the bf16 matrix cores: x = bf16(x) + bf16(x - bf16(x)) (and the same for the filter / dy), three MFMAs per product,
 * fp32 accumulation: 16 significand bits per operand, ~2e-5 of sum|x||w| per output -- 50x inside the 1e-3 the reference's own test allows
 * (test_correctness.py), not bit-compatible with the exact path.  OFF by default (the fp32 entry points then run the exact VALU kernels), the
 * way torch.backends.cudnn.allow_tf32 gates TF32; SLAK_FP32_MFMA=1 in the environment sets the initial value.  Covers kernels with a 5-tap
 * side on maps up to 64 along the long axis (the SLaK stages at 224 px); everything else stays exact. */
int slak_set_fp32_matrix_cores(int allow);
int slak_get_fp32_matrix_cores(void);            /* the process-wide switch (never the per-thread override: safe for save / restore) */
int slak_get_fp32_matrix_cores_effective(void);  /* what a call on THIS thread would do: the per-thread override if one is set, else the switch */
/* Per-thread override for the calls that follow on this thread: -1 follow the process-wide setting, 0 exact, 1 matrix cores; the mode it
 * replaces is stored to *previous (may be NULL).  Nothing in the library or the Python op module sets it by default: the op module does so
 * only where the user opted in (DepthWiseConv2dImplicitGEMM.fp32_matrix_cores_under_autocast = True / SLAK_FP32_AUTOCAST_SPLIT=1: fp32
 * activations that reach the op under torch.autocast -- the reference's default AMP flow, depthwise_conv2d_implicit_gemm.py:16). */
int slak_set_fp32_matrix_cores_thread(int mode, int* previous);

/* ---------------------------------------------------------------- boundary 1: depthwise conv */

/* Bytes of scratch each op needs for these dims (0 is possible).  `op`: 0 fwd, 1 bwd-data, 2 bwd-filter. */
size_t slak_dwconv2d_workspace_bytes(int op, int N, int C, int H, int W, int kh, int kw, int dtype);

/* y[n,c,p,q] = sum_{r,s} x[n,c,p-kh/2+r,q-kw/2+s] * w[c,0,r,s]      (forward_fp32.cu:199-263) */
int slak_dwconv2d_forward(const void* x, int x_dtype, const void* w, int w_dtype, void* y, int y_dtype,
                          int N, int C, int H, int W, int kh, int kw,
                          void* workspace, size_t workspace_bytes, void* stream);

/* dx[n,c,h,w] = sum_{r,s} dy[n,c,h+kh/2-r,w+kw/2-s] * w[c,0,r,s]    (backward_data_fp32.cu:199-263) */
int slak_dwconv2d_backward_data(const void* dy, int dy_dtype, const void* w, int w_dtype, void* dx, int dx_dtype,
                                int N, int C, int H, int W, int kh, int kw,
                                void* workspace, size_t workspace_bytes, void* stream);

/* dx += the data gradient (same arguments as slak_dwconv2d_backward_data; dx is read and written).  The three branches of a SLaK
 * block (models/SLaK.py:92-100) share their input, so autograd adds the three branch gradients with two elementwise passes
 * (read 2 + write 1 each); accumulating inside the second and third branch's kernel costs one extra read each instead.  The sum is
 * rounded to the tensor dtype after every accumulation, exactly as a bf16 / fp16 tensor add does.  Kernels that cannot accumulate
 * return SLAK_ERR_UNSUPPORTED (nothing has been launched): compute into a temporary and add. */
int slak_dwconv2d_backward_data_accumulate(const void* dy, int dy_dtype, const void* w, int w_dtype, void* dx, int dx_dtype,
                                           int N, int C, int H, int W, int kh, int kw,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* dw[c,0,r,s] = sum_{n,p,q} dy[n,c,p,q] * x[n,c,p-kh/2+r,q-kw/2+s], fp32 out, deterministic
 * (no atomics; the reference atomically adds: dwconv2d_direct_epilogue_simt.h:180)
 *                                                                   (backward_filter_fp32.cu:199-263) */
int slak_dwconv2d_backward_filter(const void* dy, int dy_dtype, const void* x, int x_dtype, float* dw,
                                  int N, int C, int H, int W, int kh, int kw,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- boundary 2: mask step       */

typedef struct {
    float* weight;        /* fp32 parameter, updated in place                                   */
    float* mask;          /* fp32 0/1 mask, same numel                                          */
    const float* grad;    /* fp32 gradient (only read by slak_mask_prune_and_grow; may be NULL) */
    float* momentum;      /* optional SGD momentum buffer masked too (sparse_core.py:327-328)   */
    long long numel;
} slak_mask_segment_t;

typedef struct slak_mask_plan slak_mask_plan_t;   /* opaque: device tables + select scratch      */

/* Build a plan over `nseg` masked tensors (descriptor array in HOST memory, device pointers inside). */
int slak_mask_plan_create(const slak_mask_segment_t* segs_host, int nseg, slak_mask_plan_t** plan_out);
/* Re-point grad / momentum (they are re-allocated by optimizers); arrays of nseg device pointers, in HOST memory. */
int slak_mask_plan_set_grads(slak_mask_plan_t* plan, const void* const* grads_host, void* stream);
int slak_mask_plan_set_momentum(slak_mask_plan_t* plan, void* const* momentum_host, void* stream);
int slak_mask_plan_destroy(slak_mask_plan_t* plan);

/* w *= mask (and momentum *= mask) for every segment, one launch            (sparse_core.py:316-333) */
int slak_mask_apply(slak_mask_plan_t* plan, void* stream);

/* One truncate_weights(): per segment, magnitude-prune then gradient-regrow then apply, all on device.
 * `prune_rate` is the host scheduler's fp64 value; k = ceil(zeros + ceil(rate*nonzeros)) is evaluated
 * on device in fp64 exactly as Python does (funcs.py:107-109).       (sparse_core.py:335-357)       */
int slak_mask_prune_and_grow(slak_mask_plan_t* plan, double prune_rate, void* stream);

/* The prune half alone (magnitude prune, sparse_core.py:337-347): masks hold the pruned masks afterwards, weights are untouched, the
 * statistics (nonzeros before, zeros before, removed, nonzeros after prune) are ready for slak_mask_read_stats.  For the growth
 * modes whose random numbers come from the host generator (funcs.random_growth, funcs.py:170-175: `torch.rand(shape).cuda() < p`):
 * the caller grows on the pruned masks and finishes with slak_mask_apply. */
int slak_mask_prune(slak_mask_plan_t* plan, double prune_rate, void* stream);

/* Copy per-segment statistics of the last prune_and_grow to the host (synchronises `stream`):
 * out_host[4*i + {0,1,2,3}] = nonzeros before, zeros before, removed by prune, nonzeros after. */
int slak_mask_read_stats(slak_mask_plan_t* plan, double* out_host, void* stream);

/* 64-bit order-independent checksum of all masks (for cross-rank agreement checks); synchronises. */
int slak_mask_checksum(slak_mask_plan_t* plan, unsigned long long* out_host, void* stream);

/* ---- next row: the three branches of one decomposed large-kernel block in ONE launch ----------------------------
 * ReparamLargeKernelConv.forward runs LoRA1 (K x 5), LoRA2 (5 x K) and small_conv (5 x 5) on the same input (models/SLaK.py:82-100).
 * forward: x is read once for the three outputs; backward_data: the three partial input gradients are summed inside the kernel
 * (autograd would add them with two elementwise passes).  16-bit tensors (dtype = SLAK_BF16 / SLAK_F16), fp32 filters
 * (C,1,K,5), (C,1,5,K), (C,1,5,5).  slak_dwconv2d_tri_supported_op(.., op) -- op 0 forward, 1 backward_data -- returns 1 where a
 * one-launch kernel exists AND measured faster than the per-branch entry points on MI355X: planes up to 16 x 16 (wave-independent
 * kernels; the three gradient contributions are summed in the fp32 accumulator and rounded once) and planes of one MFMA tile (17..32:
 * four-wave-team kernels, same rounding) for both ops; planes of 2 x 2 tiles (33..64, H % 4 == 0, W % 8 == 0) for the data gradient only
 * (two rounded partial planes -- vertical [+ small], horizontal [+ small] -- added like a tensor add: one rounding fewer than autograd's
 * two adds).  0: the caller issues the three slak_dwconv2d_* calls.  slak_dwconv2d_tri_supported = both ops.  The launches themselves
 * run wherever a kernel exists (SLAK_ERR_UNSUPPORTED otherwise).
 * slak_debug_last_kernel(): name of the kernel family the calling thread's last conv entry point launched (dispatch tests). */
int slak_dwconv2d_tri_supported_op(int dtype, int N, int C, int H, int W, int K, int op);
const char* slak_debug_last_kernel(void);
/* An empty kernel `slak::marker_kernel` with grid = id + 1 workgroups on `stream` (0 <= id <= 65535): a cut mark in a kernel trace
 * (bench.py --markers brackets its K timed steps with ids 1 and 2; tools/step_breakdown.py reads them). */
int slak_debug_marker(int id, void* stream);
int slak_dwconv2d_tri_supported(int dtype, int N, int C, int H, int W, int K);
int slak_dwconv2d_tri_forward(const void* x, const float* w_v, const float* w_h, const float* w_s, void* y_v, void* y_h, void* y_s,
                              int dtype, int N, int C, int H, int W, int K, void* stream);
/* slak_dwconv2d_forward that also leaves the batch statistics of the BatchNorm behind the conv (models/SLaK.py:38-47: conv -> bn):
 * stats[rows][C][2] = partial (sum y, sum y^2) of the stored outputs per (row, channel); *stats_rows = rows written; the caller provides room
 * for 4 N rows.  Only the LDS-DMA ring kernel (56 x 56 / 28 x 28 class, bf16) gathers them: SLAK_ERR_UNSUPPORTED otherwise. */
int slak_dwconv2d_forward_stats(const void* x, int x_dtype, const void* w, int w_dtype, void* y, int y_dtype, float* stats, int stats_capacity_rows,
                                int* stats_rows, int N, int C, int H, int W, int kh, int kw, void* stream);
/* slak_dwconv2d_tri_forward that also leaves the batch statistics of the three branch BatchNorms (models/SLaK.py:92-95: conv -> bn per
 * branch): stats[rows][C][6] = partial sums (sum y_v, sum y_v^2, sum y_h, sum y_h^2, sum y_s, sum y_s^2) of the STORED (rounded) outputs per
 * (row, channel); rows = slak_dwconv2d_tri_stats_rows(...) (0: no such kernel for the shape; bf16 only; maps beyond 64, where
 * slak_dwconv2d_tri_forward runs the wide kernel, have none: 0 rows and SLAK_ERR_UNSUPPORTED).  slak_bn3_forward_local takes them in place of
 * its own pass over the three tensors. */
int slak_dwconv2d_tri_stats_rows(int dtype, int N, int C, int H, int W, int K);
int slak_dwconv2d_tri_forward_stats(const void* x, const float* w_v, const float* w_h, const float* w_s, void* y_v, void* y_h, void* y_s,
                                    float* stats, int dtype, int N, int C, int H, int W, int K, void* stream);
int slak_dwconv2d_tri_backward_data(const void* dy_v, const void* dy_h, const void* dy_s, const float* w_v, const float* w_h,
                                    const float* w_s, void* dx, int dtype, int N, int C, int H, int W, int K, void* stream);

/* The three weight gradients of a block in one launch (x fetched from HBM once for the three correlations): dw_v (C,1,K,5), dw_h (C,1,5,K),
 * dw_s (C,1,5,5), fp32 (backward_filter_fp16.cu:187), bitwise reproducible (fixed-order reductions, no atomics on data).  Covered: H <= 14
 * and W even 8..14 or 4..7 (the 14x14 and 7x7 stages); round 4: planes of one MFMA tile (15 <= H <= 32, W even 16..32: the 28x28 stage,
 * C <= 4 x CUs) and planes of 2 x 2 tiles (32 < H, W <= 64, W % 8 == 0: the 56x56 stage).  slak_dwconv2d_tri_filter_workspace_bytes
 * returns 0 for anything else and the call SLAK_ERR_UNSUPPORTED (slak_dwconv2d_pair_backward_filter + one, or three,
 * slak_dwconv2d_backward_filter calls instead; a caller must be ready for SLAK_ERR_UNSUPPORTED from the call even after a non-zero
 * workspace answer: the device's CU count, unknown to the query, decides the work split). */
size_t slak_dwconv2d_tri_filter_workspace_bytes(int dtype, int N, int C, int H, int W, int K);
int slak_dwconv2d_tri_backward_filter(const void* dy_v, const void* dy_h, const void* dy_s, const void* x, float* dw_v, float* dw_h,
                                      float* dw_s, int dtype, int N, int C, int H, int W, int K,
                                      void* workspace, size_t workspace_bytes, void* stream);

/* The whole backward of a block's three branch convs in ONE launch -- dx (what slak_dwconv2d_tri_backward_data writes) and dw_v, dw_h, dw_s
 * (what slak_dwconv2d_tri_backward_filter writes), bit for bit -- where the planes are small enough that a launch's fixed cost and the second
 * staging of the three dY tensors dominate (round 4: H <= 14, W even 8..14 -- the 14 x 14 stage: backward_data_fp16.cu:181-243 and
 * backward_filter_fp16.cu:181-243 per branch in the reference, six launches).  slak_dwconv2d_tri_backward_supported returns 1 where the
 * launch exists; workspace: slak_dwconv2d_tri_filter_workspace_bytes.  Anything else: SLAK_ERR_UNSUPPORTED (the two calls above). */
int slak_dwconv2d_tri_backward_supported(int dtype, int N, int C, int H, int W, int K);
int slak_dwconv2d_tri_backward(const void* dy_v, const void* dy_h, const void* dy_s, const void* x, const float* w_v, const float* w_h,
                               const float* w_s, void* dx, float* dw_v, float* dw_h, float* dw_s, int dtype, int N, int C, int H, int W, int K,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The K x 5 and the 5 x 5 weight gradient of a block in one launch, for the planes the three-branch launch does not cover (round 2:
 * 15 <= H <= 32, W even 16..32 -- the 28 x 28 stage): the 5 x 5 correlation is the K x 5 one with its own dY, so x is fetched and
 * column-shifted once for both.  dw_v (C,1,K,5), dw_s (C,1,5,5), fp32, bitwise reproducible.  slak_dwconv2d_pair_filter_workspace_bytes
 * returns 0 and the call SLAK_ERR_UNSUPPORTED elsewhere (two slak_dwconv2d_backward_filter calls instead). */
size_t slak_dwconv2d_pair_filter_workspace_bytes(int dtype, int N, int C, int H, int W, int K);
int slak_dwconv2d_pair_backward_filter(const void* dy_v, const void* dy_s, const void* x, float* dw_v, float* dw_s,
                                       int dtype, int N, int C, int H, int W, int K, void* workspace, size_t workspace_bytes, void* stream);

/* Which entry point runs each step of a block's three branch convs (forward, summed data gradient, the three weight gradients) on an (N,C,H,W) input
 * with a K x 5, a 5 x K and a 5 x 5 filter.  The ONE place where the ladder is written: every field takes the first rung, in the order listed, that
 * the queries above support and `allow` admits.  Pure host code, built from slak_dwconv2d_tri_supported_op, _tri_stats_rows,
 * _tri_filter_workspace_bytes, _pair_filter_workspace_bytes and _tri_backward_supported and nothing else (capi.hip decides which KERNEL exists; this
 * decides which ENTRY POINT a block calls).  Both callers (slak_amd/block_ops.py, slak_amd/pybind/block_runner.cpp) switch on the answer.
 *   fwd    TRI_STATS    slak_dwconv2d_tri_forward_stats: FUSED, supported_op(.., 0), STATS and stats_rows > 0
 *          TRI          slak_dwconv2d_tri_forward: FUSED and supported_op(.., 0)
 *          BRANCH_STATS three slak_dwconv2d_forward_stats (each falls back to slak_dwconv2d_forward where no kernel gathers sums): STATS
 *          BRANCH       three slak_dwconv2d_forward
 *   stats_rows  rows of the [rows][C][6] array of TRI_STATS, else 0
 *   dgrad  ONE          slak_dwconv2d_tri_backward (the weight gradients are in the same launch: wgrad is ONE too) -- FUSED, WGRAD and BACKWARD,
 *                       tri filter workspace bytes > 0 and slak_dwconv2d_tri_backward_supported
 *          TRI          slak_dwconv2d_tri_backward_data: FUSED and supported_op(.., 1)
 *          BRANCH_ACC   slak_dwconv2d_backward_data, then two slak_dwconv2d_backward_data_accumulate: DGRAD_ACC
 *          BRANCH_ADD   three slak_dwconv2d_backward_data and two tensor adds
 *   wgrad  ONE          (with dgrad)
 *          TRI          slak_dwconv2d_tri_backward_filter: WGRAD and tri filter workspace bytes > 0
 *          PAIR         slak_dwconv2d_pair_backward_filter + slak_dwconv2d_backward_filter for 5 x K: WGRAD and pair filter workspace bytes > 0
 *          BRANCH       three slak_dwconv2d_backward_filter
 *   ws_wgrad    workspace bytes of the chosen ONE / TRI / PAIR launch, else 0
 * The plan describes a backward that needs all four gradients; a call that needs fewer steps down on its own (ONE: dx and the three dw; TRI wgrad: the
 * three dw; PAIR: dw_v and dw_s).  A launch may still answer SLAK_ERR_UNSUPPORTED after the plan named it (slak_set_conv_algo can change in between and
 * the pair launch honours it; the device's CU count decides the three-branch weight gradient's work split): the caller then drops one rung.
 * allow: SLAK_TRI_ALLOW_FUSED (the launches that READ the three fp32 filters: TRI_STATS / TRI forward, TRI data gradient, ONE; a caller whose filters
 * are not contiguous fp32 clears it) | _STATS (gather the BatchNorm sums in the forward launches) | _WGRAD (the TRI and PAIR weight gradients) |
 * _BACKWARD (ONE) | _DGRAD_ACC (BRANCH_ACC).  SLAK_ERR_INVALID_ARG: plan == NULL or a dimension <= 0. */
enum { SLAK_TRI_FWD_BRANCH = 0, SLAK_TRI_FWD_BRANCH_STATS = 1, SLAK_TRI_FWD_TRI = 2, SLAK_TRI_FWD_TRI_STATS = 3 };
enum { SLAK_TRI_DGRAD_BRANCH_ADD = 0, SLAK_TRI_DGRAD_BRANCH_ACC = 1, SLAK_TRI_DGRAD_TRI = 2, SLAK_TRI_DGRAD_ONE = 3 };
enum { SLAK_TRI_WGRAD_BRANCH = 0, SLAK_TRI_WGRAD_PAIR = 1, SLAK_TRI_WGRAD_TRI = 2, SLAK_TRI_WGRAD_ONE = 3 };
enum { SLAK_TRI_ALLOW_FUSED = 1, SLAK_TRI_ALLOW_STATS = 2, SLAK_TRI_ALLOW_WGRAD = 4, SLAK_TRI_ALLOW_BACKWARD = 8, SLAK_TRI_ALLOW_DGRAD_ACC = 16,
       SLAK_TRI_ALLOW_ALL = 31 };
typedef struct slak_tri_plan {
    int fwd, stats_rows, dgrad, wgrad;
    size_t ws_wgrad;
} slak_tri_plan_t;
int slak_tri_plan(int dtype, int N, int C, int H, int W, int K, unsigned allow, slak_tri_plan_t* plan);

/* ---------------------------------------------------------------- next row: block tail glue
 * The layout / normalisation / residual steps around the two pointwise GEMMs of a SLaK block
 * (models/SLaK.py:153-166: permute -> LayerNorm -> [pwconv1, GELU, pwconv2] -> gamma -> permute -> shortcut + drop_path),
 * one HBM-bound kernel per arrow and direction.  Activations bf16, statistics / residual stream / parameters fp32.
 * P = H*W pixels per image; x, dx, shortcut, out are NCHW; y, g, z, dz are NHWC (N,H,W,C) contiguous; C even, <= 1024.
 * These four functions are the `_ld` ones below called with ldc = C. */
size_t slak_block_tail_workspace_bytes(int N, int C, int P);

/* y[n,p,:] = LayerNorm_C(x[n,:,p]) * weight + bias   (F.layer_norm over the last dim of x.permute(0,2,3,1): models/SLaK.py:156-157, :253-255) */
int slak_ln_nchw_to_nhwc_forward(const void* x_bf16, const float* weight, const float* bias, void* y_bf16, float* mean, float* rstd,
                                 int N, int C, int P, float eps, void* stream);
int slak_ln_nchw_to_nhwc_backward(const void* g_bf16, const void* x_bf16, const float* weight, const float* mean, const float* rstd,
                                  void* dx_bf16, float* dweight, float* dbias, int N, int C, int P,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* out[n,c,p] = shortcut[n,c,p] + sample_scale[n] * gamma[c] * z[n,p,c]        (models/SLaK.py:161-165; sample_scale = the
 * DropPath mask/keep_prob per sample or NULL) ; backward: dz = sample_scale*gamma*dout (bf16 NHWC), dgamma = sum sample_scale*dout*z */
int slak_scale_residual_forward(const void* shortcut, int shortcut_dtype, const void* z_bf16, const float* gamma, const float* sample_scale,
                                float* out, void* out_bf16 /* NULL, or a second copy of `out` rounded to bf16: the next block's conv input */,
                                int N, int C, int P, void* stream);
/* dout_bf16 (NULL or the gradient that arrived through out_bf16) is added to dout; the sum -- the gradient of `shortcut` -- is
 * written to dout_sum (required iff dout_bf16 is given; otherwise the shortcut gradient is dout itself).
 * dz_colsum[c] = sum over n,p of the (unrounded) dz: the bias gradient of the Linear that produced z (models/SLaK.py:160). */
int slak_scale_residual_backward(const float* dout, const void* dout_bf16, float* dout_sum, const void* z_bf16, const float* gamma,
                                 const float* sample_scale, void* dz_bf16, float* dgamma, float* dz_colsum, int N, int C, int P,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* The same four ops with a row pitch on the NHWC side (`--width_factor 1.3`: C = 124 / 249 / 499 / 998).  The NCHW tensors (x, dx, shortcut,
 * out, dout) keep their logical C; y, g, z, dz are (N,H,W,ldc) contiguous, i.e. rows of ldc >= C elements.  One argument rule, which
 * slak_block_tail_family shares: 1 <= C <= ldc <= 1024 and N * ldc * P < 2^31; ldc == C needs an even C, ldc > C (C of ANY parity) needs
 * ldc % 8 == 0; else SLAK_ERR_UNSUPPORTED.  workspace >= slak_block_tail_workspace_bytes(N, ldc, P).  Arguments as the plain entry points, ldc last.
 *   - the LayerNorm statistics and every 1/C factor use the logical C; columns c >= C never enter a sum;
 *   - columns c >= C of y and of dz are WRITTEN, as +0.0, on every call (the next GEMM reads whole rows);
 *   - columns c >= C of g and z are never used: they may hold anything, NaN included;
 *   - weight, bias, gamma, dweight, dbias, dgamma, dz_colsum are [C].
 * ldc == C is the plain call: the same checks, launches and bits.
 * Kernels: a pitched call runs the small-plane families of the plain entry points (H*W <= 256: a wave per image and group of 24-64 channels, one
 * pixel per lane on odd planes) exactly where the plain call on C = ldc runs them -- the channel groups tile the pitch, a group's live channel count
 * is a wave-uniform bound, a group of pad columns only writes its +0 --, plus, for the two LayerNorm ops on odd planes, 64 channels per wave where
 * ldc / 32 exceeds the 16 waves of a workgroup (C = 998, ldc = 1024).  Then the pixel-pair register-tile kernels (even planes, ldc = 128 / 256 / 512,
 * ldc - C <= 16), then the LDS-tile kernels.  slak_block_tail_family says which.  The parameter gradients are summed in a fixed order in every family. */
int slak_ln_nchw_to_nhwc_forward_ld(const void* x_bf16, const float* weight, const float* bias, void* y_bf16, float* mean, float* rstd,
                                    int N, int C, int P, float eps, void* stream, int ldc);
int slak_ln_nchw_to_nhwc_backward_ld(const void* g_bf16, const void* x_bf16, const float* weight, const float* mean, const float* rstd,
                                     void* dx_bf16, float* dweight, float* dbias, int N, int C, int P,
                                     void* workspace, size_t workspace_bytes, void* stream, int ldc);
int slak_scale_residual_forward_ld(const void* shortcut, int shortcut_dtype, const void* z_bf16, const float* gamma, const float* sample_scale,
                                   float* out, void* out_bf16, int N, int C, int P, void* stream, int ldc);
int slak_scale_residual_backward_ld(const float* dout, const void* dout_bf16, float* dout_sum, const void* z_bf16, const float* gamma,
                                    const float* sample_scale, void* dz_bf16, float* dgamma, float* dz_colsum, int N, int C, int P,
                                    void* workspace, size_t workspace_bytes, void* stream, int ldc);

/* Which kernel family the block-tail entry points run for `op` on (N, C, P) with NHWC rows of ldc elements; ldc == C asks for the plain entry
 * point's choice.  Pure host code, callable without a device; the four ops choose their kernel through this very function, so the answer
 * IS the launch.  NONE: the entry point would not launch (invalid or unsupported arguments; shortcut_dtype matters to SLAK_TAIL_SR_FWD only).
 * TILE: LDS-tile kernels; REG: pixel-pair register-tile kernels; CHAN / CHAN1: the small-plane families, even / odd H*W. */
enum { SLAK_TAIL_LN_FWD = 0, SLAK_TAIL_LN_BWD = 1, SLAK_TAIL_SR_FWD = 2, SLAK_TAIL_SR_BWD = 3 };
enum { SLAK_TAIL_FAMILY_NONE = 0, SLAK_TAIL_FAMILY_TILE = 1, SLAK_TAIL_FAMILY_REG = 2, SLAK_TAIL_FAMILY_CHAN = 3, SLAK_TAIL_FAMILY_CHAN1 = 4 };
int slak_block_tail_family(int op, int shortcut_dtype, int N, int C, int P, int ldc);

/* Downsample layers (models/SLaK.py:285-311: LayerNorm(C, data_format="channels_first") -> Conv2d(C, C', kernel_size=2, stride=2)).  The
 * kernel/stride-2 convolution is a GEMM on non-overlapping 2x2 patches; slak_ln_patch_forward normalises the fp32 NCHW input over C and
 * writes the result (rounded to bf16, as autocast's cast in front of the conv does) directly as that GEMM's operand
 *     a[n][ho * (W/2) + wo][(kh * 2 + kw) * C + c] = LN(x)[n, c, 2 ho + kh, 2 wo + kw],
 * so the conv is Y[n] = Wp . a[n]^T (batched library GEMM, NCHW result, Wp[co][(kh*2+kw)*C + c] = weight[co, c, kh, kw]) with no im2col,
 * layout transposes or casts; _backward takes dL/da in the same layout.  C in {64, 96, 128, 192, 256, 384, 512}, H and W even. */
int slak_ln_patch_supported(int N, int C, int H, int W);
int slak_ln_patch_forward(const float* x, const float* weight, const float* bias, void* a_bf16, float* mean, float* rstd,
                          int N, int C, int H, int W, float eps, void* stream);
int slak_ln_patch_backward(const void* g_bf16, const float* x, const float* weight, const float* mean, const float* rstd,
                           float* dx, float* dweight, float* dbias, int N, int C, int H, int W,
                           void* workspace /* slak_block_tail_workspace_bytes(N, C, H*W) */, size_t workspace_bytes, void* stream);

/* Stem (models/SLaK.py:276-279: Conv2d(in_chans, C, kernel_size=4, stride=4) on the fp32 image): the 4x4 patches as the bf16 GEMM operand
 * a[n][ho * (W/4) + wo][(c * 4 + kh) * 4 + kw] = x[n, c, 4 ho + kh, 4 wo + kw]; the conv is Y[n] = weight.view(C, in_chans*16) . a[n]^T (NCHW).
 * H and W multiples of 4. */
int slak_stem_patchify(const float* x, void* a_bf16, int N, int Cin, int H, int W, void* stream);

/* dst (N, P, C) = src (N, C, P) transposed per image, bf16: the NCHW output gradient of a downsample convolution (models/SLaK.py:195-199) as the
 * row operand [N*P][C] of its weight-gradient GEMM (slak_linear_wgrad) -- torch's `grad.transpose(1, 2).reshape(...)` copy.  C % 8 == 0. */
int slak_nchw_to_pixel_major_bf16(const void* src, void* dst, int N, int C, int P, void* stream);

/* y (N, C, P) bf16 = bf16(bias[c]) broadcast: the accumulator the batched GEMM of a downsample convolution (models/SLaK.py:195-199) adds its
 * products to -- the bias of nn.Conv2d inside the GEMM (fp32 accumulate, one rounding) without torch's strided broadcast copy. */
int slak_fill_channel_bias_bf16(const float* bias, void* y_bf16, int N, int C, int P, void* stream);

/* Bias gradient of the stem / downsample convolutions: out[c] = sum over n and p of the bf16 NCHW gradient x[n][c][p], fp32, fixed summation
 * order.  Replaces `grad_output.sum((0, 2, 3))` of torch's Conv2d backward (reference: models/SLaK.py:188-199, the stem and downsample
 * nn.Conv2d layers).  workspace: slak_channel_sums_workspace_bytes(C) bytes. */
/* Forward of the stem convolution (models/SLaK.py:189-193: nn.Conv2d(3, dims[0], kernel_size=4, stride=4)) under bf16 autocast, from the fp32
 * NCHW image x (N, 3, H, W): y (N, Co, H/4, W/4) bf16 = bf16(bf16(bias) + sum_k bf16(weight[co][k]) * bf16(patch[k])) with fp32 accumulation --
 * the arithmetic of the autocast conv -- and the bf16 patch matrix a (N, P, 48) of slak_stem_patchify written in the same pass (the operand of
 * slak_stem_wgrad).  weight: fp32 (Co, 3, 4, 4) contiguous; bias: fp32 (Co) or NULL.  Supported: Cin = 3, Co % 32 == 0, Co <= 128, H % 4 == 0,
 * W % 4 == 0, (H/4)*(W/4) % 64 == 0; otherwise SLAK_ERR_UNSUPPORTED and the caller keeps slak_stem_patchify + its GEMM. */
int slak_stem_conv_forward_supported(int N, int Cin, int H, int W, int Co);
int slak_stem_conv_forward(const float* x, const float* weight, const float* bias, void* a_bf16, void* y_bf16, int N, int Cin, int H, int W, int Co,
                           void* stream);

/* Weight and bias gradient of the stem convolution (models/SLaK.py:189-193: nn.Conv2d(in_chans, dims[0], kernel_size=4, stride=4)) from the bf16
 * NCHW output gradient dy (N, Co, P) and the forward's patch matrix a (N, P, K) of slak_stem_patchify (K = Cin*16): dw (Co, K) fp32 =
 * sum_{n,p} dy[n][co][p] * a[n][p][k] -- reshaped (Co, Cin, 4, 4) it is Conv2d's weight gradient -- and db (Co) = sum_{n,p} dy (NULL: not wanted).
 * One pass over dy and a, fp32 accumulation, fixed summation order.  Supported: Co % 32 == 0, Co <= 128, P % 64 == 0, K % 8 == 0, 32 <= K <= 56
 * (Cin = 3: K = 48); otherwise SLAK_ERR_UNSUPPORTED and the caller keeps its GEMM. */
int slak_stem_wgrad_supported(int N, int Co, int P, int K);
size_t slak_stem_wgrad_workspace_bytes(int N, int Co, int P, int K);
int slak_stem_wgrad(const void* dy_bf16, const void* a_bf16, float* dw, float* db, int N, int Co, int P, int K,
                    void* workspace, size_t workspace_bytes, void* stream);

size_t slak_channel_sums_workspace_bytes(int C);
int slak_channel_sums_bf16(const void* x_bf16, float* out, int N, int C, int P, void* workspace, size_t workspace_bytes, void* stream);

/* The pointwise convolutions on the large maps (stage 1-2: M = N*H*W rows of C <= 192 or 4C <= 768 channels against a weight of a few
 * hundred KB) are HBM streams, not GEMMs: Y[M,N] = X[M,K] . Wt[N,K]^T (+ bias[N]) with both operands K-contiguous ("NT": pwconv1 /
 * pwconv2 forward take the nn.Linear weight as it is stored, models/SLaK.py:158-160; the data gradients take its transpose), bf16 in
 * and out, fp32 accumulate; gelu_out (or NULL) receives nn.GELU() of the rounded Y in the same pass.  Covered: K in {96, 192} with
 * N % 32 == 0, or N in {96, 192} with K % 16 == 0 (no gelu_out); anything else returns SLAK_ERR_UNSUPPORTED (library GEMM). */
int slak_linear_nt_supported(int M, int N, int K, int gelu);
int slak_linear_nt(const void* x_bf16, const void* wt_bf16, const void* bias_bf16 /* or NULL */, void* y_bf16, void* gelu_out_bf16 /* or NULL */,
                   int M, int N, int K, void* stream);

/* pwconv1 -> GELU -> pwconv2 in ONE pass (models/SLaK.py:158-160) where the whole second weight fits a wave's registers: x [M][C], w1 [C4][C],
 * b1 [C4], w2 [C][C4], b2 [C] (the nn.Linear parameters as stored; biases may be NULL), y1 = x w1^T + b1 and a = GELU(y1) [M][C4] (the backward
 * needs both: same bits as slak_linear_nt with gelu_out), z = a w2^T + b2 [M][C], all bf16, fp32 accumulate.  a is not read back from HBM and
 * pwconv2 is not a launch.  Round 4: C = 96, C4 = 384 (stage 1 of SLaK-T / SLaK-S); anything else: SLAK_ERR_UNSUPPORTED (two slak_linear_nt). */
int slak_linear_mlp_fwd_supported(int M, int C, int C4);
int slak_linear_mlp_fwd(const void* x_bf16, const void* w1_bf16, const void* b1_bf16, const void* w2_bf16, const void* b2_bf16,
                        void* y1_bf16, void* a_bf16, void* z_bf16, int M, int C, int C4, void* stream);

/* The fixed-order column sums that end slak_scale_residual_backward, slak_ln_nchw_to_nhwc_backward, slak_gelu_backward_bias,
 * slak_linear_nt_gelu_bwd and slak_linear_wgrad (the parameter gradients of a block's tail: results nothing else of the block's backward
 * reads) in ONE launch instead of one each: between _begin and _end ON THE CALLING THREAD those calls record their reduction instead of
 * launching it -- the partial rows stay in the workspace each call was given, so the caller must hand every call in between its OWN
 * workspace -- and _end launches one kernel that performs all of them, on the stream the calls were given, with the same additions in
 * the same order (the same bits).  Not nestable; a ninth pending reduction launches the eight before it; a call on ANOTHER stream than the
 * first recorded one is not deferred (its reduction launches at once on its own stream). */
int slak_defer_reductions_begin(void);
int slak_defer_reductions_end(void);

/* pwconv2's data gradient WITH nn.GELU()'s backward and pwconv1's bias gradient in the same pass (models/SLaK.py:159-160 backwards):
 * dy1[M,N] = round(dz[M,K] . W2[K,N]) * gelu'(y1[M,N]) (bf16, the same bits as slak_linear_nt followed by slak_gelu_backward_bias),
 * dbias[N] = column sums of the rounded dy1 (fp32, fixed order).  wt = W2^T stored [N][K].  The intermediate dact never reaches HBM.
 * Round 4: K = 96, N = 384, M % 32 == 0 (stage 1 of SLaK-T / SLaK-S); anything else: SLAK_ERR_UNSUPPORTED (the two calls). */
int slak_linear_nt_gelu_bwd_supported(int M, int N, int K);
size_t slak_linear_nt_gelu_bwd_workspace_bytes(int M, int N, int K);
int slak_linear_nt_gelu_bwd(const void* dz_bf16, const void* wt_bf16, const void* y1_bf16, void* dy1_bf16, float* dbias, int M, int N, int K,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The same launch with the next product of the block's backward in it: dt[M,K] = dy1 . W1 (pwconv1's data gradient), taken from the dy1 tiles while
 * they are on chip -- the separate slak_linear_nt launch and its re-read of dy1 (308 MB per stage-1 block of SLaK-T) are gone.  w1p = W1^T [K][N]
 * bf16 (pwconv1's nn.Linear weight transposed) in fragment-major order: viewed (3, 32, 6, 4, 2, 8) and permuted (2, 3, 0, 4, 1, 5), contiguous.
 * dy1 and dbias: the bits of slak_linear_nt_gelu_bwd; dt: bf16 of the same fp32 sums added in another order.  Shapes and workspace as above. */
int slak_pack_w1t_fragments(const void* w1t_bf16 /*[K][N] row-major*/, void* w1p_bf16 /*[K * N] out*/, int N, int K, void* stream);   /* the packer of w1p (N = 384, K = 96) */
int slak_linear_nt_gelu_bwd_dt_supported(int M, int N, int K);
int slak_linear_nt_gelu_bwd_dt(const void* dz_bf16, const void* wt_bf16, const void* y1_bf16, const void* w1p_bf16, void* dy1_bf16, void* dt_bf16,
                               float* dbias, int M, int N, int K, void* workspace, size_t workspace_bytes, void* stream);

/* Round 5 -- the pointwise Linear layers of stages 2-4 with their elementwise neighbours in the GEMM's epilogue (models/SLaK.py:156-165:
 * pwconv1 -> nn.GELU() -> pwconv2, and their data gradients): out[M][N] = a[M][K] . b[N][K]^T, both operands K-contiguous (the nn.Linear weight as it is
 * stored; the data gradients take its transpose), bf16 in and out, fp32 accumulate.  epilogue:
 *   SLAK_EPI_BIAS   out = bf16(acc + bias)                                    bias [N] bf16 or NULL
 *   SLAK_EPI_GELU   out = bf16(acc + bias), out2 = GELU(out)                  (exact erf form on the ROUNDED pre-activation, as F.gelu of a bf16 tensor; both
 *                                                                              tensors are kept because nn.GELU's backward reads the pre-activation)
 *   SLAK_EPI_DGELU  out = bf16(bf16(acc) * gelu'(y1)), dbias[N] = column sums of out   (y1 [M][N] bf16: the same dy1 bits as the GEMM followed by
 *                                                                              slak_gelu_backward_bias; dbias fp32, fixed summation order; needs the workspace)
 * Replaces on these stages: at::linear + at::gelu (two passes over [M][4C]) resp. at::mm + slak_gelu_backward_bias (the [M][4C] intermediate `dact`
 * written and read back).  Covered: epilogue GELU / DGELU with K in {192, 256, 384} and N % 256 == 0, or K in {512, 768} and N % 128 == 0 (stages 2-4 of
 * SLaK-T / -S, stages 2-3 of SLaK-B), M >= 1, tensors below 4 GiB; anything else -- SLAK_EPI_BIAS included: reserved -- SLAK_ERR_UNSUPPORTED (library GEMM +
 * elementwise pass). */
enum { SLAK_EPI_BIAS = 0, SLAK_EPI_GELU = 1, SLAK_EPI_DGELU = 2 };
int slak_linear_gemm_supported(int M, int N, int K, int epilogue);
size_t slak_linear_gemm_workspace_bytes(int M, int N, int K, int epilogue);
int slak_linear_gemm(const void* a_bf16, const void* b_bf16, const void* bias_bf16, void* out_bf16, void* out2_bf16, const void* y1_bf16, float* dbias,
                     int M, int N, int K, int epilogue, void* workspace, size_t workspace_bytes, void* stream);

/* Transposed bf16 copies dst[i] [cols][rows] of src[i] [rows][cols] (rows, cols multiples of 8) for n matrices in ONE launch (host arrays of device
 * pointers): the pointwise weights as the data-gradient GEMMs read them (dz . W2, dy1 . W1: models/SLaK.py:158-160 backwards).  Replaces one strided copy
 * kernel per weight, block and step (25 launches per SLaK-T step) by one launch per optimizer step (slak_amd/block_ops.lowp_param_t caches by version). */
int slak_transpose_bf16_batch(const void* const* src, void* const* dst, const int* rows, const int* cols, int n, void* stream);

/* Zero-padded bf16 copies of n fp32 matrices src[i] [rows][cols] in ONE launch (host arrays of device pointers; any rows / cols, source rows need
 * only the 4-byte alignment of a float): dst[i] is [dst_rows][dst_cols] bf16 with dst = bf16(src) in its upper left corner (transpose[i] == 0;
 * dst_rows >= rows, dst_cols >= cols) or dst = bf16(src)^T there (transpose[i] != 0; dst_rows >= cols, dst_cols >= rows) and +0.0 everywhere else.
 * The weights and biases of a block whose NHWC tensors carry a row pitch (slak_*_ld above) as its GEMMs read them. */
int slak_pad_cast_bf16_batch(const void* const* src_f32, void* const* dst_bf16, const int* rows, const int* cols, const int* dst_rows,
                             const int* dst_cols, const int* transpose, int n, void* stream);

/* Weight gradient of the pointwise Linear layers (models/SLaK.py:117-118 pwconv1 / pwconv2; autograd's dW = dY^T X):
 * d[N1][N2] (fp32) = x1^T x2 over the M rows of x1 [M][N1] and x2 [M][N2] (bf16, row-major), fp32 accumulate, summed in a fixed
 * order (deterministic).  Covered: N1 and N2 multiples of 192, or one of them 96 and the other a multiple of 384 (the ConvNeXt widths
 * 96 * 2^k and their 4x expansions); M >= 32; anything else returns SLAK_ERR_UNSUPPORTED (library GEMM). */
int slak_linear_wgrad_supported(int M, int N1, int N2);
size_t slak_linear_wgrad_workspace_bytes(int M, int N1, int N2);
int slak_linear_wgrad(const void* x1_bf16, const void* x2_bf16, float* d, int M, int N1, int N2, void* workspace, size_t workspace_bytes, void* stream);

/* GELU backward (exact erf form, nn.GELU()) fused with the bias gradient of the Linear in front of it (models/SLaK.py:158-160):
 * dy1 = dact * gelu'(y1); dbias[col] = sum_rows dy1.  [rows][cols] bf16 contiguous, cols % 8 == 0. */
size_t slak_gelu_bwd_workspace_bytes(int rows, int cols);
int slak_gelu_backward_bias(const void* dact_bf16, const void* y1_bf16, void* dy1_bf16, float* dbias, int rows, int cols,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Which launch runs each step of a block's pointwise MLP (models/SLaK.py:158-160: pwconv1 -> GELU -> pwconv2, its data gradient and its two weight
 * gradients) on M rows of Cp channels, C4 = rows of W1 (4 Cp).  The ONE place where the ladder is written: every step takes the first rung, in the
 * order listed, whose slak_linear_*_supported query says yes and whose kernel family `allow` admits; LIBRARY (the caller's GEMM) ends every ladder.
 * Pure host code, built from the *_supported / *_workspace_bytes queries above and nothing else, so a launch never refuses what the plan chose.
 * Both callers (slak_amd/block_ops.py, slak_amd/pybind/block_runner.cpp) switch on the answer.
 *   pw1   pwconv1 + GELU:      FUSED   slak_linear_mlp_fwd (pwconv2 is in the same launch: pw2 is not looked at)
 *                              NT      slak_linear_nt with gelu_out
 *                              GEMM    slak_linear_gemm, SLAK_EPI_GELU
 *                              LIBRARY the caller's GEMM, then GELU
 *   pw2   pwconv2:             NT slak_linear_nt | LIBRARY
 *   dy1   dz W2, GELU', db1:   FUSED_DT slak_linear_nt_gelu_bwd_dt (dt = dy1 W1 is in the same launch: dt is not looked at; needs W1^T packed by slak_pack_w1t_fragments)
 *                              FUSED   slak_linear_nt_gelu_bwd
 *                              GEMM    slak_linear_gemm, SLAK_EPI_DGELU
 *                              NT      slak_linear_nt, then slak_gelu_backward_bias
 *                              LIBRARY the caller's GEMM, then slak_gelu_backward_bias
 *   dt    dy1 W1:              NT slak_linear_nt | LIBRARY
 *   dw1, dw2  dy1^T t, dz^T a: KERNEL slak_linear_wgrad | LIBRARY: the M rows as `splits` batches of a batched GEMM, the partial products added in fp32
 *                              (splits = max(1, M / rows) lowered until it divides M; 1: one plain GEMM; rows = SLAK_SPLITK_ROWS in the environment,
 *                              read once, default 6272, <= 0: never split)
 *   ws_*  workspace bytes of the CHOSEN launch of dy1 (with slak_gelu_backward_bias's on the NT / LIBRARY rungs), dw1 and dw2; 0: none.
 * allow: SLAK_MLP_ALLOW_SKINNY (linear_skinny.hip: FUSED, FUSED_DT, NT) | _GEMM (linear_gemm.hip) | _WGRAD (linear_wgrad.hip); 0 is LIBRARY everywhere
 * (what a caller whose operands are not contiguous bf16 device tensors asks for).  SLAK_ERR_INVALID_ARG: plan == NULL or a dimension <= 0. */
enum { SLAK_MLP_LIBRARY = 0, SLAK_MLP_NT = 1, SLAK_MLP_GEMM = 2, SLAK_MLP_FUSED = 3, SLAK_MLP_FUSED_DT = 4, SLAK_MLP_KERNEL = 5 };
enum { SLAK_MLP_ALLOW_SKINNY = 1, SLAK_MLP_ALLOW_GEMM = 2, SLAK_MLP_ALLOW_WGRAD = 4, SLAK_MLP_ALLOW_ALL = 7 };
typedef struct slak_mlp_plan {
    int pw1, pw2, dy1, dt, dw1, dw2, splits;
    size_t ws_dy1, ws_dw1, ws_dw2;
} slak_mlp_plan_t;
int slak_mlp_plan(int M, int C4, int Cp, unsigned allow, slak_mlp_plan_t* plan);

/* channels_first LayerNorm of the stem / downsample layers (models/SLaK.py:192-203, :256-261): y[n,c,p] = LN_C(x[n,:,p])*w + b, NCHW in
 * and out; x/y/g/dx fp32 or bf16 (dx has the dtype of x). */
size_t slak_ln_cf_workspace_bytes(int N, int C, int P);
int slak_ln_channels_first_forward(const void* x, int x_dtype, const float* weight, const float* bias, void* y, int y_dtype,
                                   float* mean, float* rstd, int N, int C, int P, float eps, void* stream);
int slak_ln_channels_first_backward(const void* g, int g_dtype, const void* x, int x_dtype, const float* weight, const float* mean,
                                    const float* rstd, void* dx, float* dweight, float* dbias, int N, int C, int P,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* The stem's LayerNorm handing the first block a bf16 copy of its output (what the block's depthwise convs read under autocast), and taking
 * that copy's gradient back: y_bf16 (NULL: none) = bf16(y); g2_bf16 (NULL: none) is ADDED to g on load -- `.to(bfloat16)` in front of the
 * first block and autograd's `grad + grad_lowp.float()` behind it are no separate passes.  _backward_pair with g2 covers what
 * slak_ln_channels_first_backward_pair_supported says (x bf16, g fp32, C = 96 / 128 / 192: one pass over g and x, the channels of a 64-pixel tile
 * in the registers of four waves); without g2 it is slak_ln_channels_first_backward. */
int slak_ln_channels_first_forward_pair(const void* x, int x_dtype, const float* weight, const float* bias, void* y, int y_dtype, void* y_bf16,
                                        float* mean, float* rstd, int N, int C, int P, float eps, void* stream);
int slak_ln_channels_first_backward_pair_supported(int g_dtype, int x_dtype, int N, int C, int P);
int slak_ln_channels_first_backward_pair(const void* g, int g_dtype, const void* g2_bf16, const void* x, int x_dtype, const float* weight,
                                         const float* mean, const float* rstd, void* dx, float* dweight, float* dbias, int N, int C, int P,
                                         void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- next row: branch BatchNorms + adds
 * out = BN1(y1) + BN2(y2) + BN3(y3) of ReparamLargeKernelConv (models/SLaK.py:38-47, :92-95) as one statistics pass, a per-channel
 * finalise and one apply pass; backward likewise (dy_b is affine in (dout, y_b) per channel).  y_b, out, dout, dy_b: bf16 NCHW,
 * P = H*W.  The *_sums calls return THIS RANK's per-channel sums; under SyncBatchNorm the caller all-reduces them (6C doubles / 4C
 * floats, one collective per block and direction instead of three gathers) and passes the global sums and the global element count to the
 * *_apply calls (`count`, or `count_dev` -- a device double, e.g. the all-reduced count -- when non-NULL: no host synchronisation).
 * Round 3: the forward statistics are CENTRED -- slice sums of (y - k) with k the slice's first element, combined as doubles; raw fp32
 * rows from the conv launches (pre_sums) are added in double and a channel with mean^2 > 1024 var is re-measured by a two-pass read --
 * so the variance survives |mean| / std of 1e3 and more (nn.BatchNorm2d's Welford statistics do); the backward sums are the centred
 * products sum dout * (y_b - mean_b). */
size_t slak_bn3_workspace_bytes(int N, int C);
int slak_bn3_forward_sums(const void* y1, const void* y2, const void* y3, double* local_sums /*[C][6]: sum y_b, sum y_b^2*/, int N, int C, int P,
                          void* workspace, size_t workspace_bytes, void* stream,
                          const float* const* pre_sums /* NULL or as in slak_bn3_forward_local */, const int* pre_rows, int pre_stride);
int slak_bn3_forward_apply(const void* y1, const void* y2, const void* y3, const double* global_sums, double count, const double* count_dev,
                           const float* const* gamma_host3, const float* const* beta_host3, float* const* running_mean_host3,
                           float* const* running_var_host3, float eps, float momentum, int training, int update_running,
                           float* coef /*[C][4]*/, float* stats /*[C][6]*/, void* out, int N, int C, int P, void* stream);
int slak_bn3_backward_sums(const void* dout, const void* y1, const void* y2, const void* y3, const float* stats /*[C][6] of the forward*/,
                           float* local_sums /*[C][4]: sum dout, sum dout*(y_b - mean_b)*/,
                           int N, int C, int P, void* workspace, size_t workspace_bytes, void* stream);
int slak_bn3_backward_apply(const void* dout, const void* y1, const void* y2, const void* y3, const float* global_sums,
                            const float* local_sums, double count, const double* count_dev /* device count overrides `count` */,
                            const float* stats, const float* const* gamma_host3,
                            float* bcoef /*[C][9]*/, float* dgamma /*[3][C]*/, float* dbeta /*[3][C]*/,
                            void* dy1, void* dy2, void* dy3, int N, int C, int P, void* stream);
/* Single-process training step of the same op (no all-reduce between the statistics and the apply pass: the slice reduction and the
 * finalise step share a launch).  Same arithmetic and side effects as _forward_sums + _forward_apply(training = 1) resp.
 * _backward_sums + _backward_apply with global_sums = local_sums, count = N * P. */
int slak_bn3_forward_local(const void* y1, const void* y2, const void* y3, const float* const* gamma, const float* const* beta,
                           float* const* running_mean, float* const* running_var, float eps, float momentum, int update_running,
                           float* coef, float* stats, void* out, int N, int C, int P, void* workspace, size_t workspace_bytes, void* stream,
                           const float* const* pre_sums /* NULL, or 3 device pointers: branch b's partial sums, element (row, c, k) at
                                                           pre_sums[b][(row * C + c) * pre_stride + k], k = 0 (sum), 1 (sum of squares) */,
                           const int* pre_rows /* rows per branch */, int pre_stride /* 6: one slak_dwconv2d_tri_forward_stats array, pointers offset
                                                           by 0, 2, 4 floats; 2: three slak_dwconv2d_forward_stats arrays */);
int slak_bn3_backward_local(const void* dout, const void* y1, const void* y2, const void* y3, const float* stats, const float* const* gamma,
                            float* bcoef, float* dgamma, float* dbeta, void* dy1, void* dy2, void* dy3, int N, int C, int P,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Round 6: the same two calls with ONE destination per parameter gradient (dgamma3 / dbeta3: host arrays of three device pointers, [C]
 * floats each) instead of two [3][C] arrays.  Under DistributedDataParallel(gradient_as_bucket_view=True) a parameter's .grad is a view
 * of an all-reduce bucket (main.py:374-376 builds the wrapper): with these the six BatchNorm parameter gradients of a block
 * (models/SLaK.py:38-47) are written where the reducer wants them and its per-parameter copy launch disappears.  The [3][C]
 * forms above are wrappers over these (same kernels, same bits). */
/* Round 6, the SyncBatchNorm exchange with two launches fewer per block and step: _forward_sums_counted also writes this rank's element count
 * N * P into local_sums[6C] (the exchange buffer is [6C + 1] doubles: the count travels with the sums, models/SLaK.py:24-28's SyncBatchNorm
 * needs the global count); _backward_sums_dup writes the sums twice (local_sums stays for the local parameter gradients, sums_copy is what the
 * all-reduce overwrites in place). */
int slak_bn3_forward_sums_counted(const void* y1, const void* y2, const void* y3, double* local_sums /*[6C + 1]*/, int N, int C, int P,
                                  void* workspace, size_t workspace_bytes, void* stream,
                                  const float* const* pre_sums, const int* pre_rows, int pre_stride);
int slak_bn3_backward_sums_dup(const void* dout, const void* y1, const void* y2, const void* y3, const float* stats, float* local_sums /*[C][4]*/,
                               float* sums_copy /*[C][4]*/, int N, int C, int P, void* workspace, size_t workspace_bytes, void* stream);
int slak_bn3_backward_apply_to(const void* dout, const void* y1, const void* y2, const void* y3, const float* global_sums,
                               const float* local_sums, double count, const double* count_dev, const float* stats, const float* const* gamma_host3,
                               float* bcoef /*[C][9]*/, float* const* dgamma3, float* const* dbeta3,
                               void* dy1, void* dy2, void* dy3, int N, int C, int P, void* stream);
int slak_bn3_backward_local_to(const void* dout, const void* y1, const void* y2, const void* y3, const float* stats, const float* const* gamma,
                               float* bcoef, float* const* dgamma3, float* const* dbeta3, void* dy1, void* dy2, void* dy3, int N, int C, int P,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- next row: mask-aware optimizer step and EMA
 * One launch over ALL tensors each.  Descriptor arrays live in HOST memory at plan creation (device pointers inside); plans own their
 * device tables.
 *
 * slak_adamw_step = torch.optim.AdamW's update (optim_factory.py:149-150; decoupled weight decay, bias corrections evaluated in double
 * from the tensor's own step count) followed by Masking.apply_mask's w *= mask (sparse_core.py:316-333) and, optionally, the bf16 copy
 * of the updated weight, in one pass.  `step` points at a device float holding the tensor's step count AFTER this step's increment
 * (the caller adds 1 to its step buffer first: one tiny launch).  Gradients are re-allocated by autograd / DDP every step, so their
 * pointers arrive separately: `grads_dev` is a DEVICE array of nseg device pointers (NULL entry = no gradient: the tensor is skipped,
 * as torch skips p.grad is None).  Hyper-parameters are per group (the reference builds one group per layer x {decay, no_decay}:
 * optim_factory.py:73-112) and are passed by value at every call (lr follows a per-iteration schedule: engine.py:41-46). */
#define SLAK_ADAMW_MAX_GROUPS 64
typedef struct {
    float* param;            /* fp32, updated in place                                        */
    float* exp_avg;          /* fp32 first moment                                             */
    float* exp_avg_sq;       /* fp32 second moment                                            */
    const float* mask;       /* fp32 0/1 mask (Masking.masks[name]) or NULL                   */
    void* param_bf16;        /* optional bf16 copy of the updated parameter, or NULL          */
    const float* step;       /* device scalar: step count of this tensor, already incremented */
    long long numel;
    int group;               /* index into the groups array of slak_adamw_step                */
} slak_adamw_segment_t;
typedef struct { double lr, beta1, beta2, eps, weight_decay; } slak_adamw_group_t;
typedef struct slak_adamw_plan slak_adamw_plan_t;
int slak_adamw_plan_create(const slak_adamw_segment_t* segs_host, int nseg, slak_adamw_plan_t** plan_out);
int slak_adamw_step(slak_adamw_plan_t* plan, const void* const* grads_dev, const slak_adamw_group_t* groups_host, int ngroups, void* stream);
int slak_adamw_plan_destroy(slak_adamw_plan_t* plan);

/* Gradient norm, clipping and loss-scale handling folded around slak_adamw_step: what NativeScalerWithGradNormCount.__call__
 * (utils.py:384-404) does between backward() and the optimizer step, over the SAME plan and the same device table of gradient pointers.
 * Vector loads and stores only, no atomics, every reduction in a fixed order: bitwise reproducible.  No entry synchronises the host.
 *
 * A zero-element tensor has no chunk; slak_adamw_plan_create accepts NULL param / exp_avg / exp_avg_sq pointers for it (torch gives it no storage).
 *
 * slak_adamw_plan_blocks: the number of 4096-element chunks of the plan = the number of partials slak_grad_sumsq writes for it
 * (a count, so an invalid plan is reported as -SLAK_ERR_INVALID_ARG, which no count can be).
 *
 * slak_grad_sumsq = the read half of GradScaler.unscale_ (torch/amp/grad_scaler.py, _unscale_grads_ ->
 * _amp_foreach_non_finite_check_and_unscale_) and the per-parameter torch.norm(p.grad, 2) of get_grad_norm_ (utils.py:424) /
 * clip_grad_norm_ (utils.py:396): partials_dev[offset + b] = sum over chunk b of ((double)u)^2, u = g * *inv_scale_dev rounded to fp32 once
 * (inv_scale_dev NULL: 1).  A chunk holding an inf or NaN gradient writes a non-finite partial; a NULL gradient pointer writes 0.
 * The gradients are only read.  One launch per plan; a model with more than SLAK_ADAMW_MAX_GROUPS groups has several plans that write
 * disjoint ranges of one partials array.
 *
 * slak_grad_norm_finish = the outer torch.norm(torch.stack(...)) of utils.py:424, clip_grad_norm_'s clip_coef (utils.py:396) and the
 * found_inf test of GradScaler.step (utils.py:400), WITHOUT its .item(): one workgroup sums the n partials (n = 0: norm 0) in fp64 and
 * writes ctl_dev[4] = { inv_scale, clip_coef = min(1, max_norm / (norm + 1e-6)) or 1 when max_norm < 0, found_inf (0 or 1),
 * norm = (float)sqrt(total), inf or NaN on overflow }.
 *
 * slak_adamw_step_scaled = GradScaler.step(optimizer) (utils.py:400) with the write halves of unscale_ and clip_grad_norm_: slak_adamw_step
 * on g' = (g * ctl[0]) * ctl[1] (two separately rounded products), and no write at all when ctl[2] is set.  The gradients are not modified.
 * The step counts must have been advanced by the caller only when ctl[2] is 0 (a device-side op; slak_amd.optim_factory does it). */
int slak_adamw_plan_blocks(const slak_adamw_plan_t* plan);
int slak_grad_sumsq(slak_adamw_plan_t* plan, const void* const* grads_dev, const float* inv_scale_dev, double* partials_dev, long long offset, void* stream);
int slak_grad_norm_finish(const double* partials_dev, int n, const float* inv_scale_dev, double max_norm /* < 0: no clipping */, float* ctl_dev, void* stream);
int slak_adamw_step_scaled(slak_adamw_plan_t* plan, const void* const* grads_dev, const slak_adamw_group_t* groups_host, int ngroups, const float* ctl_dev,
                           void* stream);

/* slak_ema_update = ModelEma.update(model, mask) (model_sema.py:67-91) over every state-dict entry:
 *   dense  : ema = ema*decay + (1-decay)*model
 *   masked : ema = (ema*decay + model*(1-decay))*mask + (diff*decay)*model,  diff = ((ema != 0) ^ mask) & mask  (newly grown weights)
 * each product and sum rounded separately in fp32, so the result is bit-identical to the reference's chain of torch kernels.
 * dtype SLAK_F32, or SLAK_I64 for BatchNorm's num_batches_tracked (float32 arithmetic, truncating copy back, as torch does). */
typedef struct {
    void* ema;               /* EMA copy of the entry, updated in place   */
    const void* model;       /* the live model's entry                    */
    const float* mask;       /* fp32 0/1 mask of this entry or NULL       */
    long long numel;
    int dtype;               /* SLAK_F32 or SLAK_I64                      */
} slak_ema_segment_t;
typedef struct slak_ema_plan slak_ema_plan_t;
int slak_ema_plan_create(const slak_ema_segment_t* segs_host, int nseg, slak_ema_plan_t** plan_out);
int slak_ema_update(slak_ema_plan_t* plan, double decay, void* stream);
int slak_ema_plan_destroy(slak_ema_plan_t* plan);

/* ---------------------------------------------------------------- the tail of the step: pooled LayerNorm head and the criterion
 *
 * slak_pool_ln_* = models/SLaK.py's `self.norm(x.mean([-2, -1]))` (the last line of forward_features): global average pool over the P = H * W
 * pixels of every plane of x[N][C][P] (NCHW contiguous, fp32 or bf16; no alignment of a plane is assumed), then nn.LayerNorm over C.
 * fp32 statistics: the plane sums are taken relative to the image's first element and divided by P, the variance over C is two-pass.
 * Forward: ONE launch.  y[N][C] in y_dtype (fp32 or bf16); pooled[N][C] (the plane means), mean[N], rstd[N] fp32 are what the backward reads.
 * Backward: dx[n][c][p] = dpool[n][c] / P for every pixel of a plane (x's dtype), dweight[C] / dbias[C] fp32 summed over the images in image
 * order by a second launch (TWO launches).  dy in dy_dtype (fp32 or bf16).  Covers C <= 2048 and P <= 1024 with N * C * P < 2^31; anything
 * else is SLAK_ERR_UNSUPPORTED, decided on the host before any launch (slak_pool_ln_supported: host code, no device needed). */
int slak_pool_ln_supported(int x_dtype, int N, int C, int P);
size_t slak_pool_ln_workspace_bytes(int N, int C, int P);            /* of slak_pool_ln_backward (the forward needs none) */
int slak_pool_ln_forward(const void* x, int x_dtype, const float* weight, const float* bias, float eps, void* y, int y_dtype,
                         float* pooled, float* mean, float* rstd, int N, int C, int P, void* stream);
int slak_pool_ln_backward(const void* dy, int dy_dtype, const float* pooled, const float* weight, const float* mean, const float* rstd,
                          void* dx, int x_dtype, float* dweight, float* dbias, int N, int C, int P,
                          void* workspace, size_t workspace_bytes, void* stream);

/* slak_xent_* = the criterion main.py:398-403 picks: F.cross_entropy(logits, labels, label_smoothing = smoothing, ignore_index) with
 * reduction 'mean' (nn.CrossEntropyLoss; smoothing > 0: timm1/loss/cross_entropy.py:20-26, LabelSmoothingCrossEntropy) when `labels` is
 * given, sum_k -t_k log_softmax(x)_k averaged over the rows (timm1/loss/cross_entropy.py:34-36, SoftTargetCrossEntropy) when
 * `soft_targets` is.  Exactly one of the two is non-NULL.  logits[N][K] fp32 / bf16 / fp16, row n at logits + n * row_stride elements (no
 * alignment of a row is assumed); labels int64 [N]; soft_targets fp32 [N][K] contiguous.  Per row, in fp32, with m the row maximum:
 *   lse = m + log sum_k exp(x_k - m)
 *   hard label y:  loss_n = (1 - smoothing) (lse - x_y) + smoothing (lse - mean_k x_k);  d_k = g / count (p_k - (1 - smoothing) [k == y] - smoothing / K)
 *   soft target t: loss_n = lse sum_k t_k - sum_k t_k x_k;                                 d_k = g / N (p_k sum_k t_k - t_k)
 * A row whose label equals ignore_index gives loss 0, gradient 0 and is left out of count (torch's 'mean').  A label never forms an
 * address: x_y is picked up by comparing k with y while the row is read, so a label outside [0, K) reads nothing (its row then has x_y = 0).
 * Forward: ONE launch.  loss[1] = sum_n loss_n / count, lse[N], count[1] (fp32: the number of rows that count; N for soft targets).  The
 * sum over the rows is taken in row order by the workgroup that finishes last (the arrival counters of the weight-gradient kernels): bitwise
 * reproducible, no floating-point atomics.  Backward: ONE launch.  grad_out is a DEVICE pointer to one fp32 (no host read); dlogits[N][K]
 * contiguous, in the logits' dtype.  Covers 1 <= K <= 32768, any N >= 1 with N * row_stride < 2^31. */
int slak_xent_supported(int logits_dtype, int N, int K);
size_t slak_xent_workspace_bytes(int N, int K);                      /* of slak_xent_forward (the backward needs none) */
int slak_xent_forward(const void* logits, int logits_dtype, long long row_stride, const long long* labels, const float* soft_targets,
                      float smoothing, long long ignore_index, float* loss, float* lse, float* count, int N, int K,
                      void* workspace, size_t workspace_bytes, void* stream);
int slak_xent_backward(const void* logits, int logits_dtype, long long row_stride, const long long* labels, const float* soft_targets,
                       float smoothing, long long ignore_index, const float* lse, const float* count, const float* grad_out,
                       void* dlogits, int N, int K, void* stream);

/* ---------------------------------------------------------------- Mixup / CutMix of a batch
 *
 * What timm's Mixup (timm1/data/mixup.py:90-218; built at main.py:296-299, applied to every batch at engine.py:49-50) does on the device, one
 * launch per pass.  The random numbers are drawn on the HOST, in the reference's order (slak_amd/mixup.py); these entries get finished
 * per-image records.  Image n is always paired with image N-1-n, so N must be even.
 *
 * A record: what happens to one image, and the coefficients of its target row.
 *   SLAK_MIXUP_NONE    the image stays as it is, bit for bit (lam == 1, mixing switched off, an element skipped under prob < 1)
 *   SLAK_MIXUP_MIX     x_n = round(x_n a) + round(x_j b): two fp32 multiplies, each rounded, then an add -- torch's op sequence, not an fma
 *   SLAK_MIXUP_CUTMIX  x_n[:, yl:yh, xl:xh] = x_j[:, yl:yh, xl:xh]: the partner's BITS; nothing outside the box is read into or written in image n
 * with j = N-1-n and x_j the partner's ORIGINAL values.  a, b are computed on the host exactly as the reference computes lam and 1 - lam and
 * rounded to fp32 once; for every kind they are the target coefficients as well.  The records arrive one of two ways (exactly one non-NULL):
 * `shared_host`, ONE record in host memory that every image shares ('batch' mode: it travels as a kernel argument, nothing is copied to the
 * device), or `table_dev`, a DEVICE array of N records ('pair' / 'elem' modes).  A shared record is checked on the host (unknown kind, box
 * outside the image: SLAK_ERR_INVALID_ARG); a table's boxes are clipped to the image by the kernel and an unknown kind there means NONE.
 *
 * slak_mixup_images = timm1/data/mixup.py:159-207 (_mix_elem, _mix_pair, _mix_batch): x[N][C][H][W] fp32, NCHW contiguous, mixed IN PLACE
 * without a copy of the batch -- the thread that owns an offset of image n owns the same offset of image N-1-n, loads both, then stores both.
 * No alignment of an image or of a box row is assumed.  ONE launch (none when a shared record leaves every image as it is).
 * Covers fp32, even 2 <= N <= 131070, C H W <= 2^28; anything else is SLAK_ERR_UNSUPPORTED, decided on the host before any launch.
 *
 * slak_mixup_targets = timm1/data/mixup.py:17-27 (one_hot, mixup_target): labels int64 [N] -> out fp32 [N][K] contiguous,
 *   out[n][k] = round(v(y_n, k) a_n) + round(v(y_{N-1-n}, k) b_n),   v(y, k) = on_value where k == y, off_value elsewhere
 * (the caller passes off = smoothing / K and on = 1 - smoothing + off, evaluated in double and rounded to fp32 once, as torch.full / scatter_
 * do).  ONE launch.  A label never forms an address: it is compared with the column index, so a label outside [0, K) matches no column and
 * its row holds off-values only -- torch's scatter_ raises a device-side assertion there instead.  Covers even N >= 2, K >= 1, N K <= 2^30. */
#define SLAK_MIXUP_NONE 0
#define SLAK_MIXUP_MIX 1
#define SLAK_MIXUP_CUTMIX 2
typedef struct {
    int kind;                /* SLAK_MIXUP_*                                                   */
    float a, b;              /* coefficient of the image's own values / label, of its partner's */
    int yl, yh, xl, xh;      /* the CutMix box: rows [yl, yh), columns [xl, xh)                */
} slak_mixup_record_t;
int slak_mixup_images_supported(int x_dtype, int N, int C, int H, int W);
int slak_mixup_images(void* x, int x_dtype, const slak_mixup_record_t* shared_host, const slak_mixup_record_t* table_dev,
                      int N, int C, int H, int W, void* stream);
int slak_mixup_targets_supported(int N, int K);
int slak_mixup_targets(const long long* labels, const slak_mixup_record_t* shared_host, const slak_mixup_record_t* table_dev,
                       float on_value, float off_value, float* out, int N, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLAK_HIP_H */
