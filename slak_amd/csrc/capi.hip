// slak_amd/csrc/capi.hip -- extern "C" entry points of libslak_hip.so (see include/slak_hip.h).
// Argument validation lives here; the reference's extension validates almost nothing and exit()s on
// failure (forward_fp32.cu:173-196).  Every function returns a status code instead.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>

#include "slak_common.h"

namespace slak {
static std::mutex g_err_mu;
static std::string g_last_hip_error = "";
static std::atomic<int> g_conv_algo{SLAK_ALGO_AUTO};     // process-wide A/B switch (tests); read once per call
thread_local const char* g_last_kernel = "";           // slak_debug_last_kernel()
#define SLAK_RAN(name, call) (slak::g_last_kernel = (name), (call))
static constexpr int MF_TAPS_HOST = 5;        // the short side the MFMA kernels are written for
// A/B switches of the dispatch below (the kernels' own switches live in their *_supported() predicates)
static bool use_small_dma() { static const bool v = slak_env_flag("SLAK_MFMA_SMALL_DMA", true); return v; }   // 0 keeps the channel-blocked small-plane kernel
static bool use_vrows_pair() { static const bool v = slak_env_flag("SLAK_VROWS_PAIR", true); return v; }      // 0: the 56 x 56 class keeps separate K x 5 and 5 x 5 weight-gradient launches
static bool use_vrows() { static const bool v = slak_env_flag("SLAK_MFMA_VROWS", true); return v; }           // 0 keeps the transposing vertical weight-gradient kernel
static bool use_small() { static const bool v = slak_env_flag("SLAK_MFMA_SMALL", true); return v; }           // 0 keeps the generic register-staged kernel for H,W <= 16
static bool use_dma() { static const bool v = slak_env_flag("SLAK_MFMA_DMA", true); return v; }               // 0 keeps the register-staged MFMA kernels

void set_last_hip_error(hipError_t e) {
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_last_hip_error = hipGetErrorString(e);
}

static int check_conv_args(const void* a, const void* b, const void* c, int dt0, int dt1, int dt2,
                           int N, int C, int H, int W, int kh, int kw) {
    if (!a || !b || !c) return SLAK_ERR_INVALID_ARG;
    if (!dtype_ok(dt0) || !dtype_ok(dt1) || !dtype_ok(dt2)) return SLAK_ERR_INVALID_ARG;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0) return SLAK_ERR_INVALID_ARG;
    if ((kh & 1) == 0 || (kw & 1) == 0) return SLAK_ERR_INVALID_ARG;   // output shape == input shape needs odd kernels
    if ((long long)N * C * H * W >= (1LL << 31)) return SLAK_ERR_UNSUPPORTED;
    if (kh > 127 || kw > 127) return SLAK_ERR_UNSUPPORTED;
    return SLAK_OK;
}
}  // namespace slak

using namespace slak;

namespace slak { extern unsigned long long* g_dma_dbg; }

extern "C" {

/* dev hook (not in the public header): device buffer of 4x8 u64 that workgroup 0 of the DMA conv kernel fills with per-phase cycle counts */
void slak_debug_set_phase_buffer(void* p) { slak::g_dma_dbg = (unsigned long long*)p; }
/* dev hook (tests/test_dispatch_gpu.py): the name of the kernel family the calling thread's last conv / mask entry point launched -- a support
 * predicate that regresses lands a shape on a slower kernel with parity intact; this is what the dispatch tests pin */
const char* slak_debug_last_kernel(void) { return slak::g_last_kernel; }

// An empty launch whose GRID SIZE carries an id: profiling tools cut a kernel trace at these (tools/step_breakdown.py takes exactly the
// dispatches between marker 1 and marker 2 of bench.py --markers: the K timed steps, nothing else)
namespace slak { __global__ void marker_kernel(int id) { (void)id; } }
int slak_debug_marker(int id, void* stream) {
    if (id < 0 || id > 65535) return SLAK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(slak::marker_kernel, dim3((unsigned)(id + 1)), dim3(64), 0, (hipStream_t)stream, id);
    SLAK_LAUNCH_CHECK();
    return SLAK_OK;
}

const char* slak_status_string(int status) {
    switch (status) {
        case SLAK_OK: return "ok";
        case SLAK_ERR_INVALID_ARG: return "invalid argument";
        case SLAK_ERR_UNSUPPORTED: return "unsupported dtype/shape";
        case SLAK_ERR_WORKSPACE: return "workspace missing or too small";
        case SLAK_ERR_LAUNCH: return "HIP launch/runtime error";
        case SLAK_ERR_NO_DEVICE: return "no HIP device";
    }
    return "unknown status";
}

const char* slak_last_hip_error(void) {
    std::lock_guard<std::mutex> lk(g_err_mu);
    static thread_local std::string copy;
    copy = g_last_hip_error;
    return copy.c_str();
}

int slak_version(void) { return SLAK_ABI_VERSION; }

int slak_device_info(int* cu_count, int* lds_bytes_per_cu, char* arch_name, size_t arch_name_len) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return SLAK_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return SLAK_ERR_NO_DEVICE;
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (lds_bytes_per_cu) *lds_bytes_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    if (arch_name && arch_name_len) {
        size_t i = 0;
        for (; i + 1 < arch_name_len && prop.gcnArchName[i]; ++i) arch_name[i] = prop.gcnArchName[i];
        arch_name[i] = 0;
    }
    return SLAK_OK;
}

// fp32 tensors on the bf16 matrix cores (two-term split, ~2^-16 relative per product) are OPT-IN, like torch.backends.cudnn.allow_tf32:
// the default fp32 path stays the exact VALU one.  SLAK_FP32_MFMA=1 sets the initial value.
static std::atomic<int> g_fp32_mfma{slak_env_flag("SLAK_FP32_MFMA", false) ? 1 : 0};
static thread_local int t_fp32_mfma = -1;                    // per-thread override: -1 follow the process-wide setting, 0 exact, 1 matrix cores
static bool f32_ok(int dt) {
    if (dt != SLAK_F32 || g_conv_algo == SLAK_ALGO_MFMA) return true;
    return t_fp32_mfma >= 0 ? t_fp32_mfma != 0 : g_fp32_mfma.load() != 0;
}
int slak_set_fp32_matrix_cores(int allow) { g_fp32_mfma = allow ? 1 : 0; return SLAK_OK; }
int slak_get_fp32_matrix_cores(void) { return g_fp32_mfma.load(); }                            // the PROCESS-WIDE switch (what a save / restore pair wants)
int slak_get_fp32_matrix_cores_effective(void) { return t_fp32_mfma >= 0 ? t_fp32_mfma : g_fp32_mfma.load(); }   // what a call on THIS thread would do
int slak_set_fp32_matrix_cores_thread(int mode, int* previous) {
    if (mode < -1 || mode > 1) return SLAK_ERR_INVALID_ARG;
    if (previous) *previous = t_fp32_mfma;
    t_fp32_mfma = mode;
    return SLAK_OK;
}

int slak_set_conv_algo(int algo) {
    if (algo != SLAK_ALGO_AUTO && algo != SLAK_ALGO_DIRECT && algo != SLAK_ALGO_MFMA) return SLAK_ERR_INVALID_ARG;
    g_conv_algo = algo;
    return SLAK_OK;
}

// The maximum over every family of the operation, not the size for the family that would run
size_t slak_dwconv2d_workspace_bytes(int op, int N, int C, int H, int W, int kh, int kw, int dtype) {
    (void)dtype;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0) return 0;
    ConvDims d{N, C, H, W, kh, kw};
    if (op == 0 || op == 1) return std::max({dwconv_direct_workspace(d), dwconv_mfma_workspace(d), dwconv_mfma_small_workspace(d)});
    if (op == 2)
        return std::max({dwconv_wgrad_workspace(d), dwconv_mfma_wgrad_workspace(d), dwconv_mfma_wgrad_dma_workspace(d), dwconv_mfma_small_wgrad_workspace(d),
                         dwconv_mfma_small_wgrad_dma_workspace(d), dwconv_mfma_wgrad_vrows_workspace(d), dwconv_mfma_wide_wgrad_workspace(d),
                         dwconv_mfma_wgrad_vwave_workspace(d)});
    return 0;
}

// "The LDS-DMA ring kernel runs this call": the ladder's first rung, and the only kernel behind the accumulating and the statistics entry points
static bool dma_ring_usable(const ConvDims& d, int in_dtype, int w_dtype, int out_dtype) {
    return g_conv_algo != SLAK_ALGO_DIRECT && use_dma() && dwconv_mfma_dma_supported(d, in_dtype, w_dtype, out_dtype);
}

// The per-branch forward (flip = false) and data gradient (flip = true): the first family whose predicate accepts the shape, in this order.  (The data gradient of a
// stride-1 "same" cross-correlation with odd kernels == cross-correlation of dy with the filter rotated by 180 degrees: h + kh/2 - r == h - kh/2 + (kh-1-r).)
static int conv_or_data_gradient(bool flip, const void* in, int in_dtype, const void* w, int w_dtype, void* out, int out_dtype,
                                 int N, int C, int H, int W, int kh, int kw, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_conv_args(in, w, out, in_dtype, w_dtype, out_dtype, N, C, H, W, kh, kw);
    if (rc != SLAK_OK) return rc;
    ConvDims d{N, C, H, W, kh, kw};
    const hipStream_t st = (hipStream_t)stream;
    const int algo = g_conv_algo;
    if (dma_ring_usable(d, in_dtype, w_dtype, out_dtype))
        return SLAK_RAN("dwconv_mfma_dma", launch_dwconv_mfma_dma(in, in_dtype, w, w_dtype, out, out_dtype, d, flip, workspace, workspace_bytes, st));
    if (algo != SLAK_ALGO_DIRECT) {
        if (dwconv_mfma_wide_supported(d, in_dtype, w_dtype, out_dtype))
            return SLAK_RAN("dwconv_mfma_wide", launch_dwconv_mfma_wide(in, in_dtype, w, w_dtype, out, out_dtype, d, flip, st));
        if (use_small_dma() && dwconv_mfma_small_dma_supported(d, in_dtype, w_dtype, out_dtype))
            return SLAK_RAN("dwconv_mfma_small_dma", launch_dwconv_mfma_small_dma(in, in_dtype, w, w_dtype, out, out_dtype, d, flip, st));
        if (use_small() && dwconv_mfma_small_supported(d, in_dtype, w_dtype, out_dtype))
            return SLAK_RAN("dwconv_mfma_small", launch_dwconv_mfma_small(in, in_dtype, w, w_dtype, out, out_dtype, d, flip, workspace, workspace_bytes, st));
        if (f32_ok(in_dtype) && dwconv_mfma_supported(d, in_dtype, w_dtype, out_dtype))
            return SLAK_RAN(in_dtype == SLAK_F32 ? "dwconv_mfma(f32 split)" : "dwconv_mfma",
                            launch_dwconv_mfma(in, in_dtype, w, w_dtype, out, out_dtype, d, flip, workspace, workspace_bytes, st));
    }
    if (algo == SLAK_ALGO_MFMA) return SLAK_ERR_UNSUPPORTED;
    return SLAK_RAN("dwconv_direct", launch_dwconv_direct(in, in_dtype, w, w_dtype, out, out_dtype, d, flip, workspace, workspace_bytes, st));
}

int slak_dwconv2d_forward(const void* x, int x_dtype, const void* w, int w_dtype, void* y, int y_dtype,
                          int N, int C, int H, int W, int kh, int kw, void* workspace, size_t workspace_bytes, void* stream) {
    return conv_or_data_gradient(/*flip=*/false, x, x_dtype, w, w_dtype, y, y_dtype, N, C, H, W, kh, kw, workspace, workspace_bytes, stream);
}

int slak_dwconv2d_backward_data(const void* dy, int dy_dtype, const void* w, int w_dtype, void* dx, int dx_dtype,
                                int N, int C, int H, int W, int kh, int kw, void* workspace, size_t workspace_bytes, void* stream) {
    return conv_or_data_gradient(/*flip=*/true, dy, dy_dtype, w, w_dtype, dx, dx_dtype, N, C, H, W, kh, kw, workspace, workspace_bytes, stream);
}

int slak_dwconv2d_backward_data_accumulate(const void* dy, int dy_dtype, const void* w, int w_dtype, void* dx, int dx_dtype,
                                           int N, int C, int H, int W, int kh, int kw, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_conv_args(dy, w, dx, dy_dtype, w_dtype, dx_dtype, N, C, H, W, kh, kw);
    if (rc != SLAK_OK) return rc;
    ConvDims d{N, C, H, W, kh, kw};
    if (!dma_ring_usable(d, dy_dtype, w_dtype, dx_dtype)) return SLAK_ERR_UNSUPPORTED;            // the caller computes into a temporary and adds
    return SLAK_RAN("dwconv_mfma_dma", launch_dwconv_mfma_dma(dy, dy_dtype, w, w_dtype, dx, dx_dtype, d, /*flip=*/true, workspace, workspace_bytes, (hipStream_t)stream, /*accumulate=*/true));
}

/* slak_dwconv2d_forward that also leaves the batch statistics of the BatchNorm behind the conv (models/SLaK.py:38-47 conv -> bn):
 * stats[rows][C][2] = partial (sum y, sum y^2) of the stored outputs; *stats_rows = rows written (<= 4 N = the capacity the caller must
 * provide).  Only the LDS-DMA ring kernel (56 x 56 / 28 x 28 class) gathers them; SLAK_ERR_UNSUPPORTED otherwise (use slak_dwconv2d_forward). */
int slak_dwconv2d_forward_stats(const void* x, int x_dtype, const void* w, int w_dtype, void* y, int y_dtype, float* stats, int stats_capacity_rows,
                                int* stats_rows, int N, int C, int H, int W, int kh, int kw, void* stream) {
    int rc = check_conv_args(x, w, y, x_dtype, w_dtype, y_dtype, N, C, H, W, kh, kw);
    if (rc != SLAK_OK) return rc;
    if (!stats || !stats_rows) return SLAK_ERR_INVALID_ARG;
    ConvDims d{N, C, H, W, kh, kw};
    if (x_dtype != SLAK_BF16 || !dma_ring_usable(d, x_dtype, w_dtype, y_dtype)) return SLAK_ERR_UNSUPPORTED;
    return SLAK_RAN("dwconv_mfma_dma", launch_dwconv_mfma_dma(x, x_dtype, w, w_dtype, y, y_dtype, d, /*flip=*/false, nullptr, 0, (hipStream_t)stream, /*accumulate=*/false,
                                                         stats, stats_capacity_rows, stats_rows));
}

// The per-branch weight gradient: the same rule.  Only small_wgrad_dma, wgrad_vrows and wgrad_vwave go on to the next rung when their launcher refuses the shape after all.
int slak_dwconv2d_backward_filter(const void* dy, int dy_dtype, const void* x, int x_dtype, float* dw,
                                  int N, int C, int H, int W, int kh, int kw, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_conv_args(dy, x, dw, dy_dtype, x_dtype, SLAK_F32, N, C, H, W, kh, kw);
    if (rc != SLAK_OK) return rc;
    ConvDims d{N, C, H, W, kh, kw};
    const hipStream_t st = (hipStream_t)stream;
    const int algo = g_conv_algo;
    if (algo != SLAK_ALGO_DIRECT) {
        if (use_small_dma() && dwconv_mfma_small_wgrad_dma_supported(d, dy_dtype, x_dtype)) {
            rc = SLAK_RAN("dwconv_mfma_small_wgrad_dma", launch_dwconv_mfma_small_wgrad_dma(dy, dy_dtype, x, x_dtype, dw, d, workspace, workspace_bytes, st));
            if (rc != SLAK_ERR_UNSUPPORTED) return rc;
        }
        if (use_small() && dwconv_mfma_small_wgrad_supported(d, dy_dtype, x_dtype))
            return SLAK_RAN("dwconv_mfma_small_wgrad", launch_dwconv_mfma_small_wgrad(dy, dy_dtype, x, x_dtype, dw, d, workspace, workspace_bytes, st));
        if (use_dma() && use_vrows() && dwconv_mfma_wgrad_vrows_supported(d, dy_dtype, x_dtype)) {
            rc = SLAK_RAN("dwconv_mfma_wgrad_vrows", launch_dwconv_mfma_wgrad_vrows(dy, dy_dtype, x, x_dtype, dw, d, workspace, workspace_bytes, st));
            if (rc != SLAK_ERR_UNSUPPORTED) return rc;
        }
        if (use_dma() && dwconv_mfma_wgrad_vwave_supported(d, dy_dtype, x_dtype)) {     // vertical, planes of <= 32 rows
            rc = SLAK_RAN("dwconv_mfma_wgrad_vwave", launch_dwconv_mfma_wgrad_vwave(dy, dy_dtype, x, x_dtype, dw, d, workspace, workspace_bytes, st));
            if (rc != SLAK_ERR_UNSUPPORTED) return rc;
        }
        if (use_dma() && dwconv_mfma_wgrad_dma_supported(d, dy_dtype, x_dtype))
            return SLAK_RAN("dwconv_mfma_wgrad_dma", launch_dwconv_mfma_wgrad_dma(dy, dy_dtype, x, x_dtype, dw, d, workspace, workspace_bytes, st));
        if (dwconv_mfma_wide_wgrad_supported(d, dy_dtype, x_dtype))
            return SLAK_RAN("dwconv_mfma_wide_wgrad", launch_dwconv_mfma_wide_wgrad(dy, dy_dtype, x, x_dtype, dw, d, workspace, workspace_bytes, st));
        if (f32_ok(x_dtype) && dwconv_mfma_wgrad_supported(d, dy_dtype, x_dtype))
            return SLAK_RAN(x_dtype == SLAK_F32 ? "dwconv_mfma_wgrad(f32 split)" : "dwconv_mfma_wgrad",
                            launch_dwconv_mfma_wgrad(dy, dy_dtype, x, x_dtype, dw, d, workspace, workspace_bytes, st));
    }
    if (algo == SLAK_ALGO_MFMA) return SLAK_ERR_UNSUPPORTED;
    return SLAK_RAN("dwconv_wgrad", launch_dwconv_wgrad(dy, dy_dtype, x, x_dtype, dw, d, workspace, workspace_bytes, st));
}

/* One launch for the three branches of a block.  WHICH kernel exists for (op, shape) is decided here and nowhere else: the first family whose
 * predicate accepts the shape, in this order (the stream kernel is forward only).  The queries below do not consult slak_set_conv_algo or
 * SLAK_MFMA_DMA: callers cache their answers per shape for the life of the process. */
enum TriKernel { TRI_NONE, TRI_SMALL, TRI_STREAM, TRI_WIDE, TRI_TEAM };
// ... with the last rung unasked (TRI_TEAM: "the team kernel, if any"): what the launch entry points use, because the team launcher asks its own predicate
static TriKernel tri_kernel_or_team(bool dgrad, int dtype, int N, int C, int H, int W, int K) {
    if (dwconv_mfma_small_tri_supported(N, C, H, W, K, dtype)) return TRI_SMALL;                   // planes up to 16 x 16 (14 x 14, 7 x 7 stages): wave-independent
    if (!dgrad && dwconv_mfma_stream_tri_supported(N, C, H, W, K, dtype)) return TRI_STREAM;       // planes of 2 x 2 tiles, forward: one MFMA stream per wave
    if (dwconv_mfma_wide_tri_supported(N, C, H, W, K, dtype, dgrad)) return TRI_WIDE;              // round 6: maps with 64 < H, W <= 96 (96 x 96: SLaK at 384 px)
    return TRI_TEAM;                                                                               // planes of one tile or 2 x 2 tiles: four-wave teams
}
static TriKernel tri_kernel(bool dgrad, int dtype, int N, int C, int H, int W, int K) {
    const TriKernel k = tri_kernel_or_team(dgrad, dtype, N, C, H, W, K);
    return (k == TRI_TEAM && !dwconv_mfma_team_tri_supported(N, C, H, W, K, dtype, dgrad)) ? TRI_NONE : k;
}
/* Whether the measurements say the kernel that exists should be used (MI355X, profiles/r03_*): the team kernels only on planes of one MFMA tile
 * (17..32: 28 x 28, 24 x 24), and on planes of 2 x 2 tiles (33..64: 56 x 56, 48 x 48) for the data gradient (117 vs 134 us for plain + 2
 * accumulating launches at 128 x 96 x 56 x 56); without the stream kernel the forward there stays three launches (108 vs 122 us). */
static bool tri_kernel_preferred(TriKernel k, bool dgrad, int H, int W) {
    if (k != TRI_TEAM) return k != TRI_NONE;
    static const bool all = [] { const char* e = slak_dev_getenv("SLAK_TEAM_ALL"); return e && e[0] == '1'; }();     // A/B: team kernels wherever they exist
    return (H <= 32 && W <= 32) || dgrad || all;
}

/* op 0 forward, 1 backward_data.  1: use the three-branch entry point; 0: run the per-branch entry points. */
int slak_dwconv2d_tri_supported_op(int dtype, int N, int C, int H, int W, int K, int op) {
    if (op != 0 && op != 1) return 0;
    return tri_kernel_preferred(tri_kernel(op == 1, dtype, N, C, H, W, K), op == 1, H, W) ? 1 : 0;
}
/* both ops (the merged inference block, callers that want all or nothing) */
int slak_dwconv2d_tri_supported(int dtype, int N, int C, int H, int W, int K) {
    return (slak_dwconv2d_tri_supported_op(dtype, N, C, H, W, K, 0) && slak_dwconv2d_tri_supported_op(dtype, N, C, H, W, K, 1)) ? 1 : 0;
}

/* The launch entry points run whatever exists (preferred or not); SLAK_ERR_UNSUPPORTED on a shape with no kernel. */
static int tri_launch(TriKernel k, bool dgrad, const void* const* in, void* const* out, const float* const* w, float* stats,
                      int dtype, int N, int C, int H, int W, int K, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    switch (k) {
        case TRI_SMALL: return SLAK_RAN("dwconv_mfma_small_tri", launch_dwconv_mfma_small_tri(dgrad, in, out, w, dtype, N, C, H, W, K, st, stats));
        case TRI_STREAM: return SLAK_RAN("dwconv_mfma_stream_tri", launch_dwconv_mfma_stream_tri(in[0], out, w, dtype, N, C, H, W, K, st, stats));
        case TRI_WIDE: if (stats) return SLAK_ERR_UNSUPPORTED;                 // no statistics on wide maps
                       return SLAK_RAN("dwconv_mfma_wide_tri", launch_dwconv_mfma_wide_tri(dgrad, in, out, w, dtype, N, C, H, W, K, st));
        default: return SLAK_RAN("dwconv_mfma_team_tri", launch_dwconv_mfma_team_tri(dgrad, in, out, w, dtype, N, C, H, W, K, st, stats));
    }
}
int slak_dwconv2d_tri_forward(const void* x, const float* w_v, const float* w_h, const float* w_s, void* y_v, void* y_h, void* y_s,
                              int dtype, int N, int C, int H, int W, int K, void* stream) {
    if (!x || !w_v || !w_h || !w_s || !y_v || !y_h || !y_s) return SLAK_ERR_INVALID_ARG;
    const void* in[3] = {x, x, x}; void* out[3] = {y_v, y_h, y_s}; const float* w[3] = {w_v, w_h, w_s};
    return tri_launch(tri_kernel_or_team(false, dtype, N, C, H, W, K), false, in, out, w, nullptr, dtype, N, C, H, W, K, stream);
}
int slak_dwconv2d_tri_backward_data(const void* dy_v, const void* dy_h, const void* dy_s, const float* w_v, const float* w_h,
                                    const float* w_s, void* dx, int dtype, int N, int C, int H, int W, int K, void* stream) {
    if (!dy_v || !dy_h || !dy_s || !w_v || !w_h || !w_s || !dx) return SLAK_ERR_INVALID_ARG;
    const void* in[3] = {dy_v, dy_h, dy_s}; void* out[3] = {dx, dx, dx}; const float* w[3] = {w_v, w_h, w_s};
    return tri_launch(tri_kernel_or_team(true, dtype, N, C, H, W, K), true, in, out, w, nullptr, dtype, N, C, H, W, K, stream);
}

/* The forward three-branch launch that also leaves the branch BatchNorms' batch statistics: stats[rows][C][6] = per (row, channel) partial
 * sums (sum y_v, sum y_v^2, sum y_h, sum y_h^2, sum y_s, sum y_s^2) of the stored (rounded) outputs; rows = slak_dwconv2d_tri_stats_rows(...)
 * (0: this shape has no such kernel -- use slak_dwconv2d_tri_forward).  bf16 only.  The rows are those of the FIRST existing forward kernel,
 * also where that kernel gathers none (0: the small kernel on W < 8 outside the quad class, f16, the wide kernel): no falling through. */
static int tri_stats_rows(TriKernel k, int dtype, int N, int C, int H, int W, int K) {
    switch (k) {
        case TRI_SMALL: return dwconv_mfma_small_tri_stats_rows(N, C, H, W, K, dtype);
        case TRI_STREAM: return dwconv_mfma_stream_tri_stats_rows(N, C, H, W, K, dtype);
        case TRI_TEAM: return dwconv_mfma_team_tri_stats_rows(N, C, H, W, K, dtype);      // (0 where there is no team kernel either)
        case TRI_WIDE: default: return 0;                                     // the wide kernel gathers no statistics
    }
}
int slak_dwconv2d_tri_stats_rows(int dtype, int N, int C, int H, int W, int K) {
    return tri_stats_rows(tri_kernel_or_team(false, dtype, N, C, H, W, K), dtype, N, C, H, W, K);
}
int slak_dwconv2d_tri_forward_stats(const void* x, const float* w_v, const float* w_h, const float* w_s, void* y_v, void* y_h, void* y_s,
                                    float* stats, int dtype, int N, int C, int H, int W, int K, void* stream) {
    if (!x || !w_v || !w_h || !w_s || !y_v || !y_h || !y_s || !stats) return SLAK_ERR_INVALID_ARG;
    const TriKernel k = tri_kernel_or_team(false, dtype, N, C, H, W, K);
    if (tri_stats_rows(k, dtype, N, C, H, W, K) <= 0) return SLAK_ERR_UNSUPPORTED;
    const void* in[3] = {x, x, x}; void* out[3] = {y_v, y_h, y_s}; const float* w[3] = {w_v, w_h, w_s};
    return tri_launch(k, false, in, out, w, stats, dtype, N, C, H, W, K, stream);
}

/* The three weight gradients of a block's branches in one launch: which kernel, decided here and nowhere else */
enum TriWgradKernel { TRI_WGRAD_NONE, TRI_WGRAD_SMALL, TRI_WGRAD_ROWS, TRI_WGRAD_WAVE };
static TriWgradKernel tri_wgrad_kernel(int dtype, int N, int C, int H, int W, int K) {
    if (wgrad_reduce_forced()) return TRI_WGRAD_NONE;                                             // the one-launch kernels finish through the arrival counters only
    if (dwconv_mfma_small_tri_wgrad_supported(N, C, H, W, K, dtype)) return TRI_WGRAD_SMALL;
    if (dwconv_mfma_tri_wgrad_rows_supported(N, C, H, W, K, dtype)) return TRI_WGRAD_ROWS;        // planes of 2 x 2 tiles (56 x 56 class)
    if (dwconv_mfma_tri_wgrad_wave_supported(N, C, H, W, K, dtype)) return TRI_WGRAD_WAVE;        // planes of one tile (28 x 28 class)
    return TRI_WGRAD_NONE;
}

size_t slak_dwconv2d_tri_filter_workspace_bytes(int dtype, int N, int C, int H, int W, int K) {
    switch (tri_wgrad_kernel(dtype, N, C, H, W, K)) {
        case TRI_WGRAD_SMALL: return dwconv_mfma_small_tri_wgrad_workspace(N, C, K);
        case TRI_WGRAD_ROWS: return dwconv_mfma_tri_wgrad_rows_workspace(N, C, K);
        case TRI_WGRAD_WAVE: return dwconv_mfma_tri_wgrad_wave_workspace(N, C, K);
        default: return 0;
    }
}

int slak_dwconv2d_tri_backward_filter(const void* dy_v, const void* dy_h, const void* dy_s, const void* x, float* dw_v, float* dw_h,
                                      float* dw_s, int dtype, int N, int C, int H, int W, int K,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy_v || !dy_h || !dy_s || !x || !dw_v || !dw_h || !dw_s) return SLAK_ERR_INVALID_ARG;
    const void* dy[3] = {dy_v, dy_h, dy_s}; float* dw[3] = {dw_v, dw_h, dw_s};
    switch (tri_wgrad_kernel(dtype, N, C, H, W, K)) {
        case TRI_WGRAD_SMALL: return SLAK_RAN("dwconv_mfma_small_tri_wgrad", launch_dwconv_mfma_small_tri_wgrad(dy, x, dw, dtype, N, C, H, W, K, workspace, workspace_bytes, (hipStream_t)stream));
        case TRI_WGRAD_ROWS: return SLAK_RAN("dwconv_mfma_tri_wgrad_rows", launch_dwconv_mfma_tri_wgrad_rows(dy, x, dw, dtype, N, C, H, W, K, workspace, workspace_bytes, (hipStream_t)stream));
        case TRI_WGRAD_WAVE: return SLAK_RAN("dwconv_mfma_tri_wgrad_wave", launch_dwconv_mfma_tri_wgrad_wave(dy, x, dw, dtype, N, C, H, W, K, workspace, workspace_bytes, (hipStream_t)stream));
        default: return SLAK_ERR_UNSUPPORTED;
    }
}

/* Data gradient AND the three weight gradients of a block's branches in ONE launch (the 14 x 14 class: the dY planes are staged once for
 * both).  Same bits as slak_dwconv2d_tri_backward_data + slak_dwconv2d_tri_backward_filter; workspace: slak_dwconv2d_tri_filter_workspace_bytes. */
int slak_dwconv2d_tri_backward_supported(int dtype, int N, int C, int H, int W, int K) {
    return (!wgrad_reduce_forced() && dwconv_mfma_small_tri_bwd_supported(N, C, H, W, K, dtype)) ? 1 : 0;
}

int slak_dwconv2d_tri_backward(const void* dy_v, const void* dy_h, const void* dy_s, const void* x, const float* w_v, const float* w_h,
                               const float* w_s, void* dx, float* dw_v, float* dw_h, float* dw_s, int dtype, int N, int C, int H, int W, int K,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy_v || !dy_h || !dy_s || !x || !w_v || !w_h || !w_s || !dx || !dw_v || !dw_h || !dw_s) return SLAK_ERR_INVALID_ARG;
    const void* dy[3] = {dy_v, dy_h, dy_s}; float* dw[3] = {dw_v, dw_h, dw_s}; const float* w[3] = {w_v, w_h, w_s};
    return SLAK_RAN("dwconv_mfma_small_tri_bwd", launch_dwconv_mfma_small_tri_bwd(dy, x, w, dx, dw, dtype, N, C, H, W, K, workspace, workspace_bytes, (hipStream_t)stream));
}

/* The K x 5 and the 5 x 5 weight gradient of a block in ONE launch where the three-branch launch above does not reach (x and its five
 * column-shifted operands are shared: the 5 x 5 correlation is the K x 5 one with its own dY).  0 / SLAK_ERR_UNSUPPORTED: two calls.
 * Which kernel is decided here and nowhere else; the launch also honours the algo switch (slak_set_conv_algo can change between the query and
 * the launch), the size query does not. */
enum PairWgradKernel { PAIR_WGRAD_NONE, PAIR_WGRAD_VWAVE, PAIR_WGRAD_VROWS };
static PairWgradKernel pair_wgrad_kernel(const ConvDims& d, int dtype) {
    if (!use_dma() || wgrad_reduce_forced()) return PAIR_WGRAD_NONE;                              // (read once per process: a cached answer stays true)
    if (dwconv_mfma_wgrad_vwave_supported(d, dtype, dtype)) return PAIR_WGRAD_VWAVE;
    if (use_vrows() && use_vrows_pair() && dwconv_mfma_wgrad_vrows_supported(d, dtype, dtype)) return PAIR_WGRAD_VROWS;
    return PAIR_WGRAD_NONE;
}
size_t slak_dwconv2d_pair_filter_workspace_bytes(int dtype, int N, int C, int H, int W, int K) {
    ConvDims d{N, C, H, W, K, MF_TAPS_HOST};
    switch (pair_wgrad_kernel(d, dtype)) {
        case PAIR_WGRAD_VWAVE: return dwconv_mfma_wgrad_vwave_workspace(d);
        case PAIR_WGRAD_VROWS: return dwconv_mfma_wgrad_vrows_workspace(d);
        default: return 0;
    }
}
int slak_dwconv2d_pair_backward_filter(const void* dy_v, const void* dy_s, const void* x, float* dw_v, float* dw_s,
                                       int dtype, int N, int C, int H, int W, int K, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy_v || !dy_s || !x || !dw_v || !dw_s) return SLAK_ERR_INVALID_ARG;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 5) return SLAK_ERR_INVALID_ARG;
    ConvDims d{N, C, H, W, K, MF_TAPS_HOST};
    if (g_conv_algo == SLAK_ALGO_DIRECT) return SLAK_ERR_UNSUPPORTED;
    switch (pair_wgrad_kernel(d, dtype)) {
        case PAIR_WGRAD_VWAVE: return SLAK_RAN("dwconv_mfma_wgrad_vwave(pair)", launch_dwconv_mfma_wgrad_vwave(dy_v, dtype, x, dtype, dw_v, d, workspace, workspace_bytes, (hipStream_t)stream, dy_s, dw_s));
        case PAIR_WGRAD_VROWS: return SLAK_RAN("dwconv_mfma_wgrad_vrows(pair)", launch_dwconv_mfma_wgrad_vrows(dy_v, dtype, x, dtype, dw_v, d, workspace, workspace_bytes, (hipStream_t)stream, dy_s, dw_s));
        default: return SLAK_ERR_UNSUPPORTED;
    }
}

}  // extern "C"
