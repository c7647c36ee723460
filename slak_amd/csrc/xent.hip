// slak_amd/csrc/xent.hip -- the criterion of the training step (main.py:398-403): cross-entropy with hard labels (+ label smoothing, ignore_index:
// nn.CrossEntropyLoss, timm1/loss/cross_entropy.py:20-26) or soft targets (timm1/loss/cross_entropy.py:34-36), reduction 'mean'; forward and backward one
// launch each (include/slak_hip.h).
//
// One workgroup per row.  The row is read ONCE: every lane keeps a running maximum and the sum of exp(x - maximum) of its share (rescaled when the
// maximum moves), the workgroup combines the pairs.  16-byte loads between a scalar head and tail -- row n starts at n * row_stride elements, aligned
// only when the stride allows it (K = 1001, 21841: it does not).  The label NEVER forms an address: x_y is the element whose index compares equal to y
// while the row streams by, so a label outside [0, K) reads nothing.  The mean over the rows: every workgroup writes its row's loss through to the
// coherence point and arrives at a counter; the last one adds the N values in a fixed order (wgrad_finish of slak_common.h: the hand-off the
// weight-gradient kernels run) -- no floating-point atomics, the same bits every run.
#include <math.h>

#include "head_common.h"

namespace slak {

constexpr int XE_T = 256, XE_MAX_K = 32768;

typedef unsigned short xe_us8 __attribute__((ext_vector_type(8)));
typedef _Float16 xe_h8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void xe_load_vec(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void xe_load_vec(const bf16_t* p, float (&v)[8]) {
    const xe_us8 t = *reinterpret_cast<const xe_us8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = __uint_as_float((uint32_t)t[j] << 16);
}
__device__ __forceinline__ void xe_load_vec(const f16_t* p, float (&v)[8]) {
    const xe_h8 t = *reinterpret_cast<const xe_h8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
}
__device__ __forceinline__ void xe_store_vec(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void xe_store_vec(bf16_t* p, const float (&v)[8]) {
    xe_us8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = f32_to_bf16_bits(v[j]);
    *reinterpret_cast<xe_us8*>(p) = t;
}
__device__ __forceinline__ void xe_store_vec(f16_t* p, const float (&v)[8]) {
    xe_h8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (f16_t)v[j];
    *reinterpret_cast<xe_h8*>(p) = t;
}

// elements until `p` (aligned to its element size: checked on the host) reaches a 16-byte boundary, at most K
template <typename T>
__device__ __forceinline__ int xe_head(const T* p, int K) {
    const int h = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(T));
    return h < K ? h : K;
}

// f(k, x_k) for every k in [0, K), each k by exactly one thread of the workgroup
template <typename T, typename F>
__device__ __forceinline__ void xe_row_foreach(const T* __restrict__ row, int K, int tid, F&& f) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int h = xe_head(row, K), nv = (K - h) / VEC;
    if (tid < h) f(tid, to_f32(row[tid]));                       // h < VEC <= 8
    for (int v = tid; v < nv; v += XE_T) {
        const int k0 = h + v * VEC;                              // k0 + VEC <= h + nv * VEC <= K
        float x[VEC];
        xe_load_vec(row + k0, x);
#pragma unroll
        for (int j = 0; j < VEC; ++j) f(k0 + j, x[j]);
    }
    for (int k = h + nv * VEC + tid; k < K; k += XE_T) f(k, to_f32(row[k]));
}

// part[0 .. N): the rows' losses, part[N .. 2N): 1 for a row that counts, 0 for an ignored one; added in a fixed order
__device__ __forceinline__ void xe_mean_finish(const float* part, int N, float* loss, float* count, float* red, int tid) {
    float a[2] = {0.f, 0.f};
    for (int i = tid; i < N; i += XE_T) {
        a[0] += __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a[1] += __hip_atomic_load(part + N + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    hd_block_sum<2>(a, red, XE_T / 64);
    if (tid == 0) { loss[0] = a[0] / a[1]; count[0] = a[1]; }
}

template <typename T, bool SOFT>
__global__ __launch_bounds__(XE_T) void xent_fwd_kernel(const T* __restrict__ logits, long long row_stride, const long long* __restrict__ labels,
                                                        const float* __restrict__ soft, float smoothing, long long ignore_index,
                                                        float* __restrict__ loss, float* __restrict__ lse, float* __restrict__ count,
                                                        float* part, unsigned* counter, int finish, int N, int K) {
    __shared__ float red[3 * 16];
    __shared__ int last_flag;
    const int n = blockIdx.x, tid = threadIdx.x;
    const T* row = logits + (size_t)n * (size_t)row_stride;
    const float* trow = SOFT ? soft + (size_t)n * K : nullptr;
    const long long y = SOFT ? 0 : labels[n];
    float m = -INFINITY, s = 0.f, u = 0.f, w = 0.f;             // hard: u = sum x, w = x_y; soft: u = sum t, w = sum t x
    xe_row_foreach(row, K, tid, [&](int k, float x) {
        if (x > m) { s = s * expf(m - x) + 1.f; m = x; }         // (m = -inf: s = 0 * 0 + 1)
        else if (m > -INFINITY) s += expf(x - m);
        if (SOFT) { const float t = trow[k]; u += t; w += t * x; }
        else { u += x; if ((long long)k == y) w = x; }
    });
    const float M = hd_block_max(m, red, XE_T / 64);
    float a[3] = {m > -INFINITY ? s * expf(m - M) : 0.f, u, w};
    hd_block_sum<3>(a, red, XE_T / 64);
    if (tid == 0) {
        const float l = M + logf(a[0]);
        float li, valid = 1.f;
        if (SOFT) li = l * a[1] - a[2];
        else if (y == ignore_index) { li = 0.f; valid = 0.f; }
        else li = (1.f - smoothing) * (l - a[2]) + smoothing * (l - a[1] / (float)K);
        lse[n] = l;
        wgrad_store_partial(part + n, li);
        wgrad_store_partial(part + N + n, valid);
    }
    if (!finish) return;                                         // no arrival counters: the launcher runs xent_finish_kernel behind this one
    wgrad_finish(part, nullptr, counter, &last_flag, N, 0, 0, 0, 0, tid, XE_T);    // arrival only: nothing for it to sum (nch * ntap = 0); N = 1 touches no counter
    if (!last_flag) return;
    xe_mean_finish(part, N, loss, count, red, tid);
}

__global__ __launch_bounds__(XE_T) void xent_finish_kernel(const float* part, int N, float* loss, float* count) {
    __shared__ float red[2 * 16];
    xe_mean_finish(part, N, loss, count, red, threadIdx.x);
}

template <typename T, bool SOFT>
__global__ __launch_bounds__(XE_T) void xent_bwd_kernel(const T* __restrict__ logits, long long row_stride, const long long* __restrict__ labels,
                                                        const float* __restrict__ soft, float smoothing, long long ignore_index,
                                                        const float* __restrict__ lse, const float* __restrict__ count, const float* __restrict__ grad_out,
                                                        T* __restrict__ dlogits, int N, int K) {
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ float red[16];
    const int n = blockIdx.x, tid = threadIdx.x;
    const T* row = logits + (size_t)n * (size_t)row_stride;
    T* out = dlogits + (size_t)n * K;
    const float* trow = SOFT ? soft + (size_t)n * K : nullptr;
    const long long y = SOFT ? 0 : labels[n];
    const bool ignored = !SOFT && y == ignore_index;             // workgroup-uniform
    const float l = lse[n], scale = grad_out[0] / count[0];
    float tsum = 0.f;
    if (SOFT) {
        float a[1] = {0.f};
        for (int k = tid; k < K; k += XE_T) a[0] += trow[k];
        hd_block_sum<1>(a, red, XE_T / 64);
        tsum = a[0];
    }
    const float keep = 1.f - smoothing, floor_k = smoothing / (float)K;
    auto d = [&](int k, float x) -> float {
        if (ignored) return 0.f;
        const float p = expf(x - l);
        if (SOFT) return scale * (p * tsum - trow[k]);
        return scale * (p - ((long long)k == y ? keep : 0.f) - floor_k);
    };
    // the 16-byte pieces follow the alignment of the OUTPUT row; the logits are read 16 bytes at a time where that lands aligned as well
    const int h = xe_head(out, K), nv = (K - h) / VEC;
    const bool in_vec = (((uintptr_t)(row + h)) & 15u) == 0;
    if (tid < h) out[tid] = from_f32<T>(d(tid, to_f32(row[tid])));
    for (int v = tid; v < nv; v += XE_T) {
        const int k0 = h + v * VEC;                              // k0 + VEC <= K
        float x[VEC];
        if (in_vec) xe_load_vec(row + k0, x);
        else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) x[j] = to_f32(row[k0 + j]);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) x[j] = d(k0 + j, x[j]);
        xe_store_vec(out + k0, x);
    }
    for (int k = h + nv * VEC + tid; k < K; k += XE_T) out[k] = from_f32<T>(d(k, to_f32(row[k])));
}

static int xe_supported(int dt, int N, int K) { return dtype_ok(dt) && N >= 1 && K >= 1 && K <= XE_MAX_K; }

static int xe_check(const void* logits, int dt, long long row_stride, const void* labels, const void* soft, float smoothing, int N, int K) {
    if (!logits || (labels == nullptr) == (soft == nullptr)) return SLAK_ERR_INVALID_ARG;
    if (N <= 0 || K <= 0 || !dtype_ok(dt) || !(smoothing >= 0.f && smoothing < 1.f)) return SLAK_ERR_INVALID_ARG;
    if (N > 1 && row_stride < K) return SLAK_ERR_INVALID_ARG;
    if (((uintptr_t)logits % dtype_size(dt)) != 0 || (soft && ((uintptr_t)soft & 3) != 0)) return SLAK_ERR_INVALID_ARG;
    if (!xe_supported(dt, N, K)) return SLAK_ERR_UNSUPPORTED;
    return SLAK_OK;
}

}  // namespace slak

using namespace slak;

extern "C" {

int slak_xent_supported(int logits_dtype, int N, int K) { return xe_supported(logits_dtype, N, K); }

size_t slak_xent_workspace_bytes(int N, int K) {
    if (N <= 0 || K <= 0) return 0;
    return align_up((size_t)N * 2 * sizeof(float), 256);
}

int slak_xent_forward(const void* logits, int logits_dtype, long long row_stride, const long long* labels, const float* soft_targets,
                      float smoothing, long long ignore_index, float* loss, float* lse, float* count, int N, int K,
                      void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = xe_check(logits, logits_dtype, row_stride, labels, soft_targets, smoothing, N, K);
    if (rc != SLAK_OK) return rc;
    if (!loss || !lse || !count) return SLAK_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < slak_xent_workspace_bytes(N, K)) return SLAK_ERR_WORKSPACE;
    float* part = (float*)workspace;
    unsigned* counter = N > 1 ? wgrad_arrival_counters(1) : nullptr;
    const int finish = N == 1 || counter != nullptr;
    hipStream_t st = (hipStream_t)stream;
#define SLAK_XE_FWD(T)                                                                                                                        \
    do {                                                                                                                                      \
        if (soft_targets) hipLaunchKernelGGL((xent_fwd_kernel<T, true>), dim3((unsigned)N), dim3(XE_T), 0, st, (const T*)logits, row_stride, labels, \
                                             soft_targets, smoothing, ignore_index, loss, lse, count, part, counter, finish, N, K);                   \
        else hipLaunchKernelGGL((xent_fwd_kernel<T, false>), dim3((unsigned)N), dim3(XE_T), 0, st, (const T*)logits, row_stride, labels,      \
                                soft_targets, smoothing, ignore_index, loss, lse, count, part, counter, finish, N, K);                                \
    } while (0)
    if (logits_dtype == SLAK_F32) SLAK_XE_FWD(float);
    else if (logits_dtype == SLAK_BF16) SLAK_XE_FWD(bf16_t);
    else SLAK_XE_FWD(f16_t);
#undef SLAK_XE_FWD
    SLAK_LAUNCH_CHECK();
    if (!finish) {                                               // no arrival counters (SLAK_WGRAD_REDUCE=1, or none could be allocated): a second launch
        hipLaunchKernelGGL(xent_finish_kernel, dim3(1), dim3(XE_T), 0, st, part, N, loss, count);
        SLAK_LAUNCH_CHECK();
    }
    return SLAK_OK;
}

int slak_xent_backward(const void* logits, int logits_dtype, long long row_stride, const long long* labels, const float* soft_targets,
                       float smoothing, long long ignore_index, const float* lse, const float* count, const float* grad_out,
                       void* dlogits, int N, int K, void* stream) {
    const int rc = xe_check(logits, logits_dtype, row_stride, labels, soft_targets, smoothing, N, K);
    if (rc != SLAK_OK) return rc;
    if (!lse || !count || !grad_out || !dlogits) return SLAK_ERR_INVALID_ARG;
    if (((uintptr_t)dlogits % dtype_size(logits_dtype)) != 0) return SLAK_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
#define SLAK_XE_BWD(T)                                                                                                                        \
    do {                                                                                                                                      \
        if (soft_targets) hipLaunchKernelGGL((xent_bwd_kernel<T, true>), dim3((unsigned)N), dim3(XE_T), 0, st, (const T*)logits, row_stride, labels, \
                                             soft_targets, smoothing, ignore_index, lse, count, grad_out, (T*)dlogits, N, K);                 \
        else hipLaunchKernelGGL((xent_bwd_kernel<T, false>), dim3((unsigned)N), dim3(XE_T), 0, st, (const T*)logits, row_stride, labels,      \
                                soft_targets, smoothing, ignore_index, lse, count, grad_out, (T*)dlogits, N, K);                              \
    } while (0)
    if (logits_dtype == SLAK_F32) SLAK_XE_BWD(float);
    else if (logits_dtype == SLAK_BF16) SLAK_XE_BWD(bf16_t);
    else SLAK_XE_BWD(f16_t);
#undef SLAK_XE_BWD
    SLAK_LAUNCH_CHECK();
    return SLAK_OK;
}

}  // extern "C"
