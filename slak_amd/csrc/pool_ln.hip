// slak_amd/csrc/pool_ln.hip -- global average pool + LayerNorm, the last line of SLaK.forward_features (models/SLaK.py: `self.norm(x.mean([-2, -1]))`),
// forward in one launch, backward in two (include/slak_hip.h).
//
// Forward: one workgroup per image.  A wave takes a channel at a time (eight in flight), a lane a pixel of its plane (lanes stride over planes of more
// than 64 pixels): scalar loads only, a plane starts wherever n * C * P + c * P puts it (7 x 7 planes are never 16-byte aligned).  The plane sums are taken
// of x - x[n][0][0]: at activations of 30 +- 1 a plain fp32 sum of 49 values is good to 1e-4 of 1470, which is 1.5e-5 of the normalised output once the
// LayerNorm has divided by the pooled spread of 1/7 -- the centred sum keeps every bit that matters, and LayerNorm does not see the shift.  Then the
// two-pass LayerNorm over the C values in LDS.
// Backward: the LayerNorm gradient of an image needs two sums over C (1536 loads out of L2), so every workgroup of the image recomputes them and then
// writes its share of dx: (image, channel slice) workgroups, dx written as one contiguous run with 16-byte stores between a scalar head and tail.
#include "head_common.h"

namespace slak {

constexpr int PL_MAX_C = 2048, PL_MAX_P = 1024, PL_U = 8;

template <typename TX, typename TY>
__global__ __launch_bounds__(1024) void pool_ln_fwd_kernel(const TX* __restrict__ x, const float* __restrict__ weight, const float* __restrict__ bias,
                                                           TY* __restrict__ y, float* __restrict__ pooled, float* __restrict__ mean,
                                                           float* __restrict__ rstd, int C, int P, float eps) {
    __shared__ float q[PL_MAX_C];
    __shared__ float red[16];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = wave_id_uniform(), nw = blockDim.x >> 6;
    const TX* xn = x + (size_t)n * C * P;
    const float pivot = to_f32(xn[0]);
    const float fP = (float)P;
    for (int c0 = wv; c0 < C; c0 += nw * PL_U) {
        float s[PL_U];
#pragma unroll
        for (int u = 0; u < PL_U; ++u) s[u] = 0.f;
        for (int p = lane; p < P; p += 64) {
            float v[PL_U];
#pragma unroll
            for (int u = 0; u < PL_U; ++u) {
                const int c = c0 + u * nw;
                v[u] = c < C ? to_f32(xn[(size_t)c * P + p]) : pivot;          // c < C, p < P: inside the image
            }
#pragma unroll
            for (int u = 0; u < PL_U; ++u) s[u] += v[u] - pivot;
        }
#pragma unroll
        for (int u = 0; u < PL_U; ++u) {
            const float t = hd_wave_sum(s[u]);
            const int c = c0 + u * nw;
            if (lane == 0 && c < C) q[c] = t / fP;
        }
    }
    __syncthreads();
    float a[1] = {0.f};
    for (int c = tid; c < C; c += blockDim.x) a[0] += q[c];
    hd_block_sum<1>(a, red, nw);
    const float mu = a[0] / (float)C;
    float b[1] = {0.f};
    for (int c = tid; c < C; c += blockDim.x) { const float d = q[c] - mu; b[0] += d * d; }
    hd_block_sum<1>(b, red, nw);
    const float r = 1.0f / sqrtf(b[0] / (float)C + eps);
    for (int c = tid; c < C; c += blockDim.x) {
        y[(size_t)n * C + c] = from_f32<TY>((q[c] - mu) * r * weight[c] + bias[c]);
        pooled[(size_t)n * C + c] = pivot + q[c];
    }
    if (tid == 0) { mean[n] = pivot + mu; rstd[n] = r; }
}

__device__ __forceinline__ void pl_store_vec(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void pl_store_vec(bf16_t* p, const float (&v)[8]) {
    uint4 o;
    o.x = f32_to_bf16_bits(v[0]) | ((uint32_t)f32_to_bf16_bits(v[1]) << 16);
    o.y = f32_to_bf16_bits(v[2]) | ((uint32_t)f32_to_bf16_bits(v[3]) << 16);
    o.z = f32_to_bf16_bits(v[4]) | ((uint32_t)f32_to_bf16_bits(v[5]) << 16);
    o.w = f32_to_bf16_bits(v[6]) | ((uint32_t)f32_to_bf16_bits(v[7]) << 16);
    *reinterpret_cast<uint4*>(p) = o;
}

// workgroup b: image b / S, channels [s * cs, min(C, (s + 1) * cs)) with s = b % S.  part[n][2 C]: dy * xhat, then dy (summed over n by pool_ln_reduce_kernel).
// vec: dx is 16-byte aligned at its start (then element e is aligned iff e % VEC == 0); 0: scalar stores throughout.
template <typename TX, typename TG>
__global__ __launch_bounds__(256) void pool_ln_bwd_kernel(const TG* __restrict__ dy, const float* __restrict__ pooled, const float* __restrict__ weight,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd, TX* __restrict__ dx,
                                                          float* __restrict__ part, int C, int P, int S, int cs, int vec) {
    constexpr int VEC = 16 / (int)sizeof(TX);
    __shared__ float dp[PL_MAX_C];
    __shared__ float red[2 * 16];
    const int n = blockIdx.x / S, s = blockIdx.x - n * S, tid = threadIdx.x;
    const float mu = mean[n], r = rstd[n];
    const TG* g = dy + (size_t)n * C;
    const float* pn = pooled + (size_t)n * C;
    float a[2] = {0.f, 0.f};
    for (int c = tid; c < C; c += 256) {
        const float gw = to_f32(g[c]) * weight[c], xh = (pn[c] - mu) * r;
        a[0] += gw; a[1] += gw * xh;
    }
    hd_block_sum<2>(a, red, 4);
    const float c1 = a[0] / (float)C, c2 = a[1] / (float)C;
    const int ca = s * cs, cb = min(C, ca + cs);
    if (ca >= cb) return;                                       // (workgroup-uniform; the launcher sizes S so that no slice is empty)
    const float fP = (float)P;
    for (int c = ca + tid; c < cb; c += 256) {
        const float gv = to_f32(g[c]), xh = (pn[c] - mu) * r;
        dp[c - ca] = r * (gv * weight[c] - c1 - xh * c2) / fP;
        part[(size_t)n * 2 * C + c] = gv * xh;
        part[(size_t)n * 2 * C + C + c] = gv;
    }
    __syncthreads();
    const size_t e0 = ((size_t)n * C + ca) * P;                  // first element of this workgroup's run of dx
    const int total = (cb - ca) * P;                             // <= 2048 * 1024
    TX* out = dx + e0;
    int h = vec ? (int)((VEC - (e0 % VEC)) % VEC) : total;
    if (h > total) h = total;
    const int nv = (total - h) / VEC;
    if (!vec) {
        for (int i = tid; i < total; i += 256) out[i] = from_f32<TX>(dp[i / P]);
        return;
    }
    if (tid < h) out[tid] = from_f32<TX>(dp[tid / P]);           // h < VEC <= 8
    for (int v = tid; v < nv; v += 256) {
        const int i = h + v * VEC;
        int c = i / P, rem = i - c * P;
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            o[j] = dp[c];                                        // i + j < total: c < cb - ca
            if (++rem == P) { rem = 0; ++c; }
        }
        pl_store_vec(out + i, o);
    }
    for (int i = h + nv * VEC + tid; i < total; i += 256) out[i] = from_f32<TX>(dp[i / P]);
}

// dweight[c] = sum_n part[n][c], dbias[c] = sum_n part[n][C + c]: 64 columns per workgroup, the images in four runs that are added in run order
__global__ __launch_bounds__(256) void pool_ln_reduce_kernel(const float* __restrict__ part, float* __restrict__ dweight, float* __restrict__ dbias, int N, int C) {
    __shared__ float acc[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), run = threadIdx.x >> 6;
    const int per = (N + 3) / 4, n0 = run * per, n1 = min(N, n0 + per);
    float s = 0.f;
    if (col < 2 * C) {
        for (int k0 = n0; k0 < n1; k0 += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = k0 + j < n1 ? part[(size_t)(k0 + j) * 2 * C + col] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
    }
    acc[run][threadIdx.x & 63] = s;
    __syncthreads();
    if (run == 0 && col < 2 * C) {
        const float t = ((acc[0][threadIdx.x] + acc[1][threadIdx.x]) + acc[2][threadIdx.x]) + acc[3][threadIdx.x];
        if (col < C) dweight[col] = t; else dbias[col - C] = t;
    }
}

static int pl_supported(int x_dtype, int N, int C, int P) {
    return (x_dtype == SLAK_F32 || x_dtype == SLAK_BF16) && N >= 1 && C >= 1 && P >= 1 && C <= PL_MAX_C && P <= PL_MAX_P
           && (long long)N * C * P < (1LL << 31);
}
// slices of C per image in the backward: about 1024 workgroups on the chip, at least 64 channels a slice
static int pl_slices(int N, int C) {
    int S = (1024 + N - 1) / N;
    const int most = (C + 63) / 64;
    if (S > most) S = most;
    if (S < 1) S = 1;
    const int cs = (C + S - 1) / S;
    return (C + cs - 1) / cs;                                   // no empty slice
}

}  // namespace slak

using namespace slak;

extern "C" {

int slak_pool_ln_supported(int x_dtype, int N, int C, int P) { return pl_supported(x_dtype, N, C, P); }

size_t slak_pool_ln_workspace_bytes(int N, int C, int P) {
    if (N <= 0 || C <= 0 || P <= 0) return 0;
    return align_up((size_t)N * 2 * C * sizeof(float), 256);
}

int slak_pool_ln_forward(const void* x, int x_dtype, const float* weight, const float* bias, float eps, void* y, int y_dtype,
                         float* pooled, float* mean, float* rstd, int N, int C, int P, void* stream) {
    if (!x || !weight || !bias || !y || !pooled || !mean || !rstd) return SLAK_ERR_INVALID_ARG;
    if (N <= 0 || C <= 0 || P <= 0 || !dtype_ok(x_dtype) || !dtype_ok(y_dtype)) return SLAK_ERR_INVALID_ARG;
    if (!pl_supported(x_dtype, N, C, P) || !(y_dtype == SLAK_F32 || y_dtype == SLAK_BF16)) return SLAK_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)N), block(C >= 512 ? 1024 : 256);
#define SLAK_PL_FWD(TX, TY)                                                                                                       \
    hipLaunchKernelGGL((pool_ln_fwd_kernel<TX, TY>), grid, block, 0, (hipStream_t)stream, (const TX*)x, weight, bias, (TY*)y, pooled, \
                       mean, rstd, C, P, eps)
    if (x_dtype == SLAK_F32 && y_dtype == SLAK_F32) SLAK_PL_FWD(float, float);
    else if (x_dtype == SLAK_F32) SLAK_PL_FWD(float, bf16_t);
    else if (y_dtype == SLAK_F32) SLAK_PL_FWD(bf16_t, float);
    else SLAK_PL_FWD(bf16_t, bf16_t);
#undef SLAK_PL_FWD
    SLAK_LAUNCH_CHECK();
    return SLAK_OK;
}

int slak_pool_ln_backward(const void* dy, int dy_dtype, const float* pooled, const float* weight, const float* mean, const float* rstd,
                          void* dx, int x_dtype, float* dweight, float* dbias, int N, int C, int P,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !pooled || !weight || !mean || !rstd || !dx || !dweight || !dbias) return SLAK_ERR_INVALID_ARG;
    if (N <= 0 || C <= 0 || P <= 0 || !dtype_ok(x_dtype) || !dtype_ok(dy_dtype)) return SLAK_ERR_INVALID_ARG;
    if (!pl_supported(x_dtype, N, C, P) || !(dy_dtype == SLAK_F32 || dy_dtype == SLAK_BF16)) return SLAK_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < slak_pool_ln_workspace_bytes(N, C, P)) return SLAK_ERR_WORKSPACE;
    const int S = pl_slices(N, C), cs = (C + S - 1) / S;
    const int vec = ((uintptr_t)dx & 15) == 0;
    float* part = (float*)workspace;
    const dim3 grid((unsigned)(N * S));
#define SLAK_PL_BWD(TX, TG)                                                                                                        \
    hipLaunchKernelGGL((pool_ln_bwd_kernel<TX, TG>), grid, dim3(256), 0, (hipStream_t)stream, (const TG*)dy, pooled, weight, mean, rstd, \
                       (TX*)dx, part, C, P, S, cs, vec)
    if (x_dtype == SLAK_F32 && dy_dtype == SLAK_F32) SLAK_PL_BWD(float, float);
    else if (x_dtype == SLAK_F32) SLAK_PL_BWD(float, bf16_t);
    else if (dy_dtype == SLAK_F32) SLAK_PL_BWD(bf16_t, float);
    else SLAK_PL_BWD(bf16_t, bf16_t);
#undef SLAK_PL_BWD
    SLAK_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool_ln_reduce_kernel, dim3((unsigned)ceil_div(2 * C, 64)), dim3(256), 0, (hipStream_t)stream, part, dweight, dbias, N, C);
    SLAK_LAUNCH_CHECK();
    return SLAK_OK;
}

}  // extern "C"
