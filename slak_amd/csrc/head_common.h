// slak_amd/csrc/head_common.h -- wave / workgroup reductions shared by pool_ln.hip and xent.hip (fixed order: bitwise reproducible).
#pragma once
#include "slak_common.h"

namespace slak {

// xor butterflies: every lane ends with the same bits (a + b == b + a)
__device__ __forceinline__ float hd_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float hd_wave_max(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Sums of NV values over the workgroup; every thread gets them.  red: LDS, NV * 16 floats (at most 16 waves); the waves' sums are added in wave order.
template <int NV>
__device__ __forceinline__ void hd_block_sum(float (&v)[NV], float* red, int nwaves) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = hd_wave_sum(v[j]);
    __syncthreads();                                    // the previous use of `red` is over
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) red[j * 16 + w] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        float s = 0.f;
        for (int i = 0; i < nwaves; ++i) s += red[j * 16 + i];
        v[j] = s;
    }
}
__device__ __forceinline__ float hd_block_max(float v, float* red, int nwaves) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = hd_wave_max(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float m = red[0];
    for (int i = 1; i < nwaves; ++i) m = fmaxf(m, red[i]);
    return m;
}

}  // namespace slak
