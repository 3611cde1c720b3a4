// The reductions the phl translation units share: butterflies over a 64-lane wave, the maximum over a 256-thread
// workgroup, and the deterministic final sum of per-workgroup float64 partials.  Internal: everything sits in an
// anonymous namespace, so each translation unit gets its own copy.  (Kept apart from phl_device_utils.h, whose scan and
// sort kernels belong to the lattice build.)
#pragma once
#include "phl_internal.h"

namespace {

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// max over a workgroup of four waves, in every thread; red[4] is free again behind the caller's next barrier
__device__ __forceinline__ float block_max_f(float v, float *red)
{
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// out[c] = scale * sum(partial[NC i + c], i < n), c < NC: one workgroup of 256 threads, strided per-thread sums in
// index order, then a fixed tree, scaled and rounded to fp32 once -- no atomics, the same bits on every run (scale = 1.0
// is exact)
template <int NC>
__global__ __launch_bounds__(256) void k_sum_partials(const double *__restrict__ partial, int64_t n, double scale,
                                                      float *__restrict__ out)
{
    __shared__ double red[NC][256];
    double s[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) s[c] = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int c = 0; c < NC; c++) s[c] += partial[NC * i + c];
#pragma unroll
    for (int c = 0; c < NC; c++) red[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int c = 0; c < NC; c++) red[c][threadIdx.x] += red[c][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < NC) out[threadIdx.x] = (float)(red[threadIdx.x][0] * scale);
}

}  // namespace
