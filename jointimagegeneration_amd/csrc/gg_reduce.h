// The deterministic two-stage fp64 reduction of the held-out objectives (gg_loss.hip, gg_patchgan.hip): every fp32 term is added into an
// fp64 per-thread sum in a fixed (grid-stride) order, the 256 sums of a workgroup are combined by a fixed shuffle tree and a fixed loop
// over its 4 waves, one fp64 partial per workgroup goes to the caller's workspace, and a second launch adds the partials in index order.
// No floating-point atomics; the grid depends on the shape alone, so two runs on the same input give the same bits.
#pragma once
#include "gg_common.h"

namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_MAX_BLOCKS = 1024;          // workgroups per sample

inline int ls_blocks(int64_t rows) { int64_t b = (rows + LS_THREADS - 1) / LS_THREADS; return (int)(b < 1 ? 1 : (b > LS_MAX_BLOCKS ? LS_MAX_BLOCKS : b)); }

// the workgroup's sum of v (every thread calls it), valid in thread 0; fixed order
__device__ __forceinline__ double ls_block_sum(double v, double *lds)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();                          // a second call reuses lds
    if ((threadIdx.x & 63) == 0) lds[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < LS_THREADS / GG_WAVE; ++i) s += lds[i];
    return s;
}

// out[i] = (sum of partials[i's sample][b][i's term], b ascending) * scale;  i = n * terms + term
__global__ void ls_finish_kernel(const double *__restrict__ partials, int count, int terms, int blocks, double scale, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int n = i / terms, k = i - n * terms;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partials[((long long)n * blocks + b) * terms + k];
    out[i] = s * scale;
}

}  // namespace
