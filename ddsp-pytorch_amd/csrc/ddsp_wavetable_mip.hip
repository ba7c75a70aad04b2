// The mip levels of band-limited wavetables and their adjoint.
//   M[0] = W;  M[q, k, j] = sum_i W[k, i] D[q, (j - i) mod L]  for q >= 1, in fp32, i ascending, one fused multiply-add per term.
//   grad_W[k, i] = grad_M[0, k, i] + sum_{q >= 1} sum_j grad_M[q, k, j] D[q, (j - i) mod L] (D is symmetric: the same circular sum
//   up to its fp32 roundings, and read this way the exact transpose); levels ascending, j ascending inside a level, each level's sum added to the total as it completes.
// D [Q + 1, L] comes from the caller (the Dirichlet kernels, computed in fp64 on the host); row 0 is never read.
// A workgroup holds one table row and one kernel row in LDS and gives each thread kOutputs outputs kMipThreads apart, so that one
// broadcast read of the row's entry feeds kOutputs multiply-adds and the kernel reads of a wavefront are consecutive words.
// Both sums have a fixed order: the same bits every run.  L is a power of two (the mask below), 16 <= L <= 4096.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_wavetable_plan.h"

namespace {

using namespace ddsp_wavetable;

constexpr int kMipThreads = 256, kOutputs = 4, kTile = kMipThreads * kOutputs;

// grid (tiles of outputs, N, Q + 1)
__global__ void __launch_bounds__(kMipThreads) mip_build_kernel(const float *__restrict__ W, const float *__restrict__ D,
                                                                float *__restrict__ M, int N, int L)
{
    __shared__ float row[kMipMaxSize], ker[kMipMaxSize];
    const int k = blockIdx.y, q = blockIdx.z, j0 = blockIdx.x * kTile + threadIdx.x;
    const float *src = W + (long)k * L;
    float *dst = M + ((long)q * N + k) * L;
    if (q == 0) {
#pragma unroll
        for (int x = 0; x < kOutputs; ++x)
            if (j0 + x * kMipThreads < L) dst[j0 + x * kMipThreads] = src[j0 + x * kMipThreads];
        return;
    }
    for (int i = threadIdx.x; i < L; i += kMipThreads) {
        row[i] = src[i];
        ker[i] = D[(long)q * L + i];
    }
    __syncthreads();
    const int mask = L - 1;
    float acc[kOutputs] = {};
    for (int i = 0; i < L; ++i) {
        const float w = row[i];
#pragma unroll
        for (int x = 0; x < kOutputs; ++x) acc[x] = __fmaf_rn(w, ker[(j0 + x * kMipThreads - i) & mask], acc[x]);
    }
#pragma unroll
    for (int x = 0; x < kOutputs; ++x)
        if (j0 + x * kMipThreads < L) dst[j0 + x * kMipThreads] = acc[x];
}

// grid (tiles of outputs, N)
__global__ void __launch_bounds__(kMipThreads) mip_adjoint_kernel(const float *__restrict__ G, const float *__restrict__ D,
                                                                  float *__restrict__ grad_W, int N, int L, int levels)
{
    __shared__ float row[kMipMaxSize], ker[kMipMaxSize];
    const int k = blockIdx.y, i0 = blockIdx.x * kTile + threadIdx.x;
    const int mask = L - 1;
    float total[kOutputs];
#pragma unroll
    for (int x = 0; x < kOutputs; ++x) total[x] = i0 + x * kMipThreads < L ? G[(long)k * L + i0 + x * kMipThreads] : 0.0f;
    for (int q = 1; q < levels; ++q) {
        __syncthreads();                                                        // (the rows of the level before are read no more)
        for (int j = threadIdx.x; j < L; j += kMipThreads) {
            row[j] = G[((long)q * N + k) * L + j];
            ker[j] = D[(long)q * L + j];
        }
        __syncthreads();
        float acc[kOutputs] = {};
        for (int j = 0; j < L; ++j) {
            const float g = row[j];
#pragma unroll
            for (int x = 0; x < kOutputs; ++x) acc[x] = __fmaf_rn(g, ker[(j - i0 - x * kMipThreads) & mask], acc[x]);
        }
#pragma unroll
        for (int x = 0; x < kOutputs; ++x) total[x] += acc[x];
    }
#pragma unroll
    for (int x = 0; x < kOutputs; ++x)
        if (i0 + x * kMipThreads < L) grad_W[(long)k * L + i0 + x * kMipThreads] = total[x];
}

}  // namespace

extern "C" int ddsp_wavetable_mip_levels(int L)
{
    const int n = mip_levels(L);
    return n ? n : DDSP_ERANGE;
}

extern "C" int ddsp_wavetable_mip_build(const float *tables, const float *kernels, float *levels, int N, int L, void *stream)
{
    if (N < 1 || L < 2) return DDSP_EINVAL;
    if (!tables || !kernels || !levels) return DDSP_EINVAL;
    if (!mip_supported(N, L)) return DDSP_ERANGE;
    const dim3 grid((unsigned)((L + kTile - 1) / kTile), (unsigned)N, (unsigned)mip_levels(L));
    hipLaunchKernelGGL(mip_build_kernel, grid, dim3(kMipThreads), 0, (hipStream_t)stream, tables, kernels, levels, N, L);
    return (int)hipGetLastError();
}

extern "C" int ddsp_wavetable_mip_adjoint(const float *grad_levels, const float *kernels, float *grad_tables, int N, int L,
                                          void *stream)
{
    if (N < 1 || L < 2) return DDSP_EINVAL;
    if (!grad_levels || !kernels || !grad_tables) return DDSP_EINVAL;
    if (!mip_supported(N, L)) return DDSP_ERANGE;
    const dim3 grid((unsigned)((L + kTile - 1) / kTile), (unsigned)N);
    hipLaunchKernelGGL(mip_adjoint_kernel, grid, dim3(kMipThreads), 0, (hipStream_t)stream, grad_levels, kernels, grad_tables, N, L,
                       mip_levels(L));
    return (int)hipGetLastError();
}
