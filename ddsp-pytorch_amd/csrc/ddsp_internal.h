// Internal to libddsp_hip.so: optional per-kernel HIP-event timing (include/ddsp_hip.h: ddsp_profile_*) and the small helpers
// that several sources share.
#pragma once
#include <hip/hip_runtime.h>

// DDSP_TEST_HOOKS=1 at load time (ddsp_capi.hip): the process-global *_set_* hooks are live; otherwise they refuse.
bool ddsp_hooks_on();

namespace ddsp_prof {
enum KernelId { PREP = 0, TOTALS = 1, SCAN = 2, SYNTH = 3, NOISE = 4, NOISE_IR = 5 };
// Record an event pair around one launch on `s` when profiling is enabled (no-ops otherwise).
int begin(int kernel_id, hipStream_t s);
void end(int slot, hipStream_t s);
}  // namespace ddsp_prof

// One-time (per device of this process) opt-in of a kernel to more than 64 KiB of dynamic LDS.
// `done` is the caller's static per-device table.  Benign if two threads race: the attribute is idempotent.
inline hipError_t ddsp_allow_big_lds(const void *fn, bool (&done)[64])
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    dev &= 63;
    if (done[dev]) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) done[dev] = true;
    return e;
}

// Compute units of the current device, asked once per device of this process.  No lock, as ddsp_allow_big_lds above: two threads
// that race both store the same count.
inline hipError_t ddsp_device_cus(int *cus)
{
    static int cached[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!cached[dev & 63]) {
        int n = 0;
        e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
        cached[dev & 63] = n;
    }
    *cus = cached[dev & 63];
    return hipSuccess;
}

// scratch carving: offsets rounded up to 256 bytes
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// LDS operations of one wavefront execute in order: between a stage's stores and the next stage's loads only the
// compiler has to be kept from reordering.
#define DDSP_WAVE_ORDER() do { __builtin_amdgcn_wave_barrier(); asm volatile("" ::: "memory"); } while (0)

// sum over the 64 lanes of a wavefront, every lane gets it: xor butterfly 32, 16, ..., 1 (a fixed order: deterministic bits)
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// torch's 'reflect' padding (no repeated edge sample): -1 -> 1, L -> L - 2.  I: int or long, whichever the caller indexes in.
template <typename I>
__device__ __forceinline__ I reflect_index(I i, I L)
{
    if (i < 0) i = -i;
    if (i >= L) i = 2 * (L - 1) - i;
    return i;
}

// (value, bin) that torch.argmax keeps of two candidates: the first NaN, else the larger value, ties to the lower bin
__device__ __forceinline__ bool takes_over(float va, int ia, float vb, int ib)
{
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return na && nb ? ia < ib : na;
    return va > vb || (va == vb && ia < ib);
}
