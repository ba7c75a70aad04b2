// What the kernels over analysed controls share (ddsp_transform.hip, ddsp_morph.hip; DESIGN.md sections 14b and 14c): the
// test of a usable value, the convex combination and the envelope gather.  Every operation is rounded on its own and their
// order is part of both definitions: morph_controls at a weight of 0 or 1 reproduces transform_controls bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace ddsp_controls {

constexpr int kMaxH = 256;                      // harmonics, in and out: four slots of 64 per lane
constexpr int kMaxF = 257;                      // noise bands: five slots
constexpr int kHSlots = kMaxH / 64;
constexpr int kFSlots = (kMaxF + 63) / 64;

__device__ __forceinline__ bool usable(float x) { return fabsf(x) < INFINITY && x > 0.0f; }     // finite and positive

// (1 - w) x + w y, every operation rounded on its own: w = 0 selects x, w = 1 selects y
__device__ __forceinline__ float convex(float w, float x, float y)
{
    return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, w), x), __fmul_rn(w, y));
}

// E_i0(u), E_i1(u) from the staged pairs amp[h] = {A[i0, h + 1], A[i1, h + 1]}, h < H: the first harmonic below u = 1, linear
// between harmonics, A[., H] at u = H, 0 beyond.  u is compared in floating point before it becomes an index: a NaN or a huge
// u reads nothing.
__device__ __forceinline__ float2 envelope_pair(const float2 *amp, int H, double u)
{
    float2 e = make_float2(0.0f, 0.0f);                         // u > H
    if (u < 1.0) {
        e = amp[0];
    } else if (u < (double)H) {
        const int m = (int)u;                                   // 1 <= m <= H - 1
        const float mu = (float)(u - (double)m);
        const float2 lo = amp[m - 1], hi = amp[m];
        e = make_float2(convex(mu, lo.x, hi.x), convex(mu, lo.y, hi.y));
    } else if (u == (double)H) {
        e = amp[H - 1];
    }
    return e;
}

}  // namespace ddsp_controls
