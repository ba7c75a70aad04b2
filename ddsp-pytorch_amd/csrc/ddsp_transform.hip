// Transformation of analysed controls: time stretch, transposition and formant shift of the oscillator
// bank's controls f0, a, c and of the noise bands, one launch.
//   One wavefront per output frame (four to a workgroup, each with its own LDS, so there is no workgroup barrier; frames beyond
//   kMaxBlocks workgroups are walked grid-strided).  The frame's two source rows are loaded coalesced -- lane l owns the harmonics
//   l + 1, l + 65, l + 129, l + 193 --, masked by the bank's Nyquist rule, summed over the wavefront (S), scaled by a / S and
//   staged in LDS as pairs {frame i0, frame i1}, so that one 8-byte LDS read fetches a harmonic of both frames.  Every output
//   harmonic k' then gathers the two harmonics around u = k' r / q from LDS, interpolates across harmonics and across frames,
//   is masked at the output's Nyquist, and a' = sum_k' A' is a second wavefront sum.  The noise bands go through the same
//   wavefront with v = j / q.  No atomics; every sum is the fixed butterfly of wave_sum: a frame's bits depend on nothing but
//   its own inputs.
//   Every LDS or global index comes from a value that was compared in floating point first: u against [1, H), v against F - 1,
//   the position against [0, T - 1] (a NaN position counts as 0); r and q are used only where they are finite and positive.
//   The kernel is memory-bound: per output frame it reads 2 (H + F + 2) + 3 floats and writes H' + F + 2.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_controls.h"

namespace {

using namespace ddsp_controls;                  // kMaxH, kMaxF, their slots; usable, convex, envelope_pair

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;           // output frames of one workgroup at a time
constexpr int kMaxBlocks = 8192;                // (analysis.TRANSFORM_KERNEL_MAX_BLOCKS)
constexpr int kNoisePitch = 260;                // pairs of one wavefront's noise stage

__global__ void __launch_bounds__(kThreads) transform_kernel(const float *__restrict__ f0, const float *__restrict__ a,
                                                             const float *__restrict__ c, const float *__restrict__ noise,
                                                             const float *__restrict__ pos, const float *__restrict__ ratio,
                                                             const float *__restrict__ env, float *__restrict__ f0_out,
                                                             float *__restrict__ a_out, float *__restrict__ c_out,
                                                             float *__restrict__ noise_out, long T, long T_out, int H, int H_out, int F,
                                                             float nyquist, long nframes)
{
    __shared__ float2 amp_s[kWaves][kMaxH];                     // {A[i0, h + 1], A[i1, h + 1]}, the source amplitudes
    __shared__ float2 noise_s[kWaves][kNoisePitch];             // {N[i0, j], N[i1, j]}
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float2 *amp = amp_s[wv], *nz = noise_s[wv];
    const double top = (double)(T - 1);
    const float fill = 1.0f / (float)H_out;

    for (long g = (long)blockIdx.x * kWaves + wv; g < nframes; g += (long)gridDim.x * kWaves) {
        const long row = g / T_out;
        const float r = ratio[g], q = env[g];
        const bool ratios = usable(r) && usable(q);
        double p = (double)pos[g];
        if (!(p >= 0.0)) p = 0.0;                               // a NaN too
        if (p > top) p = top;
        const long i0 = (long)p;                                // 0 <= p <= T - 1: the floor
        const long i1 = i0 + 1 < T ? i0 + 1 : T - 1;
        const float lam = (float)(p - (double)i0);              // exact: p is an fp32 value or T - 1
        const long s0 = row * T + i0, s1 = row * T + i1;
        // every load of the two source rows is issued here, behind the one dependent load of the position: the masks that need
        // f0 are applied to the values, not to the loads (the rows exist whatever they hold)
        const float fa = f0[s0], fb = f0[s1], a0 = a[s0], a1 = a[s1];
        float x0[kHSlots], x1[kHSlots];
#pragma unroll
        for (int sl = 0; sl < kHSlots; ++sl) {
            const int h = 64 * sl + lane;
            x0[sl] = h < H ? c[s0 * H + h] : 0.0f;
            x1[sl] = h < H ? c[s1 * H + h] : 0.0f;
        }
        if (noise) {
#pragma unroll
            for (int sl = 0; sl < kFSlots; ++sl) {
                const int j = 64 * sl + lane;
                if (j < F) nz[j] = make_float2(noise[s0 * F + j], noise[s1 * F + j]);
            }
        }
        const bool va = usable(fa), vb = usable(fb);
        const bool live = ratios && (va || vb);
        const double rq = ratios ? (double)r / (double)q : 1.0;

        float f0o = 0.0f;
        if (live) {
            float t0 = 0.0f, t1 = 0.0f;
#pragma unroll
            for (int sl = 0; sl < kHSlots; ++sl) {
                const float k = (float)(64 * sl + lane + 1);
                if (!va || __fmul_rn(k, fa) > nyquist) x0[sl] = 0.0f;
                if (!vb || __fmul_rn(k, fb) > nyquist) x1[sl] = 0.0f;
                t0 += x0[sl];
                t1 += x1[sl];
            }
            const float S0 = wave_sum(t0), S1 = wave_sum(t1);
            const float g0 = S0 == 0.0f ? 0.0f : a0 / S0, g1 = S1 == 0.0f ? 0.0f : a1 / S1;             // S = 0: the frame is all zero
#pragma unroll
            for (int sl = 0; sl < kHSlots; ++sl) {
                const int h = 64 * sl + lane;
                if (h < H) amp[h] = make_float2(__fmul_rn(x0[sl], g0), __fmul_rn(x1[sl], g1));
            }
            const float f0s = va && vb ? (float)((1.0 - (double)lam) * (double)fa + (double)lam * (double)fb) : (va ? fa : fb);
            f0o = __fmul_rn(f0s, r);
        }
        DDSP_WAVE_ORDER();

        float out[kHSlots], part = 0.0f;
#pragma unroll
        for (int sl = 0; sl < kHSlots; ++sl) {
            const int ko = 64 * sl + lane;
            float v = 0.0f;
            if (live && ko < H_out) {
                const float2 e = envelope_pair(amp, H, (double)(ko + 1) * rq);  // u is positive and finite
                v = convex(lam, e.x, e.y);
                if (__fmul_rn((float)(ko + 1), f0o) > nyquist) v = 0.0f;
            }
            out[sl] = v;
            part += v;
        }
        const float total = wave_sum(part);
#pragma unroll
        for (int sl = 0; sl < kHSlots; ++sl) {
            const int ko = 64 * sl + lane;
            if (ko < H_out) c_out[g * H_out + ko] = total == 0.0f ? fill : out[sl] / total;
        }
        if (lane == 0) {
            f0_out[g] = f0o;
            a_out[g] = total;
        }
        if (noise) {
#pragma unroll
            for (int sl = 0; sl < kFSlots; ++sl) {
                const int j = 64 * sl + lane;
                if (j < F) {
                    float v = 0.0f;
                    const double w = (double)j / (ratios ? (double)q : 1.0);      // >= 0 and finite
                    if (ratios && w <= (double)(F - 1)) {
                        const int n = (int)w, n1 = n + 1 < F ? n + 1 : F - 1;   // 0 <= n <= F - 1
                        const float nu = (float)(w - (double)n);
                        const float2 lo = nz[n], hi = nz[n1];
                        v = convex(lam, convex(nu, lo.x, hi.x), convex(nu, lo.y, hi.y));
                    }
                    noise_out[g * F + j] = v;
                }
            }
        }
        DDSP_WAVE_ORDER();                                      // the next frame overwrites the stages
    }
}

}  // namespace

extern "C" int ddsp_transform_controls(const float *f0, const float *a, const float *c, const float *noise, const float *pos,
                                       const float *ratio, const float *env, float *f0_out, float *a_out, float *c_out,
                                       float *noise_out, long B, long T, long T_out, int H, int H_out, int F, int sample_rate,
                                       void *stream)
{
    if (B == 0) return 0;
    if (!f0 || !a || !c || !pos || !ratio || !env || !f0_out || !a_out || !c_out || (noise == nullptr) != (noise_out == nullptr) ||
        B < 0 || T <= 0 || T_out <= 0 || H <= 0 || H_out <= 0 || F <= 0 || sample_rate <= 0)
        return DDSP_EINVAL;
    if (H > kMaxH || H_out > kMaxH || F > kMaxF) return DDSP_ERANGE;
    long in_frames, out_frames;                                 // every element index fits a long: frames x 257 <= 2^56 x 2^9
    if (__builtin_mul_overflow(B, T, &in_frames) || __builtin_mul_overflow(B, T_out, &out_frames) || in_frames > (1l << 47) ||
        out_frames > (1l << 47))
        return DDSP_ERANGE;
    const long groups = (out_frames + kWaves - 1) / kWaves;
    const int blocks = (int)(groups < kMaxBlocks ? groups : kMaxBlocks);
    hipLaunchKernelGGL(transform_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, f0, a, c, noise, pos, ratio,
                       env, f0_out, a_out, c_out, noise_out, T, T_out, H, H_out, F, (float)(sample_rate / 2), out_frames);
    return (int)hipGetLastError();
}
