// Morph of two sets of analysed controls: pitch, spectral envelope and noise bands of an output frame
// lie between those of a frame of sound A and a frame of sound B, each with its own per-frame weight, one launch.
//   The structure is transform_kernel's (ddsp_transform.hip): one wavefront per output frame (four to a workgroup, each with
//   its own LDS, no workgroup barrier; frames beyond kMaxBlocks workgroups are walked grid-strided).  Behind the dependent loads
//   of the two positions and the three weights every load of the frame's four source rows -- two frames of each sound: f0, a, c
//   and the bands -- is issued at once; the masks that need f0 are applied to the values.  Lane l owns the harmonics l + 1,
//   l + 65, l + 129, l + 193.  Per sound the two rows are masked by the bank's Nyquist rule, summed over the wavefront (S),
//   scaled by a / S and staged in LDS as pairs {frame i0, frame i1}; every output harmonic k' gathers each sound's envelope at
//   u_X = k' (hz coordinates: k' f0' / f_X, the same frequency in both sounds), interpolates across harmonics, across frames
//   and across the sounds, is masked at the output's Nyquist, and a' is a last wavefront sum.  The bands need no gather (band j
//   of the output is band j of the sources): they stay in registers.  No atomics; every sum is the fixed butterfly of wave_sum.
//   The operations and their order are transform_kernel's, so that a weight of 0 or 1 reproduces ddsp_transform_controls at
//   ratio = env = 1 bit for bit (on finite, non-negative controls).
//   Every LDS or global index comes from a value that was compared in floating point first: u against [1, H_X) in
//   envelope_pair, the positions against [0, T_X - 1] (a NaN counts as 0); the weights are used only where all three are
//   finite, f_X only where it is finite and positive.
//   Per output frame the kernel reads 2 (H_a + H_b + 2 F + 4) + 5 floats and writes H' + F + 2.
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
constexpr int kMaxBlocks = 8192;                // (analysis.MORPH_KERNEL_MAX_BLOCKS)

struct Rows {                                   // what one lane holds of a sound's two frames i0 and i1
    float lam, f0[2], a[2], x[2][kHSlots], n[2][kFSlots];
};

// the frame pair of position p and every load of its two rows; nothing here depends on a loaded value but the position
__device__ __forceinline__ void load_rows(const float *__restrict__ f0, const float *__restrict__ a, const float *__restrict__ c,
                                          const float *__restrict__ noise, long T, int H, float position, long row, int lane, int F,
                                          Rows &r)
{
    const double top = (double)(T - 1);
    double p = (double)position;
    if (!(p >= 0.0)) p = 0.0;                                   // a NaN too
    if (p > top) p = top;
    const long i0 = (long)p;                                    // 0 <= p <= T - 1: the floor
    const long i1 = i0 + 1 < T ? i0 + 1 : T - 1;
    r.lam = (float)(p - (double)i0);                            // exact: p is an fp32 value or T - 1
    const long at[2] = {row * T + i0, row * T + i1};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        r.f0[e] = f0[at[e]];
        r.a[e] = a[at[e]];
#pragma unroll
        for (int sl = 0; sl < kHSlots; ++sl) {
            const int h = 64 * sl + lane;
            r.x[e][sl] = h < H ? c[at[e] * H + h] : 0.0f;
        }
#pragma unroll
        for (int sl = 0; sl < kFSlots; ++sl) {
            const int j = 64 * sl + lane;
            r.n[e][sl] = noise && j < F ? noise[at[e] * F + j] : 0.0f;
        }
    }
}

// The amplitudes the bank plays of the two rows, staged as pairs -> whether the sound is present (a voiced neighbour); f is its
// pitch at the position, without a glide from an unvoiced neighbour.  transform_kernel's operations in its order.
__device__ __forceinline__ bool stage(Rows &r, int H, int lane, float nyquist, float2 *amp, float &f)
{
    const bool v0 = usable(r.f0[0]), v1 = usable(r.f0[1]);
    f = 0.0f;
    if (!v0 && !v1) return false;
    float t0 = 0.0f, t1 = 0.0f;
#pragma unroll
    for (int sl = 0; sl < kHSlots; ++sl) {
        const float k = (float)(64 * sl + lane + 1);
        if (!v0 || __fmul_rn(k, r.f0[0]) > nyquist) r.x[0][sl] = 0.0f;
        if (!v1 || __fmul_rn(k, r.f0[1]) > nyquist) r.x[1][sl] = 0.0f;
        t0 += r.x[0][sl];
        t1 += r.x[1][sl];
    }
    const float S0 = wave_sum(t0), S1 = wave_sum(t1);
    const float g0 = S0 == 0.0f ? 0.0f : r.a[0] / S0, g1 = S1 == 0.0f ? 0.0f : r.a[1] / S1;         // S = 0: the frame is all zero
#pragma unroll
    for (int sl = 0; sl < kHSlots; ++sl) {
        const int h = 64 * sl + lane;
        if (h < H) amp[h] = make_float2(__fmul_rn(r.x[0][sl], g0), __fmul_rn(r.x[1][sl], g1));
    }
    f = v0 && v1 ? (float)((1.0 - (double)r.lam) * (double)r.f0[0] + (double)r.lam * (double)r.f0[1]) : (v0 ? r.f0[0] : r.f0[1]);
    return true;
}

__global__ void __launch_bounds__(kThreads) morph_kernel(
    const float *__restrict__ f0_a, const float *__restrict__ a_a, const float *__restrict__ c_a, const float *__restrict__ noise_a,
    const float *__restrict__ pos_a, const float *__restrict__ f0_b, const float *__restrict__ a_b, const float *__restrict__ c_b,
    const float *__restrict__ noise_b, const float *__restrict__ pos_b, const float *__restrict__ mix_f0,
    const float *__restrict__ mix_amp, const float *__restrict__ mix_noise, float *__restrict__ f0_out, float *__restrict__ a_out,
    float *__restrict__ c_out, float *__restrict__ noise_out, long T_a, long T_b, long T_out, int H_a, int H_b, int H_out, int F, int hz,
    float nyquist, long nframes)
{
    __shared__ float2 amp_s[kWaves][2][kMaxH];                  // per sound {A[i0, h + 1], A[i1, h + 1]}, the played amplitudes
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float2 *amp_a = amp_s[wv][0], *amp_b = amp_s[wv][1];
    const float fill = 1.0f / (float)H_out;

    for (long g = (long)blockIdx.x * kWaves + wv; g < nframes; g += (long)gridDim.x * kWaves) {
        const long row = g / T_out;
        float wf = mix_f0[g], wh = mix_amp[g], wn = mix_noise[g];
        Rows ra, rb;
        load_rows(f0_a, a_a, c_a, noise_a, T_a, H_a, pos_a[g], row, lane, F, ra);
        load_rows(f0_b, a_b, c_b, noise_b, T_b, H_b, pos_b[g], row, lane, F, rb);
        const bool sane = fabsf(wf) < INFINITY && fabsf(wh) < INFINITY && fabsf(wn) < INFINITY;     // a NaN fails too
        wf = fminf(fmaxf(wf, 0.0f), 1.0f);
        wh = fminf(fmaxf(wh, 0.0f), 1.0f);
        wn = fminf(fmaxf(wn, 0.0f), 1.0f);

        float fa = 0.0f, fb = 0.0f, f0o = 0.0f;
        const bool pa = sane && stage(ra, H_a, lane, nyquist, amp_a, fa);
        const bool pb = sane && stage(rb, H_b, lane, nyquist, amp_b, fb);
        const bool live = pa || pb;
        if (pa && pb) {
            if (wf == 0.0f) {
                f0o = fa;
            } else if (wf == 1.0f) {
                f0o = fb;
            } else {                                            // halfway in pitch; never outside the two, whatever exp2 rounds to
                const float mean = (float)exp2((1.0 - (double)wf) * log2((double)fa) + (double)wf * log2((double)fb));
                f0o = fminf(fmaxf(mean, fminf(fa, fb)), fmaxf(fa, fb));
            }
        } else if (live) {
            f0o = pa ? fa : fb;                                 // the amplitudes do the fade
        }
        // output harmonic k' reads sound X's envelope at u_X = k' scale_X: at its own frequency, or at its own number
        const double scale_a = hz && pa ? (double)f0o / (double)fa : 1.0, scale_b = hz && pb ? (double)f0o / (double)fb : 1.0;
        DDSP_WAVE_ORDER();

        float out[kHSlots], part = 0.0f;
#pragma unroll
        for (int sl = 0; sl < kHSlots; ++sl) {
            const int ko = 64 * sl + lane;
            float v = 0.0f;
            if (live && ko < H_out) {
                float ea = 0.0f, eb = 0.0f;
                if (pa) {
                    const float2 e = envelope_pair(amp_a, H_a, (double)(ko + 1) * scale_a);
                    ea = convex(ra.lam, e.x, e.y);
                }
                if (pb) {
                    const float2 e = envelope_pair(amp_b, H_b, (double)(ko + 1) * scale_b);
                    eb = convex(rb.lam, e.x, e.y);
                }
                v = convex(wh, ea, eb);
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
        if (noise_out) {
#pragma unroll
            for (int sl = 0; sl < kFSlots; ++sl) {
                const int j = 64 * sl + lane;
                if (j < F)
                    noise_out[g * F + j] = sane ? convex(wn, convex(ra.lam, ra.n[0][sl], ra.n[1][sl]),
                                                         convex(rb.lam, rb.n[0][sl], rb.n[1][sl])) : 0.0f;
            }
        }
        DDSP_WAVE_ORDER();                                      // the next frame overwrites the stages
    }
}

}  // namespace

extern "C" int ddsp_morph_controls(const float *f0_a, const float *a_a, const float *c_a, const float *noise_a, const float *pos_a,
                                   const float *f0_b, const float *a_b, const float *c_b, const float *noise_b, const float *pos_b,
                                   const float *mix_f0, const float *mix_amp, const float *mix_noise, float *f0_out, float *a_out,
                                   float *c_out, float *noise_out, long B, long T_a, long T_b, long T_out, int H_a, int H_b, int H_out,
                                   int F, int sample_rate, int coordinates, void *stream)
{
    if (B == 0) return 0;
    const int noises = (noise_a != nullptr) + (noise_b != nullptr) + (noise_out != nullptr);
    if (!f0_a || !a_a || !c_a || !pos_a || !f0_b || !a_b || !c_b || !pos_b || !mix_f0 || !mix_amp || !mix_noise || !f0_out || !a_out ||
        !c_out || (noises != 0 && noises != 3) || B < 0 || T_a <= 0 || T_b <= 0 || T_out <= 0 || H_a <= 0 || H_b <= 0 || H_out <= 0 ||
        F <= 0 || sample_rate <= 0 || (coordinates != DDSP_MORPH_HZ && coordinates != DDSP_MORPH_HARMONIC))
        return DDSP_EINVAL;
    if (H_a > kMaxH || H_b > kMaxH || H_out > kMaxH || F > kMaxF) return DDSP_ERANGE;
    long frames_a, frames_b, out_frames;                        // every element index fits a long: frames x 257 <= 2^47 x 2^9
    if (__builtin_mul_overflow(B, T_a, &frames_a) || __builtin_mul_overflow(B, T_b, &frames_b) ||
        __builtin_mul_overflow(B, T_out, &out_frames) || frames_a > (1l << 47) || frames_b > (1l << 47) || out_frames > (1l << 47))
        return DDSP_ERANGE;
    const long groups = (out_frames + kWaves - 1) / kWaves;
    const int blocks = (int)(groups < kMaxBlocks ? groups : kMaxBlocks);
    hipLaunchKernelGGL(morph_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, f0_a, a_a, c_a, noise_a, pos_a, f0_b,
                       a_b, c_b, noise_b, pos_b, mix_f0, mix_amp, mix_noise, f0_out, a_out, c_out, noise_out, T_a, T_b, T_out, H_a, H_b,
                       H_out, F, coordinates == DDSP_MORPH_HZ, (float)(sample_rate / 2), out_frames);
    return (int)hipGetLastError();
}
