// A pitch salience without a network: the YIN difference function of each of CREPE's frames,
// cumulative-mean normalised and read at the lag of each of the 360 pitch bins.  One launch, one wavefront per frame:
//   frame (1024 samples) -> LDS
//   d(tau) = sum_{j < 512} (x[j] - x[j + tau])^2, tau = 0 .. 511, in the direct form: lane l owns the lags 8 l .. 8 l + 7 and
//            keeps the sixteen samples x[j0 + 8 l .. j0 + 8 l + 15] in registers while j walks j0 .. j0 + 7, so eight steps of
//            j cost two 16-byte LDS reads of the window and two broadcast reads of x[j0 .. j0 + 7] for 64 (subtract, FMA) pairs
//   c(tau) = d(1) + ... + d(tau): the lane's own eight in order, then a fixed shuffle scan of the lane totals
//   d'(tau) = d(tau) tau / c(tau) (1 where c is not positive, and at tau = 0) -> LDS
//   bin b:  Catmull-Rom through d'(i_b - 1 .. i_b + 2) at w_b, salience = clip(1 - v - cost_b, 0, 1), not finite -> 0
// Every sum has one order, a frame is one wavefront's work and shares nothing with another, so results are the same bits
// from run to run and whatever else is in the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"

namespace {

constexpr int kBins = 360;
constexpr int kFrame = 1024;                    // CREPE's window at 16 kHz
constexpr int kLags = 512;                      // tau = 0 .. 511, and the number of terms of each d(tau)
constexpr int kPerLane = kLags / 64;            // consecutive lags of one lane
constexpr int kMaxBlocks = 8192;                // frames beyond this many are walked grid-strided
static_assert(kPerLane == 8, "the window below is two float4 per eight steps of j");

__global__ void __launch_bounds__(64) yin_salience_kernel(const float *__restrict__ y, const float4 *__restrict__ table,
                                                          float *__restrict__ probs, long Lr, long hop, long T, long nframes)
{
    __shared__ __attribute__((aligned(16))) float xs[kFrame];
    __shared__ __attribute__((aligned(16))) float dp[kLags];
    const int lane = threadIdx.x;

    for (long n = blockIdx.x; n < nframes; n += gridDim.x) {
        const long row = n / T, t = n - row * T;
        const float *src = y + row * Lr + t * hop;             // any alignment: one dword per lane and load
        bool bad = false;
#pragma unroll
        for (int i = 0; i < kFrame / 64; ++i) {
            const float v = src[64 * i + lane];
            bad |= !(fabsf(v) < INFINITY);                     // a NaN compares false
            xs[64 * i + lane] = v;
        }
        const bool dead = __any(bad);                          // wave-uniform: a frame with a sample that is not finite
        DDSP_WAVE_ORDER();

        float acc[kPerLane];
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) acc[k] = 0.0f;
        if (!dead) {
            const float4 *win = reinterpret_cast<const float4 *>(xs + kPerLane * lane);
            const float4 *own = reinterpret_cast<const float4 *>(xs);
            float w[2 * kPerLane];
            {
                const float4 a = win[0], b = win[1];
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
            }
#pragma unroll 2
            for (int j0 = 0; j0 < kLags; j0 += kPerLane) {
                const float4 a = win[j0 / 4 + 2], b = win[j0 / 4 + 3];      // x[j0 + 8 l + 8 .. + 15]: at most x[1023]
                const float4 p = own[j0 / 4], q = own[j0 / 4 + 1];          // x[j0 .. j0 + 7], the same address in every lane
                w[8] = a.x; w[9] = a.y; w[10] = a.z; w[11] = a.w; w[12] = b.x; w[13] = b.y; w[14] = b.z; w[15] = b.w;
                const float xj[kPerLane] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
#pragma unroll
                for (int jj = 0; jj < kPerLane; ++jj) {                     // j ascending: the order of every d(tau)
#pragma unroll
                    for (int k = 0; k < kPerLane; ++k) {
                        const float e = xj[jj] - w[jj + k];
                        acc[k] = __fmaf_rn(e, e, acc[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < kPerLane; ++k) w[k] = w[k + kPerLane];
            }
        }

        // c(tau): d(0) is left out of the sums
        float run[kPerLane];
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            s += (lane == 0 && k == 0) ? 0.0f : acc[k];
            run[k] = s;
        }
        float incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float before = __shfl_up(incl, o);
            if (lane >= o) incl += before;
        }
        float base = __shfl_up(incl, 1);                       // the lanes below this one
        if (lane == 0) base = 0.0f;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            const int tau = kPerLane * lane + k;
            const float c = base + run[k];
            dp[tau] = (tau > 0 && c > 0.0f) ? (acc[k] * (float)tau) / c : 1.0f;
        }
        DDSP_WAVE_ORDER();

        float *out = probs + n * kBins;
#pragma unroll
        for (int r = 0; r < (kBins + 63) / 64; ++r) {
            const int b = 64 * r + lane;
            if (b < kBins) {
                const float4 e = table[b];                     // {i_b, w_b, cost_b, unused}
                int i = (int)e.x;
                i = i < 1 ? 1 : (i > kLags - 3 ? kLags - 3 : i);            // the four taps stay inside d' whatever the table holds
                const float p0 = dp[i - 1], p1 = dp[i], p2 = dp[i + 1], p3 = dp[i + 2], u = e.y;
                // Catmull-Rom: p1 + u/2 ((p2 - p0) + u ((2 p0 - 5 p1 + 4 p2 - p3) + u (3 (p1 - p2) + (p3 - p0))))
                const float k3 = __fmaf_rn(3.0f, p1 - p2, p3 - p0);
                const float k2 = __fmaf_rn(4.0f, p2, __fmaf_rn(-5.0f, p1, __fmaf_rn(2.0f, p0, -p3)));
                const float k1 = p2 - p0;
                const float v = __fmaf_rn(0.5f * u, __fmaf_rn(u, __fmaf_rn(u, k3, k2), k1), p1);
                float sal = (1.0f - v) - e.z;
                sal = fabsf(sal) < INFINITY ? fminf(fmaxf(sal, 0.0f), 1.0f) : 0.0f;
                out[b] = dead ? 0.0f : sal;
            }
        }
        DDSP_WAVE_ORDER();                                     // the next frame overwrites xs and dp
    }
}

}  // namespace

extern "C" int ddsp_yin_salience(const float *y, const float *bin_table, float *probs, long B, long Lr, int hop, long T, void *stream)
{
    if (B == 0) return 0;
    if (!y || !bin_table || !probs || B < 0 || Lr < kFrame || hop <= 0 || T <= 0) return DDSP_EINVAL;
    if (((uintptr_t)bin_table & 15) != 0) return DDSP_EINVAL;  // the table is read as one float4 per bin
    if (T - 1 > (Lr - kFrame) / hop) return DDSP_EINVAL;       // (T - 1) hop + 1024 <= Lr, without forming the product
    long rows_len, nframes, nout;
    if (__builtin_mul_overflow(B, Lr, &rows_len) || __builtin_mul_overflow(B, T, &nframes) ||
        __builtin_mul_overflow(nframes, (long)kBins, &nout) || rows_len > (1l << 60) || nout > (1l << 60))
        return DDSP_ERANGE;
    const int blocks = (int)(nframes < kMaxBlocks ? nframes : kMaxBlocks);
    hipLaunchKernelGGL(yin_salience_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, y,
                       reinterpret_cast<const float4 *>(bin_table), probs, Lr, (long)hop, T, nframes);
    return (int)hipGetLastError();
}
