// The f0 half of the audio encoder (model/autoencoder/encoder.py:13-88, crepe/crepe.py:96-133) around the library work it
// keeps: the CREPE convolutions stay on MIOpen and the classifier on rocBLAS; everything between them is here.
//   resample_kernel     polyphase windowed-sinc resampler (torchaudio's Resample with its defaults, encoder.py:19,57)
//   row_stats_kernel    per-row mean and unbiased std of the resampled audio (encoder.py:60-61)
//   crepe_frames_kernel (x - mean) / std, framed by 1024 with the resampled hop, straight into conv1's zero-padded input
//                       ((254, 254), crepe.py:119): replaces F.pad, unfold and the reshape copy (encoder.py:66-72)
//   crepe_epilogue_kernel  +bias -> ReLU -> BatchNorm (eval) -> max-pool (2, 1) of one CREPE layer (crepe.py:128-133), written
//                       into the next layer's pre-padded input (31, 32), or for the last layer into the [N, L * C] row layout of
//                       permute(0, 2, 1, 3).reshape (crepe.py:101) that the classifier GEMM reads
//   pitch_decode_kernel +bias -> sigmoid (crepe.py:104) -> argmax (torch semantics) -> f0 / harmonicity / cents lookups
//                       (encoder.py:81-88, 120-128)
// NaN is carried as torch carries it: a silent row has std 0, so its frames are NaN (0 / 0), every layer keeps them NaN (ReLU
// and max-pool below propagate NaN like torch.relu / max_pool2d), and the argmax picks bin 0 of an all-NaN row.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"

namespace {

constexpr int kCrepeWin = 1024;
constexpr int kConv1Pad = 254;                  // crepe.py:119 pads (254, 254) before conv1
constexpr int kPadLo = 31, kPadHi = 32;         // crepe.py:128 default padding of layers 2..6
constexpr int kBins = 360;
constexpr int kMaxTable = 16384;                // resampler taps held in LDS (64 KiB)

unsigned grid_for(long n, int per_block)
{
    const long want = (n + per_block - 1) / per_block;
    return (unsigned)(want < 1 ? 1 : (want < 16384 ? want : 16384));
}

// y[b, j] = sum_t table[r, t] * x[b, q * orig + first[r] + t], r = j mod nw, q = j div nw; x outside [0, L) is the zero
// padding (width, width + orig) of torchaudio.  The host keeps only the taps of each phase row that lie inside the sinc's
// support (|t| < lowpass width): the others are the clamped window's residue (<= 1.8e-24 at 441 -> 160) and are skipped, which
// cuts the work 14x at 44.1 -> 16 kHz and lets the table (160 x 34 floats) live in LDS.
__global__ void __launch_bounds__(256) resample_kernel(const float *__restrict__ x, const float *__restrict__ table,
                                                       const int *__restrict__ first, float *__restrict__ y, long L, long Lr,
                                                       int orig, int nw, int ntaps)
{
    extern __shared__ float tab_s[];
    for (int i = threadIdx.x; i < nw * ntaps; i += 256) tab_s[i] = table[i];
    __syncthreads();
    const long b = blockIdx.y;
    const float *row = x + b * L;
    float *out = y + b * Lr;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < Lr; j += (long)gridDim.x * 256) {
        const long q = j / nw;
        const int r = (int)(j - q * nw);
        const long s = q * orig + first[r];
        const float *w = tab_s + r * ntaps;
        float acc = 0.0f;
        if (s >= 0 && s + ntaps <= L) {
            for (int t = 0; t < ntaps; ++t) acc = __fmaf_rn(w[t], row[s + t], acc);
        } else {
            for (int t = 0; t < ntaps; ++t) {
                const long i = s + t;
                if (i >= 0 && i < L) acc = __fmaf_rn(w[t], row[i], acc);
            }
        }
        out[j] = acc;
    }
}

// one workgroup per row: sums in fp64 (fixed-order tree, deterministic), mean then the unbiased variance about it
__global__ void __launch_bounds__(256) row_stats_kernel(const float *__restrict__ y, float *__restrict__ stats, long N)
{
    __shared__ double red[256];
    const float *row = y + (long)blockIdx.x * N;
    double s = 0.0;
    for (long i = threadIdx.x; i < N; i += 256) s += (double)row[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double mean = red[0] / (double)N;
    __syncthreads();
    double v = 0.0;
    for (long i = threadIdx.x; i < N; i += 256) {
        const double d = (double)row[i] - mean;
        v += d * d;
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[2 * blockIdx.x] = (float)mean;
        stats[2 * blockIdx.x + 1] = (float)sqrt(red[0] / (double)(N - 1));
    }
}

// frames[(b T + t), p], p < 254 + 1024 + 254: zero padding, else (y[b, t hop + p - 254] - mean_b) / std_b
__global__ void __launch_bounds__(256) crepe_frames_kernel(const float *__restrict__ y, const float *__restrict__ stats,
                                                           float *__restrict__ frames, long Lr, int hop, long T, long total)
{
    constexpr int P = kCrepeWin + 2 * kConv1Pad;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long bt = e / P;
        const int p = (int)(e - bt * P) - kConv1Pad;
        const long b = bt / T, t = bt - b * T;
        float v = 0.0f;
        if (p >= 0 && p < kCrepeWin) v = (y[b * Lr + t * hop + p] - stats[2 * b]) / stats[2 * b + 1];
        frames[e] = v;
    }
}

__device__ __forceinline__ float relu_nan(float v) { return (v <= 0.0f) ? 0.0f : v; }          // NaN stays NaN (torch.relu)
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }  // NaN wins (max_pool2d)

// conv [N, C, Lc] (no bias) -> pooled Lp = Lc / 2.  last = 0: out [N, C, 31 + Lp + 32] with zero margins; last = 1: out [N, Lp * C]
// at l * C + c.  BatchNorm comes after the ReLU and before the pool (gamma may be negative: the order does not commute).
__global__ void __launch_bounds__(256) crepe_epilogue_kernel(const float *__restrict__ conv, const float *__restrict__ bias,
                                                             const float *__restrict__ rm, const float *__restrict__ rv,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             float *__restrict__ out, long N, int C, int Lc, int last, long total)
{
    const int Lp = Lc / 2;
    const int W = last ? Lp : Lp + kPadLo + kPadHi;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        long n;
        int c, l;
        if (last) {                                   // e = (n Lp + l) C + c
            const long nl = e / C;
            c = (int)(e - nl * C);
            n = nl / Lp;
            l = (int)(nl - n * Lp);
        } else {                                      // e = (n C + c) W + w
            const long nc = e / W;
            const int w = (int)(e - nc * W);
            n = nc / C;
            c = (int)(nc - n * C);
            l = w - kPadLo;
            if (l < 0 || l >= Lp) { out[e] = 0.0f; continue; }
        }
        const float *src = conv + (n * C + c) * (long)Lc + 2 * l;
        const float inv = 1.0f / sqrtf(rv[c] + 0.0010000000474974513f);
        const float bc = bias[c], m = rm[c], g = gamma[c], bt = beta[c];
        const float v0 = __fmaf_rn((relu_nan(src[0] + bc) - m) * inv, g, bt);
        const float v1 = __fmaf_rn((relu_nan(src[1] + bc) - m) * inv, g, bt);
        out[e] = max_nan(v0, v1);
    }
}

// one wavefront per frame: lane l owns bins l, l + 64, ...; probabilities are written as they are computed
__global__ void __launch_bounds__(256) pitch_decode_kernel(const float *__restrict__ logits, const float *__restrict__ bias,
                                                           const float *__restrict__ f0_table, const float *__restrict__ cents_table,
                                                           float *__restrict__ probs, float *__restrict__ f0, float *__restrict__ harm,
                                                           float *__restrict__ cents, long N)
{
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;                                   // wave-uniform
    const float *z = logits + n * kBins;
    float *p = probs + n * kBins;
    float best = 0.0f;
    int bi = kBins;                                       // "none yet"
    for (int k = lane; k < kBins; k += 64) {
        const float v = 1.0f / (1.0f + expf(-(z[k] + bias[k])));
        p[k] = v;
        if (bi == kBins || takes_over(v, k, best, bi)) { best = v; bi = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (oi != kBins && (bi == kBins || takes_over(ov, oi, best, bi))) { best = ov; bi = oi; }
    }
    if (lane == 0) {
        f0[n] = f0_table[bi];
        harm[n] = best;
        cents[n] = cents_table[bi];
    }
}

}  // namespace

extern "C" int ddsp_resample(const float *x, const float *table, const int *first, float *y, long B, long L, int orig, int nw, int ntaps,
                             void *stream)
{
    if (B == 0) return 0;
    if (!x || !table || !first || !y || B < 0 || L <= 0 || orig <= 0 || nw <= 0 || ntaps <= 0) return DDSP_EINVAL;
    if ((long)nw * ntaps > kMaxTable || B > 65535 || L > (1l << 40) / nw) return DDSP_ERANGE;
    const long Lr = ((long)nw * L + orig - 1) / orig;
    hipLaunchKernelGGL(resample_kernel, dim3(grid_for(Lr, 256 * 4), (unsigned)B), dim3(256), sizeof(float) * (size_t)nw * ntaps,
                       (hipStream_t)stream, x, table, first, y, L, Lr, orig, nw, ntaps);
    return (int)hipGetLastError();
}

extern "C" int ddsp_crepe_frames(const float *y, float *stats, float *frames, long B, long Lr, int hop, long T, void *stream)
{
    if (B == 0) return 0;
    if (!y || !stats || !frames || B < 0 || Lr <= 0 || hop <= 0 || T <= 0) return DDSP_EINVAL;
    if (Lr < kCrepeWin || (T - 1) * hop + kCrepeWin > Lr || B > 2147483647l) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)B), dim3(256), 0, s, y, stats, Lr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const long total = B * T * (long)(kCrepeWin + 2 * kConv1Pad);
    hipLaunchKernelGGL(crepe_frames_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, y, stats, frames, Lr, hop, T, total);
    return (int)hipGetLastError();
}

extern "C" int ddsp_crepe_epilogue(const float *conv, const float *bias, const float *running_mean, const float *running_var,
                                   const float *gamma, const float *beta, float *out, long N, int C, int Lc, int last, void *stream)
{
    if (N == 0) return 0;
    if (!conv || !bias || !running_mean || !running_var || !gamma || !beta || !out || N < 0 || C <= 0 || Lc < 2) return DDSP_EINVAL;
    const int Lp = Lc / 2;
    const long total = N * (long)C * (last ? Lp : Lp + kPadLo + kPadHi);
    hipLaunchKernelGGL(crepe_epilogue_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, conv, bias, running_mean,
                       running_var, gamma, beta, out, N, C, Lc, last ? 1 : 0, total);
    return (int)hipGetLastError();
}

extern "C" int ddsp_pitch_decode(const float *logits, const float *bias, const float *f0_table, const float *cents_table, float *probs,
                                 float *f0, float *harmonicity, float *cents, long N, void *stream)
{
    if (N == 0) return 0;
    if (!logits || !bias || !f0_table || !cents_table || !probs || !f0 || !harmonicity || !cents || N < 0) return DDSP_EINVAL;
    if ((N + 3) / 4 > 2147483647l) return DDSP_ERANGE;
    hipLaunchKernelGGL(pitch_decode_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, bias, f0_table,
                       cents_table, probs, f0, harmonicity, cents, N);
    return (int)hipGetLastError();
}
