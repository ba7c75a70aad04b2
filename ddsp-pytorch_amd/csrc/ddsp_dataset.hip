// The training set's audio stages (dataset/audio_dataset.py of the reference) between the file read and the encoder:
//   pcm_to_mono_kernel    interleaved PCM [L, C] as the WAV file stores it -> mono fp32 [L]: torchaudio.load(normalize=True)'s
//                         scaling, then y.mean(dim=0) when C > 1 (audio_dataset.py:30-37)
//   make_examples_kernel  the conf-rate mono audio of several files, concatenated -> one row per example: the hop-pad
//                         (pad = len % hop, split (pad // 2, pad - pad // 2), :46-47), unfold(0, duration, step) (:50-59) and the
//                         encoder's (p // 2, p - p // 2) zero margins, p = n_fft - hop (:86, 90), in one pass
// Both are pure data movement plus at most C - 1 adds and one divide per sample: memory bound, one sample per thread.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ddsp_hip.h"

namespace {

unsigned grid_for(long n, int per_block)
{
    const long want = (n + per_block - 1) / per_block;
    return (unsigned)(want < 1 ? 1 : (want < 16384 ? want : 16384));
}

template <typename T> __device__ __forceinline__ float pcm_sample(T v);
// int16 / 32768 and int32 / 2^31: the conversion to fp32 rounds once (exact for int16), the power-of-two scale is exact
template <> __device__ __forceinline__ float pcm_sample<int16_t>(int16_t v) { return (float)v * (1.0f / 32768.0f); }
template <> __device__ __forceinline__ float pcm_sample<int32_t>(int32_t v) { return __int2float_rn(v) * (1.0f / 2147483648.0f); }
template <> __device__ __forceinline__ float pcm_sample<float>(float v) { return v; }

// y[i] = (sum over c of x[i, c]) / C, summed from 0.0 in channel order and divided (IEEE, not by a reciprocal): torch's CPU
// mean over dim 0 of a contiguous [C, L] tensor.  C == 1 is y[0] itself (audio_dataset.py:33-34: no mean is taken).
template <typename T>
__global__ void __launch_bounds__(256) pcm_to_mono_kernel(const T *__restrict__ pcm, float *__restrict__ y, long L, int C)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < L; i += (long)gridDim.x * 256) {
        const T *frame = pcm + i * C;
        if (C == 1) {
            y[i] = pcm_sample<T>(frame[0]);
            continue;
        }
        float s = 0.0f;
        for (int c = 0; c < C; ++c) s += pcm_sample<T>(frame[c]);
        y[i] = s / (float)C;
    }
}

// Row r (example e = e0 + r) of file f (the last f with files[f].first <= e) holds padded positions (e - first) * step + i,
// i < duration, of that file, i.e. source samples (e - first) * step + i - front; a source index outside [0, len) is the
// hop-pad's zero.  enc_in rows add p_lo zeros in front and p - p_lo behind.  Every read is also bounded by y_len, whatever
// the table says.
__global__ void __launch_bounds__(256) make_examples_kernel(const float *__restrict__ y, long y_len, const long *__restrict__ files,
                                                            int n_files, long e0, long E, long duration, long step, int p,
                                                            float *__restrict__ enc_in, float *__restrict__ audio)
{
    const int p_lo = p / 2;
    const long W = enc_in ? duration + p : duration;
    for (long r = blockIdx.y; r < E; r += gridDim.y) {
        const long e = e0 + r;
        int lo = 0, hi = n_files - 1;                     // files[.].first is non-decreasing
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if (files[4 * mid + 3] <= e) lo = mid; else hi = mid - 1;
        }
        const long start = files[4 * lo], len = files[4 * lo + 1], front = files[4 * lo + 2], first = files[4 * lo + 3];
        const long base = (e - first) * step - front;
        for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < W; c += (long)gridDim.x * 256) {
            const long i = enc_in ? c - p_lo : c;
            float v = 0.0f;
            if (i >= 0 && i < duration) {
                const long src = base + i;
                if (src >= 0 && src < len && start + src >= 0 && start + src < y_len) v = y[start + src];
                if (audio) audio[r * duration + i] = v;
            }
            if (enc_in) enc_in[r * W + c] = v;
        }
    }
}

}  // namespace

extern "C" int ddsp_pcm_to_mono(const void *pcm, float *y, long L, int C, int format, void *stream)
{
    if (L == 0) return 0;
    if (!pcm || !y || L < 0 || C <= 0) return DDSP_EINVAL;
    if (format != DDSP_PCM_S16 && format != DDSP_PCM_S32 && format != DDSP_PCM_F32) return DDSP_EINVAL;
    if (C > 65535 || L > LONG_MAX / C) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(grid_for(L, 256)), block(256);
    if (format == DDSP_PCM_S16)
        hipLaunchKernelGGL(pcm_to_mono_kernel<int16_t>, grid, block, 0, s, (const int16_t *)pcm, y, L, C);
    else if (format == DDSP_PCM_S32)
        hipLaunchKernelGGL(pcm_to_mono_kernel<int32_t>, grid, block, 0, s, (const int32_t *)pcm, y, L, C);
    else
        hipLaunchKernelGGL(pcm_to_mono_kernel<float>, grid, block, 0, s, (const float *)pcm, y, L, C);
    return (int)hipGetLastError();
}

extern "C" int ddsp_make_examples(const float *y, long y_len, const long *files, int n_files, long e0, long E, long duration,
                                  long step, int p, float *enc_in, float *audio, void *stream)
{
    if (E == 0) return 0;
    if (!y || !files || (!enc_in && !audio) || y_len <= 0 || n_files <= 0 || e0 < 0 || E < 0 || duration <= 0 || step <= 0 || p < 0)
        return DDSP_EINVAL;
    const long W = duration + (enc_in ? p : 0);
    if (duration > INT_MAX || e0 > LONG_MAX - E || E > LONG_MAX / W) return DDSP_ERANGE;
    const unsigned rows = (unsigned)(E < 65535 ? E : 65535);
    hipLaunchKernelGGL(make_examples_kernel, dim3(grid_for(W, 256 * 4), rows), dim3(256), 0, (hipStream_t)stream, y, y_len, files,
                       n_files, e0, E, duration, step, p, enc_in, audio);
    return (int)hipGetLastError();
}
