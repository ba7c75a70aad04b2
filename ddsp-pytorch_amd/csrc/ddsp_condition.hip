// Conditioning statistics and auto-adjust: what brings a foreign performance into the range a decoder
// was trained on.  Three kernels:
//   condition_stats_kernel   the note-on frames' loudness histogram and the two fixed-point sums.  One workgroup per unit, units
//                            walked grid-strided: a unit is a row (per-row mode: B histograms, written with plain stores) or
//                            kChunk consecutive frames of the whole set (pooled mode: a workgroup keeps one LDS histogram over all
//                            its units and adds its non-zero cells and its two sums to the pooled accumulators once, with integer
//                            atomicAdd on global memory; the launcher zeroes the accumulators with one hipMemsetAsync in front).
//                            Cells are counted with LDS atomics; the sums go through the wavefront (xor butterfly) and then the
//                            workgroup.  Everything added is an integer: no result depends on the order of arrival.
//   condition_tables_kernel  one wavefront per group: an inclusive scan of the cells, 64 at a time with a carried total, kept in
//                            LDS; lane k, k + 64, ... binary-searches the cell of quantile k and writes S[k]; lane 0 writes the
//                            means and the count.
//   condition_apply_kernel   one thread per frame, the row's source and target tables staged in LDS: the binary search, the map,
//                            the octave shift and the too-little-to-go-on guard (decided from device memory, never by the host).
//                            Grid: a row's tiles of 256 frames in x, the rows over y and z, no loop (a grid-strided walk kept
//                            every pointer live across the loop and spilled scalar registers).
// Every index into LDS or global memory comes from an integer that was bounded first: a cell from a float compared against
// [0, bins), a table index from a search over [0, Q].
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBins = DDSP_CONDITION_MAX_BINS;
constexpr int kMaxQ = DDSP_CONDITION_MAX_QUANTILES;
constexpr int kMaxBlocks = 2048;                // rows in flight (statistics per row, tables)
constexpr int kPooledBlocks = 512;              // workgroups that merge into one pooled histogram
constexpr long kGridY = 65535;                  // apply: rows along y, the rest along z
constexpr long kMaxTiles = 1l << 23;            // apply: workgroups of one launch
constexpr long kChunk = 1024;                   // frames of one pooled unit
constexpr float kFixed = 16777216.0f;           // 2^24: the sums' fixed point
constexpr float kLimit = 32768.0f;              // 2^15: a frame at or beyond it is not counted ...
constexpr long kMaxGroupFrames = 1l << 24;      // ... and a group holds at most this many: |sum| < 2^15 2^24 2^24 = 2^63

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(kThreads) condition_stats_kernel(const float *__restrict__ loud, const float *__restrict__ cents,
                                                                   const float *__restrict__ harm, const uint8_t *__restrict__ voiced,
                                                                   uint32_t *__restrict__ hist, unsigned long long *__restrict__ sums,
                                                                   long units, long unit_frames, long frames, int pooled, int bins,
                                                                   float lo, float scale, float silence, float confidence)
{
    __shared__ uint32_t cell[kMaxBins];
    __shared__ long long part[kWaves][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int b = tid; b < bins; b += kThreads) cell[b] = 0;
    __syncthreads();
    long long sn = 0, sl = 0;
    const float top = (float)bins;

    for (long u = blockIdx.x; u < units; u += gridDim.x) {
        const long begin = u * unit_frames;
        const long end = begin + unit_frames < frames ? begin + unit_frames : frames;
        for (long i = begin + tid; i < end; i += kThreads) {
            const float l = loud[i], n = cents[i], h = harm[i];
            // (a NaN fails every comparison: not finite is not on)
            const bool on = fabsf(l) < kLimit && fabsf(n) < kLimit && l > silence && h >= confidence && (!voiced || voiced[i]);
            if (on) {
                const float x = __fmul_rn(__fsub_rn(l, lo), scale);
                const int b = !(x >= 0.0f) ? 0 : (x >= top ? bins - 1 : (int)floorf(x));
                atomicAdd(&cell[b], 1u);
                sn += llrintf(__fmul_rn(n, kFixed));
                sl += llrintf(__fmul_rn(l, kFixed));
            }
        }
        if (!pooled) {                                          // the row's own histogram, with plain stores
            sn = wave_sum_i64(sn);
            sl = wave_sum_i64(sl);
            if (lane == 0) { part[wv][0] = sn; part[wv][1] = sl; }
            __syncthreads();                                    // every cell and every part is in
            for (int b = tid; b < bins; b += kThreads) {
                hist[u * bins + b] = cell[b];
                cell[b] = 0;
            }
            if (tid == 0) {
                long long tn = 0, tl = 0;
                for (int w = 0; w < kWaves; ++w) { tn += part[w][0]; tl += part[w][1]; }
                sums[2 * u] = (unsigned long long)tn;
                sums[2 * u + 1] = (unsigned long long)tl;
            }
            sn = sl = 0;
            __syncthreads();                                    // the next row starts from zeroed cells and free parts
        }
    }
    if (pooled) {                                               // one merge per workgroup (two's complement: the sums wrap as int64)
        sn = wave_sum_i64(sn);
        sl = wave_sum_i64(sl);
        if (lane == 0) { part[wv][0] = sn; part[wv][1] = sl; }
        __syncthreads();
        for (int b = tid; b < bins; b += kThreads) {
            const uint32_t v = cell[b];
            if (v) atomicAdd(&hist[b], v);
        }
        if (tid == 0) {
            long long tn = 0, tl = 0;
            for (int w = 0; w < kWaves; ++w) { tn += part[w][0]; tl += part[w][1]; }
            if (tn) atomicAdd(&sums[0], (unsigned long long)tn);
            if (tl) atomicAdd(&sums[1], (unsigned long long)tl);
        }
    }
}

__global__ void __launch_bounds__(64) condition_tables_kernel(const uint32_t *__restrict__ hist, const long long *__restrict__ sums,
                                                              float *__restrict__ tables, double *__restrict__ mean_pitch,
                                                              double *__restrict__ mean_loudness, long *__restrict__ count,
                                                              long groups, int bins, int Q, float lo, float hi)
{
    __shared__ uint32_t cum[kMaxBins];                          // inclusive cumulative counts
    const int lane = threadIdx.x;
    const double dlo = (double)lo, width = ((double)hi - (double)lo) / (double)bins;
    const unsigned long long q = (unsigned long long)Q;

    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint32_t *h = hist + g * bins;
        uint32_t carry = 0;
        for (int base = 0; base < bins; base += 64) {           // (every lane walks every step: the shuffles are uniform)
            const int b = base + lane;
            uint32_t v = b < bins ? h[b] : 0u;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = __shfl_up(v, o);
                if (lane >= o) v += up;
            }
            v += carry;
            if (b < bins) cum[b] = v;
            carry = __shfl(v, 63);
        }
        DDSP_WAVE_ORDER();
        const unsigned long long N = carry;
        for (int k = lane; k <= Q; k += 64) {
            float s = __builtin_nanf("");
            if (N) {
                const unsigned long long kn = (unsigned long long)k * N;
                const unsigned long long need = kn ? kn : 1ull;     // k = 0: the first cell that holds a frame
                int a = 0, e = bins - 1;                            // the smallest b with Q C_b >= need (Q C_last = Q N >= need)
                while (a < e) {
                    const int m = (a + e) >> 1;
                    if (q * cum[m] >= need) e = m; else a = m + 1;
                }
                const unsigned long long below = a ? cum[a - 1] : 0u, c = cum[a] - below;   // c > 0: C rises at a
                double f = (double)((long long)kn - (long long)(q * below)) / (double)(q * c);
                f = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
                s = (float)(dlo + ((double)a + f) * width);
            }
            tables[g * (Q + 1) + k] = s;
        }
        if (lane == 0) {
            const double den = (double)N * 16777216.0;
            mean_pitch[g] = N ? (double)sums[2 * g] / den : __builtin_nan("");
            mean_loudness[g] = N ? (double)sums[2 * g + 1] / den : __builtin_nan("");
            count[g] = (long)N;
        }
        DDSP_WAVE_ORDER();                                      // the next group overwrites cum
    }
}

__global__ void __launch_bounds__(kThreads) condition_apply_kernel(const float *__restrict__ f0, const float *__restrict__ cents,
                                                                   const float *__restrict__ loud, const float *__restrict__ S,
                                                                   const double *__restrict__ s_mean, const long *__restrict__ s_count,
                                                                   const float *__restrict__ Tt, const double *__restrict__ t_mean,
                                                                   const float *__restrict__ strength_rows, float *__restrict__ f0_out,
                                                                   float *__restrict__ cents_out, float *__restrict__ loud_out,
                                                                   int *__restrict__ octaves_out, long *__restrict__ count_out, long B,
                                                                   long T, int Q, int flags, int octaves,
                                                                   float strength, int min_frames)
{
    __shared__ float src[kMaxQ + 1], tgt[kMaxQ + 1];
    const int tid = threadIdx.x;

    // flags: bit 0 a source table per row, bit 1 a target table per row, bits 2.. the octave mode; `octaves` is the forced shift
    // (FORCED) or the largest one (AUTO)
    const int mode = flags >> 2;
    const long tile = blockIdx.x;                               // grid: a row's tiles in x, the rows over y and z
    const long row = (long)blockIdx.z * gridDim.y + blockIdx.y;
    if (row < B) {
        const long gs = flags & 1 ? row : 0, gt = flags & 2 ? row : 0;
        int bad = 0;
        for (int k = tid; k <= Q; k += kThreads) {
            const float a = S[gs * (Q + 1) + k], b = Tt[gt * (Q + 1) + k];
            src[k] = a;
            tgt[k] = b;
            bad |= (a != a) | (b != b);
        }
        bad = __syncthreads_or(bad);                            // (and the tables are staged)
        const long have = s_count[gs];
        const bool keep = bad || have < min_frames;             // too little to go on: the row as it came
        int oct = 0;
        if (!keep && mode == DDSP_CONDITION_OCTAVES_FORCED) oct = octaves;
        if (!keep && mode == DDSP_CONDITION_OCTAVES_AUTO) {
            double x = rint(((t_mean[gt] - s_mean[gs]) * 7180.0) / 1200.0);       // ties to even
            if (fabs(x) <= 1.0e9) {                                               // (not a NaN, not infinite)
                const double cap = (double)octaves;
                x = x < -cap ? -cap : (x > cap ? cap : x);
                oct = (int)x;
            }
        }
        const float step = (float)(((double)oct * 1200.0) / 7180.0);
        const float mix = strength_rows ? strength_rows[row] : strength;
        const long t = tile * kThreads + tid;
        if (t < T) {
            const long i = row * T + t;
            const float f = f0[i], n = cents[i], l = loud[i];
            float fo = f, no = n, lo = l;
            if (!keep) {
                fo = ldexpf(f, oct);
                no = __fadd_rn(n, step);
                if (fabsf(l) < INFINITY) {                      // a loudness that is not finite passes through
                    float mapped;
                    if (l < src[0]) {
                        mapped = __fadd_rn(l, __fsub_rn(tgt[0], src[0]));
                    } else if (l >= src[Q]) {
                        mapped = __fadd_rn(l, __fsub_rn(tgt[Q], src[Q]));
                    } else {
                        int a = 0, e = Q;                       // src[a] <= l < src[e] throughout
                        while (e - a > 1) {
                            const int m = (a + e) >> 1;
                            if (src[m] <= l) a = m; else e = m;
                        }
                        const float d = __fsub_rn(src[a + 1], src[a]);
                        const float w = d > 0.0f ? __fdiv_rn(__fsub_rn(l, src[a]), d) : 0.5f;
                        mapped = __fadd_rn(tgt[a], __fmul_rn(w, __fsub_rn(tgt[a + 1], tgt[a])));
                    }
                    lo = __fadd_rn(l, __fmul_rn(mix, __fsub_rn(mapped, l)));
                }
            }
            f0_out[i] = fo;
            cents_out[i] = no;
            loud_out[i] = lo;
        }
        if (tile == 0 && tid == 0) {
            if (octaves_out) octaves_out[row] = oct;
            if (count_out) count_out[row] = have;
        }
    }
}

inline size_t hist_bytes(long groups, int bins) { return ((size_t)groups * (size_t)bins * 4 + 7) & ~(size_t)7; }

// lo < hi, both finite, and a finite positive cell scale
inline bool cells_ok(int bins, float lo, float hi, float *scale)
{
    if (bins < 1 || bins > kMaxBins || !(hi > lo) || !(fabsf(lo) < INFINITY) || !(fabsf(hi) < INFINITY)) return false;
    const float span = hi - lo, s = (float)bins / span;
    if (!(s > 0.0f) || !(s < INFINITY)) return false;
    *scale = s;
    return true;
}

}  // namespace

extern "C" size_t ddsp_condition_accum_bytes(long groups, int bins)
{
    if (groups <= 0 || bins < 1 || bins > kMaxBins || groups > (1l << 32)) return 0;
    return hist_bytes(groups, bins) + (size_t)groups * 16;
}

extern "C" int ddsp_condition_launch_shape(int pooled, long rows, long T, int *blocks, long *unit_frames)
{
    if (!blocks || !unit_frames || rows < 0 || T <= 0) return DDSP_EINVAL;
    long frames;
    if (__builtin_mul_overflow(rows, T, &frames) || frames >= (1l << 32)) return DDSP_ERANGE;
    const long units = pooled ? (frames + kChunk - 1) / kChunk : rows;
    const long cap = pooled ? kPooledBlocks : kMaxBlocks;
    *blocks = (int)(units < cap ? units : cap);
    *unit_frames = pooled ? kChunk : T;
    return 0;
}

extern "C" int ddsp_condition_stats(const float *loudness, const float *cents, const float *harmonicity, const uint8_t *voiced,
                                    void *accum, long rows, long T, int pooled, int bins, float lo, float hi, float silence,
                                    float confidence, void *stream)
{
    float scale = 0.0f;
    if (rows < 0 || T <= 0 || !cells_ok(bins, lo, hi, &scale) || silence != silence || confidence != confidence) return DDSP_EINVAL;
    if (rows == 0) return 0;
    if (!loudness || !cents || !harmonicity || !accum) return DDSP_EINVAL;
    int blocks;
    long unit_frames;
    const int rc = ddsp_condition_launch_shape(pooled, rows, T, &blocks, &unit_frames);
    if (rc) return rc;
    const long frames = rows * T;
    if ((pooled ? frames : T) > kMaxGroupFrames) return DDSP_ERANGE;      // the fixed-point sums stay below 2^63
    const long groups = pooled ? 1 : rows;
    uint32_t *hist = (uint32_t *)accum;
    unsigned long long *sums = (unsigned long long *)((char *)accum + hist_bytes(groups, bins));
    if (pooled) {
        const hipError_t e = hipMemsetAsync(accum, 0, hist_bytes(1, bins) + 16, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    const long units = pooled ? (frames + unit_frames - 1) / unit_frames : rows;
    hipLaunchKernelGGL(condition_stats_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, loudness, cents,
                       harmonicity, voiced, hist, sums, units, unit_frames, frames, pooled ? 1 : 0, bins, lo, scale, silence, confidence);
    return (int)hipGetLastError();
}

extern "C" int ddsp_condition_tables(const void *accum, float *tables, double *mean_pitch, double *mean_loudness, long *frames,
                                     long groups, int bins, int quantiles, float lo, float hi, void *stream)
{
    float scale = 0.0f;
    if (groups < 0 || !cells_ok(bins, lo, hi, &scale) || quantiles < 1 || quantiles > kMaxQ) return DDSP_EINVAL;
    if (groups == 0) return 0;
    if (!accum || !tables || !mean_pitch || !mean_loudness || !frames) return DDSP_EINVAL;
    if (groups > (1l << 32)) return DDSP_ERANGE;
    const uint32_t *hist = (const uint32_t *)accum;
    const long long *sums = (const long long *)((const char *)accum + hist_bytes(groups, bins));
    const int blocks = (int)(groups < kMaxBlocks ? groups : kMaxBlocks);
    hipLaunchKernelGGL(condition_tables_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, hist, sums, tables, mean_pitch,
                       mean_loudness, frames, groups, bins, quantiles, lo, hi);
    return (int)hipGetLastError();
}

extern "C" int ddsp_condition_apply(const float *f0, const float *cents, const float *loudness, const float *source_tables,
                                    const double *source_mean_pitch, const long *source_frames, const float *target_tables,
                                    const double *target_mean_pitch, const float *strength_rows, float *f0_out, float *cents_out,
                                    float *loudness_out, int *octaves_out, long *frames_out, long B, long T, long source_groups,
                                    long target_groups, int quantiles, int octave_mode, int octaves, int max_octaves, float strength,
                                    long min_frames, void *stream)
{
    if (B < 0 || T <= 0 || quantiles < 1 || quantiles > kMaxQ || octave_mode < DDSP_CONDITION_OCTAVES_OFF ||
        octave_mode > DDSP_CONDITION_OCTAVES_FORCED || max_octaves < 0 || max_octaves > DDSP_CONDITION_MAX_OCTAVES ||
        octaves < -DDSP_CONDITION_MAX_OCTAVES || octaves > DDSP_CONDITION_MAX_OCTAVES || strength != strength)
        return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!f0 || !cents || !loudness || !source_tables || !source_mean_pitch || !source_frames || !target_tables || !target_mean_pitch ||
        !f0_out || !cents_out || !loudness_out || (source_groups != 1 && source_groups != B) || (target_groups != 1 && target_groups != B))
        return DDSP_EINVAL;
    long frames;
    if (__builtin_mul_overflow(B, T, &frames) || frames >= (1l << 32)) return DDSP_ERANGE;
    const long tiles = (T + kThreads - 1) / kThreads;
    if (B * tiles > kMaxTiles) return DDSP_ERANGE;                      // (a launch holds fewer than 2^32 threads)
    const long gy = B < kGridY ? B : kGridY, gz = (B + gy - 1) / gy;     // (B <= 2^23: gz <= 129)
    hipLaunchKernelGGL(condition_apply_kernel, dim3((unsigned)tiles, (unsigned)gy, (unsigned)gz), dim3(kThreads), 0,
                       (hipStream_t)stream, f0, cents, loudness, source_tables, source_mean_pitch, source_frames, target_tables, target_mean_pitch, strength_rows, f0_out, cents_out,
                       loudness_out, octaves_out, frames_out, B, T, quantiles,
                       (source_groups > 1 ? 1 : 0) | (target_groups > 1 ? 2 : 0) | (octave_mode << 2),
                       octave_mode == DDSP_CONDITION_OCTAVES_FORCED ? octaves : max_octaves, strength,
                       (int)(min_frames < 0 ? 0 : (min_frames > (1l << 30) ? (1l << 30) : min_frames)));    // (a count is below 2^25)
    return (int)hipGetLastError();
}
