// Auto-tune: how a performance is tuned, and its notes moved onto a scale with vibrato and inflection
// kept.  Positions are integers counting 2^-16 cent on the MIDI scale (include/ddsp_hip.h has the definition).  Three kernels:
//   tuning_stats_kernel     the on frames' pitch-class histogram, 1200 one-cent cells.  Built like condition_stats_kernel: one
//                           workgroup per unit, units walked grid-strided; a unit is a row (per-row mode: plain stores) or kChunk
//                           consecutive frames of the whole set (pooled mode: one LDS histogram over all of a workgroup's units,
//                           its non-zero cells merged once with integer atomicAdd behind the launcher's hipMemsetAsync).
//   tuning_estimate_kernel  one wavefront per group: the histogram staged in LDS, folded to 100 deviations, the 100 costs (lane k
//                           and k + 64 each walk the 100 deviations), an argmin butterfly under the tie order, the 12 profile
//                           sums, and lane 0's 12 x 12 root scores.
//   tuning_apply_kernel     one wavefront per row, four sweeps over tiles of 64 frames, the row's intermediates (32 bytes per
//                           frame) in LDS, or in the caller's workspace for rows beyond kLdsFrames:
//                             1  position, nearest allowed note, the note recurrence (a ballot finds the first lane that leaves
//                                the running note: one iteration per note change, not per frame; these three live in
//                                ddsp_tuning_common.h, which the note kernels of ddsp_notes.hip share), an int64 prefix sum of the
//                                positions, max-scans for the frame a note and a run of on frames began at
//                             2  a note's last frame forms its length, its sum and its correction, and leaves it at the note's
//                                first frame; a run's last frame leaves its index at the run's first frame
//                             3  the frames' corrections and their int64 prefix sum
//                             4  the glide window inside the run, the amount, the outputs
// Every index into LDS or global memory is a frame index in [0, T), a cell in [0, 1200) formed by a floor-mod, or a pitch class
// in [0, 12) formed by one.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_tuning_common.h"

namespace {

using namespace ddsp_tuning;

constexpr int kThreads = 256;
constexpr int kCells = DDSP_TUNING_CELLS;
constexpr int kLdsFrames = DDSP_TUNING_LDS_FRAMES;
constexpr int kFrameBytes = 32;                 // apply: one int64 and six ints per frame
constexpr int kMaxBlocks = 2048;                // rows in flight (statistics per row, estimate)
constexpr int kPooledBlocks = 512;              // workgroups that merge into one pooled histogram
constexpr long kChunk = 1024;                   // frames of one pooled unit
constexpr long kMaxGroupFrames = 1l << 24;      // frames of one statistic

__global__ void __launch_bounds__(kThreads) tuning_stats_kernel(const float *__restrict__ cents, const float *__restrict__ harm,
                                                                const float *__restrict__ loud, const uint8_t *__restrict__ voiced,
                                                                uint32_t *__restrict__ hist, long units, long unit_frames, long frames,
                                                                int pooled, float silence, float confidence)
{
    __shared__ uint32_t cell[kCells];
    const int tid = threadIdx.x;
    for (int b = tid; b < kCells; b += kThreads) cell[b] = 0;
    __syncthreads();

    for (long u = blockIdx.x; u < units; u += gridDim.x) {
        const long begin = u * unit_frames;
        const long end = begin + unit_frames < frames ? begin + unit_frames : frames;
        for (long i = begin + tid; i < end; i += kThreads) {
            const float n = cents[i];
            if (frame_on(n, harm, loud, voiced, i, silence, confidence))
                atomicAdd(&cell[floor_mod(position(n) + 32768, kOctave) >> 16], 1u);      // (|position| + 2^15 < 2^31)
        }
        if (!pooled) {                                          // the row's own histogram, with plain stores
            __syncthreads();
            for (int b = tid; b < kCells; b += kThreads) {
                hist[u * kCells + b] = cell[b];
                cell[b] = 0;
            }
            __syncthreads();                                    // the next row starts from zeroed cells
        }
    }
    if (pooled) {                                               // one merge per workgroup
        __syncthreads();
        for (int b = tid; b < kCells; b += kThreads) {
            const uint32_t v = cell[b];
            if (v) atomicAdd(&hist[b], v);
        }
    }
}

// the order of two (cost, offset) candidates: the smaller cost, then the smaller |o|, then the non-negative one
__device__ __forceinline__ bool better(long long ca, int oa, long long cb, int ob)
{
    if (ca != cb) return ca < cb;
    const int aa = oa < 0 ? -oa : oa, ab = ob < 0 ? -ob : ob;
    if (aa != ab) return aa < ab;
    return oa > ob;
}

__global__ void __launch_bounds__(64) tuning_estimate_kernel(const uint32_t *__restrict__ hist, int *__restrict__ offset,
                                                             int *__restrict__ root, long *__restrict__ profile,
                                                             long *__restrict__ count, long groups, int mask, int forced_root)
{
    __shared__ uint32_t h[kCells];
    __shared__ long long fold[100];
    __shared__ long long prof[12];
    const int lane = threadIdx.x;

    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        for (int i = lane; i < kCells; i += 64) h[i] = hist[g * kCells + i];
        DDSP_WAVE_ORDER();
        long long n = 0;
        for (int d = lane; d < 100; d += 64) {
            long long s = 0;
#pragma unroll
            for (int p = 0; p < 12; ++p) s += h[100 * p + d];
            fold[d] = s;
            n += s;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        DDSP_WAVE_ORDER();
        long long best = LLONG_MAX;
        int best_o = 0;
        for (int k = lane; k < 100; k += 64) {
            const int o = k - 50;
            long long cost = 0;
            for (int d = 0; d < 100; ++d) {
                const int a = floor_mod(d - o, 100), b = a ? 100 - a : 0;
                cost += fold[d] * (a < b ? a : b);
            }
            if (better(cost, o, best, best_o)) { best = cost; best_o = o; }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const long long oc = __shfl_xor(best, s);
            const int oo = __shfl_xor(best_o, s);
            if (better(oc, oo, best, best_o)) { best = oc; best_o = oo; }
        }
        const int o = n ? best_o : 0;                           // (every lane holds the same winner: the order is total)
        if (lane < 12) {
            long long s = 0;
            for (int j = -50; j < 50; ++j) s += h[floor_mod(100 * lane + o + j, kCells)];
            prof[lane] = s;
            profile[g * 12 + lane] = (long)s;
        }
        DDSP_WAVE_ORDER();
        if (lane == 0) {
            int r_best = forced_root >= 0 ? forced_root : 0;
            if (forced_root < 0) {
                long long s_best = -1;
                for (int r = 0; r < 12; ++r) {
                    long long s = 0;
                    for (int p = 0; p < 12; ++p) s += (mask >> floor_mod(p - r, 12)) & 1 ? prof[p] : 0;
                    if (s > s_best) { s_best = s; r_best = r; }     // ties stay with the smallest r
                }
            }
            offset[g] = o;
            root[g] = r_best;
            count[g] = (long)n;
        }
        DDSP_WAVE_ORDER();                                      // the next group overwrites h, fold and prof
    }
}

template <bool kLds>
__global__ void __launch_bounds__(64)
tuning_apply_kernel(const float *__restrict__ f0, const float *__restrict__ cents, const float *__restrict__ harm,
                    const float *__restrict__ loud, const uint8_t *__restrict__ voiced, const int *__restrict__ offset,
                    const int *__restrict__ root, const float *__restrict__ amount_rows, float *__restrict__ f0_out,
                    float *__restrict__ cents_out, int *__restrict__ notes_out, int *__restrict__ correction_out,
                    unsigned char *__restrict__ workspace, int T, int per_row, int mask, int forced_root, long long hysteresis,
                    int min_note, int glide, int flags, float amount, float silence, float confidence)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tune_lds[];
    __shared__ int step_down[12], step_up[12];  // from a pitch class (relative to the root): semitones to the allowed note at or below, and from the next class to the one above
    const int lane = threadIdx.x;
    const long row = blockIdx.x;
    unsigned char *store = kLds ? tune_lds : workspace + row * (long)T * kFrameBytes;
    long long *sums = (long long *)store;       // pass 1: prefix sums of the positions; pass 3: of the corrections
    int *pos_at = (int *)(sums + T);            // the position u, kOff for an off frame
    int *note_at = pos_at + T;                  // note_t, kOff for an off frame
    int *note_first = note_at + T;              // the frame this frame's note began at
    int *run_first = note_first + T;            // the frame this frame's run of on frames began at
    int *note_corr = run_first + T;             // at a note's first frame: its correction (vibrato) or whether it is corrected
    int *run_last = note_corr + T;              // at a run's first frame: its last frame

    const long g = per_row ? row : 0;
    const int o = clamp_offset(offset[g]);
    const int rt = forced_root >= 0 ? forced_root : floor_mod(root[g], 12);
    const long long shift = 65536ll * o, conc = flags & DDSP_TUNING_CONCERT ? shift : 0;
    const bool vibrato = flags & DDSP_TUNING_VIBRATO;
    fill_steps(step_down, step_up, mask, lane);
    __syncthreads();
    const long base = row * (long)T;
    const float *nrow = cents + base;

    // 1
    int cur = 0, prev_on = 0, note_carry = -1, run_carry = -1;
    long long sum_carry = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        const float n = in ? nrow[t] : NAN;
        const bool on = in && frame_on(n, harm, loud, voiced, base + t, silence, confidence);
        const int u = on ? position(n) : kOff;
        const long long v = on ? (long long)u - shift : 0;
        const int q = on ? nearest_allowed(v, rt, step_down, step_up) : 0;
        int before_on = __shfl_up((int)on, 1);
        if (lane == 0) before_on = prev_on;
        const bool fresh = on && !before_on;                                    // a run of on frames begins
        const int before_note = prev_on ? cur : kOff;                           // the note of frame t0 - 1
        const int note = tile_notes(on, fresh, v, q, hysteresis, cur, lane);
        int pn = __shfl_up(note, 1);
        if (lane == 0) pn = before_note;
        int nf = scan_max(on && pn != note ? t : -1, lane);
        nf = nf > note_carry ? nf : note_carry;
        int rf = scan_max(fresh ? t : -1, lane);
        rf = rf > run_carry ? rf : run_carry;
        const long long p = scan_sum(v, lane) + sum_carry;
        if (in) {
            sums[t] = p;
            pos_at[t] = u;
            note_at[t] = note;
            note_first[t] = nf;
            run_first[t] = rf;
        }
        note_carry = __shfl(nf, 63);
        run_carry = __shfl(rf, 63);
        sum_carry = __shfl(p, 63);
        prev_on = __shfl((int)on, 63);                                          // (lane 63 on: its note is cur)
    }
    __syncthreads();

    // 2
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        if (t < T && pos_at[t] != kOff) {
            const int note = note_at[t];
            const int next = t + 1 < T ? note_at[t + 1] : kOff;                 // (an off frame's note is kOff)
            if (next != note) {
                const int s = note_first[t];
                const long long L = t - s + 1;
                int value = 0;
                if (L >= min_note) {
                    const long long total = sums[t] - (s > 0 ? sums[s - 1] : 0);
                    value = vibrato ? (int)(rdiv(note * kSemitone * L - total, L) - conc) : 1;
                }
                note_corr[s] = value;
            }
            if (next == kOff) run_last[run_first[t]] = t;
        }
    }
    __syncthreads();

    // 3
    sum_carry = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        long long c = 0;
        if (in && pos_at[t] != kOff) {
            const int value = note_corr[note_first[t]];
            c = vibrato ? value : (value ? note_at[t] * kSemitone - ((long long)pos_at[t] - shift) - conc : 0);
        }
        const long long p = scan_sum(c, lane) + sum_carry;
        if (in) sums[t] = p;
        sum_carry = __shfl(p, 63);
    }
    __syncthreads();

    // 4
    float mix = amount_rows ? amount_rows[row] : amount;
    mix = mix >= 0.0f ? (mix <= 1.0f ? mix : 1.0f) : 0.0f;                      // (a NaN is 0)
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        if (t < T) {
            const float n = nrow[t], f = f0[base + t];
            float no = n, fo = f;
            long long d = 0;
            if (pos_at[t] != kOff) {
                const int first = run_first[t], last = run_last[first];
                const int a = t - glide > first ? t - glide : first, b = t + glide < last ? t + glide : last;
                const long long total = sums[b] - (a > 0 ? sums[a - 1] : 0);
                d = llrint((double)mix * (double)rdiv(total, b - a + 1));
            }
            if (d) {
                no = n + (float)((double)d / (65536.0 * 7180.0));
                fo = (float)((double)f * exp2((double)d / (65536.0 * 1200.0)));
            }
            cents_out[base + t] = no;
            f0_out[base + t] = fo;
            if (notes_out) notes_out[base + t] = note_at[t];
            if (correction_out) correction_out[base + t] = (int)d;
        }
    }
}

inline bool launch_shape(int pooled, long rows, long T, int *blocks, long *unit_frames, long *units)
{
    long frames;
    if (__builtin_mul_overflow(rows, T, &frames) || frames >= (1l << 32)) return false;
    *units = pooled ? (frames + kChunk - 1) / kChunk : rows;
    const long cap = pooled ? kPooledBlocks : kMaxBlocks;
    *blocks = (int)(*units < cap ? *units : cap);
    *unit_frames = pooled ? kChunk : T;
    return true;
}

}  // namespace

extern "C" size_t ddsp_tuning_accum_bytes(long groups)
{
    if (groups <= 0 || groups > (1l << 32)) return 0;
    return (size_t)groups * kCells * 4;
}

extern "C" int ddsp_tuning_stats(const float *cents, const float *harmonicity, const float *loudness, const uint8_t *voiced,
                                 void *accum, long rows, long T, int pooled, float silence, float confidence, void *stream)
{
    if (rows < 0 || T <= 0 || silence != silence || confidence != confidence) return DDSP_EINVAL;
    if (rows == 0) return 0;
    if (!cents || !accum) return DDSP_EINVAL;
    int blocks;
    long unit_frames, units;
    if (!launch_shape(pooled, rows, T, &blocks, &unit_frames, &units)) return DDSP_ERANGE;
    const long frames = rows * T;
    if ((pooled ? frames : T) > kMaxGroupFrames) return DDSP_ERANGE;
    if (pooled) {
        const hipError_t e = hipMemsetAsync(accum, 0, (size_t)kCells * 4, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(tuning_stats_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, cents, harmonicity, loudness,
                       voiced, (uint32_t *)accum, units, unit_frames, frames, pooled ? 1 : 0, silence, confidence);
    return (int)hipGetLastError();
}

extern "C" int ddsp_tuning_estimate(const void *accum, int *offset, int *root, long *profile, long *frames, long groups, int mask,
                                    int forced_root, void *stream)
{
    if (groups < 0 || mask <= 0 || mask > 0xFFF || forced_root < -1 || forced_root > 11) return DDSP_EINVAL;
    if (groups == 0) return 0;
    if (!accum || !offset || !root || !profile || !frames) return DDSP_EINVAL;
    if (groups > (1l << 32)) return DDSP_ERANGE;
    const int blocks = (int)(groups < kMaxBlocks ? groups : kMaxBlocks);
    hipLaunchKernelGGL(tuning_estimate_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, (const uint32_t *)accum, offset,
                       root, profile, frames, groups, mask, forced_root);
    return (int)hipGetLastError();
}

extern "C" size_t ddsp_tuning_workspace_bytes(long B, long T)
{
    if (B <= 0 || T <= kLdsFrames || T >= kMaxRowFrames || B > (1l << 31) / T) return 0;
    return (size_t)B * (size_t)T * kFrameBytes;
}

extern "C" int ddsp_tuning_apply(const float *f0, const float *cents, const float *harmonicity, const float *loudness,
                                 const uint8_t *voiced, const int *offset, const int *root, const float *amount_rows, float *f0_out,
                                 float *cents_out, int *notes_out, int *correction_out, void *workspace, long B, long T, long groups,
                                 int mask, int forced_root, long hysteresis, long min_note_frames, long glide, int flags, float amount,
                                 float silence, float confidence, void *stream)
{
    if (B < 0 || T <= 0 || mask <= 0 || mask > 0xFFF || forced_root < -1 || forced_root > 11 || hysteresis < 0 ||
        hysteresis > kMaxHysteresis || min_note_frames < 0 || glide < 0 || (flags & ~(DDSP_TUNING_VIBRATO | DDSP_TUNING_CONCERT)) ||
        silence != silence || confidence != confidence || (!amount_rows && !(amount >= 0.0f && amount <= 1.0f)))
        return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!f0 || !cents || !offset || (!root && forced_root < 0) || !f0_out || !cents_out || (groups != 1 && groups != B)) return DDSP_EINVAL;
    long frames;
    if (T >= kMaxRowFrames || __builtin_mul_overflow(B, T, &frames) || frames >= (1l << 31)) return DDSP_ERANGE;
    const int min_note = (int)(min_note_frames > T + 1 ? T + 1 : min_note_frames);       // (a note is at most T frames long)
    const int reach = (int)(glide > T ? T : glide);                                       // (and so is a run)
    hipStream_t s = (hipStream_t)stream;
    if (T <= kLdsFrames) {
        hipLaunchKernelGGL(tuning_apply_kernel<true>, dim3((unsigned)B), dim3(64), (size_t)T * kFrameBytes, s, f0, cents, harmonicity,
                           loudness, voiced, offset, root, amount_rows, f0_out, cents_out, notes_out, correction_out,
                           (unsigned char *)nullptr, (int)T, groups > 1 ? 1 : 0, mask, forced_root, (long long)hysteresis, min_note, reach,
                           flags, amount, silence, confidence);
    } else {
        if (!workspace) return DDSP_EINVAL;
        hipLaunchKernelGGL(tuning_apply_kernel<false>, dim3((unsigned)B), dim3(64), 0, s, f0, cents, harmonicity, loudness, voiced, offset,
                           root, amount_rows, f0_out, cents_out, notes_out, correction_out, (unsigned char *)workspace, (int)T,
                           groups > 1 ? 1 : 0, mask, forced_root, (long long)hysteresis, min_note, reach, flags, amount, silence,
                           confidence);
    }
    return (int)hipGetLastError();
}
