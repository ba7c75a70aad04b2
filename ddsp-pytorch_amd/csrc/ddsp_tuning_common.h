// What the auto-tune kernels (ddsp_tuning.hip) and the note kernels (ddsp_notes.hip, section 10f) share:
// the position of a frame, the on test, the two 12-entry nearest-allowed tables, the note recurrence over a tile of 64 frames,
// and the integer helpers of the definition in include/ddsp_hip.h.  One copy, so that both see the same notes to the bit.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

namespace ddsp_tuning {

constexpr long kMaxRowFrames = 1l << 24;        // T below it keeps 2 |note S L| and every prefix sum far below 2^63
constexpr long long kSemitone = 100ll * 65536;
constexpr int kOctave = 12 * 100 * 65536;
constexpr long long kMaxHysteresis = 1200ll * 65536;
constexpr double kOrigin = 2346.0614660728625;  // 1997.3794084376191 - 1200 log2(44) + 6900
constexpr int kOff = INT_MIN;

__device__ __forceinline__ bool frame_on(float n, const float *harm, const float *loud, const uint8_t *voiced, long i, float silence,
                                         float confidence)
{
    bool on = fabsf(n) <= 4.0f;                 // (a NaN fails every comparison)
    if (harm) on = on && harm[i] >= confidence;
    if (loud) on = on && loud[i] > silence;
    if (voiced) on = on && voiced[i] != 0;
    return on;
}

// |n| <= 4: |7180 n + K| < 31067 cents, the position's magnitude below 2^31.  The product is exact, the sum rounds once.
__device__ __forceinline__ int position(float n) { return (int)llrint((7180.0 * (double)n + kOrigin) * 65536.0); }

__device__ __forceinline__ int floor_mod(int a, int b)
{
    const int m = a % b;
    return m < 0 ? m + b : m;
}

__device__ __forceinline__ long long floor_div(long long a, long long b)     // b > 0
{
    const long long q = a / b;
    return (a % b) < 0 ? q - 1 : q;
}

__device__ __forceinline__ long long rdiv(long long a, long long b) { return floor_div(2 * a + b, 2 * b); }

__device__ __forceinline__ long long magnitude(long long a) { return a < 0 ? -a : a; }

// an offset as the kernels use it (an estimate lies in -50 .. 49; a hand-made one is kept inside the arithmetic's range)
__device__ __forceinline__ int clamp_offset(int o) { return o < -50 ? -50 : (o > 50 ? 50 : o); }

template <typename V>
__device__ __forceinline__ V scan_sum(V v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const V up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

__device__ __forceinline__ int scan_max(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(v, o);
        if (lane >= o && up > v) v = up;
    }
    return v;
}

// Lanes 0 .. 11 fill the two tables (in LDS; the caller synchronises): from a pitch class (relative to the root), semitones to
// the allowed note at or below, and from the next class to the one above.
__device__ __forceinline__ void fill_steps(int *step_down, int *step_up, int mask, int lane)
{
    if (lane < 12) {
        int k = 0;
        while (k < 11 && !((mask >> floor_mod(lane - k, 12)) & 1)) ++k;       // (mask != 0: one of twelve is allowed)
        step_down[lane] = k;
        k = 0;
        while (k < 11 && !((mask >> floor_mod(lane + 1 + k, 12)) & 1)) ++k;
        step_up[lane] = k;
    }
}

// the allowed note nearest to v (relative to the performance's own grid), ties to the lower note
__device__ __forceinline__ int nearest_allowed(long long v, int rt, const int *step_down, const int *step_up)
{
    const int c = (int)floor_div(v, kSemitone), rel = floor_mod(c - rt, 12);
    const int lo = c - step_down[rel], hi = c + 1 + step_up[rel];
    return v - lo * kSemitone <= hi * kSemitone - v ? lo : hi;
}

// The note recurrence over one tile of 64 frames, one frame per lane: a ballot finds the first lane that leaves the running
// note `cur` (wave-uniform, carried from tile to tile), so the loop takes one turn per note change, not per frame.
// -> the lane's note_t, kOff for an off frame.
__device__ __forceinline__ int tile_notes(bool on, bool fresh, long long v, int q, long long hysteresis, int &cur, int lane)
{
    const long long reach = on ? magnitude(v - q * kSemitone) + hysteresis : 0;
    int note = kOff, from = 0;
    for (;;) {
        const bool leaves = on && lane >= from && (fresh || magnitude(v - cur * kSemitone) > reach);
        const unsigned long long m = __ballot(leaves);
        if (!m) {
            if (on && lane >= from) note = cur;
            break;
        }
        const int first = __ffsll((long long)m) - 1;
        if (on && lane >= from && lane < first) note = cur;
        cur = __shfl(q, first);
        if (lane == first) note = cur;
        from = first + 1;
        if (from >= 64) break;
    }
    return note;
}

}  // namespace ddsp_tuning
