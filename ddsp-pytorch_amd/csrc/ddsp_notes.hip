// Notes: the note events of a pitch track, and note events rendered back to frame-rate controls.
// Positions are integers counting 2^-16 cent on the MIDI scale, as in ddsp_tuning.hip (include/ddsp_hip.h has the definition).
//   notes_extract_kernel   one wavefront per row (a workgroup each, as tuning_apply_kernel: walking the rows grid-strided keeps
//                          every pointer live across the loop and spills scalar registers), tiles of 64 frames, no per-frame storage.  A tile's
//                          notes come from the recurrence ddsp_tuning_common.h shares with tuning_apply_kernel.  A note is emitted
//                          by the frame AFTER its last one (so a note still open at a tile's end is emitted by the next tile; the
//                          tiles run up to frame T, which is off, for a note that ends with the row); what crosses a tile boundary is wave-uniform: the running note, the open
//                          note's first frame, its sum of v and its largest level so far, the kept notes so far, whether the last
//                          frame was on.  Inside a tile one segmented scan (heads at the notes' first frames) carries the int64
//                          sum and the level's maximum together; a ballot of the emitting lanes and a popcount of the lower ones
//                          give the output slot.
//   notes_render_kernel    one thread per output frame, a workgroup per tile of 256 frames of one row.  Two binary searches on
//                          the row's onsets bound the notes the tile can touch; those records (and one either side, for the
//                          glide and the release) are staged in LDS when they fit, else read from global memory; each thread
//                          then searches its own note.
// Every record index is in [0, min(count, N)) and every frame index in [0, T), whatever the records hold: unsorted onsets give
// unspecified values, never an access out of bounds.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_tuning_common.h"

namespace {

using namespace ddsp_tuning;

constexpr int kTile = 256;                      // render: frames of one workgroup
constexpr int kStage = 320;                     // render: records staged in LDS (20 bytes each)
constexpr long kMaxSteps = 1l << 24;            // render: glide, attack, release, delay and ramp stay below it
constexpr long long kMaxDetune = 1ll << 30;
constexpr long long kMaxTranspose = 128 * kSemitone;
constexpr long long kHold = 6900ll * 65536;     // render: the pitch held where no note gives one (A4)

// The larger of two levels under a total order, so that any order of the frames gives the same bits: a NaN never wins (the
// canonical NaN stands for "no level yet"), and +0 beats -0.
__device__ __forceinline__ float level_max(float a, float b)
{
    if (b != b) return a;
    if (a != a) return b;
    if (b > a) return b;
    if (b == a && signbit(a) && !signbit(b)) return b;
    return a;
}

__global__ void __launch_bounds__(64)
notes_extract_kernel(const float *__restrict__ cents, const float *__restrict__ harm, const float *__restrict__ loud,
                     const uint8_t *__restrict__ voiced, const int *__restrict__ offset, const int *__restrict__ root,
                     int *__restrict__ onset_out, int *__restrict__ frames_out, int *__restrict__ pitch_out,
                     int *__restrict__ detune_out, float *__restrict__ level_out, int *__restrict__ count_out, int T, int N,
                     int per_row, int mask, int forced_root, long long hysteresis, int min_note, int gate_loudness, float silence,
                     float confidence)
{
    __shared__ int step_down[12], step_up[12];
    const int lane = threadIdx.x;
    fill_steps(step_down, step_up, mask, lane);
    __syncthreads();
    const float *gate = gate_loudness ? loud : nullptr;
    const unsigned long long below = (1ull << lane) - 1;

    const long row = blockIdx.x;
    const long g = per_row ? row : 0;
    const int rt = forced_root >= 0 ? forced_root : floor_mod(root[g], 12);
    const long long shift = 65536ll * clamp_offset(offset[g]);
    const long base = row * (long)T, slot0 = row * (long)N;
    const float *nrow = cents + base;

    int cur = 0, prev_on = 0, first_carry = 0, kept = 0;
    long long sum_carry = 0;
    float level_carry = NAN;

    // (t0 <= T: frame T, which is off, emits a note that ends on the row's last frame, also where that ends a tile)
    for (int t0 = 0; t0 <= T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        const float n = in ? nrow[t] : NAN;
        const bool on = in && frame_on(n, harm, gate, voiced, base + t, silence, confidence);
        const long long v = on ? (long long)position(n) - shift : 0;
        const int q = on ? nearest_allowed(v, rt, step_down, step_up) : 0;
        int before_on = __shfl_up((int)on, 1);
        if (lane == 0) before_on = prev_on;
        const bool fresh = on && !before_on;
        const int before_note = prev_on ? cur : kOff;                       // the note of frame t0 - 1
        const int note = tile_notes(on, fresh, v, q, hysteresis, cur, lane);
        int pn = __shfl_up(note, 1);
        if (lane == 0) pn = before_note;
        const bool head = on && pn != note;                                 // a note begins here
        int nf = scan_max(head ? t : -1, lane);                             // the first frame of this frame's note
        nf = nf >= 0 ? nf : first_carry;

        // the note's sum of v and its largest level up to this frame: a segmented scan, the open note's carries entering at lane 0
        long long s = v;
        float lv = on && loud ? loud[base + t] : NAN;
        lv = lv != lv ? NAN : lv;                                           // (any NaN is "no level")
        if (lane == 0 && on && !head) {
            s += sum_carry;
            lv = level_max(level_carry, lv);
        }
        int flag = head;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long us = __shfl_up(s, o);
            const float ul = __shfl_up(lv, o);
            const int uf = __shfl_up(flag, o);
            if (lane >= o && !flag) {
                s += us;
                lv = level_max(lv, ul);
                flag = uf;
            }
        }

        // the frame after a note's last one emits it; lane 0 speaks for the note the last tile left open
        int e_first = __shfl_up(nf, 1);
        long long e_sum = __shfl_up(s, 1);
        float e_level = __shfl_up(lv, 1);
        if (lane == 0) {
            e_first = first_carry;
            e_sum = sum_carry;
            e_level = level_carry;
        }
        const long long L = (long long)t - e_first;                         // the note's last frame is t - 1
        const bool keep = pn != kOff && pn != note && L >= min_note;
        const unsigned long long m = __ballot(keep);
        const long slot = kept + __popcll(m & below);
        if (keep && slot < N) {
            onset_out[slot0 + slot] = e_first;
            frames_out[slot0 + slot] = (int)L;
            pitch_out[slot0 + slot] = pn;
            detune_out[slot0 + slot] = -(int)rdiv(pn * kSemitone * L - e_sum, L);     // minus the auto-tune's correction, ties included
            level_out[slot0 + slot] = e_level;
        }
        kept += __popcll(m);

        prev_on = __shfl((int)on, 63);                                      // (lane 63 on: its note is cur)
        first_carry = __shfl(nf, 63);
        sum_carry = __shfl(s, 63);
        level_carry = __shfl(lv, 63);
    }

    for (long i = (kept < N ? kept : N) + lane; i < N; i += 64) {
        onset_out[slot0 + i] = -1;
        frames_out[slot0 + i] = 0;
        pitch_out[slot0 + i] = INT_MIN;
        detune_out[slot0 + i] = 0;
        level_out[slot0 + i] = NAN;
    }
    if (lane == 0) count_out[row] = kept;
}

struct RenderOptions {
    long long transpose;                        // units
    long long glide, attack, release, delay, ramp;
    double depth, omega;                        // vibrato: units, radians per frame
    float floor_level, default_level;
    int flags;
};

// the number of i in [lo, hi) with onset_i <= t, the onsets taken as non-decreasing; `onset` points at record `origin`
__device__ __forceinline__ int onsets_upto(const int *onset, int origin, int lo, int hi, int t)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (onset[mid - origin] <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kTile)
notes_render_kernel(const int *__restrict__ onset_in, const int *__restrict__ frames_in, const int *__restrict__ pitch_in,
                    const int *__restrict__ detune_in, const float *__restrict__ level_in, const int *__restrict__ count,
                    const int *__restrict__ offset, float *__restrict__ f0_out, float *__restrict__ cents_out,
                    float *__restrict__ loud_out, float *__restrict__ harm_out, uint8_t *__restrict__ voiced_out,
                    long *__restrict__ position_out, int *__restrict__ owner_out, int T, int N, int tiles, int per_row, RenderOptions opt)
{
    __shared__ int s_onset[kStage], s_frames[kStage], s_pitch[kStage], s_detune[kStage];
    __shared__ float s_level[kStage];
    const long row = blockIdx.x / tiles;
    const int t0 = (int)(blockIdx.x % tiles) * kTile;
    const int t = t0 + threadIdx.x;
    const int t_last = t0 + kTile - 1 < T - 1 ? t0 + kTile - 1 : T - 1;
    const long rec0 = row * (long)N;
    int n = count[row];
    n = n < 0 ? 0 : (n > N ? N : n);

    // the notes the tile can touch: i* of its first frame up to i* of its last, one more below (the glide's note i - 1, and
    // i* itself sits one below the count of onsets passed) and one above (L' reads the next onset)
    const int *g_onset = onset_in + rec0;
    const int first = onsets_upto(g_onset, 0, 0, n, t0), last = onsets_upto(g_onset, 0, first, n, t_last);
    const int lo = first - 2 > 0 ? first - 2 : 0, hi = last + 1 < n ? last + 1 : n;
    const bool staged = hi - lo <= kStage;
    if (staged) {
        for (int i = lo + threadIdx.x; i < hi; i += kTile) {
            s_onset[i - lo] = g_onset[i];
            s_frames[i - lo] = frames_in[rec0 + i];
            s_pitch[i - lo] = pitch_in[rec0 + i];
            s_detune[i - lo] = detune_in[rec0 + i];
            s_level[i - lo] = level_in[rec0 + i];
        }
    }
    __syncthreads();
    if (t >= T) return;
    // Record i of the row, lo <= i < hi, is element i - lo of whichever copy there is.  (Every pointer stays inside its array: an
    // LDS array's address moved below its start wraps in the 32-bit LDS address space, and the flat address made from it lies
    // beyond the aperture.)
    const int *r_onset = staged ? s_onset : g_onset + lo, *r_frames = staged ? s_frames : frames_in + rec0 + lo;
    const int *r_pitch = staged ? s_pitch : pitch_in + rec0 + lo, *r_detune = staged ? s_detune : detune_in + rec0 + lo;
    const float *r_level = staged ? s_level : level_in + rec0 + lo;
    auto onset_of = [&](int i) { return (long long)r_onset[i - lo]; };
    auto frames_of = [&](int i) { return (long long)r_frames[i - lo]; };

    const long long shift = opt.flags & DDSP_NOTES_CONCERT ? 0 : 65536ll * clamp_offset(offset[per_row ? row : 0]);
    auto valid = [&](int i) {
        const long long d = r_detune[i - lo];
        const int pitch = r_pitch[i - lo];
        return frames_of(i) >= 1 && pitch >= 0 && pitch <= 127 && d >= -kMaxDetune && d <= kMaxDetune;
    };
    auto centre = [&](int i) {                                                  // b_i of a valid note
        return r_pitch[i - lo] * kSemitone + (opt.flags & DDSP_NOTES_KEEP_DETUNE ? r_detune[i - lo] : 0) + shift + opt.transpose;
    };

    const int i = onsets_upto(r_onset, lo, first, last, t) - 1;                 // i*, -1: before every onset
    long long p = kHold;
    double loudness = (double)opt.floor_level;
    int owner = -1;
    if (i < 0) {
        if (n > 0 && valid(0)) p = centre(0);
    } else if (valid(i)) {
        const long long b = centre(i), k = (long long)t - onset_of(i), frames = frames_of(i);
        p = b;
        if (k < frames) {
            owner = i;
            if (opt.glide > 0 && k < opt.glide && i > 0 && valid(i - 1) && onset_of(i) <= onset_of(i - 1) + frames_of(i - 1))
                p += rdiv((centre(i - 1) - b) * (opt.glide - k), opt.glide + 1);
            if (opt.depth > 0.0 && k >= opt.delay) {
                const double swell = (double)(k - opt.delay + 1) / (double)opt.ramp;
                p += llrint(opt.depth * (swell < 1.0 ? swell : 1.0) * sin(opt.omega * (double)(k - opt.delay)));
            }
            long long len = frames;                                             // L'
            if (i + 1 < n) {
                const long long gap = onset_of(i + 1) - onset_of(i);
                len = gap < len ? gap : len;
            }
            const float own = r_level[i - lo];
            const double lv = own != own ? (double)opt.default_level : (double)own;
            double ga = 1.0, gr = 1.0;
            if (opt.attack > 0) {
                ga = (double)(k + 1) / (double)opt.attack;
                ga = ga < 1.0 ? ga : 1.0;
            }
            if (opt.release > 0) {
                gr = (double)(len - k) / (double)opt.release;
                gr = gr < 1.0 ? gr : 1.0;
            }
            loudness = (double)opt.floor_level + (lv - (double)opt.floor_level) * ga * gr;
        }
    }
    const double c = (double)p / 65536.0;                                       // exact: |p| < 2^53
    const long at = row * (long)T + t;
    cents_out[at] = (float)((c - kOrigin) / 7180.0);
    f0_out[at] = (float)(440.0 * exp2((c - 6900.0) / 1200.0));
    loud_out[at] = (float)loudness;
    harm_out[at] = owner >= 0 ? 1.0f : 0.0f;
    voiced_out[at] = owner >= 0 ? 1 : 0;
    if (position_out) position_out[at] = (long)p;
    if (owner_out) owner_out[at] = owner;
}

}  // namespace

extern "C" int ddsp_notes_extract(const float *cents, const float *harmonicity, const float *loudness, const uint8_t *voiced,
                                  const int *offset, const int *root, int *onset, int *frames, int *pitch, int *detune, float *level,
                                  int *count, long B, long T, long N, long groups, int mask, int forced_root, long hysteresis,
                                  long min_note_frames, int gate_loudness, float silence, float confidence, void *stream)
{
    if (B < 0 || T <= 0 || N < 0 || mask <= 0 || mask > 0xFFF || forced_root < -1 || forced_root > 11 || hysteresis < 0 ||
        hysteresis > kMaxHysteresis || min_note_frames < 0 || silence != silence || confidence != confidence ||
        (gate_loudness != 0 && gate_loudness != 1))
        return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!cents || !offset || (!root && forced_root < 0) || !count || (groups != 1 && groups != B) || (gate_loudness && !loudness) ||
        (N > 0 && (!onset || !frames || !pitch || !detune || !level)))
        return DDSP_EINVAL;
    long total;
    if (T >= kMaxRowFrames || __builtin_mul_overflow(B, T, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    if (__builtin_mul_overflow(B, N, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    const int min_note = (int)(min_note_frames > T + 1 ? T + 1 : min_note_frames);       // (a note is at most T frames long)
    hipLaunchKernelGGL(notes_extract_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, cents, harmonicity, loudness,   // (B <= B T < 2^31)
                       voiced, offset, root, onset, frames, pitch, detune, level, count, (int)T, (int)N, groups > 1 ? 1 : 0, mask,
                       forced_root, (long long)hysteresis, min_note, gate_loudness, silence, confidence);
    return (int)hipGetLastError();
}

extern "C" int ddsp_notes_render(const int *onset, const int *frames, const int *pitch, const int *detune, const float *level,
                                 const int *count, const int *offset, float *f0, float *cents, float *loudness, float *harmonicity,
                                 uint8_t *voiced, long *position, int *owner, long B, long T, long N, long groups, int flags,
                                 long transpose, long glide, long attack, long release, long vibrato_delay, long vibrato_ramp,
                                 double vibrato_depth, double vibrato_omega, float floor_level, float default_level, void *stream)
{
    auto steps = [](long x) { return x >= 0 && x < kMaxSteps; };
    if (B < 0 || T <= 0 || N < 0 || (flags & ~(DDSP_NOTES_KEEP_DETUNE | DDSP_NOTES_CONCERT)) || transpose < -kMaxTranspose ||
        transpose > kMaxTranspose || !steps(glide) || !steps(attack) || !steps(release) || !steps(vibrato_delay) || vibrato_ramp < 1 ||
        !steps(vibrato_ramp) || !(vibrato_depth >= 0.0 && vibrato_depth <= (double)kMaxTranspose) || !(fabs(vibrato_omega) <= 1e6) ||
        !(fabsf(floor_level) <= 3.0e38f) || !(fabsf(default_level) <= 3.0e38f))
        return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!count || !offset || !f0 || !cents || !loudness || !harmonicity || !voiced || (groups != 1 && groups != B) ||
        (N > 0 && (!onset || !frames || !pitch || !detune || !level)))
        return DDSP_EINVAL;
    long total;
    if (T >= kMaxRowFrames || __builtin_mul_overflow(B, T, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    if (__builtin_mul_overflow(B, N, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    const long tiles = (T + kTile - 1) / kTile;                                 // B tiles <= B T < 2^31
    RenderOptions opt;
    opt.transpose = transpose;
    opt.glide = glide;
    opt.attack = attack;
    opt.release = release;
    opt.delay = vibrato_delay;
    opt.ramp = vibrato_ramp;
    opt.depth = vibrato_depth;
    opt.omega = vibrato_omega;
    opt.floor_level = floor_level;
    opt.default_level = default_level;
    opt.flags = flags;
    hipLaunchKernelGGL(notes_render_kernel, dim3((unsigned)(B * tiles)), dim3(kTile), 0, (hipStream_t)stream, onset, frames, pitch, detune,
                       level, count, offset, f0, cents, loudness, harmonicity, voiced, position, owner, (int)T, (int)N, (int)tiles,
                       groups > 1 ? 1 : 0, opt);
    return (int)hipGetLastError();
}
