// Notes (DESIGN.md sections 10f and 10g): the note events of a pitch track, and note events rendered back to frame-rate controls.
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
//   notes_expression_kernel  (section 10g) one thread per frame, the render's tiles, staging and search: each frame's distance from
//                          the centre of the note that owns it.
//   notes_render_kernel<true>  (section 10g) the render plus, on the on frames, the bend and the loudness of a source note read at
//                          the time map's position: at most two neighbouring source frames, by global loads.
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
constexpr double kMaxAmount = 16.0;             // expressive render: |bend_amount| and |dyn_amount| up to it

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

// the expressive render's source (section 10g): the records of the performance the curves were taken from, and the curves
struct ExprSource {
    const int *source, *onset, *frames, *count;
    const float *level;
    const int *bend;
    const float *loudness;
    int T, N, keep_attack, keep_release;
    double bend_amount, dyn_amount;
};

// the same inside the kernel: the curves' pointers, which wait in vector registers, keep their address space (global memory)
template <typename V>
using global_ptr = const V __attribute__((address_space(1))) *;

struct ExprCurves {
    global_ptr<int> source, onset, frames;
    global_ptr<float> level;
    global_ptr<int> bend;
    global_ptr<float> loudness;
    const int *count;
    int T, N, keep_attack, keep_release;
    double bend_amount, dyn_amount;
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

struct Staging {
    int onset[kStage], frames[kStage], pitch[kStage], detune[kStage];
    float level[kStage];
};

// What stage_records found for a tile of one row: the row's arrays in global memory, whether the tile's records are staged, and
// the record ranges.
struct Tile {
    const int *onset, *frames, *pitch, *detune;
    const float *level;                             // (NULL for a caller that reads no level)
    bool staged;
    int n, lo, first, last;                         // min(count, N); the staged range's start; i* + 1 of the tile's first and last frame
};

// The records a tile can touch.  Record i of the row, lo <= i < hi, is element i - lo of the staging arrays when the tile's records
// are staged (kStaged), else element i of the row's arrays in global memory.  Which of the two is a compile-time matter, so that
// a staged record is read through the LDS address space itself and never through a flat pointer that may be either: such a
// pointer's aperture is decided by the address register alone -- the instruction's offset field is ignored -- so wherever the
// compiler splits i - lo into a register part below the array's start and a constant (lo = max(first, 2) - 2 offers one), a flat
// load of the first staged array leaves the aperture and faults.
template <bool kStaged>
struct TileRecords {
    const Staging &s;
    const Tile &tile;

    __device__ __forceinline__ int onset_at(int i) const
    {
        if constexpr (kStaged) return s.onset[i - tile.lo]; else return tile.onset[i];
    }
    __device__ __forceinline__ int frames_at(int i) const
    {
        if constexpr (kStaged) return s.frames[i - tile.lo]; else return tile.frames[i];
    }
    __device__ __forceinline__ int pitch_at(int i) const
    {
        if constexpr (kStaged) return s.pitch[i - tile.lo]; else return tile.pitch[i];
    }
    __device__ __forceinline__ int detune_at(int i) const
    {
        if constexpr (kStaged) return s.detune[i - tile.lo]; else return tile.detune[i];
    }
    __device__ __forceinline__ float level_at(int i) const
    {
        if constexpr (kStaged) return s.level[i - tile.lo]; else return tile.level[i];
    }
    __device__ __forceinline__ long long onset_of(int i) const { return (long long)onset_at(i); }
    __device__ __forceinline__ long long frames_of(int i) const { return (long long)frames_at(i); }
    __device__ __forceinline__ bool valid(int i) const
    {
        const long long d = detune_at(i);
        const int p = pitch_at(i);
        return frames_of(i) >= 1 && p >= 0 && p <= 127 && d >= -kMaxDetune && d <= kMaxDetune;
    }
    // i* of frame t, -1: before every onset
    __device__ __forceinline__ int owner_of(int t) const
    {
        int from = tile.first, to = tile.last;
        while (from < to) {
            const int mid = from + ((to - from) >> 1);
            if (onset_at(mid) <= t) from = mid + 1; else to = mid;
        }
        return from - 1;
    }
};

// The notes the tile [t0, t_last] can touch: i* of its first frame up to i* of its last, one more below (the glide's note i - 1,
// and i* itself sits one below the count of onsets passed) and one above (L' reads the next onset).  They are staged in LDS when
// they fit, else read from global memory; `level_in` may be NULL for a caller that reads no level.  Ends with a barrier: every
// thread of the workgroup calls it.
__device__ __forceinline__ Tile stage_records(Staging &s, const int *onset_in, const int *frames_in, const int *pitch_in,
                                              const int *detune_in, const float *level_in, const int *count, long row, int N, int t0,
                                              int t_last)
{
    Tile r;
    const long rec0 = row * (long)N;
    int n = count[row];
    n = n < 0 ? 0 : (n > N ? N : n);
    r.onset = onset_in + rec0;
    r.frames = frames_in + rec0;
    r.pitch = pitch_in + rec0;
    r.detune = detune_in + rec0;
    r.level = level_in ? level_in + rec0 : nullptr;
    const int first = onsets_upto(r.onset, 0, 0, n, t0), last = onsets_upto(r.onset, 0, first, n, t_last);
    const int lo = first - 2 > 0 ? first - 2 : 0, hi = last + 1 < n ? last + 1 : n;
    r.staged = hi - lo <= kStage;
    if (r.staged) {
        for (int i = lo + threadIdx.x; i < hi; i += kTile) {
            s.onset[i - lo] = r.onset[i];
            s.frames[i - lo] = r.frames[i];
            s.pitch[i - lo] = r.pitch[i];
            s.detune[i - lo] = r.detune[i];
            if (level_in) s.level[i - lo] = r.level[i];
        }
    }
    __syncthreads();
    r.n = n;
    r.lo = lo;
    r.first = first;
    r.last = last;
    return r;
}

// a wave-uniform value kept in vector registers from here on
template <typename V>
__device__ __forceinline__ V in_vector_registers(V v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// Destination frame k of a note that sounds len frames -> the position (q, f) in its source note of Ls frames, f in 2^-16 frame:
// the first `keep_attack` and the last `keep_release` frames map one to one, the middle is stretched linearly between them.
// 0 <= k < len, Ls >= 1; every product stays below 2^48.
__device__ __forceinline__ void time_map(long long k, long long len, long long Ls, long long keep_attack, long long keep_release,
                                         long long &q, long long &f)
{
    long long a = keep_attack < Ls ? keep_attack : Ls;
    a = a < len ? a : len;
    long long r = keep_release < Ls - a ? keep_release : Ls - a;
    r = r < len - a ? r : len - a;
    f = 0;
    if (k < a) {
        q = k;
    } else if (k >= len - r) {
        q = Ls - (len - k);
    } else {
        const long long x = (k - a + 1) * (Ls - a - r + 1), D = len - a - r + 1;      // (D >= 2: a <= k < len - r)
        q = a - 1 + x / D;
        f = ((x % D) << 16) / D;
    }
    if (q < 0) {
        q = 0;
        f = 0;
    } else if (q >= Ls - 1) {
        q = Ls - 1;
        f = 0;
    }
}

template <bool kStaged>
__device__ __forceinline__ void expression_frame(const Staging &s, const Tile &tile, const float *__restrict__ cents,
                                                 const int *__restrict__ offset, int *__restrict__ bend_out, int *__restrict__ owner_out,
                                                 long row, int t, int T, int per_row)
{
    const TileRecords<kStaged> r{s, tile};
    const long at = row * (long)T + t;
    const int i = r.owner_of(t);
    long long bend = 0;
    int owner = -1;
    if (i >= 0 && r.valid(i) && (long long)t - r.onset_of(i) < r.frames_of(i)) {
        const float n = cents[at];
        if (fabsf(n) <= 4.0f) {                                                 // (a NaN fails the comparison)
            owner = i;
            bend = (long long)position(n) - 65536ll * clamp_offset(offset[per_row ? row : 0]) - r.pitch_at(i) * kSemitone -
                   r.detune_at(i);
            bend = bend < INT_MIN ? INT_MIN : (bend > INT_MAX ? INT_MAX : bend);        // (records that do not match the track)
        }
    }
    bend_out[at] = (int)bend;
    if (owner_out) owner_out[at] = owner;
}

__global__ void __launch_bounds__(kTile)
notes_expression_kernel(const float *__restrict__ cents, const int *__restrict__ onset_in, const int *__restrict__ frames_in,
                        const int *__restrict__ pitch_in, const int *__restrict__ detune_in, const int *__restrict__ count,
                        const int *__restrict__ offset, int *__restrict__ bend_out, int *__restrict__ owner_out, int T, int N, int tiles,
                        int per_row)
{
    __shared__ Staging s;
    const long row = blockIdx.x / tiles;
    const int t0 = (int)(blockIdx.x % tiles) * kTile;
    const int t = t0 + threadIdx.x;
    const int t_last = t0 + kTile - 1 < T - 1 ? t0 + kTile - 1 : T - 1;
    const Tile tile = stage_records(s, onset_in, frames_in, pitch_in, detune_in, nullptr, count, row, N, t0, t_last);
    if (t >= T) return;
    if (tile.staged)
        expression_frame<true>(s, tile, cents, offset, bend_out, owner_out, row, t, T, per_row);
    else
        expression_frame<false>(s, tile, cents, offset, bend_out, owner_out, row, t, T, per_row);
}

template <bool kExpr, bool kStaged>
__device__ __forceinline__ void render_frame(const Staging &s, const Tile &tile, const int *__restrict__ offset, float *__restrict__ f0_out,
                                             float *__restrict__ cents_out, float *__restrict__ loud_out, float *__restrict__ harm_out,
                                             uint8_t *__restrict__ voiced_out, long *__restrict__ position_out, int *__restrict__ owner_out,
                                             long row, int t, int T, int N, int per_row, const RenderOptions &opt, const ExprCurves &e)
{
    const TileRecords<kStaged> r{s, tile};
    const int n = tile.n;
    auto onset_of = [&](int i) { return r.onset_of(i); };
    auto frames_of = [&](int i) { return r.frames_of(i); };
    auto valid = [&](int i) { return r.valid(i); };

    const long long shift = opt.flags & DDSP_NOTES_CONCERT ? 0 : 65536ll * clamp_offset(offset[per_row ? row : 0]);
    auto centre = [&](int i) {                                                  // b_i of a valid note
        return r.pitch_at(i) * kSemitone + (opt.flags & DDSP_NOTES_KEEP_DETUNE ? r.detune_at(i) : 0) + shift + opt.transpose;
    };

    const int i = r.owner_of(t);                                                // i*, -1: before every onset
    long long p = kHold;
    double loudness = (double)opt.floor_level;
    int owner = -1;
    [[maybe_unused]] long long on_k = 0, on_len = 0;                            // k and L' of an on frame
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
            const float own = r.level_at(i);
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
            on_k = k;
            on_len = len;
        }
    }
    if constexpr (kExpr) {
        // The note's own curves, read from its source note j at the time map's position: at most two neighbouring source frames,
        // both inside the source note (f > 0 only with q < Ls - 1), which lies inside [0, Tsrc).
        int n_src = e.count[row];
        n_src = n_src < 0 ? 0 : (n_src > e.N ? e.N : n_src);
        long long j = -1;
        if (owner >= 0 && on_k < on_len) j = e.source ? (long long)e.source[row * (long)N + owner] : (long long)owner;
        if (j >= 0 && j < n_src) {                                              // (k < L' wherever the onsets are in order)
            const long src = row * (long)e.N + j;
            const long long Ls = e.frames[src], so = e.onset[src];
            if (Ls >= 1 && so >= 0 && so + Ls <= e.T) {
                long long q, f;
                time_map(on_k, on_len, Ls, e.keep_attack, e.keep_release, q, f);
                const long sat = row * (long)e.T + so + q;
                long long bend = e.bend[sat];
                if (f) bend += floor_div(((long long)e.bend[sat + 1] - bend) * f + 32768, 65536);
                p += llrint(e.bend_amount * (double)bend);
                const float sl = e.level[src];
                if (e.loudness && sl == sl && e.dyn_amount != 0.0) {
                    double l = (double)e.loudness[sat];
                    if (f) l += ((double)e.loudness[sat + 1] - l) * ((double)f / 65536.0);
                    loudness += e.dyn_amount * (l - (double)sl);
                }
            }
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

template <bool kExpr>
__global__ void __launch_bounds__(kTile)
notes_render_kernel(const int *__restrict__ onset_in, const int *__restrict__ frames_in, const int *__restrict__ pitch_in,
                    const int *__restrict__ detune_in, const float *__restrict__ level_in, const int *__restrict__ count,
                    const int *__restrict__ offset, float *__restrict__ f0_out, float *__restrict__ cents_out,
                    float *__restrict__ loud_out, float *__restrict__ harm_out, uint8_t *__restrict__ voiced_out,
                    long *__restrict__ position_out, int *__restrict__ owner_out, int T, int N, int tiles, int per_row, RenderOptions opt,
                    ExprSource ex)
{
    __shared__ Staging s;
    // (the source's pointers and amounts wait in vector registers: held as scalars beside the render's own arguments they leave
    // the 64-bit divisions too few scalar registers, and six are spilled)
    [[maybe_unused]] ExprCurves e = {};
    if constexpr (kExpr) {
        e.source = in_vector_registers((global_ptr<int>)(uintptr_t)ex.source);
        e.onset = in_vector_registers((global_ptr<int>)(uintptr_t)ex.onset);
        e.frames = in_vector_registers((global_ptr<int>)(uintptr_t)ex.frames);
        e.level = in_vector_registers((global_ptr<float>)(uintptr_t)ex.level);
        e.bend = in_vector_registers((global_ptr<int>)(uintptr_t)ex.bend);
        e.loudness = in_vector_registers((global_ptr<float>)(uintptr_t)ex.loudness);
        e.bend_amount = in_vector_registers(ex.bend_amount);
        e.dyn_amount = in_vector_registers(ex.dyn_amount);
        e.count = ex.count;
        e.T = ex.T;
        e.N = ex.N;
        e.keep_attack = ex.keep_attack;
        e.keep_release = ex.keep_release;
    }
    const long row = blockIdx.x / tiles;
    const int t0 = (int)(blockIdx.x % tiles) * kTile;
    const int t = t0 + threadIdx.x;
    const int t_last = t0 + kTile - 1 < T - 1 ? t0 + kTile - 1 : T - 1;
    const Tile tile = stage_records(s, onset_in, frames_in, pitch_in, detune_in, level_in, count, row, N, t0, t_last);
    if (t >= T) return;
    if (tile.staged)
        render_frame<kExpr, true>(s, tile, offset, f0_out, cents_out, loud_out, harm_out, voiced_out, position_out, owner_out, row, t, T, N,
                                  per_row, opt, e);
    else
        render_frame<kExpr, false>(s, tile, offset, f0_out, cents_out, loud_out, harm_out, voiced_out, position_out, owner_out, row, t, T, N,
                                   per_row, opt, e);
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

// What ddsp_notes_render and ddsp_notes_render_expr share: the checks in their fixed order (options, an empty batch, pointers,
// sizes) and the launch; `ex` is NULL for the plain render.
static int render_launch(const int *onset, const int *frames, const int *pitch, const int *detune, const float *level, const int *count,
                         const int *offset, float *f0, float *cents, float *loudness, float *harmonicity, uint8_t *voiced, long *position,
                         int *owner, long B, long T, long N, long groups, int flags, long transpose, long glide, long attack, long release,
                         long vibrato_delay, long vibrato_ramp, double vibrato_depth, double vibrato_omega, float floor_level,
                         float default_level, const ExprSource *ex, long Tsrc, long Nsrc, void *stream)
{
    auto steps = [](long x) { return x >= 0 && x < kMaxSteps; };
    if (B < 0 || T <= 0 || N < 0 || (flags & ~(DDSP_NOTES_KEEP_DETUNE | DDSP_NOTES_CONCERT)) || transpose < -kMaxTranspose ||
        transpose > kMaxTranspose || !steps(glide) || !steps(attack) || !steps(release) || !steps(vibrato_delay) || vibrato_ramp < 1 ||
        !steps(vibrato_ramp) || !(vibrato_depth >= 0.0 && vibrato_depth <= (double)kMaxTranspose) || !(fabs(vibrato_omega) <= 1e6) ||
        !(fabsf(floor_level) <= 3.0e38f) || !(fabsf(default_level) <= 3.0e38f))
        return DDSP_EINVAL;
    if (ex && (Tsrc <= 0 || Nsrc < 0 || !(fabs(ex->bend_amount) <= kMaxAmount) || !(fabs(ex->dyn_amount) <= kMaxAmount) ||
               !steps((long)ex->keep_attack) || !steps((long)ex->keep_release)))
        return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!count || !offset || !f0 || !cents || !loudness || !harmonicity || !voiced || (groups != 1 && groups != B) ||
        (N > 0 && (!onset || !frames || !pitch || !detune || !level)))
        return DDSP_EINVAL;
    if (ex && (!ex->count || !ex->bend || (Nsrc > 0 && (!ex->onset || !ex->frames || !ex->level)))) return DDSP_EINVAL;
    long total;
    if (T >= kMaxRowFrames || __builtin_mul_overflow(B, T, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    if (__builtin_mul_overflow(B, N, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    if (ex && (Tsrc >= kMaxRowFrames || __builtin_mul_overflow(B, Tsrc, &total) || total >= (1l << 31) ||
               __builtin_mul_overflow(B, Nsrc, &total) || total >= (1l << 31)))
        return DDSP_ERANGE;
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
    ExprSource src = {};
    if (ex) {
        src = *ex;
        src.T = (int)Tsrc;
        src.N = (int)Nsrc;
    }
    hipLaunchKernelGGL(ex ? notes_render_kernel<true> : notes_render_kernel<false>, dim3((unsigned)(B * tiles)), dim3(kTile), 0,
                       (hipStream_t)stream, onset, frames, pitch, detune, level, count, offset, f0, cents, loudness, harmonicity, voiced,
                       position, owner, (int)T, (int)N, (int)tiles, groups > 1 ? 1 : 0, opt, src);
    return (int)hipGetLastError();
}

extern "C" int ddsp_notes_render(const int *onset, const int *frames, const int *pitch, const int *detune, const float *level,
                                 const int *count, const int *offset, float *f0, float *cents, float *loudness, float *harmonicity,
                                 uint8_t *voiced, long *position, int *owner, long B, long T, long N, long groups, int flags,
                                 long transpose, long glide, long attack, long release, long vibrato_delay, long vibrato_ramp,
                                 double vibrato_depth, double vibrato_omega, float floor_level, float default_level, void *stream)
{
    return render_launch(onset, frames, pitch, detune, level, count, offset, f0, cents, loudness, harmonicity, voiced, position, owner, B, T,
                         N, groups, flags, transpose, glide, attack, release, vibrato_delay, vibrato_ramp, vibrato_depth, vibrato_omega,
                         floor_level, default_level, nullptr, 0, 0, stream);
}

extern "C" int ddsp_notes_render_expr(const int *onset, const int *frames, const int *pitch, const int *detune, const float *level,
                                      const int *count, const int *offset, float *f0, float *cents, float *loudness,
                                      float *harmonicity, uint8_t *voiced, long *position, int *owner, long B, long T, long N,
                                      long groups, int flags, long transpose, long glide, long attack, long release, long vibrato_delay,
                                      long vibrato_ramp, double vibrato_depth, double vibrato_omega, float floor_level,
                                      float default_level, const int *source, const int *src_onset, const int *src_frames,
                                      const float *src_level, const int *src_count, const int *bend, const float *src_loudness,
                                      long Tsrc, long Nsrc, double bend_amount, double dyn_amount, long keep_attack, long keep_release,
                                      void *stream)
{
    ExprSource ex = {};
    ex.source = source;
    ex.onset = src_onset;
    ex.frames = src_frames;
    ex.count = src_count;
    ex.level = src_level;
    ex.bend = bend;
    ex.loudness = src_loudness;
    ex.keep_attack = (int)(keep_attack < 0 ? -1 : (keep_attack < kMaxSteps ? keep_attack : kMaxSteps));      // (checked below)
    ex.keep_release = (int)(keep_release < 0 ? -1 : (keep_release < kMaxSteps ? keep_release : kMaxSteps));
    ex.bend_amount = bend_amount;
    ex.dyn_amount = dyn_amount;
    return render_launch(onset, frames, pitch, detune, level, count, offset, f0, cents, loudness, harmonicity, voiced, position, owner, B, T,
                         N, groups, flags, transpose, glide, attack, release, vibrato_delay, vibrato_ramp, vibrato_depth, vibrato_omega,
                         floor_level, default_level, &ex, Tsrc, Nsrc, stream);
}

extern "C" int ddsp_notes_expression(const float *cents, const int *onset, const int *frames, const int *pitch, const int *detune,
                                     const int *count, const int *offset, int *bend, int *owner, long B, long T, long N, long groups,
                                     void *stream)
{
    if (B < 0 || T <= 0 || N < 0) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!cents || !count || !offset || !bend || (groups != 1 && groups != B) || (N > 0 && (!onset || !frames || !pitch || !detune)))
        return DDSP_EINVAL;
    long total;
    if (T >= kMaxRowFrames || __builtin_mul_overflow(B, T, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    if (__builtin_mul_overflow(B, N, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    const long tiles = (T + kTile - 1) / kTile;                                 // B tiles <= B T < 2^31
    hipLaunchKernelGGL(notes_expression_kernel, dim3((unsigned)(B * tiles)), dim3(kTile), 0, (hipStream_t)stream, cents, onset, frames,
                       pitch, detune, count, offset, bend, owner, (int)T, (int)N, (int)tiles, groups > 1 ? 1 : 0);
    return (int)hipGetLastError();
}
