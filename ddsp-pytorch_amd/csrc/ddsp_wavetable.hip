// Wavetable synthesis: N learnable single-cycle tables of L points, one phase accumulator per batch row
// reading them at f0 with linear interpolation, mixed by the controller's per-frame weights.
//   wt_forward_kernel   one launch.  A workgroup of 1024 threads takes units (row, chunk of whole frames) from a capped grid.  It
//                       walks a chunk in iterations of whole frames, a thread per sample: the fp32 increment of every sample, an
//                       fp64 inclusive scan over the workgroup (the phase), then the N tables at the sample's entry.  A chunk that
//                       does not start the row first sums the increments in front of it.  LDS form: the [L + 1][N] image of the
//                       tables (ddsp_wavetable_plan.h) is staged once per workgroup; global form: the same walk reads W itself.
//   wt_backward_kernel  the same walk, two phases per iteration.  A: a thread per sample rebuilds its phase, adds its share of
//                       grad_W to the workgroup's private table (atomics, LDS or a slice of scratch) and leaves a record of what
//                       the frame sums need.  B: the threads regroup as (frame, four tables, part) and sum the records in a fixed
//                       order into the partial gradients of the frame and its two neighbours.
//   wt_finish_kernel    the second launch: per frame the three partials, the normalisation's backward and grad_a; per table entry
//                       the workgroups' private tables in workgroup order.
// Band-limited tables are the same three kernels with kBl set: W is then the mip levels M [Q + 1, N, L]
// (ddsp_wavetable_mip.hip builds them) and a sample reads two of them.  A unit keeps in LDS the levels its frames can reach when
// they fit: the forward their images to read, the backward their private gradient copies to scatter into (it reads the levels from
// memory); the backward's private table is [Q + 1, N, L] in scratch, to which what LDS collected is added.
// Every frame index is clamped into [0, T), every entry into [0, L), every level into [0, Q], every sample index is below T hop.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_osc_common.h"
#include "ddsp_wavetable_plan.h"

namespace {

using namespace ddsp_wavetable;
static_assert(kPlanERange == DDSP_ERANGE, "the planner's status is the entry points' return code");
static_assert(kHeadBytes >= sizeof(double) * (kThreads / 64) && kHeadBytes % 16 == 0, "one fp64 total per wavefront");

std::atomic<int> g_mode{0};     // ddsp_wavetable_set_form
std::atomic<int> g_grid{0};     // ddsp_wavetable_set_grid
std::atomic<long> g_mip_lds{0}; // ddsp_wavetable_set_mip_lds

struct WtParams {
    const float *f0, *c, *a, *W;
    float *y;
    double *phase_io;
    const float *grad_y;        // backward
    float *part_c, *part_a, *priv;
    float *grad_c, *grad_a, *grad_W;
    int B, T, N, L, hop;
    int P4, Q;                  // image pitch in 16-byte units; units that hold tables = ceil(N / 4)
    int iter_frames, chunk_frames, chunks, parts;
    int nlev, fit;              // band-limited: W is M [nlev, N, L] and a unit stages up to `fit` levels; otherwise 1 and 0
    unsigned *masks;            // band-limited backward: the levels each workgroup's private table holds anything in
    long units;
    int vec;                    // c rows can be read as float4
    float scale, sr;
};

struct Sample {
    int i0, i1;
    float w0, w1;
};

// F.interpolate(linear, align_corners=False) of output sample n: the bracketing frames and their weights
__device__ __forceinline__ Sample locate(const WtParams &p, int n)
{
    Sample s;
    const float src = fmaxf(__fmaf_rn(p.scale, (float)n + 0.5f, -0.5f), 0.0f);
    int i0 = (int)src;
    i0 = i0 < p.T - 1 ? i0 : p.T - 1;
    s.i0 = i0;
    s.i1 = i0 + 1 < p.T - 1 ? i0 + 1 : p.T - 1;
    ddsp_osc::upsample_weights(p.scale, n, (float)i0, s.w0, s.w1);
    return s;
}

// cycles per sample at sample n: up(fl32(f0 / sample_rate)) in fp32
__device__ __forceinline__ float increment(const WtParams &p, const float *f0row, const Sample &s)
{
    const float g0 = f0row[s.i0] / p.sr, g1 = f0row[s.i1] / p.sr;
    return __fmaf_rn(s.w0, g0, s.w1 * g1);
}

__device__ __forceinline__ double wave_sum64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// inclusive scan of v over the workgroup on top of `carry`; carry becomes the total.  Fixed order: the same bits every run.
__device__ __forceinline__ double block_scan(double v, double *head, double &carry)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    if (lane == 63) head[wave] = v;
    __syncthreads();
    double pre = carry, tot = carry;
    for (int w = 0; w < kThreads / 64; ++w) {
        const double h = head[w];
        if (w < wave) pre += h;
        tot += h;
    }
    __syncthreads();
    carry = tot;
    return pre + v;
}

// the increments of the row's samples [0, n_end), summed over the workgroup
__device__ __forceinline__ double row_prefix(const WtParams &p, const float *f0row, int n_end, double *head)
{
    double part = 0.0;
    for (int n = threadIdx.x; n < n_end; n += kThreads) part += (double)increment(p, f0row, locate(p, n));
    part = wave_sum64(part);
    if ((threadIdx.x & 63) == 0) head[threadIdx.x >> 6] = part;
    __syncthreads();
    double tot = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) tot += head[w];
    __syncthreads();
    return tot;
}

// entry j in [0, L) and the fraction towards j + 1 of the phase P (cycles)
__device__ __forceinline__ void table_position(double P, int L, int &j, float &fr)
{
    const double pos = (P - floor(P)) * (double)L;
    int e = (int)pos;
    e = e < L - 1 ? e : L - 1;      // (also p L rounded up to L, an infinite or NaN phase)
    e = e > 0 ? e : 0;
    j = e;
    fr = (float)(pos - (double)e);
}

// tables 4 q .. 4 q + 3 at entries j and j + 1 (wrapped); tables past N read as 0
template <bool kLds>
__device__ __forceinline__ void fetch4(const WtParams &p, const float *W, const float4 *img, int q, int j, float4 &lo, float4 &hi)
{
    if constexpr (kLds) {
        lo = img[image_unit(j, p.P4) + q];
        hi = img[image_unit(j + 1, p.P4) + q];
    } else {
        const int j1 = j + 1 == p.L ? 0 : j + 1;
        float l[4], h[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int k = 4 * q + x;
            const bool ok = k < p.N;
            const float *row = W + (long)(ok ? k : 0) * p.L;
            l[x] = ok ? row[j] : 0.0f;
            h[x] = ok ? row[j1] : 0.0f;
        }
        lo = make_float4(l[0], l[1], l[2], l[3]);
        hi = make_float4(h[0], h[1], h[2], h[3]);
    }
}

__device__ __forceinline__ float4 load4(const float *row, int q, int N, int vec)
{
    if (vec) return reinterpret_cast<const float4 *>(row)[q];
    const int k = 4 * q;
    return make_float4(row[k], k + 1 < N ? row[k + 1] : 0.0f, k + 2 < N ? row[k + 2] : 0.0f, k + 3 < N ? row[k + 3] : 0.0f);
}

__device__ __forceinline__ float4 lerp4(float fr, const float4 &lo, const float4 &hi)
{
    return make_float4(__fmaf_rn(fr, hi.x - lo.x, lo.x), __fmaf_rn(fr, hi.y - lo.y, lo.y), __fmaf_rn(fr, hi.z - lo.z, lo.z),
                       __fmaf_rn(fr, hi.w - lo.w, lo.w));
}

// the [L + 1][N] image: coalesced reads of W, row L repeats row 0, the pad tables are 0
__device__ __forceinline__ void stage_image(const WtParams &p, const float *W, float *img)
{
    const int rows = p.L + 1, NP = 4 * p.P4;
    for (long i = threadIdx.x; i < (long)NP * rows; i += kThreads) {
        const int k = (int)(i / rows), row = (int)(i % rows);
        img[4 * image_unit(row, p.P4) + k] = k < p.N ? W[(long)k * p.L + (row == p.L ? 0 : row)] : 0.0f;
    }
}

// ---- band-limited tables -------------------------------------------------------------------------------
// The two levels a sample hears and the weight of the upper one, from its increment u: r = L u = m 2^e with m in [0.5, 1) gives
// level e and t = 2 m - 1, all exact in fp32.  not (r > 0.5) -- u <= 0 and NaN too -- is level 0 alone; r >= L / 2 is the top alone.
struct Level {
    int q, q1;
    float t;
};

__device__ __forceinline__ Level mip_level(float u, int L, int top)
{
    Level lv = {0, 1, 0.0f};
    const float r = (float)L * u;
    if (!(r > 0.5f)) return lv;
    if (!(r < 0.5f * (float)L)) {
        lv.q = lv.q1 = top;
        return lv;
    }
    const int bits = __float_as_int(r);                                         // (0.5 < r < L / 2: a normal number)
    lv.q = ((bits >> 23) & 0xff) - 126;
    lv.q1 = lv.q + 1;
    lv.t = __fmaf_rn(2.0f, __int_as_float((bits & 0x007fffff) | 0x3f000000), -1.0f);
    return lv;
}

// What a unit stages, the same in every thread: the images of the levels [lo, hi] sit in LDS, level lo first.
struct Staged {
    int lo, hi;         // lo > hi: nothing staged
    bool use;           // this unit reads them (its own levels fit); otherwise it reads M from memory
};

// The levels the frames [t_begin - 1, t_end] can make a sample of the chunk hear: every increment is an interpolation of two of
// their g = f0 / sample_rate, so it lies between the smallest and the largest g, widened by 2^-20 for the interpolation's roundings.
// (A lane whose level falls outside what is staged reads memory: the range decides speed, never what is read.)
__device__ __forceinline__ void unit_levels(const WtParams &p, const float *f0row, int t_begin, int t_end, int *slots, int &lo, int &hi)
{
    const int fa = t_begin > 0 ? t_begin - 1 : 0, fb = t_end < p.T - 1 ? t_end : p.T - 1;
    const int top = p.nlev - 1;
    int l = top, h = 0;
    for (int f = fa + (int)threadIdx.x; f <= fb; f += kThreads) {
        const float g = f0row[f] / p.sr;
        const Level a = mip_level(g * (1.0f - 0x1p-20f), p.L, top), b = mip_level(g * (1.0f + 0x1p-20f), p.L, top);
        const int x = a.q < b.q ? a.q : b.q, y = a.q1 > b.q1 ? a.q1 : b.q1;
        l = x < l ? x : l;
        h = y > h ? y : h;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int l2 = __shfl_xor(l, o), h2 = __shfl_xor(h, o);
        l = l2 < l ? l2 : l;
        h = h2 > h ? h2 : h;
    }
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = l | (h << 8);
    __syncthreads();
    l = top;
    h = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        const int v = slots[w], x = v & 0xff, y = v >> 8;
        l = x < l ? x : l;
        h = y > h ? y : h;
    }
    __syncthreads();
    lo = l < h ? l : h;
    hi = h < top ? h : top;
}

// decide the unit's path and stage what it needs; every thread calls it with the same arguments (barriers inside)
__device__ __forceinline__ void stage_levels(const WtParams &p, float4 *img, long img_units, int lo, int hi, Staged &st)
{
    st.use = hi - lo + 1 <= p.fit;
    if (!st.use || (lo >= st.lo && hi <= st.hi)) return;
    st.lo = lo;
    st.hi = hi;
    for (int q = lo; q <= hi; ++q)
        stage_image(p, p.W + (long)q * p.N * p.L, reinterpret_cast<float *>(img + (long)(q - lo) * img_units));
    __syncthreads();
}

// The backward keeps in LDS not the levels it reads (those come from memory) but the private grad_M of the levels it scatters to:
// the same window [lo, hi], the same image layout.  What a window holds goes to the workgroup's slice in memory when the window
// moves and at the end -- with atomics, like every other addition to the slice, so that all of them meet in L2.
__device__ __forceinline__ void flush_private(const WtParams &p, const float *win, long img_units, const Staged &st, float *slice)
{
    const long NL = (long)p.N * p.L;
    for (int q = st.lo; q <= st.hi; ++q) {
        const float *im = win + 4 * (long)(q - st.lo) * img_units;
        for (long i = threadIdx.x; i < NL; i += kThreads) {
            const int k = (int)(i / p.L), row = (int)(i % p.L);
            float v = im[4 * image_unit(row, p.P4) + k];
            if (row == 0) v += im[4 * image_unit(p.L, p.P4) + k];               // row L belongs to entry 0
            if (v != 0.0f) unsafeAtomicAdd(slice + q * NL + i, v);
        }
    }
}

// the backward's stage_levels: every thread calls it with the same arguments, after a barrier behind the last scatter
__device__ __forceinline__ void open_private(const WtParams &p, float *win, long img_units, int lo, int hi, Staged &st, float *slice)
{
    st.use = hi - lo + 1 <= p.fit;
    if (!st.use || (lo >= st.lo && hi <= st.hi)) return;
    flush_private(p, win, img_units, st, slice);
    __syncthreads();
    st.lo = lo;
    st.hi = hi;
    for (long i = threadIdx.x; i < 4 * img_units * (hi - lo + 1); i += kThreads) win[i] = 0.0f;
    __syncthreads();
}

// tables 4 g .. 4 g + 3 read at (j, fr): the unlimited table, or the blend of the sample's two levels
template <bool kLds, bool kBl>
__device__ __forceinline__ float4 entry4(const WtParams &p, const float4 *img, long img_units, const Staged &st, bool staged, int g,
                                         int j, float fr, const Level &lv)
{
    float4 lo, hi;
    if constexpr (!kBl) {
        fetch4<kLds>(p, p.W, img, g, j, lo, hi);
        return lerp4(fr, lo, hi);
    } else {
        // t == 0 -- level 0 alone, the top level alone, an exact octave -- reads one level and returns it as it is: the unlimited
        // kernel's bits where that level is the table, whatever level q + 1 holds
        const long NL = (long)p.N * p.L;
        float4 v0, v1;
        if (kLds && staged) {
            fetch4<true>(p, p.W, img + (long)(lv.q - st.lo) * img_units, g, j, lo, hi);
            v0 = lerp4(fr, lo, hi);
            if (lv.t == 0.0f) return v0;
            fetch4<true>(p, p.W, img + (long)(lv.q1 - st.lo) * img_units, g, j, lo, hi);
            v1 = lerp4(fr, lo, hi);
        } else {
            fetch4<false>(p, p.W + lv.q * NL, img, g, j, lo, hi);
            v0 = lerp4(fr, lo, hi);
            if (lv.t == 0.0f) return v0;
            fetch4<false>(p, p.W + lv.q1 * NL, img, g, j, lo, hi);
            v1 = lerp4(fr, lo, hi);
        }
        const float t = lv.t, omt = 1.0f - lv.t;                                // (exact)
        return make_float4(__fmaf_rn(t, v1.x, omt * v0.x), __fmaf_rn(t, v1.y, omt * v0.y), __fmaf_rn(t, v1.z, omt * v0.z),
                           __fmaf_rn(t, v1.w, omt * v0.w));
    }
}

__device__ __forceinline__ bool is_staged(const Staged &st, const Level &lv) { return st.use && lv.q >= st.lo && lv.q1 <= st.hi; }

template <bool kLds, bool kBl>
__global__ void __launch_bounds__(kThreads) wt_forward_kernel(const WtParams p)
{
    extern __shared__ float4 smem[];
    double *head = reinterpret_cast<double *>(smem);
    int *slots = reinterpret_cast<int *>(smem) + 32;                            // (behind the wavefronts' totals)
    const float4 *img = smem + kHeadBytes / 16;
    const long img_units = image_unit(p.L, p.P4) + p.P4;
    Staged st = {1, 0, false};
    if constexpr (kLds && !kBl) {
        stage_image(p, p.W, reinterpret_cast<float *>(smem + kHeadBytes / 16));
        __syncthreads();
    }
    const int tid = threadIdx.x;
    const long Ns = (long)p.T * p.hop;
    for (long unit = blockIdx.x; unit < p.units; unit += gridDim.x) {
        const int b = (int)(unit / p.chunks), ch = (int)(unit % p.chunks);
        const int t_begin = ch * p.chunk_frames;
        const int t_end = t_begin + p.chunk_frames < p.T ? t_begin + p.chunk_frames : p.T;
        const float *f0row = p.f0 + (long)b * p.T;
        const float *arow = p.a + (long)b * p.T;
        const float *crow = p.c + (long)b * p.T * p.N;
        if constexpr (kLds && kBl) {
            int lo, hi;
            unit_levels(p, f0row, t_begin, t_end, slots, lo, hi);
            stage_levels(p, smem + kHeadBytes / 16, img_units, lo, hi, st);
        }
        double carry = p.phase_io ? p.phase_io[b] : 0.0;
        if (t_begin > 0) carry += row_prefix(p, f0row, t_begin * p.hop, head);
        for (int t0 = t_begin; t0 < t_end; t0 += p.iter_frames) {
            const int t1 = t0 + p.iter_frames < t_end ? t0 + p.iter_frames : t_end;
            const int cnt = (t1 - t0) * p.hop;                                  // <= kThreads
            const int n = t0 * p.hop + tid;
            const bool active = tid < cnt;
            Sample s = {0, 0, 0.0f, 0.0f};
            float u = 0.0f;
            if (active) {
                s = locate(p, n);
                u = increment(p, f0row, s);
            }
            const double P = block_scan((double)u, head, carry);
            if (!active) continue;
            int j;
            float fr;
            table_position(P, p.L, j, fr);
            Level lv = {0, 0, 0.0f};
            bool staged = false;
            if constexpr (kBl) {
                lv = mip_level(u, p.L, p.nlev - 1);
                staged = is_staged(st, lv);
            }
            const float *c0 = crow + (long)s.i0 * p.N, *c1 = crow + (long)s.i1 * p.N;
            float A0 = 0.0f, A1 = 0.0f;
            double S0 = 0.0, S1 = 0.0;
            for (int q = 0; q < p.Q; ++q) {
                const float4 v = entry4<kLds, kBl>(p, img, img_units, st, staged, q, j, fr, lv);
                const float4 x0 = load4(c0, q, p.N, p.vec), x1 = load4(c1, q, p.N, p.vec);
                A0 = __fmaf_rn(x0.x, v.x, A0); A0 = __fmaf_rn(x0.y, v.y, A0); A0 = __fmaf_rn(x0.z, v.z, A0); A0 = __fmaf_rn(x0.w, v.w, A0);
                A1 = __fmaf_rn(x1.x, v.x, A1); A1 = __fmaf_rn(x1.y, v.y, A1); A1 = __fmaf_rn(x1.z, v.z, A1); A1 = __fmaf_rn(x1.w, v.w, A1);
                S0 += (double)x0.x; S0 += (double)x0.y; S0 += (double)x0.z; S0 += (double)x0.w;
                S1 += (double)x1.x; S1 += (double)x1.y; S1 += (double)x1.z; S1 += (double)x1.w;
            }
            const float au = __fmaf_rn(s.w0, arow[s.i0], s.w1 * arow[s.i1]);
            const float M = __fmaf_rn(s.w0, A0 / (float)S0, s.w1 * (A1 / (float)S1));
            p.y[(long)b * Ns + n] = au * M;
        }
        // the carried phase: chunks == 1 with a phase_io (the planner), so no other workgroup reads this row's word
        if (p.phase_io && ch == p.chunks - 1 && tid == 0) p.phase_io[b] = carry - floor(carry);
    }
}

// Band-limited (kBl): the levels are read from memory, the private table is [nlev, N, L] in scratch, and kLds says that a unit keeps
// the private copies of the levels it scatters to in LDS when they fit (open_private).  A level of the slice is zeroed when the
// workgroup first adds to it, and a word per workgroup tells the finish which levels those are: the rest is never written or read.
template <bool kLds, bool kBl>
__global__ void __launch_bounds__(kThreads) wt_backward_kernel(const WtParams p)
{
    extern __shared__ float4 smem[];
    double *head = reinterpret_cast<double *>(smem);
    int *slots = reinterpret_cast<int *>(smem) + 32;
    const long img_units = image_unit(p.L, p.P4) + p.P4;
    const float4 *img = smem + kHeadBytes / 16;
    float *priv_lds = reinterpret_cast<float *>(smem + kHeadBytes / 16 + img_units);
    float *win = reinterpret_cast<float *>(smem + kHeadBytes / 16);            // band-limited: the private window, p.fit images
    float4 *rec = smem + kHeadBytes / 16 + (kBl ? p.fit * img_units : (kLds ? 2 * img_units : 0));
    const int tid = threadIdx.x;
    const long NL = (long)p.N * p.L;
    float *slice = p.priv + (long)blockIdx.x * NL * p.nlev;
    Staged st = {1, 0, false};
    unsigned zeroed = 0;        // band-limited: the levels of the slice this workgroup has zeroed, which are those it adds to
    if constexpr (kLds && !kBl) {
        stage_image(p, p.W, reinterpret_cast<float *>(smem + kHeadBytes / 16));
        for (long i = tid; i < 4 * img_units; i += kThreads) priv_lds[i] = 0.0f;
    } else if constexpr (!kBl) {
        for (long i = tid; i < NL; i += kThreads) slice[i] = 0.0f;
        __threadfence_block();
    }
    __syncthreads();
    const long Ns = (long)p.T * p.hop;
    const int kinds = p.Q + 1;                                                  // units of four tables, then the loudness
    for (long unit = blockIdx.x; unit < p.units; unit += gridDim.x) {
        const int b = (int)(unit / p.chunks), ch = (int)(unit % p.chunks);
        const int t_begin = ch * p.chunk_frames;
        const int t_end = t_begin + p.chunk_frames < p.T ? t_begin + p.chunk_frames : p.T;
        const float *f0row = p.f0 + (long)b * p.T;
        const float *arow = p.a + (long)b * p.T;
        const float *crow = p.c + (long)b * p.T * p.N;
        if constexpr (kLds && kBl) {
            int lo, hi;
            unit_levels(p, f0row, t_begin, t_end, slots, lo, hi);
            open_private(p, win, img_units, lo, hi, st, slice);
        }
        double carry = p.phase_io ? p.phase_io[b] : 0.0;
        if (t_begin > 0) carry += row_prefix(p, f0row, t_begin * p.hop, head);
        for (int t0 = t_begin; t0 < t_end; t0 += p.iter_frames) {
            const int t1 = t0 + p.iter_frames < t_end ? t0 + p.iter_frames : t_end;
            const int nf = t1 - t0;
            const int cnt = nf * p.hop;
            const int n = t0 * p.hop + tid;
            const bool active = tid < cnt;
            Sample s = {0, 0, 0.0f, 0.0f};
            float u = 0.0f;
            if (active) {
                s = locate(p, n);
                u = increment(p, f0row, s);
            }
            Level lv = {0, 0, 0.0f};
            if constexpr (kBl) {    // the levels this iteration adds to, over the workgroup (read behind the scan's barriers)
                unsigned bits = 0;
                if (active) {
                    lv = mip_level(u, p.L, p.nlev - 1);
                    bits = 1u << lv.q;
                    if (lv.t != 0.0f) bits |= 1u << lv.q1;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) bits |= __shfl_xor(bits, o);
                if ((tid & 63) == 0) slots[tid >> 6] = (int)bits;
            }
            const double P = block_scan((double)u, head, carry);
            if constexpr (kBl) {    // a level is zeroed when the workgroup first adds to it: most levels never are
                unsigned need = 0;
                for (int w = 0; w < kThreads / 64; ++w) need |= (unsigned)slots[w];
                const unsigned fresh = need & ~zeroed;                          // (the same in every thread)
                if (fresh) {
                    for (int q = 0; q < p.nlev; ++q)
                        if (fresh >> q & 1)
                            for (long i = tid; i < NL; i += kThreads) slice[q * NL + i] = 0.0f;
                    __threadfence_block();
                    __syncthreads();
                    zeroed |= fresh;
                }
            }
            // ---- A: a thread per sample ----
            if (active) {
                int j;
                float fr;
                table_position(P, p.L, j, fr);
                const float *c0 = crow + (long)s.i0 * p.N, *c1 = crow + (long)s.i1 * p.N;
                double S0 = 0.0, S1 = 0.0;
                for (int q = 0; q < p.Q; ++q) {
                    const float4 x0 = load4(c0, q, p.N, p.vec), x1 = load4(c1, q, p.N, p.vec);
                    S0 += (double)x0.x; S0 += (double)x0.y; S0 += (double)x0.z; S0 += (double)x0.w;
                    S1 += (double)x1.x; S1 += (double)x1.y; S1 += (double)x1.z; S1 += (double)x1.w;
                }
                const float Sf0 = (float)S0, Sf1 = (float)S1;
                const float r0 = s.w0 / Sf0, r1 = s.w1 / Sf1;
                const float au = __fmaf_rn(s.w0, arow[s.i0], s.w1 * arow[s.i1]);
                const float gy = p.grad_y[(long)b * Ns + n];
                const float qv = gy * au;
                const float glo = qv * (1.0f - fr), ghi = qv * fr;
                const int j1 = j + 1 == p.L ? 0 : j + 1;
                bool staged = false;
                float w[4] = {glo, ghi, 0.0f, 0.0f};                            // level q at j and j + 1, level q + 1 at j and j + 1
                if constexpr (kBl) {
                    staged = is_staged(st, lv);
                    const float omt = 1.0f - lv.t;
                    w[0] = glo * omt; w[1] = ghi * omt; w[2] = glo * lv.t; w[3] = ghi * lv.t;
                }
                float *const s0p = slice + lv.q * NL, *const s1p = slice + lv.q1 * NL;
                float A0 = 0.0f, A1 = 0.0f;
                for (int q = 0; q < p.Q; ++q) {
                    const float4 v = entry4<kLds && !kBl, kBl>(p, img, img_units, st, false, q, j, fr, lv);
                    const float4 x0 = load4(c0, q, p.N, p.vec), x1 = load4(c1, q, p.N, p.vec);
                    A0 = __fmaf_rn(x0.x, v.x, A0); A0 = __fmaf_rn(x0.y, v.y, A0); A0 = __fmaf_rn(x0.z, v.z, A0); A0 = __fmaf_rn(x0.w, v.w, A0);
                    A1 = __fmaf_rn(x1.x, v.x, A1); A1 = __fmaf_rn(x1.y, v.y, A1); A1 = __fmaf_rn(x1.z, v.z, A1); A1 = __fmaf_rn(x1.w, v.w, A1);
                    const float m[4] = {__fmaf_rn(r0, x0.x, r1 * x1.x), __fmaf_rn(r0, x0.y, r1 * x1.y), __fmaf_rn(r0, x0.z, r1 * x1.z),
                                        __fmaf_rn(r0, x0.w, r1 * x1.w)};
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const int k = 4 * q + x;
                        if (k >= p.N) break;
                        if (kBl && kLds && staged) {
                            float *const w0p = win + 4 * (long)(lv.q - st.lo) * img_units, *const w1p = win + 4 * (long)(lv.q1 - st.lo) * img_units;
                            atomicAdd(w0p + 4 * image_unit(j, p.P4) + k, w[0] * m[x]);
                            atomicAdd(w0p + 4 * image_unit(j + 1, p.P4) + k, w[1] * m[x]);
                            if (lv.t != 0.0f) {
                                atomicAdd(w1p + 4 * image_unit(j, p.P4) + k, w[2] * m[x]);
                                atomicAdd(w1p + 4 * image_unit(j + 1, p.P4) + k, w[3] * m[x]);
                            }
                        } else if constexpr (kBl) {
                            unsafeAtomicAdd(s0p + (long)k * p.L + j, w[0] * m[x]);
                            unsafeAtomicAdd(s0p + (long)k * p.L + j1, w[1] * m[x]);
                            if (lv.t != 0.0f) {
                                unsafeAtomicAdd(s1p + (long)k * p.L + j, w[2] * m[x]);
                                unsafeAtomicAdd(s1p + (long)k * p.L + j1, w[3] * m[x]);
                            }
                        } else if constexpr (kLds) {
                            atomicAdd(priv_lds + 4 * image_unit(j, p.P4) + k, glo * m[x]);
                            atomicAdd(priv_lds + 4 * image_unit(j + 1, p.P4) + k, ghi * m[x]);
                        } else {
                            unsafeAtomicAdd(slice + (long)k * p.L + j, glo * m[x]);
                            unsafeAtomicAdd(slice + (long)k * p.L + j1, ghi * m[x]);
                        }
                    }
                }
                const float M = __fmaf_rn(s.w0, A0 / Sf0, s.w1 * (A1 / Sf1));
                const float ga = gy * M;
                // the frame's three targets: slot 0 is frame t - 1, 1 is t, 2 is t + 1
                const int t = n / p.hop;
                int s0 = s.i0 - t + 1, s1 = s.i1 - t + 1;
                s0 = s0 < 0 ? 0 : (s0 > 2 ? 2 : s0);
                s1 = s1 < 0 ? 0 : (s1 > 2 ? 2 : s1);
                float e[3], g[3];
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    e[x] = (s0 == x ? qv * s.w0 : 0.0f) + (s1 == x ? qv * s.w1 : 0.0f);
                    g[x] = (s0 == x ? ga * s.w0 : 0.0f) + (s1 == x ? ga * s.w1 : 0.0f);
                }
                rec[2 * tid] = make_float4(__int_as_float(j), fr, e[0], e[1]);
                rec[2 * tid + 1] = make_float4(e[2], g[0], g[1], g[2]);
            }
            __syncthreads();
            // ---- B: (frame, kind, part); the parts of one sum sit in neighbouring lanes ----
            const int items = nf * kinds * p.parts;
            for (int base = 0; base < items; base += kThreads) {
                const int it = base + tid;
                const bool valid = it < items;
                const int part = it % p.parts, grp = it / p.parts;
                const int kind = grp % kinds, f = grp / kinds;
                float acc[3][4] = {};
                if (valid) {
                    for (int r = part; r < p.hop; r += p.parts) {
                        const float4 ra = rec[2 * (f * p.hop + r)], rb = rec[2 * (f * p.hop + r) + 1];
                        if (kind < p.Q) {
                            Level lv = {0, 0, 0.0f};
                            if constexpr (kBl)                                  // (the record has no room: the sample's increment again)
                                lv = mip_level(increment(p, f0row, locate(p, (t0 + f) * p.hop + r)), p.L, p.nlev - 1);
                            const float4 v = entry4<kLds && !kBl, kBl>(p, img, img_units, st, false, kind, __float_as_int(ra.x), ra.y, lv);
                            const float e[3] = {ra.z, ra.w, rb.x};
#pragma unroll
                            for (int x = 0; x < 3; ++x) {
                                acc[x][0] = __fmaf_rn(e[x], v.x, acc[x][0]);
                                acc[x][1] = __fmaf_rn(e[x], v.y, acc[x][1]);
                                acc[x][2] = __fmaf_rn(e[x], v.z, acc[x][2]);
                                acc[x][3] = __fmaf_rn(e[x], v.w, acc[x][3]);
                            }
                        } else {
                            acc[0][0] += rb.y;
                            acc[1][0] += rb.z;
                            acc[2][0] += rb.w;
                        }
                    }
                }
                for (int o = p.parts >> 1; o > 0; o >>= 1) {
#pragma unroll
                    for (int x = 0; x < 3; ++x)
#pragma unroll
                        for (int z = 0; z < 4; ++z) acc[x][z] += __shfl_xor(acc[x][z], o);
                }
                if (valid && part == 0) {
                    const long frame = (long)b * p.T + t0 + f;
                    if (kind < p.Q) {
#pragma unroll
                        for (int x = 0; x < 3; ++x)
#pragma unroll
                            for (int z = 0; z < 4; ++z)
                                if (4 * kind + z < p.N) p.part_c[(frame * 3 + x) * p.N + 4 * kind + z] = acc[x][z];
                    } else {
#pragma unroll
                        for (int x = 0; x < 3; ++x) p.part_a[frame * 3 + x] = acc[x][0];
                    }
                }
            }
            __syncthreads();
        }
    }
    if constexpr (kBl) {
        if constexpr (kLds) {
            __syncthreads();
            flush_private(p, win, img_units, st, slice);
        }
        if (tid == 0) p.masks[blockIdx.x] = zeroed;                             // the finish reads no other level of this slice
    } else if constexpr (kLds) {   // the private image -> this workgroup's [N, L] slice; row L belongs to entry 0
        __syncthreads();
        for (long i = tid; i < NL; i += kThreads) {
            const int k = (int)(i / p.L), row = (int)(i % p.L);
            float v = priv_lds[4 * image_unit(row, p.P4) + k];
            if (row == 0) v += priv_lds[4 * image_unit(p.L, p.P4) + k];
            slice[i] = v;
        }
    }
}

constexpr int kFinishThreads = 256;

// blocks [0, frame_blocks): a wavefront per frame; the rest: a thread per table entry
__global__ void __launch_bounds__(kFinishThreads) wt_finish_kernel(const WtParams p, long frame_blocks, int nwg)
{
    const int lane = threadIdx.x & 63;
    if ((long)blockIdx.x < frame_blocks) {
        const long frame = (long)blockIdx.x * (kFinishThreads / 64) + (threadIdx.x >> 6);
        if (frame >= (long)p.B * p.T) return;
        const int t = (int)(frame % p.T);
        const float *c = p.c + frame * p.N;
        // G[k]: the partials aimed at this frame, from frame t - 1, t and t + 1 in that order
        auto gathered = [&](int k) {
            float g = p.part_c[(frame * 3 + 1) * p.N + k];
            if (t > 0) g = p.part_c[((frame - 1) * 3 + 2) * p.N + k] + g;
            if (t + 1 < p.T) g += p.part_c[((frame + 1) * 3 + 0) * p.N + k];
            return g;
        };
        double S = 0.0;
        float D = 0.0f;
        for (int k = lane; k < p.N; k += 64) {
            S += (double)c[k];
            D = __fmaf_rn(gathered(k), c[k], D);
        }
        const float Sf = (float)wave_sum64(S);
        D = wave_sum(D) / Sf;
        for (int k = lane; k < p.N; k += 64) p.grad_c[frame * p.N + k] = (gathered(k) - D) / Sf;
        if (lane == 0) {
            float g = p.part_a[frame * 3 + 1];
            if (t > 0) g = p.part_a[(frame - 1) * 3 + 2] + g;
            if (t + 1 < p.T) g += p.part_a[(frame + 1) * 3 + 0];
            p.grad_a[frame] = g;
        }
        return;
    }
    const long NL = (long)p.N * p.L * p.nlev;                                   // (band-limited: grad_W is grad_M [nlev, N, L])
    const long i = ((long)blockIdx.x - frame_blocks) * kFinishThreads + threadIdx.x;
    if (i >= NL) return;
    float v = 0.0f;
    if (p.masks) {      // a workgroup that added nothing to the level holds zeros there: skipped, the order of the rest kept
        const unsigned bit = 1u << (int)(i / ((long)p.N * p.L));
        for (int w = 0; w < nwg; ++w)
            if (p.masks[w] & bit) v += p.priv[(long)w * NL + i];
    } else {
        for (int w = 0; w < nwg; ++w) v += p.priv[(long)w * NL + i];
    }
    p.grad_W[i] = v;
}

// shape checks shared by the entry points: DDSP_EINVAL, then (the caller: empty batch, pointers), then DDSP_ERANGE
int bad_shape(long B, long T, long N, long L, long hop, long sample_rate)
{
    return (B < 0 || T < 1 || N < 1 || L < 2 || hop < 1 || sample_rate < 1) ? DDSP_EINVAL : 0;
}
int out_of_range(long B, long T, long N, long L, long hop)
{
    if (!supported(N, L) || hop > kMaxHop || T > kMaxSamples / hop || B > (1l << 24)) return DDSP_ERANGE;
    if (B * T > (1l << 31) / (3 * N)) return DDSP_ERANGE;                       // part_c indices
    return 0;
}

void fill_params(WtParams &p, const Plan &pl, int B, int T, int N, int L, int hop, int sample_rate)
{
    p.B = B; p.T = T; p.N = N; p.L = L; p.hop = hop;
    p.P4 = pitch4(N);
    p.Q = (N + 3) / 4;
    p.nlev = 1;
    p.fit = 0;
    p.iter_frames = pl.iter_frames;
    p.chunk_frames = pl.chunk_frames;
    p.chunks = pl.chunks;
    p.parts = pl.parts;
    p.units = pl.units;
    p.vec = N % 4 == 0 && (uintptr_t)p.c % 16 == 0;
    p.scale = 1.0f / (float)hop;
    p.sr = (float)sample_rate;
}

template <typename K>
hipError_t launch(K kernel, bool (&done)[64], const Plan &pl, const WtParams &p, hipStream_t s)
{
    if (pl.lds_bytes > 64 * 1024) {
        const hipError_t e = ddsp_allow_big_lds(reinterpret_cast<const void *>(kernel), done);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid), dim3(kThreads), pl.lds_bytes, s, p);
    return hipGetLastError();
}

}  // namespace

extern "C" int ddsp_wavetable_supported(int N, int L) { return supported(N, L) ? 1 : 0; }

extern "C" int ddsp_wavetable_form(int B, int T, int N, int L, int hop)
{
    if (bad_shape(B, T, N, L, hop, 1) || B == 0) return DDSP_EINVAL;
    if (out_of_range(B, T, N, L, hop)) return DDSP_ERANGE;
    const int mode = g_mode.load(), cap = g_grid.load();
    const Plan f = plan(B, T, N, L, hop, false, false, mode, cap), b = plan(B, T, N, L, hop, true, false, mode, cap);
    if (f.status) return f.status;
    if (b.status) return b.status;
    return f.form | (b.form << 2);
}

extern "C" size_t ddsp_wavetable_scratch_bytes(int B, int T, int N, int L, int hop)
{
    (void)B; (void)T; (void)N; (void)L; (void)hop;
    return 0;       // neither form of the forward keeps anything: the backward rebuilds the phases from f0
}

extern "C" int ddsp_wavetable_forward(const float *f0, const float *c, const float *a, const float *tables, float *y, void *scratch,
                                      double *phase_io, int B, int T, int N, int L, int hop, int sample_rate, void *stream)
{
    (void)scratch;
    if (bad_shape(B, T, N, L, hop, sample_rate)) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!f0 || !c || !a || !tables || !y) return DDSP_EINVAL;
    if (out_of_range(B, T, N, L, hop)) return DDSP_ERANGE;
    const Plan pl = plan(B, T, N, L, hop, false, phase_io != nullptr, g_mode.load(), g_grid.load());
    if (pl.status) return pl.status;
    WtParams p = {};
    p.f0 = f0; p.c = c; p.a = a; p.W = tables; p.y = y; p.phase_io = phase_io;
    fill_params(p, pl, B, T, N, L, hop, sample_rate);
    static bool done_lds[64], done_glb[64];
    return (int)(pl.form == kFormLds ? launch(wt_forward_kernel<true, false>, done_lds, pl, p, (hipStream_t)stream)
                                     : launch(wt_forward_kernel<false, false>, done_glb, pl, p, (hipStream_t)stream));
}

extern "C" size_t ddsp_wavetable_backward_scratch_bytes(int B, int T, int N, int L, int hop)
{
    if (bad_shape(B, T, N, L, hop, 1) || B == 0 || out_of_range(B, T, N, L, hop)) return 0;
    // (the plan without a start phase: with one the row is one unit and the grid no larger)
    return backward_scratch_bytes(B, T, N, L, plan(B, T, N, L, hop, true, false, g_mode.load(), g_grid.load()).grid);
}

extern "C" int ddsp_wavetable_backward(const float *grad_y, const float *f0, const float *c, const float *a, const float *tables,
                                       const double *phase_in, void *scratch, float *grad_c, float *grad_a, float *grad_tables,
                                       int B, int T, int N, int L, int hop, int sample_rate, void *stream)
{
    if (bad_shape(B, T, N, L, hop, sample_rate)) return DDSP_EINVAL;
    if (B == 0) return 0;                                                       // (nothing is written: the caller zeroes grad_tables)
    if (!grad_y || !f0 || !c || !a || !tables || !scratch || !grad_c || !grad_a || !grad_tables) return DDSP_EINVAL;
    if (out_of_range(B, T, N, L, hop)) return DDSP_ERANGE;
    // (a start phase makes the row one unit, as in the forward it re-walks)
    const Plan pl = plan(B, T, N, L, hop, true, phase_in != nullptr, g_mode.load(), g_grid.load());
    if (pl.status) return pl.status;
    WtParams p = {};
    p.f0 = f0; p.c = c; p.a = a; p.W = tables; p.grad_y = grad_y;
    p.phase_io = const_cast<double *>(phase_in);                                // (read only: the backward kernel never writes it)
    char *ws = static_cast<char *>(scratch);
    p.part_c = reinterpret_cast<float *>(ws);
    p.part_a = reinterpret_cast<float *>(ws + part_c_bytes(B, T, N));
    p.priv = reinterpret_cast<float *>(ws + part_c_bytes(B, T, N) + part_a_bytes(B, T));
    p.grad_c = grad_c; p.grad_a = grad_a; p.grad_W = grad_tables;
    fill_params(p, pl, B, T, N, L, hop, sample_rate);
    static bool done_lds[64], done_glb[64];
    const hipError_t e = pl.form == kFormLds ? launch(wt_backward_kernel<true, false>, done_lds, pl, p, (hipStream_t)stream)
                                             : launch(wt_backward_kernel<false, false>, done_glb, pl, p, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const long frame_blocks = ((long)B * T + kFinishThreads / 64 - 1) / (kFinishThreads / 64);
    const long entry_blocks = ((long)N * L + kFinishThreads - 1) / kFinishThreads;
    hipLaunchKernelGGL(wt_finish_kernel, dim3((unsigned)(frame_blocks + entry_blocks)), dim3(kFinishThreads), 0, (hipStream_t)stream, p,
                       frame_blocks, pl.grid);
    return (int)hipGetLastError();
}

extern "C" int ddsp_wavetable_set_form(int mode)
{
    if (mode != 0 && !ddsp_hooks_on()) return DDSP_EPERM;
    if (mode < 0 || (mode & 3) == 3 || (mode & 0xfc) || mode >= (1 << 24)) return DDSP_ERANGE;
    g_mode.store(mode);
    return 0;
}

extern "C" int ddsp_wavetable_set_grid(int workgroups)
{
    if (workgroups != 0 && !ddsp_hooks_on()) return DDSP_EPERM;
    if (workgroups < 0 || workgroups > kMaxGrid) return DDSP_ERANGE;
    g_grid.store(workgroups);
    return 0;
}

// ---- band-limited entry points: the same walk over the mip levels M [Q + 1, N, L] ---------------------------
namespace {

int out_of_range_bl(long B, long T, long N, long L, long hop)
{
    const int rc = out_of_range(B, T, N, L, hop);
    return rc ? rc : (mip_supported(N, L) ? 0 : DDSP_ERANGE);
}

}  // namespace

extern "C" int ddsp_wavetable_form_bl(int B, int T, int N, int L, int hop)
{
    if (bad_shape(B, T, N, L, hop, 1) || B == 0) return DDSP_EINVAL;
    if (out_of_range_bl(B, T, N, L, hop)) return DDSP_ERANGE;
    const int mode = g_mode.load(), cap = g_grid.load();
    const size_t budget = (size_t)g_mip_lds.load();
    const MipPlan f = plan_mip(B, T, N, L, hop, false, false, mode, cap, budget), b = plan_mip(B, T, N, L, hop, true, false, mode, cap, budget);
    if (f.walk.status) return f.walk.status;
    if (b.walk.status) return b.walk.status;
    return f.walk.form | (b.walk.form << 2) | (f.fit << 8) | (b.fit << 16);
}

extern "C" int ddsp_wavetable_forward_bl(const float *f0, const float *c, const float *a, const float *levels, float *y,
                                         double *phase_io, int B, int T, int N, int L, int hop, int sample_rate, void *stream)
{
    if (bad_shape(B, T, N, L, hop, sample_rate)) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!f0 || !c || !a || !levels || !y) return DDSP_EINVAL;
    if (out_of_range_bl(B, T, N, L, hop)) return DDSP_ERANGE;
    const MipPlan mp = plan_mip(B, T, N, L, hop, false, phase_io != nullptr, g_mode.load(), g_grid.load(), (size_t)g_mip_lds.load());
    if (mp.walk.status) return mp.walk.status;
    WtParams p = {};
    p.f0 = f0; p.c = c; p.a = a; p.W = levels; p.y = y; p.phase_io = phase_io;
    fill_params(p, mp.walk, B, T, N, L, hop, sample_rate);
    p.nlev = mp.levels;
    p.fit = mp.fit;
    static bool done_lds[64], done_glb[64];
    return (int)(mp.fit ? launch(wt_forward_kernel<true, true>, done_lds, mp.walk, p, (hipStream_t)stream)
                        : launch(wt_forward_kernel<false, true>, done_glb, mp.walk, p, (hipStream_t)stream));
}

extern "C" size_t ddsp_wavetable_backward_bl_scratch_bytes(int B, int T, int N, int L, int hop)
{
    if (bad_shape(B, T, N, L, hop, 1) || B == 0 || out_of_range_bl(B, T, N, L, hop)) return 0;
    const MipPlan mp = plan_mip(B, T, N, L, hop, true, false, g_mode.load(), g_grid.load(), (size_t)g_mip_lds.load());
    return mip_backward_scratch_bytes(B, T, N, L, mp.levels, mp.walk.grid);
}

extern "C" int ddsp_wavetable_backward_bl(const float *grad_y, const float *f0, const float *c, const float *a, const float *levels,
                                          const double *phase_in, void *scratch, float *grad_c, float *grad_a, float *grad_levels,
                                          int B, int T, int N, int L, int hop, int sample_rate, void *stream)
{
    if (bad_shape(B, T, N, L, hop, sample_rate)) return DDSP_EINVAL;
    if (B == 0) return 0;                                                       // (nothing is written: the caller zeroes grad_levels)
    if (!grad_y || !f0 || !c || !a || !levels || !scratch || !grad_c || !grad_a || !grad_levels) return DDSP_EINVAL;
    if (out_of_range_bl(B, T, N, L, hop)) return DDSP_ERANGE;
    const MipPlan mp = plan_mip(B, T, N, L, hop, true, phase_in != nullptr, g_mode.load(), g_grid.load(), (size_t)g_mip_lds.load());
    if (mp.walk.status) return mp.walk.status;
    // (the scratch was sized for the plan without a start phase, whose grid is no smaller)
    const int grid_sized = plan_mip(B, T, N, L, hop, true, false, g_mode.load(), g_grid.load(), (size_t)g_mip_lds.load()).walk.grid;
    WtParams p = {};
    p.f0 = f0; p.c = c; p.a = a; p.W = levels; p.grad_y = grad_y;
    p.phase_io = const_cast<double *>(phase_in);                                // (read only)
    char *ws = static_cast<char *>(scratch);
    p.part_c = reinterpret_cast<float *>(ws);
    p.part_a = reinterpret_cast<float *>(ws + part_c_bytes(B, T, N));
    p.priv = reinterpret_cast<float *>(ws + part_c_bytes(B, T, N) + part_a_bytes(B, T));
    if (mp.walk.grid > grid_sized) return DDSP_EINVAL;                          // (never: a start phase makes a row one unit, so no more units)
    p.masks = reinterpret_cast<unsigned *>(ws + part_c_bytes(B, T, N) + part_a_bytes(B, T) + mip_private_bytes(N, L, mp.levels, grid_sized));
    p.grad_c = grad_c; p.grad_a = grad_a; p.grad_W = grad_levels;
    fill_params(p, mp.walk, B, T, N, L, hop, sample_rate);
    p.nlev = mp.levels;
    p.fit = mp.fit;
    static bool done_lds[64], done_glb[64];
    const hipError_t e = mp.fit ? launch(wt_backward_kernel<true, true>, done_lds, mp.walk, p, (hipStream_t)stream)
                                : launch(wt_backward_kernel<false, true>, done_glb, mp.walk, p, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const long frame_blocks = ((long)B * T + kFinishThreads / 64 - 1) / (kFinishThreads / 64);
    const long entry_blocks = ((long)mp.levels * N * L + kFinishThreads - 1) / kFinishThreads;
    hipLaunchKernelGGL(wt_finish_kernel, dim3((unsigned)(frame_blocks + entry_blocks)), dim3(kFinishThreads), 0, (hipStream_t)stream, p,
                       frame_blocks, mp.walk.grid);
    return (int)hipGetLastError();
}

extern "C" int ddsp_wavetable_set_mip_lds(long bytes)
{
    if (bytes != 0 && !ddsp_hooks_on()) return DDSP_EPERM;
    if (bytes < 0 || bytes > (long)kMaxLdsBytes) return DDSP_ERANGE;
    g_mip_lds.store(bytes);
    return 0;
}
