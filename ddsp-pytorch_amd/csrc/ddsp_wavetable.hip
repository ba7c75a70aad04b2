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
// Every frame index is clamped into [0, T), every entry into [0, L), every sample index is below T hop.
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
__device__ __forceinline__ void fetch4(const WtParams &p, const float4 *img, int q, int j, float4 &lo, float4 &hi)
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
            const float *row = p.W + (long)(ok ? k : 0) * p.L;
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
__device__ __forceinline__ void stage_image(const WtParams &p, float *img)
{
    const int rows = p.L + 1, NP = 4 * p.P4;
    for (long i = threadIdx.x; i < (long)NP * rows; i += kThreads) {
        const int k = (int)(i / rows), row = (int)(i % rows);
        img[4 * image_unit(row, p.P4) + k] = k < p.N ? p.W[(long)k * p.L + (row == p.L ? 0 : row)] : 0.0f;
    }
}

template <bool kLds>
__global__ void __launch_bounds__(kThreads) wt_forward_kernel(const WtParams p)
{
    extern __shared__ float4 smem[];
    double *head = reinterpret_cast<double *>(smem);
    const float4 *img = smem + kHeadBytes / 16;
    if constexpr (kLds) {
        stage_image(p, reinterpret_cast<float *>(smem + kHeadBytes / 16));
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
            const float *c0 = crow + (long)s.i0 * p.N, *c1 = crow + (long)s.i1 * p.N;
            float A0 = 0.0f, A1 = 0.0f;
            double S0 = 0.0, S1 = 0.0;
            for (int q = 0; q < p.Q; ++q) {
                float4 lo, hi;
                fetch4<kLds>(p, img, q, j, lo, hi);
                const float4 v = lerp4(fr, lo, hi);
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

template <bool kLds>
__global__ void __launch_bounds__(kThreads) wt_backward_kernel(const WtParams p)
{
    extern __shared__ float4 smem[];
    double *head = reinterpret_cast<double *>(smem);
    const long img_units = image_unit(p.L, p.P4) + p.P4;
    const float4 *img = smem + kHeadBytes / 16;
    float *priv_lds = reinterpret_cast<float *>(smem + kHeadBytes / 16 + img_units);
    float4 *rec = smem + kHeadBytes / 16 + (kLds ? 2 * img_units : 0);
    const int tid = threadIdx.x;
    const long NL = (long)p.N * p.L;
    float *slice = p.priv + (long)blockIdx.x * NL;
    if constexpr (kLds) {
        stage_image(p, reinterpret_cast<float *>(smem + kHeadBytes / 16));
        for (long i = tid; i < 4 * img_units; i += kThreads) priv_lds[i] = 0.0f;
    } else {
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
            const double P = block_scan((double)u, head, carry);
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
                float A0 = 0.0f, A1 = 0.0f;
                for (int q = 0; q < p.Q; ++q) {
                    float4 lo, hi;
                    fetch4<kLds>(p, img, q, j, lo, hi);
                    const float4 v = lerp4(fr, lo, hi);
                    const float4 x0 = load4(c0, q, p.N, p.vec), x1 = load4(c1, q, p.N, p.vec);
                    A0 = __fmaf_rn(x0.x, v.x, A0); A0 = __fmaf_rn(x0.y, v.y, A0); A0 = __fmaf_rn(x0.z, v.z, A0); A0 = __fmaf_rn(x0.w, v.w, A0);
                    A1 = __fmaf_rn(x1.x, v.x, A1); A1 = __fmaf_rn(x1.y, v.y, A1); A1 = __fmaf_rn(x1.z, v.z, A1); A1 = __fmaf_rn(x1.w, v.w, A1);
                    const float m[4] = {__fmaf_rn(r0, x0.x, r1 * x1.x), __fmaf_rn(r0, x0.y, r1 * x1.y), __fmaf_rn(r0, x0.z, r1 * x1.z),
                                        __fmaf_rn(r0, x0.w, r1 * x1.w)};
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const int k = 4 * q + x;
                        if (k >= p.N) break;
                        if constexpr (kLds) {
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
                            float4 lo, hi;
                            fetch4<kLds>(p, img, kind, __float_as_int(ra.x), lo, hi);
                            const float4 v = lerp4(ra.y, lo, hi);
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
    if constexpr (kLds) {   // the private image -> this workgroup's [N, L] slice; row L belongs to entry 0
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
    const long NL = (long)p.N * p.L;
    const long i = ((long)blockIdx.x - frame_blocks) * kFinishThreads + threadIdx.x;
    if (i >= NL) return;
    float v = 0.0f;
    for (int w = 0; w < nwg; ++w) v += p.priv[(long)w * NL + i];
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
    return (int)(pl.form == kFormLds ? launch(wt_forward_kernel<true>, done_lds, pl, p, (hipStream_t)stream)
                                     : launch(wt_forward_kernel<false>, done_glb, pl, p, (hipStream_t)stream));
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
    const hipError_t e = pl.form == kFormLds ? launch(wt_backward_kernel<true>, done_lds, pl, p, (hipStream_t)stream)
                                             : launch(wt_backward_kernel<false>, done_glb, pl, p, (hipStream_t)stream);
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
