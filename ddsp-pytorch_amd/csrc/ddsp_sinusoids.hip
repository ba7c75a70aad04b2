// Inharmonic sinusoid bank: K sinusoids per batch row, each with its own frame-rate frequency track.
//   f [B,T,K] Hz, c [B,T,K], a [B,T,1] -> y [B, T hop] = up(a) sum_k up(wn_k) sin(2 pi P_k), P_k the inclusive sum of the linearly
//   interpolated g_k = f_k / sample_rate, which has a closed form per segment (ddsp_sinusoids_plan.h): with the segment's start
//   phase Phi[s], P = Phi[s] + (j + 1) (g[s] + d (j + e) / (2 hop)).  Phases are fp64, kept modulo 1.
//   sn_forward_kernel   one launch.  A workgroup of 256 threads takes units (row, chunk of segments) from a capped grid.  A chunk
//                       that does not start the row first sums the segment totals in front of it (a thread per partial, the same
//                       operations in the same order as the walk: the output's bits do not depend on the plan).  An iteration
//                       stages F segments in LDS -- masks, normalised weights, g, d / (2 hop), and Phi by a sequential fp64
//                       prefix per partial -- then walks their samples, a thread per sample looping over the partials: two fp64
//                       FMAs, the reduction into [-1/2, 1/2], v_sin_f32 (which takes turns) and two fp32 FMAs each; the walk
//                       stops at the highest partial that has a weight at any staged frame.
//   sn_backward_kernel  the same units and staging; a thread per (segment, partial) walks the segment's samples from per-sample
//                       records in LDS and keeps every sum it owns in registers: the partial gradients of the weights at the four
//                       frames the samples reach, its share of grad_a, and for grad_f the segment's sum of q and the sums weighted
//                       by the coefficients of g[s] and g[s + 1].  No atomics: the same bits every run.
//   sn_finish_kernel    a wavefront per frame: the partials aimed at the frame, the normalisation's backward, the mask, grad_a.
//   sn_finish_f_kernel  (only with grad_f) a thread per (row, partial): the fp64 suffix sum over the segments and the closed
//                       form's adjoint.
// Every frame index is clamped into [0, T), every LDS frame index into the staged window, every sample index is below T hop.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_osc_common.h"
#include "ddsp_sinusoids_plan.h"

namespace {

using namespace ddsp_sinusoids;
static_assert(kPlanERange == DDSP_ERANGE, "the planner's status is the entry points' return code");

std::atomic<int> g_mode{0};     // ddsp_sinusoids_set_form
std::atomic<int> g_grid{0};     // ddsp_sinusoids_set_grid

struct SnParams {
    const float *f, *c, *a;
    float *y;
    double *phase_io;           // forward: read and replaced; backward: read only
    const float *grad_y;
    float *part_c, *part_a, *part_f;
    float *grad_f, *grad_c, *grad_a;
    int B, T, K, hop;
    int F, chunk_segments, chunks, tile;
    long units;
    int normalize, live;
    int head, e;                // hop / 2; 1 for an even hop, 0 for an odd one
    float scale, nyq;
    double sr, two_hop, seg_coef;       // seg_coef = hop (hop - 1 + e): a segment's total is hop g[s] + seg_coef d / (2 hop)
};

struct Lds {
    double *carry, *base0;      // [K]: the phase at the start of the next segment to stage; the row's start phase (head samples)
    double *phi, *dh;           // [F][K]: the segment's start phase, d / (2 hop)
    double *g;                  // [F + 1][K]: g of the frames s0 .. s0 + F
    float *wn;                  // [F + 3][K]: the weights of the frames s0 - 1 .. s0 + F + 1
    int *kmax;                  // partials [kmax, K) have zero weight at every staged frame
};

__device__ __forceinline__ Lds carve(const SnParams &p, void *smem)
{
    Lds l;
    char *q = static_cast<char *>(smem);
    const size_t K = (size_t)p.K;
    l.kmax = reinterpret_cast<int *>(q);     q += 16;
    l.carry = reinterpret_cast<double *>(q); q += 8 * K;
    l.base0 = reinterpret_cast<double *>(q); q += 8 * K;
    l.phi = reinterpret_cast<double *>(q);   q += 8 * K * p.F;
    l.dh = reinterpret_cast<double *>(q);    q += 8 * K * p.F;
    l.g = reinterpret_cast<double *>(q);     q += 8 * K * (p.F + 1);
    l.wn = reinterpret_cast<float *>(q);
    return l;
}
__device__ __forceinline__ char *behind_staged(const SnParams &p, void *smem)
{
    return static_cast<char *>(smem) + ((16 + (size_t)p.K * (16 + 16 * (size_t)p.F + 8 * ((size_t)p.F + 1) + 4 * ((size_t)p.F + 3)) + 63) & ~(size_t)63);
}

struct Sample {
    int i0, i1;
    float w0, w1;
};

// F.interpolate(linear, align_corners=False) of output sample n: the bracketing frames and their fp32 weights
__device__ __forceinline__ Sample locate(const SnParams &p, int n)
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

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ double wave_sum64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// a valid entry: finite and >= 0
__device__ __forceinline__ bool entry_valid(float f) { return f >= 0.0f && f <= 3.402823466e38f; }
__device__ __forceinline__ double entry_g(const SnParams &p, float f) { return entry_valid(f) ? (double)f / p.sr : 0.0; }
__device__ __forceinline__ bool entry_audible(const SnParams &p, float f) { return entry_valid(f) && !(f > p.nyq); }

__device__ __forceinline__ double frac1(double x) { return x - floor(x); }

// one step of the frame-rate prefix: the phase at the start of segment s + 1 from the one at the start of s
__device__ __forceinline__ double advance(const SnParams &p, double cr, double g0, double dhv)
{
    const double tot = fma(dhv, p.seg_coef, (double)p.hop * g0);
    return frac1(cr + tot);
}

// the unit's start: carry[k] = the phase in front of segment s_begin (for s_begin = 0: in front of the head)
__device__ __forceinline__ void start_unit(const SnParams &p, const Lds &l, int b, int s_begin)
{
    const float *frow = p.f + (long)b * p.T * p.K;
    for (int k = threadIdx.x; k < p.K; k += kThreads) {
        double cr = p.phase_io ? p.phase_io[(long)b * p.K + k] : 0.0;
        if (s_begin > 0) {
            double g0 = entry_g(p, frow[k]);
            cr = frac1(fma((double)p.head, g0, cr));
            for (int r = 0; r < s_begin; ++r) {
                const int t1 = r + 1 < p.T - 1 ? r + 1 : p.T - 1;
                const double g1 = entry_g(p, frow[(long)t1 * p.K + k]);
                cr = advance(p, cr, g0, (g1 - g0) / p.two_hop);
                g0 = g1;
            }
        }
        l.carry[k] = cr;
    }
}

// the fp64 sum of a staged frame's weights over the wavefront, rounded once: every lane gets it (a fixed order)
__device__ __forceinline__ float weight_sum(const float *w, int K)
{
    double S = 0.0;
    for (int k = threadIdx.x & 63; k < K; k += 64) S += (double)w[k];
    return (float)wave_sum64(S);
}

// Stage the segments s0 .. s0 + nseg - 1 of row b (nseg <= F); every thread calls it; barriers inside, none pending at the end
// but the one the caller places before it reads.
__device__ __forceinline__ void stage(const SnParams &p, const Lds &l, int b, int s0, int nseg)
{
    const int tid = threadIdx.x, K = p.K;
    const float *frow = p.f + (long)b * p.T * K, *crow = p.c + (long)b * p.T * K;
    const int FW = p.F + 3;
    if (tid == 0) *l.kmax = 0;
    __syncthreads();
    for (int i = tid; i < FW * K; i += kThreads) {
        const int fi = i / K, k = i - fi * K;
        const int t = clampi(s0 - 1 + fi, 0, p.T - 1);
        const float fv = frow[(long)t * K + k];
        const float w = entry_audible(p, fv) ? crow[(long)t * K + k] : 0.0f;
        l.wn[i] = w;
        if (!(w == 0.0f)) atomicMax(l.kmax, k + 1);                             // (NaN counts: it has to reach the output)
        if (fi >= 1 && fi <= p.F + 1) l.g[(fi - 1) * K + k] = entry_g(p, fv);
    }
    __syncthreads();
    if (p.normalize) {
        for (int fi = tid >> 6; fi < FW; fi += kThreads / 64) {
            float *w = l.wn + fi * K;
            const float Sf = weight_sum(w, K);
            for (int k = tid & 63; k < K; k += 64) w[k] = Sf == 0.0f ? 0.0f : w[k] / Sf;
        }
    }
    for (int k = tid; k < K; k += kThreads) {
        double cr = l.carry[k];
        for (int si = 0; si < nseg; ++si) {
            const double g0 = l.g[si * K + k], g1 = l.g[(si + 1) * K + k];
            const double dhv = (g1 - g0) / p.two_hop;
            if (s0 + si == 0) {
                l.base0[k] = cr;
                cr = frac1(fma((double)p.head, g0, cr));
            }
            l.phi[si * K + k] = cr;
            l.dh[si * K + k] = dhv;
            if (p.live && p.y && s0 + si == p.T - 1)    // the phase of the row's last sample, carried to the next block
                p.phase_io[(long)b * K + k] = frac1(fma((double)(p.hop - p.head), g0, cr));
            cr = advance(p, cr, g0, dhv);
        }
        l.carry[k] = cr;
    }
    __syncthreads();
}

// the samples of the segments s0 .. s0 + nseg - 1: [n_begin, n_end)
__device__ __forceinline__ void sample_range(const SnParams &p, int s0, int nseg, int &n_begin, int &n_end)
{
    n_begin = s0 == 0 ? 0 : p.head + s0 * p.hop;
    n_end = s0 + nseg >= p.T ? p.T * p.hop : p.head + (s0 + nseg) * p.hop;
}

__global__ void __launch_bounds__(kThreads) sn_forward_kernel(const SnParams p)
{
    extern __shared__ double smem[];
    const Lds l = carve(p, smem);
    const int tid = threadIdx.x, K = p.K;
    const long Ns = (long)p.T * p.hop;
    for (long unit = blockIdx.x; unit < p.units; unit += gridDim.x) {
        const int b = (int)(unit / p.chunks), ch = (int)(unit % p.chunks);
        const int s_begin = ch * p.chunk_segments;
        const int s_end = s_begin + p.chunk_segments < p.T ? s_begin + p.chunk_segments : p.T;
        const float *arow = p.a + (long)b * p.T;
        __syncthreads();                                                        // (the last unit's readers of the LDS are done)
        start_unit(p, l, b, s_begin);
        __syncthreads();
        for (int s0 = s_begin; s0 < s_end; s0 += p.F) {
            const int nseg = s0 + p.F < s_end ? p.F : s_end - s0;
            stage(p, l, b, s0, nseg);
            int n_begin, n_end;
            sample_range(p, s0, nseg, n_begin, n_end);
            for (int n = n_begin + tid; n < n_end; n += kThreads) {
                const Sample sm = locate(p, n);
                const int wi0 = clampi(sm.i0 - (s0 - 1), 0, p.F + 2), wi1 = clampi(sm.i1 - (s0 - 1), 0, p.F + 2);
                const int m = n - p.head;
                const bool hd = m < 0;
                const int s = hd ? 0 : m / p.hop;
                const int j = hd ? n : m - s * p.hop;
                const int si = clampi(s - s0, 0, nseg - 1);
                const double mult = (double)(j + 1), xe = hd ? 0.0 : (double)(j + p.e);
                const double *pb = hd ? l.base0 : l.phi + si * K, *pg = l.g + si * K, *pd = l.dh + si * K;
                const float *pw0 = l.wn + wi0 * K, *pw1 = l.wn + wi1 * K;
                float acc = 0.0f;
                // partials that are silent at every staged frame (above Nyquist for the whole stretch, as the upper partials of
                // most notes are) would add zero to every sum: the walk stops at the highest one that is heard
                const int kmax = *l.kmax;
                for (int k = 0; k < kmax; ++k) {
                    const double t1 = fma(pd[k], xe, pg[k]);
                    const double P = fma(mult, t1, pb[k]);
                    const float r = (float)(P - rint(P));
                    const float sv = __builtin_amdgcn_sinf(r);
                    const float wv = __fmaf_rn(sm.w0, pw0[k], sm.w1 * pw1[k]);
                    acc = __fmaf_rn(wv, sv, acc);
                }
                const float au = __fmaf_rn(sm.w0, arow[sm.i0], sm.w1 * arow[sm.i1]);
                p.y[(long)b * Ns + n] = au * acc;
            }
            __syncthreads();
        }
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
struct Record {
    float gyau, gy, w0, w1, cA, cB;
    int bits;           // j (head samples: n) in bits 0-11, head in bit 12, the slots of i0 and i1 in bits 13-14 and 15-16
    int pad;
};
static_assert(sizeof(Record) == kRecordBytes, "the planner sizes the tile");

template <bool kGradF>
__global__ void __launch_bounds__(kThreads) sn_backward_kernel(const SnParams p)
{
    extern __shared__ double smem[];
    const Lds l = carve(p, smem);
    float *ra = reinterpret_cast<float *>(behind_staged(p, smem));              // [F][kSlots][K]
    Record *rec = reinterpret_cast<Record *>(ra + (size_t)kSlots * p.F * p.K);  // [tile]
    const int tid = threadIdx.x, K = p.K;
    const long Ns = (long)p.T * p.hop;
    for (long unit = blockIdx.x; unit < p.units; unit += gridDim.x) {
        const int b = (int)(unit / p.chunks), ch = (int)(unit % p.chunks);
        const int s_begin = ch * p.chunk_segments;
        const int s_end = s_begin + p.chunk_segments < p.T ? s_begin + p.chunk_segments : p.T;
        const float *arow = p.a + (long)b * p.T;
        __syncthreads();
        start_unit(p, l, b, s_begin);
        __syncthreads();
        for (int s0 = s_begin; s0 < s_end; s0 += p.F) {
            const int nseg = s0 + p.F < s_end ? p.F : s_end - s0;
            stage(p, l, b, s0, nseg);
            int n_begin, n_end;
            sample_range(p, s0, nseg, n_begin, n_end);
            const int cnt = n_end - n_begin, items = nseg * K;
            for (int base = 0; base < items; base += kThreads) {                // one round unless K > kThreads
                const int it = base + tid;
                const bool own = it < items;
                const int si = own ? it / K : 0, k = own ? it - si * K : 0;
                const int s = s0 + si;
                // the segment's samples, relative to n_begin
                int lo, hi;
                {
                    int a0, a1;
                    sample_range(p, s, 1, a0, a1);
                    lo = a0 - n_begin;
                    hi = a1 - n_begin;
                }
                const double phiv = l.phi[si * K + k], b0v = l.base0[k], gv = l.g[si * K + k], dhv = l.dh[si * K + k];
                const float wn0 = l.wn[si * K + k], wn1 = l.wn[(si + 1) * K + k], wn2 = l.wn[(si + 2) * K + k],
                            wn3 = l.wn[(si + 3) * K + k];                       // frames s - 1 .. s + 2
                float E0 = 0.0f, E1 = 0.0f, E2 = 0.0f, E3 = 0.0f, R0 = 0.0f, R1 = 0.0f, R2 = 0.0f, R3 = 0.0f;
                float Q = 0.0f, A = 0.0f, Bc = 0.0f;
                for (int tile0 = 0; tile0 < cnt; tile0 += p.tile) {
                    const int tl = cnt - tile0 < p.tile ? cnt - tile0 : p.tile;
                    __syncthreads();                                            // (the last tile's readers are done)
                    for (int i = tid; i < tl; i += kThreads) {
                        const int n = n_begin + tile0 + i;
                        const Sample sm = locate(p, n);
                        const int m = n - p.head;
                        const bool hd = m < 0;
                        const int sg = hd ? 0 : m / p.hop;
                        const int j = hd ? n : m - sg * p.hop;
                        const float gy = p.grad_y[(long)b * Ns + n];
                        const float au = __fmaf_rn(sm.w0, arow[sm.i0], sm.w1 * arow[sm.i1]);
                        Record r;
                        r.gyau = gy * au;
                        r.gy = gy;
                        r.w0 = sm.w0;
                        r.w1 = sm.w1;
                        // P = Phi[s] + cA g[s] + cB g[s + 1]; the head and the last segment hear one frame only
                        r.cB = (hd || sg >= p.T - 1) ? 0.0f : (float)(j + 1) * ((float)(j + p.e) / (float)(2 * p.hop));
                        r.cA = (float)(j + 1) - r.cB;
                        r.bits = j | (hd ? 1 << 12 : 0) | (clampi(sm.i0 - (sg - 1), 0, 3) << 13) | (clampi(sm.i1 - (sg - 1), 0, 3) << 15);
                        r.pad = 0;
                        rec[i] = r;
                    }
                    __syncthreads();
                    if (!own) continue;
                    const int i_lo = lo > tile0 ? lo : tile0, i_hi = hi < tile0 + tl ? hi : tile0 + tl;
                    for (int i = i_lo; i < i_hi; ++i) {
                        const Record r = rec[i - tile0];
                        const int j = r.bits & 0xfff;
                        const bool hd = (r.bits >> 12) & 1;
                        const int x0 = (r.bits >> 13) & 3, x1 = (r.bits >> 15) & 3;
                        const double mult = (double)(j + 1), xe = hd ? 0.0 : (double)(j + p.e);
                        const double t1 = fma(dhv, xe, gv);
                        const double P = fma(mult, t1, hd ? b0v : phiv);
                        const float rf = (float)(P - rint(P));
                        const float sv = __builtin_amdgcn_sinf(rf);
                        const bool usual = x0 == 1 && x1 == 2;
                        const float u0 = usual ? wn1 : (x0 == 0 ? wn0 : (x0 == 1 ? wn1 : (x0 == 2 ? wn2 : wn3)));
                        const float u1 = usual ? wn2 : (x1 == 0 ? wn0 : (x1 == 1 ? wn1 : (x1 == 2 ? wn2 : wn3)));
                        const float wv = __fmaf_rn(r.w0, u0, r.w1 * u1);
                        const float v = r.gyau * sv;                            // towards the weights
                        const float u = (r.gy * wv) * sv;                       // towards the loudness
                        if (usual) {
                            E1 = __fmaf_rn(r.w0, v, E1);
                            E2 = __fmaf_rn(r.w1, v, E2);
                            R1 = __fmaf_rn(r.w0, u, R1);
                            R2 = __fmaf_rn(r.w1, u, R2);
                        } else {            // the row's ends, and a sample whose fp32 source index fell across a frame
                            const float e0 = r.w0 * v, e1 = r.w1 * v, r0 = r.w0 * u, r1 = r.w1 * u;
                            E0 += (x0 == 0 ? e0 : 0.0f) + (x1 == 0 ? e1 : 0.0f);
                            E1 += (x0 == 1 ? e0 : 0.0f) + (x1 == 1 ? e1 : 0.0f);
                            E2 += (x0 == 2 ? e0 : 0.0f) + (x1 == 2 ? e1 : 0.0f);
                            E3 += (x0 == 3 ? e0 : 0.0f) + (x1 == 3 ? e1 : 0.0f);
                            R0 += (x0 == 0 ? r0 : 0.0f) + (x1 == 0 ? r1 : 0.0f);
                            R1 += (x0 == 1 ? r0 : 0.0f) + (x1 == 1 ? r1 : 0.0f);
                            R2 += (x0 == 2 ? r0 : 0.0f) + (x1 == 2 ? r1 : 0.0f);
                            R3 += (x0 == 3 ? r0 : 0.0f) + (x1 == 3 ? r1 : 0.0f);
                        }
                        if constexpr (kGradF) {
                            const float cv = __builtin_amdgcn_cosf(rf);
                            const float q = ((r.gyau * ddsp_osc::kTwoPi32) * wv) * cv;
                            if (!hd) Q += q;
                            A = __fmaf_rn(r.cA, q, A);
                            Bc = __fmaf_rn(r.cB, q, Bc);
                        }
                    }
                }
                if (own) {
                    const long seg = (long)b * p.T + s;
                    float *pc = p.part_c + seg * kSlots * K + k;
                    pc[0] = E0; pc[K] = E1; pc[2 * K] = E2; pc[3 * K] = E3;
                    float *r4 = ra + (size_t)si * kSlots * K + k;
                    r4[0] = R0; r4[K] = R1; r4[2 * K] = R2; r4[3 * K] = R3;
                    if constexpr (kGradF) {
                        float *pf = p.part_f + seg * 3 * K + k;
                        pf[0] = Q; pf[K] = A; pf[2 * K] = Bc;
                    }
                }
            }
            __syncthreads();
            // grad_a's partials: the sum over the partials per (segment, slot), lanes strided, then the butterfly
            for (int pr = tid >> 6; pr < nseg * kSlots; pr += kThreads / 64) {
                const float *src = ra + (size_t)pr * K;
                float v = 0.0f;
                for (int k = tid & 63; k < K; k += 64) v += src[k];
                v = wave_sum(v);
                if ((tid & 63) == 0) p.part_a[((long)b * p.T + s0) * kSlots + pr] = v;
            }
            __syncthreads();
        }
    }
}

constexpr int kFinishThreads = 256;

// a wavefront per frame
__global__ void __launch_bounds__(kFinishThreads) sn_finish_kernel(const SnParams p)
{
    const int lane = threadIdx.x & 63, K = p.K;
    const long frame = (long)blockIdx.x * (kFinishThreads / 64) + (threadIdx.x >> 6);
    if (frame >= (long)p.B * p.T) return;
    const int t = (int)(frame % p.T);
    const float *f = p.f + frame * K, *c = p.c + frame * K;
    // the partials aimed at this frame: slot x of segment s aims at frame s - 1 + x; segments t - 2, t - 1, t, t + 1 in that order
    auto gathered = [&](const float *part, long stride, int k) {
        float g = part[(frame * kSlots + 1) * stride + k];
        if (t > 0) g = part[((frame - 1) * kSlots + 2) * stride + k] + g;
        if (t > 1) g = part[((frame - 2) * kSlots + 3) * stride + k] + g;
        if (t + 1 < p.T) g += part[((frame + 1) * kSlots + 0) * stride + k];
        return g;
    };
    if (p.normalize) {
        double S = 0.0;
        for (int k = lane; k < K; k += 64) S += (double)(entry_audible(p, f[k]) ? c[k] : 0.0f);
        const float Sf = (float)wave_sum64(S);
        float D = 0.0f;
        for (int k = lane; k < K; k += 64) {
            const float w = entry_audible(p, f[k]) ? c[k] : 0.0f;
            D = __fmaf_rn(gathered(p.part_c, K, k), Sf == 0.0f ? 0.0f : w / Sf, D);
        }
        D = wave_sum(D);
        for (int k = lane; k < K; k += 64)
            p.grad_c[frame * K + k] = (entry_audible(p, f[k]) && Sf != 0.0f) ? (gathered(p.part_c, K, k) - D) / Sf : 0.0f;
    } else {
        for (int k = lane; k < K; k += 64) p.grad_c[frame * K + k] = entry_audible(p, f[k]) ? gathered(p.part_c, K, k) : 0.0f;
    }
    if (lane == 0) p.grad_a[frame] = gathered(p.part_a, 1, 0);
}

// a thread per (row, partial): grad_g[t] = A[t] + Bc[t - 1] + (hop + 1 - e) / 2 R[t] + (hop - 1 + e) / 2 R[t - 1] (+ head R[-1] at
// t = 0), R[t] = the sum of Q over the segments behind t, in fp64 from the row's end
__global__ void __launch_bounds__(kFinishThreads) sn_finish_f_kernel(const SnParams p)
{
    const long id = (long)blockIdx.x * kFinishThreads + threadIdx.x;
    if (id >= (long)p.B * p.K) return;
    const int K = p.K;
    const long b = id / K;
    const int k = (int)(id - b * K);
    const float *pf = p.part_f + b * p.T * 3 * K + k;
    const float *f = p.f + b * p.T * K + k;
    float *out = p.grad_f + b * p.T * K + k;
    const double hA = 0.5 * (double)(p.hop + 1 - p.e), hB = 0.5 * (double)(p.hop - 1 + p.e);
    double R = 0.0;
    for (int t = p.T - 1; t >= 0; --t) {
        const float *row = pf + (long)t * 3 * K;
        const double Rm1 = R + (double)row[0];
        double gg = (double)row[K] + hA * R;
        if (t > 0) gg += (double)(row - 3 * K)[2 * K] + hB * Rm1;
        else gg += (double)p.head * Rm1;
        out[(long)t * K] = entry_valid(f[(long)t * K]) ? (float)(gg / p.sr) : 0.0f;
        R = Rm1;
    }
}

// shape checks shared by the entry points: DDSP_EINVAL, then (the caller: empty batch, pointers), then DDSP_ERANGE
int bad_shape(long B, long T, long K, long hop, long sample_rate) { return (B < 0 || T < 1 || K < 1 || hop < 1 || sample_rate < 1) ? DDSP_EINVAL : 0; }
int out_of_range(long B, long T, long K, long hop)
{
    if (!supported(K, hop) || T > kMaxSamples / hop || B > (1l << 24)) return DDSP_ERANGE;
    if (B * T > (1l << 40) / (kSlots * K)) return DDSP_ERANGE;                  // (scratch indices are 64-bit; a sanity limit)
    return 0;
}

void fill_params(SnParams &p, const Plan &pl, int B, int T, int K, int hop, int sample_rate, int normalize)
{
    p.B = B; p.T = T; p.K = K; p.hop = hop;
    p.F = pl.iter_segments;
    p.chunk_segments = pl.chunk_segments;
    p.chunks = pl.chunks;
    p.tile = pl.tile;
    p.units = pl.units;
    p.normalize = normalize ? 1 : 0;
    p.live = p.phase_io != nullptr;
    p.head = hop / 2;
    p.e = hop % 2 == 0 ? 1 : 0;
    p.scale = 1.0f / (float)hop;
    p.nyq = (float)(sample_rate / 2);
    p.sr = (double)sample_rate;
    p.two_hop = 2.0 * (double)hop;
    p.seg_coef = (double)hop * (double)(hop - 1 + p.e);
}

template <typename Kn>
hipError_t launch(Kn kernel, bool (&done)[64], const Plan &pl, const SnParams &p, hipStream_t s)
{
    if (pl.lds_bytes > kSmallLds) {
        const hipError_t e = ddsp_allow_big_lds(reinterpret_cast<const void *>(kernel), done);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid), dim3(kThreads), pl.lds_bytes, s, p);
    return hipGetLastError();
}

}  // namespace

extern "C" int ddsp_sinusoids_supported(int K, int hop) { return supported(K, hop) ? 1 : 0; }

extern "C" size_t ddsp_sinusoids_scratch_bytes(int B, int T, int K, int hop)
{
    (void)B; (void)T; (void)K; (void)hop;
    return 0;       // one launch that keeps nothing: a chunk re-sums the segment totals in front of it, the backward re-walks from f
}

extern "C" int ddsp_sinusoids_forward(const float *f, const float *c, const float *a, float *y, void *scratch, double *phase_io, int B,
                                      int T, int K, int hop, int sample_rate, int normalize, void *stream)
{
    (void)scratch;
    if (bad_shape(B, T, K, hop, sample_rate)) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!f || !c || !a || !y) return DDSP_EINVAL;
    if (out_of_range(B, T, K, hop)) return DDSP_ERANGE;
    const Plan pl = plan(B, T, K, hop, false, phase_io != nullptr, g_mode.load(), g_grid.load());
    if (pl.status) return pl.status;
    SnParams p = {};
    p.f = f; p.c = c; p.a = a; p.y = y; p.phase_io = phase_io;
    fill_params(p, pl, B, T, K, hop, sample_rate, normalize);
    static bool done[64];
    return (int)launch(sn_forward_kernel, done, pl, p, (hipStream_t)stream);
}

extern "C" size_t ddsp_sinusoids_backward_scratch_bytes(int B, int T, int K, int hop, int want_grad_f)
{
    if (bad_shape(B, T, K, hop, 1) || B == 0 || out_of_range(B, T, K, hop)) return 0;
    return backward_scratch_bytes(B, T, K, want_grad_f != 0);
}

extern "C" int ddsp_sinusoids_backward(const float *grad_y, const float *f, const float *c, const float *a, void *scratch, float *grad_f,
                                       float *grad_c, float *grad_a, const double *phase, int B, int T, int K, int hop, int sample_rate,
                                       int normalize, void *stream)
{
    if (bad_shape(B, T, K, hop, sample_rate)) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!grad_y || !f || !c || !a || !scratch || !grad_c || !grad_a) return DDSP_EINVAL;
    if (out_of_range(B, T, K, hop)) return DDSP_ERANGE;
    // (a start phase makes the row one unit, as in the forward it re-walks; the partials' bits do not depend on the chunks)
    const Plan pl = plan(B, T, K, hop, true, phase != nullptr, g_mode.load(), g_grid.load());
    if (pl.status) return pl.status;
    SnParams p = {};
    p.f = f; p.c = c; p.a = a; p.grad_y = grad_y;
    p.phase_io = const_cast<double *>(phase);                                   // (read only: p.y is null, so stage() never writes it)
    char *ws = static_cast<char *>(scratch);
    p.part_c = reinterpret_cast<float *>(ws);
    p.part_a = reinterpret_cast<float *>(ws + part_c_bytes(B, T, K));
    p.part_f = grad_f ? reinterpret_cast<float *>(ws + part_c_bytes(B, T, K) + part_a_bytes(B, T)) : nullptr;
    p.grad_f = grad_f; p.grad_c = grad_c; p.grad_a = grad_a;
    fill_params(p, pl, B, T, K, hop, sample_rate, normalize);
    static bool done_f[64], done_n[64];
    const hipError_t e = grad_f ? launch(sn_backward_kernel<true>, done_f, pl, p, (hipStream_t)stream)
                                : launch(sn_backward_kernel<false>, done_n, pl, p, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const long frame_blocks = ((long)B * T + kFinishThreads / 64 - 1) / (kFinishThreads / 64);
    hipLaunchKernelGGL(sn_finish_kernel, dim3((unsigned)frame_blocks), dim3(kFinishThreads), 0, (hipStream_t)stream, p);
    const hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess) return (int)e2;
    if (grad_f) {
        const long blocks = ((long)B * K + kFinishThreads - 1) / kFinishThreads;
        hipLaunchKernelGGL(sn_finish_f_kernel, dim3((unsigned)blocks), dim3(kFinishThreads), 0, (hipStream_t)stream, p);
    }
    return (int)hipGetLastError();
}

extern "C" int ddsp_sinusoids_set_form(int mode)
{
    if (mode != 0 && !ddsp_hooks_on()) return DDSP_EPERM;
    if (mode < 0 || (mode & 0xff)) return DDSP_ERANGE;
    g_mode.store(mode);
    return 0;
}

extern "C" int ddsp_sinusoids_set_grid(int workgroups)
{
    if (workgroups != 0 && !ddsp_hooks_on()) return DDSP_EPERM;
    if (workgroups < 0 || workgroups > kMaxGrid) return DDSP_ERANGE;
    g_grid.store(workgroups);
    return 0;
}
