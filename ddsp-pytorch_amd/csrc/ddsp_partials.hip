// Inharmonic analysis, the inverse of the sinusoid bank: from audio and K frequency tracks the per-frame
// complex amplitudes of the partials along the bank's own fp64 phase tracks, the bank's controls a and c, each partial's
// reassigned frequency, and the tonal part / residual of the audio.
//   prefix       one thread per (row, partial) walks the T segments: g = f / sr, d / (2 hop) and Phi, the phase at the segment's
//                start kept modulo 1 -- the terms of section 5d's prefix in the same order (ddsp_sinusoids.hip: stage, advance), so
//                the analysis demodulates along the phase the bank plays, to the bit.  Frame-rate work: T K fp64 additions.
//   analysis     one workgroup per (row, frame): w audio (and w' audio when f_re is wanted) -> LDS; lane l of every wavefront owns
//                the partials l + 1, l + 65, l + 129, l + 193, so every LDS read is a broadcast and no partial is reduced across
//                lanes; the four wavefronts take a quarter of the window each, in ascending j.  All lanes of a wavefront are on
//                the same sample, so its segment is wave-uniform: per segment and owned partial a lane loads Phi, g and
//                d / (2 hop), per (sample, partial) it runs the forward's two fp64 FMAs, P - rint(P) rounded to fp32,
//                v_sin_f32 / v_cos_f32 (which take turns) and two FMAs, four with D.  Slots of 64 partials that are wholly masked
//                at the frame are skipped (the same for every lane).  The wavefronts' sums are added in wavefront order, a in a
//                fixed butterfly: the same bits whatever the batch.
//   resynthesis  one workgroup per (row, segment between two frame centres -- which is the prefix's segment): C[t], C[t + 1] - C[t],
//                Phi, g and d / (2 hop) of every partial staged in LDS; a lane owns a sample and walks the partials in ascending k
//                up to the last non-zero one.
// The matrix cores are not used: the operand exp(-2 pi i P_k[j]) (K x W) is generated per frame and multiplies one vector, so
// nothing is reused; the work is the sine / cosine pair per (partial, sample) behind two fp64 FMAs, which is VALU work.
// Every frame index is below T, every partial index read is clamped below K, every sample index is inside [0, T hop).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"

namespace {

constexpr int kMaxW = 4096;                     // window samples (even)
constexpr int kMaxK = 256;                      // partials: four slots of 64 per lane
constexpr int kSlots = kMaxK / 64;
constexpr int kMaxHop = 1024;
constexpr long kMaxSamples = 1l << 24;          // T hop (sample indices fit an int with room)
constexpr int kMaxBlocks = 8192;                // frames / segments beyond this many are walked grid-strided
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr size_t kWindowBytes = (size_t)kMaxW * sizeof(float);
constexpr size_t kSmallLds = 64 * 1024;

__device__ __forceinline__ bool usable(float f) { return fabsf(f) < INFINITY && f > 0.0f; }
__device__ __forceinline__ double frac1(double x) { return x - floor(x); }

__device__ __forceinline__ double wave_sum64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One thread per (row, partial), grid-strided above the cap.  Section 5d's prefix with P0 = 0: Phi[0] = frac(head g[0]),
// Phi[s + 1] = frac(Phi[s] + tot[s]), tot[s] = fma(d / (2 hop), hop (hop - 1 + e), hop g[s]), d = g[s + 1] - g[s] (0 behind the last frame).
__global__ void __launch_bounds__(kThreads) pt_prefix_kernel(const float *__restrict__ f, double *__restrict__ phi, double *__restrict__ g,
                                                             double *__restrict__ dh, long rows_k, int T, int K, int hop, double sr)
{
    for (long id = (long)blockIdx.x * kThreads + threadIdx.x; id < rows_k; id += (long)gridDim.x * kThreads) {
        const long b = id / K;
        const int k = (int)(id - b * K);
        const long base = b * T * K + k;
        const int head = hop / 2, e = hop % 2 == 0 ? 1 : 0;
        const double two_hop = 2.0 * (double)hop, seg_coef = (double)hop * (double)(hop - 1 + e);
        const float f0 = f[base];
        double g0 = usable(f0) ? (double)f0 / sr : 0.0;
        double cr = frac1(fma((double)head, g0, 0.0));
        for (int s = 0; s < T; ++s) {
            const int t1 = s + 1 < T - 1 ? s + 1 : T - 1;
            const float f1 = f[base + (long)t1 * K];
            const double g1 = usable(f1) ? (double)f1 / sr : 0.0;
            const double dhv = (g1 - g0) / two_hop;
            const long at = base + (long)s * K;
            phi[at] = cr;
            g[at] = g0;
            dh[at] = dhv;
            const double tot = fma(dhv, seg_coef, (double)hop * g0);
            cr = frac1(cr + tot);
            g0 = g1;
        }
    }
}

// the periodic Hann window and its derivative per sample, (pi / W) sin(2 pi j / W), evaluated in fp64 and rounded once
__global__ void pt_window_kernel(float *__restrict__ win, float *__restrict__ dwin, int W)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < W) {
        win[j] = (float)(0.5 - 0.5 * cospi(2.0 * (double)j / (double)W));
        dwin[j] = (float)(M_PI / (double)W * sinpi(2.0 * (double)j / (double)W));
    }
}

// sum_{j < m} w[j] = m / 2 - sin(pi m / W) cos(pi (m - 1) / W) / (2 sin(pi / W))
__device__ double window_prefix(long m, int W)
{
    const double w = (double)W;
    return 0.5 * (double)m - 0.5 * sinpi((double)m / w) * cospi((double)(m - 1) / w) / sinpi(1.0 / w);
}

struct Tracks {
    const double *phi, *g, *dh;                 // the row's [T, K]
    int T, K, hop, head, e, N;
};

// One wavefront's share of a frame: sum_j x[j] exp(-2 pi i P_k[n0 + j]) over its window samples [jlo, jhi) (all inside the clip),
// j ascending, for the lane's partials k = 64 sl + lane, sl < LIVE; with DERIV the same under the second window.  The samples are
// walked piece by piece: the head (n < hop / 2, phase (n + 1) g[0]) and then one piece per segment, whose Phi, g and d / (2 hop)
// the lane loads once.
template <int LIVE, bool DERIV>
__device__ __forceinline__ void pt_window_sums(const Tracks &tr, const float *xs, const float *ds, int n0, int jlo, int jhi, int lane,
                                               float (&cr)[kSlots], float (&ci)[kSlots], float (&dr)[kSlots], float (&di)[kSlots])
{
    int j = jlo;
    while (j < jhi) {
        const int n = n0 + j;
        const bool hd = n < tr.head;
        int s = hd ? 0 : (n - tr.head) / tr.hop;
        s = s < tr.T - 1 ? s : tr.T - 1;
        const int piece_end = hd ? tr.head : (s == tr.T - 1 ? tr.N : tr.head + (s + 1) * tr.hop);
        const int jj0 = hd ? n : n - tr.head - s * tr.hop;
        int cnt = piece_end - n;
        cnt = cnt < jhi - j ? cnt : jhi - j;
        double phi[LIVE], g[LIVE], dh[LIVE];
#pragma unroll
        for (int sl = 0; sl < LIVE; ++sl) {
            const int k = 64 * sl + lane < tr.K ? 64 * sl + lane : tr.K - 1;
            const long at = (long)s * tr.K + k;
            phi[sl] = hd ? 0.0 : tr.phi[at];
            g[sl] = tr.g[at];
            dh[sl] = hd ? 0.0 : tr.dh[at];
        }
        for (int i = 0; i < cnt; ++i) {
            const float x = xs[j + i];
            const float d = DERIV ? ds[j + i] : 0.0f;
            const double mult = (double)(jj0 + i + 1), xe = (double)(jj0 + i + tr.e);
#pragma unroll
            for (int sl = 0; sl < LIVE; ++sl) {
                const double t1 = fma(dh[sl], xe, g[sl]);
                const double P = fma(mult, t1, phi[sl]);
                const float r = (float)(P - rint(P));
                const float c = __builtin_amdgcn_cosf(r), sn = __builtin_amdgcn_sinf(r);
                cr[sl] = __fmaf_rn(x, c, cr[sl]);
                ci[sl] = __fmaf_rn(-x, sn, ci[sl]);
                if (DERIV) {
                    dr[sl] = __fmaf_rn(d, c, dr[sl]);
                    di[sl] = __fmaf_rn(-d, sn, di[sl]);
                }
            }
        }
        j += cnt;
    }
}

// the weight of frame tf in up(.)[n]: the bank's upsampling in integers, m = 2 n + 1 - hop = 2 hop i0 + rem
__device__ __forceinline__ double up_weight(int n, int tf, int T, int hop, double inv_2hop)
{
    const int m = 2 * n + 1 - hop;
    int i0 = 0, rem = 0;
    if (m > 0) {
        i0 = m / (2 * hop);
        rem = m - 2 * hop * i0;
    }
    if (i0 >= T - 1) { i0 = T - 1; rem = 0; }
    const int i1 = i0 + 1 < T ? i0 + 1 : T - 1;
    const double fr = (double)rem * inv_2hop;
    return (i0 == tf ? 1.0 - fr : 0.0) + (i1 == tf ? fr : 0.0);
}

// One workgroup per (row, frame).  DERIV: f_re is written too (the frame's f where it is not defined).
template <bool DERIV>
__global__ void __launch_bounds__(kThreads) pt_analysis_kernel(const float *__restrict__ audio, const float *__restrict__ f,
                                                               const uint8_t *__restrict__ voiced, const double *__restrict__ phi,
                                                               const double *__restrict__ g, const double *__restrict__ dh,
                                                               const float *__restrict__ win, const float *__restrict__ dwin,
                                                               float *__restrict__ C, float *__restrict__ a_out, float *__restrict__ c_out,
                                                               float *__restrict__ f_re, int T, int hop, int N, int lead, int W, int K,
                                                               int chunk, int ncoef_cap, float nyquist, long nframes, int t_lo, int t_hi,
                                                               double hz_per_rad)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *wx = smem;                                           // [kWaves chunk] w[j] audio[s + j], 0 outside the clip
    float *wdx = smem + kWaves * chunk;                         // [kWaves chunk] w'[j] audio[s + j]            (DERIV)
    float *part = smem + (DERIV ? 2 : 1) * kWaves * chunk;      // [kWaves][C re, C im(, D re, D im)][kMaxK]
    double *coef = reinterpret_cast<double *>(part + (DERIV ? 4 : 2) * kWaves * kMaxK);    // [ncoef_cap]       (DERIV)
    __shared__ float scale_s;
    __shared__ float wave_amp[kWaves];
    __shared__ int slot_live[kSlots];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int kParts = DERIV ? 4 : 2;

    for (long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
        const long row = fr / T;
        const int t = (int)(fr - row * T);
        const bool sounding = !voiced || voiced[fr] != 0;
        float fk = 0.0f;
        bool keep = false;
        if (tid < K) {
            fk = f[fr * K + tid];
            keep = sounding && usable(fk) && !(fk > nyquist);
        }
        const bool any = __ballot(keep) != 0ull;                // wavefront wv holds the partials of slot wv
        if (lane == 0) slot_live[wv] = any ? 1 : 0;
        __syncthreads();
        int live = 0;
#pragma unroll
        for (int sl = 0; sl < kSlots; ++sl)
            if (slot_live[sl]) live = sl + 1;
        live = __builtin_amdgcn_readfirstlane(live);
        const bool interior = DERIV && live > 0 && t >= t_lo && t <= t_hi;      // (the same for the whole workgroup)

        const int s = t * hop - lead;
        const int j0 = s < 0 ? -s : 0, j1 = N - s < W ? N - s : W;              // the window's samples inside the clip
        for (int j = tid; j < kWaves * chunk; j += kThreads) {
            float x = 0.0f, d = 0.0f;
            if (live && j >= j0 && j < j1) {
                const float av = audio[row * N + s + j];
                x = __fmul_rn(win[j], av);
                if (DERIV) d = __fmul_rn(dwin[j], av);
            }
            wx[j] = x;
            if (DERIV) wdx[j] = d;
        }
        if (tid == 0) scale_s = (float)(2.0 / (window_prefix(j1, W) - window_prefix(j0, W)));

        // the window mean of up(.) as weights on the frames the window reaches: a wavefront per frame, lanes over its samples
        int tfirst = 0, ncoef = 0;
        if (interior) {
            tfirst = s < hop / 2 ? 0 : (s - hop / 2) / hop;
            int last = s + W - 1 < hop / 2 ? 0 : (s + W - 1 - hop / 2) / hop;
            last = last + 1 < T - 1 ? last + 1 : T - 1;
            tfirst = tfirst < T - 1 ? tfirst : T - 1;
            ncoef = last - tfirst + 1;
            ncoef = ncoef < ncoef_cap ? ncoef : ncoef_cap;
            const double inv_2hop = 1.0 / (2.0 * (double)hop);
            for (int i = wv; i < ncoef; i += kWaves) {
                const int tf = tfirst + i;
                int lo = tf == 0 ? 0 : (tf - 1) * hop + hop / 2;
                int hi = tf >= T - 1 ? N : (tf + 1) * hop + hop / 2;
                lo = lo > s ? lo : s;
                hi = hi < s + W ? hi : s + W;
                double acc = 0.0;
                for (int n = lo + lane; n < hi; n += 64) acc = fma((double)win[n - s], up_weight(n, tf, T, hop, inv_2hop), acc);
                acc = wave_sum64(acc);
                if (lane == 0) coef[i] = acc;
            }
        }
        __syncthreads();
        const float scale = scale_s;

        float cr[kSlots], ci[kSlots], dr[kSlots], di[kSlots];
#pragma unroll
        for (int sl = 0; sl < kSlots; ++sl) cr[sl] = ci[sl] = dr[sl] = di[sl] = 0.0f;
        {
            Tracks tr;
            tr.phi = phi + row * T * K;
            tr.g = g + row * T * K;
            tr.dh = dh + row * T * K;
            tr.T = T; tr.K = K; tr.hop = hop; tr.head = hop / 2; tr.e = hop % 2 == 0 ? 1 : 0; tr.N = N;
            const int base = wv * chunk;
            int jlo = j0 > base ? j0 : base, jhi = j1 < base + chunk ? j1 : base + chunk;
            jlo -= base;
            jhi -= base;
            const float *xs = wx + base, *ds = wdx + base;
            switch (live) {                                     // the same for every lane: one branch per frame, none inside
            case 1: pt_window_sums<1, DERIV>(tr, xs, ds, s + base, jlo, jhi, lane, cr, ci, dr, di); break;
            case 2: pt_window_sums<2, DERIV>(tr, xs, ds, s + base, jlo, jhi, lane, cr, ci, dr, di); break;
            case 3: pt_window_sums<3, DERIV>(tr, xs, ds, s + base, jlo, jhi, lane, cr, ci, dr, di); break;
            case 4: pt_window_sums<4, DERIV>(tr, xs, ds, s + base, jlo, jhi, lane, cr, ci, dr, di); break;
            default: break;
            }
        }
#pragma unroll
        for (int sl = 0; sl < kSlots; ++sl) {
            const int h = 64 * sl + lane;
            if (h < K) {
                part[(kParts * wv) * kMaxK + h] = cr[sl];
                part[(kParts * wv + 1) * kMaxK + h] = ci[sl];
                if (DERIV) {
                    part[(kParts * wv + 2) * kMaxK + h] = dr[sl];
                    part[(kParts * wv + 3) * kMaxK + h] = di[sl];
                }
            }
        }
        __syncthreads();

        float out_r = 0.0f, out_i = 0.0f, amp = 0.0f;
        const int h = tid;                                      // kThreads == kMaxK: a thread per partial
        if (h < K) {
            float refined = 0.0f;
            bool measured = false;
            if (keep) {
                float sums[kParts];
#pragma unroll
                for (int q = 0; q < kParts; ++q) {
                    float v = part[q * kMaxK + h];
#pragma unroll
                    for (int w = 1; w < kWaves; ++w) v += part[(kParts * w + q) * kMaxK + h];   // wavefront order
                    sums[q] = v;
                }
                out_r = sums[0] * scale;
                out_i = sums[1] * scale;
                if (DERIV && interior) {
                    const float num = __fmaf_rn(sums[kParts - 1], sums[0], -__fmul_rn(sums[kParts - 2], sums[1]));     // Im(D conj C)
                    const float den = __fmaf_rn(sums[1], sums[1], __fmul_rn(sums[0], sums[0]));
                    double sw = 0.0, sf = 0.0;
                    for (int i = 0; i < ncoef; ++i) {
                        const double cf = coef[i];
                        const float fv = f[((row * T + tfirst + i) * K) + h];
                        sw += cf;
                        sf = fma(cf, usable(fv) ? (double)fv : 0.0, sf);
                    }
                    const float value = (float)(sf / sw - hz_per_rad * ((double)num / (double)den));
                    if (den != 0.0f && fabsf(value) < INFINITY) {
                        refined = value;
                        measured = true;
                    }
                }
            }
            amp = sqrtf(__fmaf_rn(out_i, out_i, out_r * out_r));
            C[2 * (fr * K + h)] = out_r;
            C[2 * (fr * K + h) + 1] = out_i;
            if (DERIV) {
                if (measured) f_re[fr * K + h] = refined;
                else reinterpret_cast<uint32_t *>(f_re)[fr * K + h] = reinterpret_cast<const uint32_t *>(f)[fr * K + h];    // the entry's bits
            }
        }
        const float ws = wave_sum(amp);
        if (lane == 0) wave_amp[wv] = ws;
        __syncthreads();
        float a = wave_amp[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) a += wave_amp[w];
        if (h < K) c_out[fr * K + h] = a == 0.0f ? 1.0f / (float)K : amp / a;
        if (tid == 0) a_out[fr] = a;
        __syncthreads();                                        // the next frame overwrites the LDS
    }
}
static_assert(kThreads == kMaxK, "the analysis kernel finishes one partial per thread");

// One workgroup per (row, segment): segment 0 is the head (the samples before the first frame centre), segment sg = 1 .. T the
// prefix's segment sg - 1, between the centres of the frames sg - 1 and sg (the last one: from the last centre on).
__global__ void __launch_bounds__(kThreads) pt_resynth_kernel(const float2 *__restrict__ C, const double *__restrict__ phi,
                                                              const double *__restrict__ g, const double *__restrict__ dh,
                                                              const float *__restrict__ audio, float *__restrict__ harm,
                                                              float *__restrict__ resid, int T, int hop, int N, int K, long nseg)
{
    __shared__ float4 cs[kMaxK];                                // {re, im of C[t0], re, im of C[t1] - C[t0]}
    __shared__ double phi_s[kMaxK], g_s[kMaxK], dh_s[kMaxK];
    __shared__ int live_s;
    const int tid = threadIdx.x;
    const float denom = 2.0f * (float)hop;
    const int e = hop % 2 == 0 ? 1 : 0;

    for (long u = blockIdx.x; u < nseg; u += gridDim.x) {
        const long row = u / (T + 1);
        const int sg = (int)(u - row * (T + 1));
        const int t0 = sg == 0 ? 0 : sg - 1;
        int t1 = sg == 0 ? 1 : sg;
        t1 = t1 < T ? t1 : T - 1;
        const int begin = sg == 0 ? 0 : (sg - 1) * hop + hop / 2;
        const int end = sg == T ? N : sg * hop + hop / 2;
        const bool inner = sg > 0 && sg < T;
        if (begin >= end) continue;                             // (the same for the whole workgroup)

        if (tid == 0) live_s = 0;
        __syncthreads();
        for (int k = tid; k < K; k += kThreads) {
            const float2 c0 = C[(row * T + t0) * K + k], c1 = C[(row * T + t1) * K + k];
            const float4 v = make_float4(c0.x, c0.y, c1.x - c0.x, c1.y - c0.y);
            cs[k] = v;
            if (!(v.x == 0.0f && v.y == 0.0f && v.z == 0.0f && v.w == 0.0f)) atomicMax(&live_s, k + 1);     // a NaN counts
            const long at = (row * T + t0) * K + k;
            phi_s[k] = sg == 0 ? 0.0 : phi[at];
            g_s[k] = g[at];
            dh_s[k] = sg == 0 ? 0.0 : dh[at];
        }
        __syncthreads();
        const int live = live_s;                                // partials beyond the last non-zero one add nothing

        for (int n = begin + tid; n < end; n += kThreads) {
            const int jj = n - begin;
            const double mult = (double)(jj + 1), xe = (double)(jj + e);
            const float fr = inner ? (float)(2 * (n - t0 * hop) + 1 - hop) / denom : 0.0f;      // pos - t0
            float acc = 0.0f;
            for (int k = 0; k < live; ++k) {                    // k ascending: the order of the sum
                const float4 v = cs[k];
                const double t1v = fma(dh_s[k], xe, g_s[k]);
                const double P = fma(mult, t1v, phi_s[k]);
                const float r = (float)(P - rint(P));
                const float vr = __fmaf_rn(v.z, fr, v.x), vi = __fmaf_rn(v.w, fr, v.y);
                acc = __fmaf_rn(vr, __builtin_amdgcn_cosf(r), acc);
                acc = __fmaf_rn(-vi, __builtin_amdgcn_sinf(r), acc);
            }
            harm[row * N + n] = acc;
            if (resid) resid[row * N + n] = audio[row * N + n] - acc;
        }
        __syncthreads();                                        // the next segment overwrites the LDS
    }
}

bool in_range(long K, long hop, long W) { return K >= 1 && K <= kMaxK && hop >= 1 && hop <= kMaxHop && W >= 2 && W <= kMaxW; }

// cells = B T K; false unless T hop <= 2^24 and B T K and B T hop are at most 2^40 (byte counts and indices then fit a long)
bool sizes(long B, long T, int K, int hop, long *N, long *cells)
{
    long frames, total;
    if (T > kMaxSamples / hop) return false;
    *N = T * hop;
    if (__builtin_mul_overflow(B, T, &frames) || __builtin_mul_overflow(frames, (long)K, cells) || *cells > (1l << 40)) return false;
    if (__builtin_mul_overflow(B, *N, &total) || total > (1l << 40)) return false;
    return true;
}

// the workspace: the window [kMaxW], its derivative [kMaxW], then Phi, g and d / (2 hop) [B, T, K] fp64 each; parts 256-byte aligned
struct Workspace {
    float *win, *dwin;
    double *phi, *g, *dh;
};
inline size_t track_bytes(long cells) { return align256((size_t)cells * sizeof(double)); }
inline Workspace carve(void *workspace, long cells)
{
    char *p = static_cast<char *>(workspace);
    Workspace w;
    w.win = reinterpret_cast<float *>(p);
    w.dwin = reinterpret_cast<float *>(p + kWindowBytes);
    w.phi = reinterpret_cast<double *>(p + 2 * kWindowBytes);
    w.g = reinterpret_cast<double *>(p + 2 * kWindowBytes + track_bytes(cells));
    w.dh = reinterpret_cast<double *>(p + 2 * kWindowBytes + 2 * track_bytes(cells));
    return w;
}

int prefix_pass(const float *f, const Workspace &w, long B, long T, int K, int hop, int sample_rate, hipStream_t stream)
{
    const long rows_k = B * K;
    const long want = (rows_k + kThreads - 1) / kThreads;
    const int blocks = (int)(want < kMaxBlocks ? want : kMaxBlocks);         // (row, partial) pairs beyond the grid are strided
    hipLaunchKernelGGL(pt_prefix_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, f, w.phi, w.g, w.dh, rows_k, (int)T, K, hop,
                       (double)sample_rate);
    return (int)hipGetLastError();
}

template <typename Kn>
hipError_t launch_analysis(Kn kernel, bool (&done)[64], int blocks, size_t lds, hipStream_t s, const float *audio, const float *f,
                           const uint8_t *voiced, const Workspace &w, float *C, float *a, float *c, float *f_re, int T, int hop, int N,
                           int lead, int W, int K, int chunk, int ncoef_cap, float nyquist, long nframes, int t_lo, int t_hi,
                           double hz_per_rad)
{
    if (lds > kSmallLds) {
        const hipError_t e = ddsp_allow_big_lds(reinterpret_cast<const void *>(kernel), done);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), lds, s, audio, f, voiced, w.phi, w.g, w.dh, w.win, w.dwin, C, a, c,
                       f_re, T, hop, N, lead, W, K, chunk, ncoef_cap, nyquist, nframes, t_lo, t_hi, hz_per_rad);
    return hipGetLastError();
}

}  // namespace

extern "C" int ddsp_partials_supported(int K, int hop, int W) { return in_range(K, hop, W) && !(W & 1) ? 1 : 0; }

extern "C" size_t ddsp_partials_workspace_bytes(long B, long T, int K, int hop, int W)
{
    long N, cells;
    if (B <= 0 || T <= 0 || K <= 0 || hop <= 0 || W < 2 || (W & 1) || !in_range(K, hop, W) || !sizes(B, T, K, hop, &N, &cells)) return 0;
    return 2 * kWindowBytes + 3 * track_bytes(cells);
}

extern "C" int ddsp_partials_analysis(const float *audio, const float *f, const uint8_t *voiced, float *C, float *a, float *c,
                                      float *f_re, void *workspace, long B, long T, int K, int hop, int W, int sample_rate, void *stream)
{
    if (B < 0 || T <= 0 || K <= 0 || hop <= 0 || W < 2 || (W & 1) || sample_rate <= 0) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!audio || !f || !C || !a || !c || !workspace || ((uintptr_t)workspace & 15) != 0) return DDSP_EINVAL;
    long N, cells;
    if (!in_range(K, hop, W) || !sizes(B, T, K, hop, &N, &cells)) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    const Workspace w = carve(workspace, cells);
    int rc = prefix_pass(f, w, B, T, K, hop, sample_rate, s);
    if (rc) return rc;
    hipLaunchKernelGGL(pt_window_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, w.win, w.dwin, W);
    if ((rc = (int)hipGetLastError())) return rc;
    const long d = (long)W - hop;
    const long lead = d >= 0 ? d / 2 : -((-d + 1) / 2);         // floor((W - hop) / 2)
    const long t_lo = lead > 0 ? (lead + hop - 1) / hop : 0;    // the frames t_lo .. t_hi have 0 <= s_t and s_t + W <= N
    const long room = N - W + lead;
    const long t_hi = room < 0 ? -1 : (room / hop < T - 1 ? room / hop : T - 1);
    const int chunk = ((W + 15) / 16) * 4;                      // a wavefront's share of the window
    const int ncoef_cap = (W + hop - 1) / hop + 2;              // frames a window's samples interpolate
    const long nframes = B * T;
    const int blocks = (int)(nframes < kMaxBlocks ? nframes : kMaxBlocks);
    const float nyquist = (float)(sample_rate / 2);
    static bool done_plain[64], done_deriv[64];
    hipError_t e;
    if (f_re) {
        const size_t lds = (size_t)(2 * kWaves * chunk + 4 * kWaves * kMaxK) * sizeof(float) + (size_t)ncoef_cap * sizeof(double);
        e = launch_analysis(pt_analysis_kernel<true>, done_deriv, blocks, lds, s, audio, f, voiced, w, C, a, c, f_re, (int)T, hop, (int)N,
                            (int)lead, W, K, chunk, ncoef_cap, nyquist, nframes, (int)t_lo, (int)t_hi, (double)sample_rate / (2.0 * M_PI));
    } else {
        const size_t lds = (size_t)(kWaves * chunk + 2 * kWaves * kMaxK) * sizeof(float);
        e = launch_analysis(pt_analysis_kernel<false>, done_plain, blocks, lds, s, audio, f, voiced, w, C, a, c, f_re, (int)T, hop, (int)N,
                            (int)lead, W, K, chunk, ncoef_cap, nyquist, nframes, (int)t_lo, (int)t_hi, 0.0);
    }
    return (int)e;
}

extern "C" int ddsp_partials_resynth(const float *C, const float *f, const float *audio, float *harm, float *resid, void *workspace,
                                     long B, long T, int K, int hop, int sample_rate, unsigned flags, void *stream)
{
    if (B < 0 || T <= 0 || K <= 0 || hop <= 0 || sample_rate <= 0 || (flags & ~DDSP_PARTIALS_PHASE_READY)) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!C || !f || !harm || !workspace || (resid && !audio) || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)C & 7) != 0)
        return DDSP_EINVAL;
    long N, cells;
    if (!in_range(K, hop, 2) || !sizes(B, T, K, hop, &N, &cells)) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    const Workspace w = carve(workspace, cells);
    if (!(flags & DDSP_PARTIALS_PHASE_READY)) {
        const int rc = prefix_pass(f, w, B, T, K, hop, sample_rate, s);
        if (rc) return rc;
    }
    const long nseg = B * (T + 1);
    const int blocks = (int)(nseg < kMaxBlocks ? nseg : kMaxBlocks);
    hipLaunchKernelGGL(pt_resynth_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, reinterpret_cast<const float2 *>(C), w.phi, w.g,
                       w.dh, audio, harm, resid, (int)T, hop, (int)N, K, nseg);
    return (int)hipGetLastError();
}
