// Harmonic analysis, the inverse of the oscillator bank: from audio and its pitch track the per-frame
// complex amplitudes of the harmonics, the bank's controls a and c, and the harmonic part / residual of the audio.
//   phase pass   theta[n] = sum_{m <= n} up(f0*)[m] / sr in turns, per row: fp64 increments turned into 0.64 fixed point, summed
//                as integers (exact, so any order gives the same bits) and stored per sample as a 32-bit fraction of a turn
//                (rounded to nearest).  k theta mod 1 is then one wrapping 32-bit multiply, shared by both kernels below.
//                Two launches over (row, chunk of 4096 samples): the chunks' totals, then the scan inside every chunk.
//   analysis     one workgroup per (row, frame): w audio and the phase words of the window -> LDS; lane l of every wavefront owns
//                the harmonics l + 1, l + 65, l + 129, l + 193, so every LDS read is a broadcast and no harmonic is reduced across
//                lanes; the four wavefronts take a quarter of the window each.  Slots of 64 harmonics wholly above the frame's
//                Nyquist are skipped (the same for every lane).  v_sin_f32 / v_cos_f32 take turns directly.  The wavefronts'
//                partial sums are added in wavefront order, a in a fixed butterfly: the same bits whatever the batch.
//   resynthesis  one workgroup per (row, segment between two frame centres): all its samples interpolate one frame pair, staged
//                in LDS as C[t] and C[t + 1] - C[t]; a lane owns a sample and walks the harmonics up to the last non-zero one.
//   refinement   (section 14a) a sibling of the analysis over the frames whose window lies inside the clip: w audio, w' audio (w' the
//                window's derivative per sample) and the phase words -> LDS, C_k and D_k by four FMAs behind the same cosine / sine,
//                num = sum_k k Im(D_k conj C_k) and den = sum_k k^2 |C_k|^2 in the analysis' fixed butterfly, and
//                g[t] = (window mean of up(f0*)) - (sr / 2 pi) num / den; a second launch of one thread per frame carries g to
//                the frames at the clip's ends and clamps every frame around the anchor track.
// The matrix cores are not used: the operand exp(-2 pi i k theta[j]) (H x W) is generated per frame and multiplies one vector,
// so nothing is reused; the work is the sine / cosine pair per (harmonic, sample), which is VALU work.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"

namespace {

constexpr int kMaxW = 4096;                     // window samples (even)
constexpr int kMaxH = 256;                      // harmonics: four slots of 64 per lane
constexpr int kSlots = kMaxH / 64;
constexpr int kMaxBlocks = 8192;                // frames / segments / rows beyond this many are walked grid-strided
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPhaseThreads = 1024;
constexpr int kPhasePer = 4;                    // consecutive samples of one thread of the phase pass
constexpr long kPhaseChunk = (long)kPhaseThreads * kPhasePer;       // samples of one workgroup of the phase pass
constexpr size_t kWindowBytes = (size_t)kMaxW * sizeof(float);      // the workspace: the window table, chunk totals, theta [B, N]

__device__ __forceinline__ float live_f0(float f) { return (fabsf(f) < INFINITY && f > 0.0f) ? f : 0.0f; }

// up(f0*)[n] / sr as a 0.64 fixed-point fraction of a turn (whole turns dropped).  pos - i0 = rem / (2 hop) with the integers
// m = 2 n + 1 - hop = 2 hop i0 + rem: i0 and rem are exact, the fraction is rem times the host's rounded reciprocal (exact for a
// power-of-two hop, within 2^-52 otherwise), and there is no fp64 division per sample.
__device__ __forceinline__ unsigned long long phase_increment(const float *__restrict__ f, long T, long hop, long n, double inv_2hop,
                                                              double inv_sr)
{
    const long m = 2 * n + 1 - hop;
    long i0 = 0, rem = 0;
    if (m > 0) {
        i0 = (long)((double)m * inv_2hop);
        rem = m - 2 * hop * i0;
        if (rem < 0) { --i0; rem += 2 * hop; }
        if (rem >= 2 * hop) { ++i0; rem -= 2 * hop; }
    }
    if (i0 >= T - 1) { i0 = T - 1; rem = 0; }
    const long i1 = i0 + 1 < T ? i0 + 1 : T - 1;
    const double fr = (double)rem * inv_2hop;
    const double a = (double)live_f0(f[i0]), b = (double)live_f0(f[i1]);
    double q = (a + (b - a) * fr) * inv_sr;
    q -= floor(q);
    return (unsigned long long)(q * 18446744073709551616.0);    // q < 1: at most 2^64 - 2^11
}

// sum of v over the workgroup, in every thread (integers: any order gives the same bits); `lds` holds a word per wavefront
__device__ __forceinline__ unsigned long long phase_block_sum(unsigned long long v, unsigned long long *lds, int lane, int wv)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) lds[wv] = v;
    __syncthreads();
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kPhaseThreads / 64; ++w) total += lds[w];
    __syncthreads();                                            // lds is rewritten by the caller's next use
    return total;
}

// One workgroup per (row, chunk of kPhaseChunk samples), launched twice: first the chunk's total increment -> totals [B, nchunk],
// then (FINAL) the totals of the row's earlier chunks, the scan inside the chunk and the phase words -> theta [B, N].
template <bool FINAL>
__global__ void __launch_bounds__(kPhaseThreads) harm_phase_kernel(const float *__restrict__ f0, uint32_t *__restrict__ theta,
                                                                   unsigned long long *__restrict__ totals, long T, long hop, long N,
                                                                   long nchunk, long nwork, double inv_2hop, double inv_sr)
{
    __shared__ unsigned long long wave_total[kPhaseThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (long g = blockIdx.x; g < nwork; g += gridDim.x) {
        const long row = g / nchunk, ch = g - row * nchunk;
        const float *f = f0 + row * T;
        const long n0 = ch * kPhaseChunk + (long)tid * kPhasePer;
        unsigned long long pre[kPhasePer], s = 0;
#pragma unroll
        for (int i = 0; i < kPhasePer; ++i) {
            s += n0 + i < N ? phase_increment(f, T, hop, n0 + i, inv_2hop, inv_sr) : 0ull;
            pre[i] = s;
        }
        if (!FINAL) {
            const unsigned long long total = phase_block_sum(s, wave_total, lane, wv);
            if (tid == 0) totals[g] = total;
            continue;
        }
        unsigned long long earlier = 0;
        for (long c = tid; c < ch; c += kPhaseThreads) earlier += totals[row * nchunk + c];
        const unsigned long long carry = phase_block_sum(earlier, wave_total, lane, wv);
        unsigned long long incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long before = __shfl_up(incl, o);
            if (lane >= o) incl += before;
        }
        if (lane == 63) wave_total[wv] = incl;
        __syncthreads();
        unsigned long long before = carry + (incl - s);
#pragma unroll
        for (int w = 0; w < kPhaseThreads / 64; ++w)
            if (w < wv) before += wave_total[w];
        uint32_t *out = theta + row * N;
#pragma unroll
        for (int i = 0; i < kPhasePer; ++i)
            if (n0 + i < N) out[n0 + i] = (uint32_t)((before + pre[i] + 0x80000000ull) >> 32);
        __syncthreads();                                        // wave_total is rewritten by the next chunk
    }
}

// the periodic Hann window, evaluated in fp64 and rounded once
__global__ void harm_window_kernel(float *__restrict__ win, int W)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < W) win[j] = (float)(0.5 - 0.5 * cospi(2.0 * (double)j / (double)W));
}

// sum_{j < m} w[j] = m / 2 - sin(pi m / W) cos(pi (m - 1) / W) / (2 sin(pi / W))
__device__ double window_prefix(long m, int W)
{
    const double w = (double)W;
    return 0.5 * (double)m - 0.5 * sinpi((double)m / w) * cospi((double)(m - 1) / w) / sinpi(1.0 / w);
}

__device__ __forceinline__ float turns_of(uint32_t word) { return (float)(int)word * 0x1p-32f; }    // in [-0.5, 0.5]

// One wavefront's share of a frame: sum_j x[j] exp(-2 pi i k theta[j]) for the lane's harmonics k = 64 sl + lane + 1, sl < LIVE,
// j ascending (the order of every sum).  x and theta are read as broadcasts, four samples at a time.
template <int LIVE>
__device__ __forceinline__ void harm_window_sums(const float *xs_, const uint32_t *ps_, int chunk, int lane, float (&re)[kSlots],
                                                 float (&im)[kSlots])
{
    const float4 *xs = reinterpret_cast<const float4 *>(xs_);
    const uint4 *ps = reinterpret_cast<const uint4 *>(ps_);
    for (int q = 0; q < chunk / 4; ++q) {
        const float4 x4 = xs[q];
        const uint4 p4 = ps[q];
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
        const uint32_t pv[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            uint32_t word = pv[e] * (uint32_t)(lane + 1);       // k theta mod 1; the next slot is 64 theta further
#pragma unroll
            for (int sl = 0; sl < LIVE; ++sl, word += pv[e] << 6) {
                const float ang = turns_of(word);
                re[sl] = __fmaf_rn(xv[e], __builtin_amdgcn_cosf(ang), re[sl]);
                im[sl] = __fmaf_rn(-xv[e], __builtin_amdgcn_sinf(ang), im[sl]);
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads) harm_analysis_kernel(const float *__restrict__ audio, const float *__restrict__ f0,
                                                                 const uint8_t *__restrict__ voiced,
                                                                 const uint32_t *__restrict__ theta, const float *__restrict__ win,
                                                                 float *__restrict__ C, float *__restrict__ a_out,
                                                                 float *__restrict__ c_out, long T, long hop, long N, long lead, int W,
                                                                 int H, int chunk, float nyquist, long nframes)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *wx = smem;                                           // [kWaves chunk] w[j] audio[s + j], 0 outside the clip
    uint32_t *ph = reinterpret_cast<uint32_t *>(smem + kWaves * chunk);         // [kWaves chunk] theta[s + j]
    float *part = smem + 2 * kWaves * chunk;                    // [kWaves][re, im][kMaxH]
    __shared__ float scale_s;
    __shared__ float wave_amp[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slots = (H + 63) / 64;

    for (long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
        const long row = fr / T, t = fr - row * T;
        const float f = f0[fr];
        const bool alive = fabsf(f) < INFINITY && f > 0.0f && (!voiced || voiced[fr] != 0);
        int live = 0;                                           // slots of 64 harmonics whose first one is not above Nyquist
        if (alive)
            for (int sl = 0; sl < slots; ++sl)
                if (!((float)(64 * sl + 1) * f > nyquist)) live = sl + 1;
        live = __builtin_amdgcn_readfirstlane(live);

        const long s = t * hop - lead;
        const long j0 = s < 0 ? -s : 0, j1 = N - s < W ? N - s : W;             // the window's samples inside the clip
        for (int j = tid; j < kWaves * chunk; j += kThreads) {
            float x = 0.0f;
            uint32_t p = 0;
            if (live && j >= j0 && j < j1) {
                const long n = row * N + s + j;
                x = __fmul_rn(win[j], audio[n]);
                p = theta[n];
            }
            wx[j] = x;
            ph[j] = p;
        }
        if (tid == 0) scale_s = (float)(2.0 / (window_prefix(j1, W) - window_prefix(j0, W)));
        __syncthreads();
        const float scale = scale_s;

        float re[kSlots], im[kSlots];
#pragma unroll
        for (int sl = 0; sl < kSlots; ++sl) re[sl] = im[sl] = 0.0f;
        const float *xs = wx + wv * chunk;
        const uint32_t *ps = ph + wv * chunk;
        switch (live) {                                         // the same for every lane: one branch per frame, none inside
        case 1: harm_window_sums<1>(xs, ps, chunk, lane, re, im); break;
        case 2: harm_window_sums<2>(xs, ps, chunk, lane, re, im); break;
        case 3: harm_window_sums<3>(xs, ps, chunk, lane, re, im); break;
        case 4: harm_window_sums<4>(xs, ps, chunk, lane, re, im); break;
        default: break;
        }
#pragma unroll
        for (int sl = 0; sl < kSlots; ++sl) {
            const int h = 64 * sl + lane;
            if (h < H) {
                part[(2 * wv) * kMaxH + h] = re[sl];
                part[(2 * wv + 1) * kMaxH + h] = im[sl];
            }
        }
        __syncthreads();

        float cr = 0.0f, ci = 0.0f, amp = 0.0f;
        const int h = tid;                                      // kThreads == kMaxH: a thread per harmonic
        if (h < H) {
            if (alive && !((float)(h + 1) * f > nyquist)) {
                float sr = part[h], si = part[kMaxH + h];
#pragma unroll
                for (int w = 1; w < kWaves; ++w) {              // wavefront order
                    sr += part[(2 * w) * kMaxH + h];
                    si += part[(2 * w + 1) * kMaxH + h];
                }
                cr = sr * scale;
                ci = si * scale;
            }
            amp = sqrtf(__fmaf_rn(ci, ci, cr * cr));
            C[2 * (fr * H + h)] = cr;
            C[2 * (fr * H + h) + 1] = ci;
        }
        const float ws = wave_sum(amp);
        if (lane == 0) wave_amp[wv] = ws;
        __syncthreads();
        float a = wave_amp[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) a += wave_amp[w];
        if (h < H) c_out[fr * H + h] = a == 0.0f ? 1.0f / (float)H : amp / a;
        if (tid == 0) a_out[fr] = a;
    }
}
static_assert(kThreads == kMaxH, "the analysis kernel finishes one harmonic per thread");

__global__ void __launch_bounds__(kThreads) harm_resynth_kernel(const float2 *__restrict__ C, const uint32_t *__restrict__ theta,
                                                                const float *__restrict__ audio, float *__restrict__ harm,
                                                                float *__restrict__ resid, long T, long hop, long N, int H, long nseg)
{
    __shared__ float4 cs[kMaxH];                                // {re, im of C[t0], re, im of C[t1] - C[t0]}
    __shared__ int live_s;
    const int tid = threadIdx.x;
    const float denom = 2.0f * (float)hop;

    for (long g = blockIdx.x; g < nseg; g += gridDim.x) {
        // segment 0: the samples before the first frame centre (pos clamps to 0); segment sg = 1 .. T - 1: between the centres of
        // frames sg - 1 and sg; segment T: from the last centre on (both frames are T - 1)
        const long row = g / (T + 1), sg = g - row * (T + 1);
        const long t0 = sg == 0 ? 0 : sg - 1;
        long t1 = sg == 0 ? 1 : sg;
        t1 = t1 < T ? t1 : T - 1;
        const long begin = sg == 0 ? 0 : (sg - 1) * hop + hop / 2;
        const long end = sg == T ? N : sg * hop + hop / 2;
        const bool inner = sg > 0 && sg < T;
        if (begin >= end) continue;                             // (the same for the whole workgroup)

        if (tid == 0) live_s = 0;
        __syncthreads();
        for (int h = tid; h < H; h += kThreads) {
            const float2 c0 = C[(row * T + t0) * H + h], c1 = C[(row * T + t1) * H + h];
            const float4 v = make_float4(c0.x, c0.y, c1.x - c0.x, c1.y - c0.y);
            cs[h] = v;
            if (!(v.x == 0.0f && v.y == 0.0f && v.z == 0.0f && v.w == 0.0f)) atomicMax(&live_s, h + 1);     // a NaN counts
        }
        __syncthreads();
        const int live = live_s;                                // harmonics beyond the last non-zero one add nothing

        for (long n = begin + tid; n < end; n += kThreads) {
            const uint32_t p = theta[row * N + n];
            const float fr = inner ? (float)(2 * (n - t0 * hop) + 1 - hop) / denom : 0.0f;     // pos - t0
            float acc = 0.0f;
            uint32_t word = 0;
            for (int h = 0; h < live; ++h) {                    // k ascending: the order of the sum
                const float4 v = cs[h];
                word += p;                                      // (h + 1) theta mod 1
                const float ang = turns_of(word);
                const float cr = __fmaf_rn(v.z, fr, v.x), ci = __fmaf_rn(v.w, fr, v.y);
                acc = __fmaf_rn(cr, __builtin_amdgcn_cosf(ang), acc);
                acc = __fmaf_rn(-ci, __builtin_amdgcn_sinf(ang), acc);
            }
            harm[row * N + n] = acc;
            if (resid) resid[row * N + n] = audio[row * N + n] - acc;
        }
        __syncthreads();                                        // the next segment overwrites cs and live_s
    }
}

// ---------------------------------------------------------------------------------------------------- refinement (section 14a)

// the periodic Hann window and its derivative per sample, (pi / W) sin(2 pi j / W), evaluated in fp64 and rounded once
__global__ void harm_window_pair_kernel(float *__restrict__ win, float *__restrict__ dwin, int W)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < W) {
        win[j] = (float)(0.5 - 0.5 * cospi(2.0 * (double)j / (double)W));
        dwin[j] = (float)(M_PI / (double)W * sinpi(2.0 * (double)j / (double)W));
    }
}

// up(f0*)[n] in fp64: the interpolation of phase_increment, before the division by the sample rate
__device__ __forceinline__ double up_f0(const float *__restrict__ f, long T, long hop, long n, double inv_2hop)
{
    const long m = 2 * n + 1 - hop;
    long i0 = 0, rem = 0;
    if (m > 0) {
        i0 = (long)((double)m * inv_2hop);
        rem = m - 2 * hop * i0;
        if (rem < 0) { --i0; rem += 2 * hop; }
        if (rem >= 2 * hop) { ++i0; rem -= 2 * hop; }
    }
    if (i0 >= T - 1) { i0 = T - 1; rem = 0; }
    const long i1 = i0 + 1 < T ? i0 + 1 : T - 1;
    const double a = (double)live_f0(f[i0]), b = (double)live_f0(f[i1]);
    return a + (b - a) * ((double)rem * inv_2hop);
}

// harm_window_sums with the second window beside the first: C = sum_j (w x)[j] e, D = sum_j (w' x)[j] e, e = exp(-2 pi i k theta[j])
template <int LIVE>
__device__ __forceinline__ void harm_refine_sums(const float *xs_, const float *ds_, const uint32_t *ps_, int chunk, int lane,
                                                 float (&cr)[kSlots], float (&ci)[kSlots], float (&dr)[kSlots], float (&di)[kSlots])
{
    const float4 *xs = reinterpret_cast<const float4 *>(xs_);
    const float4 *ds = reinterpret_cast<const float4 *>(ds_);
    const uint4 *ps = reinterpret_cast<const uint4 *>(ps_);
    for (int q = 0; q < chunk / 4; ++q) {
        const float4 x4 = xs[q], d4 = ds[q];
        const uint4 p4 = ps[q];
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
        const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
        const uint32_t pv[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            uint32_t word = pv[e] * (uint32_t)(lane + 1);
#pragma unroll
            for (int sl = 0; sl < LIVE; ++sl, word += pv[e] << 6) {
                const float ang = turns_of(word);
                const float c = __builtin_amdgcn_cosf(ang), s = __builtin_amdgcn_sinf(ang);
                cr[sl] = __fmaf_rn(xv[e], c, cr[sl]);
                ci[sl] = __fmaf_rn(-xv[e], s, ci[sl]);
                dr[sl] = __fmaf_rn(dv[e], c, dr[sl]);
                di[sl] = __fmaf_rn(-dv[e], s, di[sl]);
            }
        }
    }
}

// sum of v over the 256 threads in every thread: the butterfly inside a wavefront, then the wavefronts in order
__device__ __forceinline__ float refine_block_sum(float v, float *wave_part, int lane, int wv)
{
    const float ws = wave_sum(v);
    if (lane == 0) wave_part[wv] = ws;
    __syncthreads();
    float total = wave_part[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) total += wave_part[w];
    __syncthreads();                                            // wave_part is rewritten by the next sum
    return total;
}

// One workgroup per (row, frame).  raw [B, T] receives g[t] for a frame that is alive and whose window [t_lo, t_hi] lies inside the
// clip, and the bits of f0[t] for every other one (and where den = 0 or g is not finite); num and den (nullable) the two sums, 0
// where none were formed.
__global__ void __launch_bounds__(kThreads) harm_refine_kernel(const float *__restrict__ audio, const float *__restrict__ f0,
                                                               const uint8_t *__restrict__ voiced,
                                                               const uint32_t *__restrict__ theta, const float *__restrict__ win,
                                                               const float *__restrict__ dwin, float *__restrict__ raw,
                                                               float *__restrict__ num_out, float *__restrict__ den_out, long T,
                                                               long hop, long N, long lead, int W, int H, int chunk, float nyquist,
                                                               long nframes, long t_lo, long t_hi, double inv_2hop, double hz_per_rad)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *wx = smem;                                           // [kWaves chunk] w[j] audio[s + j]
    float *wdx = smem + kWaves * chunk;                         // [kWaves chunk] w'[j] audio[s + j]
    uint32_t *ph = reinterpret_cast<uint32_t *>(smem + 2 * kWaves * chunk);     // [kWaves chunk] theta[s + j]
    float *part = smem;                                         // [kWaves][C re, C im, D re, D im][kMaxH], over the staged window
    __shared__ float wave_part[kWaves];
    __shared__ double wave_mean[2 * kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slots = (H + 63) / 64;

    for (long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
        const long row = fr / T, t = fr - row * T;
        const float f = f0[fr];
        const bool alive = fabsf(f) < INFINITY && f > 0.0f && (!voiced || voiced[fr] != 0);
        int live = 0;
        if (alive && t >= t_lo && t <= t_hi)
            for (int sl = 0; sl < slots; ++sl)
                if (!((float)(64 * sl + 1) * f > nyquist)) live = sl + 1;
        live = __builtin_amdgcn_readfirstlane(live);
        if (live == 0) {                                        // (the same for the whole workgroup)
            if (tid == 0) {
                reinterpret_cast<uint32_t *>(raw)[fr] = reinterpret_cast<const uint32_t *>(f0)[fr];
                if (num_out) num_out[fr] = 0.0f;
                if (den_out) den_out[fr] = 0.0f;
            }
            continue;
        }

        const long s = t * hop - lead;                          // 0 <= s and s + W <= N
        double mw = 0.0, mf = 0.0;                              // sum_j w[j], sum_j w[j] up(f0*)[s + j], j ascending per thread
        for (int j = tid; j < kWaves * chunk; j += kThreads) {
            float x = 0.0f, d = 0.0f;
            uint32_t p = 0;
            if (j < W) {
                const long n = row * N + s + j;
                const float wj = win[j], a = audio[n];
                x = __fmul_rn(wj, a);
                d = __fmul_rn(dwin[j], a);
                p = theta[n];
                mw += (double)wj;
                mf = fma((double)wj, up_f0(f0 + row * T, T, hop, s + j, inv_2hop), mf);
            }
            wx[j] = x;
            wdx[j] = d;
            ph[j] = p;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mw += __shfl_xor(mw, o);
            mf += __shfl_xor(mf, o);
        }
        if (lane == 0) {
            wave_mean[2 * wv] = mw;
            wave_mean[2 * wv + 1] = mf;
        }
        __syncthreads();
        double mean = 0.0;                                      // read here: the next frame's sums may be written before this one ends
        if (tid == 0) {
            double sw = wave_mean[0], sf = wave_mean[1];
            for (int w = 1; w < kWaves; ++w) {                  // wavefront order
                sw += wave_mean[2 * w];
                sf += wave_mean[2 * w + 1];
            }
            mean = sf / sw;
        }

        float cr[kSlots], ci[kSlots], dr[kSlots], di[kSlots];
#pragma unroll
        for (int sl = 0; sl < kSlots; ++sl) cr[sl] = ci[sl] = dr[sl] = di[sl] = 0.0f;
        const float *xs = wx + wv * chunk, *ds = wdx + wv * chunk;
        const uint32_t *ps = ph + wv * chunk;
        switch (live) {
        case 1: harm_refine_sums<1>(xs, ds, ps, chunk, lane, cr, ci, dr, di); break;
        case 2: harm_refine_sums<2>(xs, ds, ps, chunk, lane, cr, ci, dr, di); break;
        case 3: harm_refine_sums<3>(xs, ds, ps, chunk, lane, cr, ci, dr, di); break;
        case 4: harm_refine_sums<4>(xs, ds, ps, chunk, lane, cr, ci, dr, di); break;
        default: break;
        }
        __syncthreads();                                        // every wavefront has read its share: part overwrites the window
#pragma unroll
        for (int sl = 0; sl < kSlots; ++sl) {
            const int h = 64 * sl + lane;
            if (h < H) {
                part[(4 * wv) * kMaxH + h] = cr[sl];
                part[(4 * wv + 1) * kMaxH + h] = ci[sl];
                part[(4 * wv + 2) * kMaxH + h] = dr[sl];
                part[(4 * wv + 3) * kMaxH + h] = di[sl];
            }
        }
        __syncthreads();

        float tn = 0.0f, td = 0.0f;
        const int h = tid;                                      // a thread per harmonic
        if (h < H && !((float)(h + 1) * f > nyquist)) {
            float c_re = part[h], c_im = part[kMaxH + h], d_re = part[2 * kMaxH + h], d_im = part[3 * kMaxH + h];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) {                  // wavefront order
                c_re += part[(4 * w) * kMaxH + h];
                c_im += part[(4 * w + 1) * kMaxH + h];
                d_re += part[(4 * w + 2) * kMaxH + h];
                d_im += part[(4 * w + 3) * kMaxH + h];
            }
            const float k = (float)(h + 1);
            tn = __fmul_rn(k, __fmaf_rn(d_im, c_re, -__fmul_rn(d_re, c_im)));                  // k Im(D conj C)
            td = __fmul_rn(__fmul_rn(k, k), __fmaf_rn(c_im, c_im, __fmul_rn(c_re, c_re)));     // k^2 |C|^2
        }
        const float num = refine_block_sum(tn, wave_part, lane, wv);
        const float den = refine_block_sum(td, wave_part, lane, wv);    // (its last barrier also frees part for the next frame)
        if (tid == 0) {
            const float g = (float)(mean - hz_per_rad * ((double)num / (double)den));
            raw[fr] = (den != 0.0f && fabsf(g) < INFINITY) ? g : f;
            if (num_out) num_out[fr] = num;
            if (den_out) den_out[fr] = den;
        }
    }
}

// One thread per frame: an alive frame before t_lo (after t_hi) moves by the ratio raw / f0 of frame t_lo (t_hi), where that one is
// alive; every alive frame is clamped to anchor 2^(+-max_cents / 1200); a frame that is not alive keeps its bits.  t_lo > t_hi:
// no window lies inside the clip.  f0_out must not overlap f0 or raw.
__global__ void harm_refine_finish_kernel(const float *__restrict__ f0, const float *__restrict__ anchor,
                                          const uint8_t *__restrict__ voiced, const float *__restrict__ raw, float *__restrict__ f0_out,
                                          long T, long nframes, long t_lo, long t_hi, double down, double up)
{
    for (long fr = (long)blockIdx.x * blockDim.x + threadIdx.x; fr < nframes; fr += (long)gridDim.x * blockDim.x) {
        const long row = fr / T, t = fr - row * T;
        const float f = f0[fr];
        if (!(fabsf(f) < INFINITY && f > 0.0f && (!voiced || voiced[fr] != 0))) {
            reinterpret_cast<uint32_t *>(f0_out)[fr] = reinterpret_cast<const uint32_t *>(f0)[fr];
            continue;
        }
        double g = (double)raw[fr];
        if (t_lo <= t_hi && (t < t_lo || t > t_hi)) {
            const long e = row * T + (t < t_lo ? t_lo : t_hi);
            const float fe = f0[e];
            if (fabsf(fe) < INFINITY && fe > 0.0f && (!voiced || voiced[e] != 0)) g = (double)f * ((double)raw[e] / (double)fe);
        }
        const double a = (double)anchor[fr];
        f0_out[fr] = (float)fmin(fmax(g, a * down), a * up);
    }
}

// N = T hop; false unless B N and B (T + 1) H are at most 2^56 elements (byte counts and indices then fit a long)
bool harm_sizes(long B, long T, int hop, int H, long *N, long *total)
{
    long frames, cells;
    if (__builtin_mul_overflow(T, (long)hop, N) || __builtin_mul_overflow(B, *N, total) || *total > (1l << 56)) return false;
    if (__builtin_mul_overflow(B, T + 1, &frames) || __builtin_mul_overflow(frames, (long)H, &cells) || cells > (1l << 56)) return false;
    return true;
}

// the workspace: the window table [kMaxW], the phase pass's chunk totals [B, nchunk], theta [B, N]; parts 256-byte aligned
inline long harm_chunks(long N) { return (N + kPhaseChunk - 1) / kPhaseChunk; }
inline size_t harm_theta_offset(long B, long N) { return kWindowBytes + align256((size_t)(B * harm_chunks(N)) * sizeof(unsigned long long)); }
inline uint32_t *harm_theta(void *workspace, long B, long N)
{
    return reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + harm_theta_offset(B, N));
}

int harm_phase_pass(const float *f0, void *workspace, long B, long T, int hop, long N, int sample_rate, hipStream_t stream)
{
    unsigned long long *totals = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + kWindowBytes);
    uint32_t *theta = harm_theta(workspace, B, N);
    const long nchunk = harm_chunks(N), nwork = B * nchunk;
    const int blocks = (int)(nwork < kMaxBlocks ? nwork : kMaxBlocks);
    const double inv_2hop = 1.0 / (2.0 * (double)hop), inv_sr = 1.0 / (double)sample_rate;
    hipLaunchKernelGGL(harm_phase_kernel<false>, dim3((unsigned)blocks), dim3(kPhaseThreads), 0, stream, f0, theta, totals, T, (long)hop,
                       N, nchunk, nwork, inv_2hop, inv_sr);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(harm_phase_kernel<true>, dim3((unsigned)blocks), dim3(kPhaseThreads), 0, stream, f0, theta, totals, T, (long)hop,
                       N, nchunk, nwork, inv_2hop, inv_sr);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" size_t ddsp_harm_workspace_bytes(long B, long T, int hop)
{
    long N, total;
    if (B <= 0 || T <= 0 || hop <= 0 || !harm_sizes(B, T, hop, 1, &N, &total)) return 0;
    return harm_theta_offset(B, N) + align256((size_t)total * sizeof(uint32_t));
}

extern "C" int ddsp_harm_analysis(const float *audio, const float *f0, const uint8_t *voiced, float *C, float *a, float *c,
                                  void *workspace, long B, long T, int hop, int W, int H, int sample_rate, void *stream)
{
    if (B == 0) return 0;
    if (!audio || !f0 || !C || !a || !c || !workspace || B < 0 || T <= 0 || hop <= 0 || W < 2 || (W & 1) || H <= 0 || sample_rate <= 0)
        return DDSP_EINVAL;
    if (((uintptr_t)workspace & 15) != 0) return DDSP_EINVAL;
    long N, total;
    if (W > kMaxW || H > kMaxH || !harm_sizes(B, T, hop, H, &N, &total)) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    int rc = harm_phase_pass(f0, workspace, B, T, hop, N, sample_rate, s);
    if (rc) return rc;
    float *win = static_cast<float *>(workspace);
    const uint32_t *theta = harm_theta(workspace, B, N);
    hipLaunchKernelGGL(harm_window_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, win, W);
    if ((rc = (int)hipGetLastError())) return rc;
    const long d = (long)W - hop;
    const long lead = d >= 0 ? d / 2 : -((-d + 1) / 2);         // floor((W - hop) / 2)
    const int chunk = ((W + 15) / 16) * 4;                      // a wavefront's share of the window, in whole float4
    const size_t lds = (size_t)(2 * kWaves * chunk + 2 * kWaves * kMaxH) * sizeof(float);
    const long nframes = B * T;
    const int blocks = (int)(nframes < kMaxBlocks ? nframes : kMaxBlocks);
    hipLaunchKernelGGL(harm_analysis_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, s, audio, f0, voiced, theta, win, C, a, c, T,
                       (long)hop, N, lead, W, H, chunk, (float)(sample_rate / 2), nframes);
    return (int)hipGetLastError();
}

extern "C" int ddsp_harm_resynth(const float *C, const float *f0, const float *audio, float *harm, float *resid, void *workspace,
                                 long B, long T, int hop, int H, int sample_rate, unsigned flags, void *stream)
{
    if (B == 0) return 0;
    if (!C || !f0 || !harm || !workspace || (resid && !audio) || B < 0 || T <= 0 || hop <= 0 || H <= 0 || sample_rate <= 0 ||
        (flags & ~DDSP_HARM_PHASE_READY))
        return DDSP_EINVAL;
    if (((uintptr_t)workspace & 15) != 0 || ((uintptr_t)C & 7) != 0) return DDSP_EINVAL;
    long N, total;
    if (H > kMaxH || !harm_sizes(B, T, hop, H, &N, &total)) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & DDSP_HARM_PHASE_READY)) {
        const int rc = harm_phase_pass(f0, workspace, B, T, hop, N, sample_rate, s);
        if (rc) return rc;
    }
    const uint32_t *theta = harm_theta(workspace, B, N);
    const long nseg = B * (T + 1);
    const int blocks = (int)(nseg < kMaxBlocks ? nseg : kMaxBlocks);
    hipLaunchKernelGGL(harm_resynth_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, reinterpret_cast<const float2 *>(C), theta,
                       audio, harm, resid, T, (long)hop, N, H, nseg);
    return (int)hipGetLastError();
}

// the refinement's workspace: that of the analysis, then the derivative window [kMaxW], then raw [B, T]
extern "C" size_t ddsp_harm_refine_workspace_bytes(long B, long T, int hop)
{
    const size_t base = ddsp_harm_workspace_bytes(B, T, hop);
    return base ? base + kWindowBytes + align256((size_t)(B * T) * sizeof(float)) : 0;
}

extern "C" int ddsp_harm_refine(const float *audio, const float *f0_in, const float *f0_anchor, const uint8_t *voiced, float *f0_out,
                                float *num_out, float *den_out, void *workspace, long B, long T, int hop, int W, int H,
                                int sample_rate, float max_cents, unsigned flags, void *stream)
{
    if (B == 0) return 0;
    if (!audio || !f0_in || !f0_anchor || !f0_out || !workspace || B < 0 || T <= 0 || hop <= 0 || W < 2 || (W & 1) || H <= 0 ||
        sample_rate <= 0 || !(max_cents > 0.0f) || !(max_cents < INFINITY) || flags || f0_out == f0_in)
        return DDSP_EINVAL;
    if (((uintptr_t)workspace & 15) != 0) return DDSP_EINVAL;
    long N, total;
    if (W > kMaxW || H > kMaxH || !harm_sizes(B, T, hop, H, &N, &total)) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    int rc = harm_phase_pass(f0_in, workspace, B, T, hop, N, sample_rate, s);
    if (rc) return rc;
    char *after = static_cast<char *>(workspace) + ddsp_harm_workspace_bytes(B, T, hop);
    float *win = static_cast<float *>(workspace), *dwin = reinterpret_cast<float *>(after);
    float *raw = reinterpret_cast<float *>(after + kWindowBytes);
    const uint32_t *theta = harm_theta(workspace, B, N);
    hipLaunchKernelGGL(harm_window_pair_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, win, dwin, W);
    if ((rc = (int)hipGetLastError())) return rc;
    const long d = (long)W - hop;
    const long lead = d >= 0 ? d / 2 : -((-d + 1) / 2);         // floor((W - hop) / 2)
    const long t_lo = lead > 0 ? (lead + hop - 1) / hop : 0;    // the frames t_lo .. t_hi have 0 <= s_t and s_t + W <= N
    const long room = N - W + lead;
    const long t_hi = room < 0 ? -1 : (room / hop < T - 1 ? room / hop : T - 1);
    const int chunk = ((W + 15) / 16) * 4;
    const size_t staged = (size_t)3 * kWaves * chunk, sums = (size_t)4 * kWaves * kMaxH;        // the sums reuse the window's LDS
    const size_t lds = (staged > sums ? staged : sums) * sizeof(float);
    const long nframes = B * T;
    const int blocks = (int)(nframes < kMaxBlocks ? nframes : kMaxBlocks);
    hipLaunchKernelGGL(harm_refine_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, s, audio, f0_in, voiced, theta, win, dwin, raw,
                       num_out, den_out, T, (long)hop, N, lead, W, H, chunk, (float)(sample_rate / 2), nframes, t_lo, t_hi,
                       1.0 / (2.0 * (double)hop), (double)sample_rate / (2.0 * M_PI));
    if ((rc = (int)hipGetLastError())) return rc;
    const long per = (nframes + 255) / 256;
    hipLaunchKernelGGL(harm_refine_finish_kernel, dim3((unsigned)(per < kMaxBlocks ? per : kMaxBlocks)), dim3(256), 0, s, f0_in,
                       f0_anchor, voiced, raw, f0_out, T, nframes, t_lo, t_hi, exp2(-(double)max_cents / 1200.0),
                       exp2((double)max_cents / 1200.0));
    return (int)hipGetLastError();
}
