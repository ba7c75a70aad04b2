// Griffin-Lim phase reconstruction (torchaudio 0.8.1 functional.griffinlim, as style_transfer.py:149-156 and helper.py:105-112
// call it) with every iteration on the device and no host synchronisation.  One iteration of the stock formulation is
// istft (irfft, window, overlap-add, envelope division, trim) + stft (reflect pad, frame, window, rfft) + five element-wise
// ops: about 20 launches and a `.item()` per call of torch.istft.  Here it is three launches:
//   synthesis  one wavefront per frame (pair of frames below 2048 points): the angles from R, R_prev (or the initial ones),
//              times S, complex-to-real inverse transform, times the window / n_fft -> frames [B*T, n_fft]
//   overlap    one thread per output sample: the sum over the frames that cover it in ascending frame order, divided by the
//              window envelope (computed once by the caller), zero past the natural length -> y [B, L]
//   analysis   one wavefront per frame (pair): y reflect-padded, windowed, forward real transform -> R [B*T, F]
// The overlap-add is a launch of its own rather than a gather inside the analysis: a gathered sample would be re-summed by
// each of the n_fft / hop frames that read it, an overlap-add launch sums it once (4 bytes written, n_fft / hop reads of the
// frames once each).  The final istft is synthesis + overlap into the caller's y, which doubles as the iteration's signal.
// State is frame-major ([B, T, F]: one wavefront's bins are contiguous); the caller's [B, F, T] magnitude and angles are
// transposed once on entry.  No atomics: each value is produced by one lane in a fixed order, results are deterministic.
//
// Transforms: ddsp_wave_fft.h.  n_fft = 64 .. 1024: two frames a, b packed as one complex sequence (a + i b); the inverse takes
// Z[k] = A[k] + i B[k] over the Hermitian-extended spectra (imaginary parts of bins 0 and n_fft/2 dropped, as a c2r transform
// does), the forward splits A = (Z[k] + conj Z[n-k]) / 2, B = -i (Z[k] - conj Z[n-k]) / 2.  n_fft = 2048: one real frame per
// wavefront through a 1024-point complex transform (ddsp_wave_fft.h's split2048 / pack2048).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_wave_fft.h"

namespace {

using ddsp_wfft::cf;
using ddsp_wfft::PairFft;
using ddsp_wfft::PairUnit;

constexpr int kMaxBlocks = 16384;   // grid-stride cap of the transform kernels (twiddle set-up is per block)

struct GlParams {
    const float *S;        // [BT, F] magnitude ** (1 / power), frame-major
    const cf *ang0;        // [BT, F] initial angles, or null: all 1 (rand_init=False)
    const cf *R;           // [BT, F] the last rebuilt spectrum, or null: iteration 0 (use ang0)
    const cf *Rprev;       // [BT, F] the one before, or null: no momentum term
    cf *Rout;              // [BT, F] analysis output
    float *frames;         // [BT, n_fft]
    const float *y;        // [B, L] the iteration's signal (analysis input)
    const float *window;   // [n_fft] (zero-padded and centred like torch.stft's)
    long nframes;          // BT = B * T
    long T, L;
    int hop, F;
    float c;               // fl32(momentum / (1 + momentum))
};

// S * angles at element idx (torchaudio 0.8.1: angles = R - c R_prev; angles / (sqrt(re^2 + im^2) + 1e-16))
__device__ __forceinline__ cf spec_at(const GlParams &p, long idx)
{
    const float s = p.S[idx];
    cf a;
    if (!p.R) {
        a = p.ang0 ? p.ang0[idx] : make_float2(1.0f, 0.0f);
    } else {
        a = p.R[idx];
        if (p.Rprev) {
            const cf q = p.Rprev[idx];
            a = make_float2(a.x - p.c * q.x, a.y - p.c * q.y);
        }
        const float n = sqrtf(a.x * a.x + a.y * a.y) + 1e-16f;
        a = make_float2(a.x / n, a.y / n);
    }
    return make_float2(s * a.x, s * a.y);
}

// ---- n_fft = 64 .. 1024: frame pairs -----------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(64) gl_synth_pair_kernel(GlParams p, long nunits)
{
    using U = PairUnit<N>;
    constexpr int R1 = U::R1, PL = U::PL, BT = U::BT, STRIDE = U::STRIDE, BINS = U::BINS;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *bufZ = reinterpret_cast<cf *>(smem_f);
    cf *bufW = bufZ + U::BUF;
    const int lane = threadIdx.x;
    PairFft<N> fft;
    fft.init(lane);
    float wreg[R1];                                             // window / N (irfft's 1/N, exact: N is a power of two)
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) wreg[n1] = p.window[64 * n1 + lane] * (1.0f / (float)N);

    for (long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const long f0 = unit * 2 * BT;
        for (int t = lane; t < BT * BINS; t += 64) {
            const int b = t / BINS, k = t - b * BINS;
            const long fa = f0 + 2 * b, fb = fa + 1;
            const cf xa = fa < p.nframes ? spec_at(p, fa * p.F + k) : make_float2(0.0f, 0.0f);
            const cf xb = fb < p.nframes ? spec_at(p, fb * p.F + k) : make_float2(0.0f, 0.0f);
            cf *zrow = bufZ + b * STRIDE;
            if (k == 0 || k == N / 2) {
                zrow[k] = make_float2(xa.x, xb.x);
            } else {
                zrow[k] = make_float2(xa.x - xb.y, xa.y + xb.x);            // A + i B
                zrow[N - k] = make_float2(xa.x + xb.y, xb.x - xa.y);        // conj A + i conj B
            }
        }
        DDSP_WAVE_ORDER();
        cf v[PL];
#pragma unroll
        for (int b = 0; b < BT; ++b)
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) v[b * R1 + n1] = bufZ[b * STRIDE + 64 * n1 + lane];
        DDSP_WAVE_ORDER();
        fft.template run<true>(v, bufW);
#pragma unroll
        for (int i = 0; i < PL; ++i) bufW[fft.natural(i)] = v[i];
        DDSP_WAVE_ORDER();
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            const long fa = f0 + 2 * b;
            if (fa < p.nframes) {                                           // wave-uniform
                float *dst = p.frames + fa * N;
                const bool two = fa + 1 < p.nframes;
#pragma unroll
                for (int n1 = 0; n1 < R1; ++n1) {
                    const int j = 64 * n1 + lane;
                    const cf z = bufW[b * STRIDE + j];
                    dst[j] = z.x * wreg[n1];
                    if (two) dst[N + j] = z.y * wreg[n1];
                }
            }
        }
        DDSP_WAVE_ORDER();
    }
}

template <int N>
__global__ void __launch_bounds__(64) gl_analysis_pair_kernel(GlParams p, long nunits)
{
    using U = PairUnit<N>;
    constexpr int R1 = U::R1, PL = U::PL, BT = U::BT, STRIDE = U::STRIDE, BINS = U::BINS;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *bufZ = reinterpret_cast<cf *>(smem_f);
    const int lane = threadIdx.x;
    PairFft<N> fft;
    fft.init(lane);
    float wreg[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) wreg[n1] = p.window[64 * n1 + lane];

    for (long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const long f0 = unit * 2 * BT;
        cf v[PL];
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            float xs[2][R1];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const long f = f0 + 2 * b + h;
                if (f < p.nframes) {                                        // wave-uniform
                    const long row = f / p.T, t = f - row * p.T;
                    const float *y = p.y + row * p.L;
                    const long start = t * p.hop - N / 2;
#pragma unroll
                    for (int n1 = 0; n1 < R1; ++n1) xs[h][n1] = y[reflect_index(start + 64 * n1 + lane, p.L)];
                } else {
#pragma unroll
                    for (int n1 = 0; n1 < R1; ++n1) xs[h][n1] = 0.0f;
                }
            }
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) v[b * R1 + n1] = make_float2(xs[0][n1] * wreg[n1], xs[1][n1] * wreg[n1]);
        }
        fft.template run<false>(v, bufZ);
#pragma unroll
        for (int i = 0; i < PL; ++i) bufZ[fft.natural(i)] = v[i];
        DDSP_WAVE_ORDER();
        for (int t = lane; t < BT * BINS; t += 64) {
            const int b = t / BINS, k = t - b * BINS;
            const int km = (N - k) & (N - 1);
            const cf zk = bufZ[b * STRIDE + k], zm = bufZ[b * STRIDE + km];
            const long fa = f0 + 2 * b, fb = fa + 1;
            if (fa < p.nframes) p.Rout[fa * p.F + k] = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
            if (fb < p.nframes) p.Rout[fb * p.F + k] = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
        }
        DDSP_WAVE_ORDER();
    }
}

// ---- n_fft = 2048: one real frame per wavefront through a 1024-point complex transform (ddsp_wave_fft.h) -------------------
// Forward: z[m] = x[2m] w[2m] + i x[2m+1] w[2m+1], Z = FFT_1024(z), split2048.  Inverse: pack2048, IFFT_1024.
constexpr int kM = 1024;

__global__ void __launch_bounds__(64) gl_synth2048_kernel(GlParams p)
{
    constexpr int N = 2048, R1 = 16;
    constexpr int NB = ddsp_wfft::buf_elems<R1>();
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *bufZ = reinterpret_cast<cf *>(smem_f);
    cf *bufW = bufZ + NB;
    const int lane = threadIdx.x;
    ddsp_wfft::Twiddles<R1> tw;
    ddsp_wfft::make_twiddles<R1>(tw, lane);
    const cf wbase = ddsp_wfft::lane_w2048(lane);
    float2 wreg[R1];                                                        // window / N at the lane's sample pairs
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) {
        const float2 w = reinterpret_cast<const float2 *>(p.window)[64 * n1 + lane];
        wreg[n1] = make_float2(w.x * (1.0f / (float)N), w.y * (1.0f / (float)N));
    }

    for (long f = blockIdx.x; f < p.nframes; f += gridDim.x) {
        const long base = f * p.F;
#pragma unroll 1
        for (int it = 0; it < 9; ++it) {
            const int k = lane + 64 * it;
            if (k <= kM / 2) {
                cf X1 = spec_at(p, base + k), X2 = spec_at(p, base + kM - k);      // bins k and M - k (k = 0: bin 1024)
                if (k == 0) { X1.y = 0.0f; X2.y = 0.0f; }                          // c2r: the DC and Nyquist bins are real
                cf Y1, Y2;
                ddsp_wfft::pack2048(X1, X2, ddsp_wfft::twiddle2048(wbase, it), Y1, Y2);
                bufZ[k] = Y1;
                if (k != 0 && k != kM / 2) bufZ[kM - k] = Y2;
            }
        }
        DDSP_WAVE_ORDER();
        cf v[R1];
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) v[n1] = bufZ[64 * n1 + lane];
        DDSP_WAVE_ORDER();
        ddsp_wfft::fft_wave<R1, true, false>(v, tw, bufW, lane);
        ddsp_wfft::store_natural<R1>(v, bufW, lane);
        DDSP_WAVE_ORDER();
        float2 *dst = reinterpret_cast<float2 *>(p.frames + f * N);
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) {
            const cf z = bufW[64 * n1 + lane];
            dst[64 * n1 + lane] = make_float2(z.x * wreg[n1].x, z.y * wreg[n1].y);
        }
        DDSP_WAVE_ORDER();
    }
}

__global__ void __launch_bounds__(64) gl_analysis2048_kernel(GlParams p)
{
    constexpr int N = 2048, R1 = 16;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *bufZ = reinterpret_cast<cf *>(smem_f);
    const int lane = threadIdx.x;
    ddsp_wfft::Twiddles<R1> tw;
    ddsp_wfft::make_twiddles<R1>(tw, lane);
    const cf wbase = ddsp_wfft::lane_w2048(lane);
    float2 wreg[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) wreg[n1] = reinterpret_cast<const float2 *>(p.window)[64 * n1 + lane];

    for (long f = blockIdx.x; f < p.nframes; f += gridDim.x) {
        const long row = f / p.T, t = f - row * p.T;
        const float *y = p.y + row * p.L;
        const long start = t * p.hop - N / 2;
        cf v[R1];
        if (start >= 0 && start + N <= p.L) {                              // wave-uniform: the frame lies inside the row
            const float *r = y + start + 2 * lane;
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) v[n1] = make_float2(r[128 * n1] * wreg[n1].x, r[128 * n1 + 1] * wreg[n1].y);
        } else {
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) {
                const long i0 = start + 2 * (64 * n1 + lane);
                v[n1] = make_float2(y[reflect_index(i0, p.L)] * wreg[n1].x, y[reflect_index(i0 + 1, p.L)] * wreg[n1].y);
            }
        }
        ddsp_wfft::fft_wave<R1, false, false>(v, tw, bufZ, lane);
        ddsp_wfft::store_natural<R1>(v, bufZ, lane);
        DDSP_WAVE_ORDER();
        cf *out = p.Rout + f * p.F;
#pragma unroll 1
        for (int it = 0; it < 9; ++it) {
            const int k = lane + 64 * it;
            if (k <= kM / 2) {
                cf X1, X2;
                ddsp_wfft::split2048(bufZ[k], bufZ[(kM - k) & (kM - 1)], ddsp_wfft::twiddle2048(wbase, it), X1, X2);
                out[k] = X1;
                if (k != kM / 2) out[kM - k] = X2;                                 // k = 0: the Nyquist bin 1024
            }
        }
        DDSP_WAVE_ORDER();
    }
}

// ---- overlap-add, envelope, trim --------------------------------------------------------------------------------------------
// y[b, j] = (sum over t ascending of frames[b, t, m - t hop]) / env[j] for m = j + n_fft/2 inside the natural signal
// (j < Lnat), 0 past it.
__global__ void __launch_bounds__(256) gl_overlap_kernel(const float *__restrict__ frames, const float *__restrict__ env,
                                                         float *__restrict__ y, long B, long T, int N, int hop, long L, long Lnat)
{
    const long total = B * L;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / L, j = i - b * L;
        float out = 0.0f;
        if (j < Lnat) {
            const long m = j + N / 2;
            const long tlo = m < N ? 0 : (m - N) / hop + 1;
            const long thi = (m / hop < T - 1) ? m / hop : T - 1;
            const float *fr = frames + b * T * N;
            float s = 0.0f;
            for (long t = tlo; t <= thi; ++t) s += fr[t * N + (m - t * hop)];
            out = s / env[j];
        }
        y[i] = out;
    }
}

// in [B, F, T] -> out [B, T, F]
template <typename V>
__global__ void __launch_bounds__(256) gl_transpose_kernel(const V *__restrict__ in, V *__restrict__ out, int F, int T)
{
    __shared__ V tile[32][33];
    const long b = blockIdx.z;
    const int f0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int f = f0 + r, t = t0 + tx;
        if (f < F && t < T) tile[r][tx] = in[(b * F + f) * T + t];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, f = f0 + tx;
        if (t < T && f < F) out[(b * T + t) * F + f] = tile[tx][r];
    }
}

struct Layout {
    size_t S, A0, R0, R1, frames, total;
};

Layout layout(long B, long T, int n_fft, int with_angles)
{
    const size_t bt = (size_t)B * (size_t)T, F = (size_t)(n_fft / 2 + 1);
    Layout l;
    l.S = 0;
    l.A0 = l.S + align256(bt * F * sizeof(float));
    l.R0 = l.A0 + (with_angles ? align256(bt * F * sizeof(cf)) : 0);
    l.R1 = l.R0 + align256(bt * F * sizeof(cf));
    l.frames = l.R1 + align256(bt * F * sizeof(cf));
    l.total = l.frames + align256(bt * (size_t)n_fft * sizeof(float));
    return l;
}

template <int N>
hipError_t launch_synth(const GlParams &p, hipStream_t s)
{
    if constexpr (N == 2048) {
        const size_t lds = sizeof(cf) * 2 * ddsp_wfft::buf_elems<16>();
        const long blocks = p.nframes < kMaxBlocks ? p.nframes : kMaxBlocks;
        hipLaunchKernelGGL(gl_synth2048_kernel, dim3((unsigned)blocks), dim3(64), lds, s, p);
    } else {
        using U = PairUnit<N>;
        const long nunits = (p.nframes + 2 * U::BT - 1) / (2 * U::BT);
        const long blocks = nunits < kMaxBlocks ? nunits : kMaxBlocks;
        hipLaunchKernelGGL((gl_synth_pair_kernel<N>), dim3((unsigned)blocks), dim3(64), sizeof(cf) * 2 * U::BUF, s, p, nunits);
    }
    return hipGetLastError();
}

template <int N>
hipError_t launch_analysis(const GlParams &p, hipStream_t s)
{
    if constexpr (N == 2048) {
        const size_t lds = sizeof(cf) * ddsp_wfft::buf_elems<16>();
        const long blocks = p.nframes < kMaxBlocks ? p.nframes : kMaxBlocks;
        hipLaunchKernelGGL(gl_analysis2048_kernel, dim3((unsigned)blocks), dim3(64), lds, s, p);
    } else {
        using U = PairUnit<N>;
        const long nunits = (p.nframes + 2 * U::BT - 1) / (2 * U::BT);
        const long blocks = nunits < kMaxBlocks ? nunits : kMaxBlocks;
        hipLaunchKernelGGL((gl_analysis_pair_kernel<N>), dim3((unsigned)blocks), dim3(64), sizeof(cf) * U::BUF, s, p, nunits);
    }
    return hipGetLastError();
}

hipError_t launch_overlap(const GlParams &p, const float *env, float *y, long B, int N, long Lnat, hipStream_t s)
{
    const long total = B * p.L;
    long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(gl_overlap_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p.frames, env, y, B, p.T, N, p.hop, p.L, Lnat);
    return hipGetLastError();
}

template <int N>
hipError_t run(GlParams p, const float *env, float *y, long B, long Lnat, int n_iter, cf *R[2], hipStream_t s)
{
    hipError_t e;
    for (int i = 0; i < n_iter; ++i) {
        p.R = i >= 1 ? R[(i - 1) & 1] : nullptr;
        p.Rprev = (i >= 2 && p.c != 0.0f) ? R[i & 1] : nullptr;    // R_(i-2): overwritten by this iteration's analysis, after use
        p.Rout = R[i & 1];
        if ((e = launch_synth<N>(p, s)) != hipSuccess) return e;
        if ((e = launch_overlap(p, env, y, B, N, Lnat, s)) != hipSuccess) return e;
        if ((e = launch_analysis<N>(p, s)) != hipSuccess) return e;
    }
    p.R = n_iter >= 1 ? R[(n_iter - 1) & 1] : nullptr;
    p.Rprev = (n_iter >= 2 && p.c != 0.0f) ? R[n_iter & 1] : nullptr;
    p.Rout = nullptr;
    if ((e = launch_synth<N>(p, s)) != hipSuccess) return e;
    return launch_overlap(p, env, y, B, N, Lnat, s);
}

// One launcher of the three on the caller's buffers (the test hook ddsp_griffinlim_stage)
template <int N>
hipError_t run_stage(int stage, const GlParams &p, const float *env, float *out, long B, long Lnat, hipStream_t s)
{
    switch (stage) {
    case DDSP_GL_STAGE_SYNTH: return launch_synth<N>(p, s);
    case DDSP_GL_STAGE_OVERLAP: return launch_overlap(p, env, out, B, N, Lnat, s);
    default: return launch_analysis<N>(p, s);
    }
}

}  // namespace

extern "C" int ddsp_griffinlim_stage(int stage, const float *S, const float *ang0, const float *R, const float *Rprev, const float *in,
                                     const float *window, const float *env, float *out, long B, long T, int n_fft, int hop, long L,
                                     float c, void *stream)
{
    if (!ddsp_hooks_on()) return DDSP_EPERM;
    if (!out || B <= 0 || T <= 0 || hop <= 0 || L <= 0 || !(c >= 0.0f && c < 1.0f)) return DDSP_EINVAL;
    switch (stage) {
    case DDSP_GL_STAGE_SYNTH: if (!S || !window) return DDSP_EINVAL; break;
    case DDSP_GL_STAGE_OVERLAP: if (!in || !env) return DDSP_EINVAL; break;
    case DDSP_GL_STAGE_ANALYSIS: if (!in || !window) return DDSP_EINVAL; break;
    default: return DDSP_EINVAL;
    }
    // ddsp_griffinlim's own range checks, in its order
    if (!ddsp_griffinlim_supported(n_fft)) return DDSP_ERANGE;
    if (1 + L / hop != T || L <= n_fft / 2 || B > 65535 || T > (1l << 24)) return DDSP_ERANGE;
    if ((double)B * (double)T * (double)n_fft > (double)(1l << 40)) return DDSP_ERANGE;
    GlParams p;
    p.S = S;
    p.ang0 = (const cf *)ang0;
    p.R = (const cf *)R;
    p.Rprev = (const cf *)Rprev;
    p.Rout = stage == DDSP_GL_STAGE_ANALYSIS ? (cf *)out : nullptr;
    p.frames = stage == DDSP_GL_STAGE_SYNTH ? out : const_cast<float *>(in);     // (the overlap launch only reads them)
    p.y = in;
    p.window = window;
    p.nframes = B * T;
    p.T = T;
    p.L = L;
    p.hop = hop;
    p.F = n_fft / 2 + 1;
    p.c = c;
    const long natural = (long)n_fft + (long)hop * (T - 1) - n_fft / 2;          // as in ddsp_griffinlim
    const long Lnat = L < natural ? L : natural;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    switch (n_fft) {
    case 64: e = run_stage<64>(stage, p, env, out, B, Lnat, s); break;
    case 128: e = run_stage<128>(stage, p, env, out, B, Lnat, s); break;
    case 256: e = run_stage<256>(stage, p, env, out, B, Lnat, s); break;
    case 512: e = run_stage<512>(stage, p, env, out, B, Lnat, s); break;
    case 1024: e = run_stage<1024>(stage, p, env, out, B, Lnat, s); break;
    default: e = run_stage<2048>(stage, p, env, out, B, Lnat, s); break;
    }
    return (int)e;
}

extern "C" int ddsp_griffinlim_supported(int n_fft) { return ddsp_wfft::real_size_supported(n_fft) ? 1 : 0; }

extern "C" size_t ddsp_griffinlim_workspace_bytes(long B, long T, int n_fft, int with_angles)
{
    if (B <= 0 || T <= 0 || !ddsp_griffinlim_supported(n_fft)) return 0;
    return layout(B, T, n_fft, with_angles).total;
}

extern "C" int ddsp_griffinlim(const float *mag, const float *angles, const float *window, const float *env, float *y, void *workspace,
                               size_t workspace_bytes, long B, long T, int n_fft, int hop, long L, int n_iter, float c, void *stream)
{
    if (!mag || !window || !env || !y || !workspace || B <= 0 || T <= 0 || hop <= 0 || L <= 0 || n_iter < 0 || !(c >= 0.0f && c < 1.0f))
        return DDSP_EINVAL;
    if (!ddsp_griffinlim_supported(n_fft)) return DDSP_ERANGE;
    // torch.stft center=True: T = 1 + L / hop frames; reflect padding needs n_fft / 2 < L; grid z / y limits of the transpose
    if (1 + L / hop != T || L <= n_fft / 2 || B > 65535 || T > (1l << 24)) return DDSP_ERANGE;
    if ((double)B * (double)T * (double)n_fft > (double)(1l << 40)) return DDSP_ERANGE;
    const Layout l = layout(B, T, n_fft, angles != nullptr);
    if (workspace_bytes < l.total) return DDSP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int F = n_fft / 2 + 1;
    GlParams p;
    p.S = (const float *)(ws + l.S);
    p.ang0 = angles ? (const cf *)(ws + l.A0) : nullptr;
    p.R = p.Rprev = nullptr;
    p.Rout = nullptr;
    p.frames = (float *)(ws + l.frames);
    p.y = y;
    p.window = window;
    p.nframes = B * T;
    p.T = T;
    p.L = L;
    p.hop = hop;
    p.F = F;
    p.c = c;
    cf *R[2] = {(cf *)(ws + l.R0), (cf *)(ws + l.R1)};

    const dim3 tgrid((unsigned)((T + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)B);
    hipLaunchKernelGGL(gl_transpose_kernel<float>, tgrid, dim3(256), 0, s, mag, (float *)(ws + l.S), F, (int)T);
    if (angles) hipLaunchKernelGGL(gl_transpose_kernel<float2>, tgrid, dim3(256), 0, s, (const float2 *)angles, (float2 *)(ws + l.A0), F, (int)T);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;

    // retained samples the natural signal covers: istft keeps [n_fft/2, n_fft/2 + L) of n_fft + hop (T - 1) samples
    const long natural = (long)n_fft + (long)hop * (T - 1) - n_fft / 2;
    const long Lnat = L < natural ? L : natural;
    switch (n_fft) {
    case 64: e = run<64>(p, env, y, B, Lnat, n_iter, R, s); break;
    case 128: e = run<128>(p, env, y, B, Lnat, n_iter, R, s); break;
    case 256: e = run<256>(p, env, y, B, Lnat, n_iter, R, s); break;
    case 512: e = run<512>(p, env, y, B, Lnat, n_iter, R, s); break;
    case 1024: e = run<1024>(p, env, y, B, Lnat, n_iter, R, s); break;
    default: e = run<2048>(p, env, y, B, Lnat, n_iter, R, s); break;
    }
    return (int)e;
}
