// A-weighted loudness (model/autoencoder/encoder.py:131-156) as ONE kernel from the waveform to one value per frame:
//   X = torch.stft(x, n_fft, hop, center=False, no window)       frame f = x[f hop .. f hop + n_fft)
//   loudness[b, f] = mean_k ((20 log10(|X[f, k]| + 1e-20) + a_weight[k]) / 90 + 1),   k = 0 .. n_fft / 2
// instead of torch.stft's framing copy and library FFT, the magnitude / log / add / scale passes over the whole spectrogram and
// the mean.  Transforms are the wavefront-private FFTs of ddsp_wave_fft.h (a wavefront owns its frames and shares nothing):
//   * n_fft = 64 ... 1024: frames 2q and 2q + 1 of one row are packed as one complex sequence a + i b (a row's last frame of an
//     odd count is paired with zeros); a wavefront takes 512 / n_fft pairs at a time (one for 1024).  Bin k of each frame comes
//     out of the Hermitian split A = (Z_k + conj Z_{n-k}) / 2, B = -i (Z_k - conj Z_{n-k}) / 2.  Pairing inside a row keeps every
//     row's result independent of the rest of the batch.
//   * n_fft = 2048: one real frame per wavefront through a 1024-point complex transform of z[m] = x[2m] + i x[2m+1] and the
//     real-split step (the one-frame form of ddsp_mss_fft.hip).
// The mean over bins is a per-lane sum in bin order and a fixed butterfly across the wavefront: deterministic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_wave_fft.h"

namespace {

constexpr int kMaxBlocks = 8192;

struct LoudParams {
    const float *x;
    const double *aw;              // [n_fft / 2 + 1]: float64, as the reference's parameter is
    float *out;                    // [B * F]
    long B, L, F, PR, npairs;      // PR = frame pairs per row = ceil(F / 2)
    int hop;
};

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one bin's contribution, in the reference's operation order (encoder.py:148-151); |X| as a correctly rounded sqrt of |X|^2.
// The fp32 spectrum plus the float64 weight is rounded to fp32 once, as torch's in-place `stft += a_weight` does.
__device__ __forceinline__ float bin_term(float re, float im, double aw)
{
    const float mag = sqrtf(__fmaf_rn(re, re, im * im));
    const float db = (float)((double)(log10f(mag + 1e-20f) * 20.0f) + aw);
    return db / 90.0f + 1.0f;
}

template <int N>
struct PairUnit {
    static constexpr int R1 = N / 64;                    // 1, 2, 4, 8, 16
    static constexpr int PL = R1 < 8 ? 8 : R1;           // points per lane
    static constexpr int BT = PL / R1;                   // frame pairs per unit
    static constexpr int STRIDE = N + (R1 < 8 ? 4 * R1 : 0);
    static constexpr int EXCH = ddsp_wfft::buf_elems<(R1 < 8 ? 8 : R1)>();
    static constexpr int BUF = BT * STRIDE > EXCH ? BT * STRIDE : EXCH;
    static constexpr int BINS = N / 2 + 1;
};

template <int N>
__global__ void __launch_bounds__(64) loudness_pair_kernel(LoudParams p, long nunits)
{
    using U = PairUnit<N>;
    using ddsp_wfft::cf;
    constexpr int R1 = U::R1, PL = U::PL, BT = U::BT, STRIDE = U::STRIDE, BINS = U::BINS;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);
    const int lane = threadIdx.x;

    ddsp_wfft::Twiddles<(R1 < 8 ? 8 : R1)> tw;
    cf t1s[R1 < 8 ? (R1 > 1 ? R1 : 1) : 1];
    if constexpr (R1 >= 8) {
        ddsp_wfft::make_twiddles<R1>(tw, lane);
    } else {
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) {
            float sn, cs;
            sincospif(2.0f * (float)(((lane >> 3) * k2) & 63) / 64.0f, &sn, &cs);
            tw.t2[0][k2] = make_float2(cs, -sn);
        }
#pragma unroll
        for (int k1 = 0; k1 < (R1 > 1 ? R1 : 1); ++k1) {
            float sn, cs;
            sincospif(2.0f * (float)((lane * k1) & (N - 1)) / (float)N, &sn, &cs);
            t1s[k1] = make_float2(cs, -sn);
        }
    }
    // result register i of this lane -> natural-order address (pair's row * STRIDE + bin)
    auto natural = [&](int i) {
        if constexpr (R1 == 16) return lane + 64 * (i >> 3) + 128 * (i & 7);
        else {
            const int sq = lane & 7, k2 = lane >> 3;
            return (sq / R1) * STRIDE + (sq % R1) + R1 * (k2 + 8 * i);
        }
    };

    for (long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        long frame[BT];
        int nvalid[BT];
        cf v[PL];
#pragma unroll
        for (int b = 0; b < BT; ++b) {                    // wave-uniform slot bookkeeping
            const long pair = unit * BT + b;
            nvalid[b] = 0;
            frame[b] = 0;
            long start = 0;
            if (pair < p.npairs) {
                const long row = pair / p.PR, fa = 2 * (pair - row * p.PR);
                frame[b] = row * p.F + fa;
                nvalid[b] = (fa + 1 < p.F) ? 2 : 1;
                start = row * p.L + fa * p.hop;
            }
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) {
                const float *r = p.x + start + 64 * n1 + lane;
                const float re = nvalid[b] > 0 ? r[0] : 0.0f;
                const float im = nvalid[b] > 1 ? r[p.hop] : 0.0f;
                v[b * R1 + n1] = make_float2(re, im);
            }
        }
        if constexpr (R1 == 16) ddsp_wfft::fft_wave<16, false, false>(v, tw, buf, lane);
        else if constexpr (R1 == 8) ddsp_wfft::fft_wave_batched<8, false>(v, tw.t1, tw.t2[0], buf, lane);
        else ddsp_wfft::fft_wave_batched<R1, false>(v, t1s, tw.t2[0], buf, lane);
#pragma unroll
        for (int i = 0; i < PL; ++i) buf[natural(i)] = v[i];
        DDSP_WAVE_ORDER();
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            const cf *zrow = buf + b * STRIDE;
            float sa = 0.0f, sb = 0.0f;
            for (int k = lane; k < BINS; k += 64) {
                const cf zk = zrow[k], zm = zrow[(N - k) & (N - 1)];
                const double aw = p.aw[k];
                sa += bin_term(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y), aw);
                sb += bin_term(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x), aw);
            }
            sa = wave_sum(sa);
            sb = wave_sum(sb);
            if (lane == 0 && nvalid[b] > 0) {
                p.out[frame[b]] = sa / (float)BINS;
                if (nvalid[b] > 1) p.out[frame[b] + 1] = sb / (float)BINS;
            }
        }
        DDSP_WAVE_ORDER();
    }
}

// n_fft = 2048: Z = FFT_1024(x[2m] + i x[2m+1]);  Fe = (Z[k] + conj Z[M-k]) / 2,  Fo = -i (Z[k] - conj Z[M-k]) / 2,
// T = W_2048^k Fo:  X[k] = Fe + T,  X[M-k] = conj(Fe - T)  (a lane owns bins k and M - k, k = 0 .. 512; k = 0 gives bins 0 and M)
__global__ void __launch_bounds__(64) loudness_2048_kernel(LoudParams p, long nunits)
{
    using ddsp_wfft::cf;
    constexpr int N = 2048, M = 1024, R1 = 16;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);
    const int lane = threadIdx.x;
    ddsp_wfft::Twiddles<R1> tw;
    ddsp_wfft::make_twiddles<R1>(tw, lane);
    cf wbase;                                             // W_2048^lane
    {
        float sn, cs;
        sincospif(2.0f * (float)lane / (float)N, &sn, &cs);
        wbase = make_float2(cs, -sn);
    }
    // W_2048^(lane + 64 it) = W_2048^lane * W_32^it with exact-to-the-ulp constants (no running product)
    constexpr float c32[9] = {1.0f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f, 0.70710678118654752f,
                              0.55557023301960218f, 0.38268343236508977f, 0.19509032201612825f, 0.0f};
    constexpr float s32[9] = {0.0f, 0.19509032201612825f, 0.38268343236508977f, 0.55557023301960218f, 0.70710678118654752f,
                              0.83146961230254524f, 0.92387953251128674f, 0.98078528040323043f, 1.0f};
    for (long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const long b = unit / p.F, fr = unit - b * p.F;
        const float *rs = p.x + b * p.L + fr * p.hop;
        cf v[R1];
        if (((uintptr_t)rs & 7) == 0) {                   // wave-uniform: 8-byte aligned frame start
            const float2 *r = reinterpret_cast<const float2 *>(rs);
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) v[n1] = r[64 * n1 + lane];
        } else {
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) v[n1] = make_float2(rs[2 * (64 * n1 + lane)], rs[2 * (64 * n1 + lane) + 1]);
        }
        ddsp_wfft::fft_wave<R1, false, false>(v, tw, buf, lane);
        ddsp_wfft::store_natural<R1>(v, buf, lane);
        DDSP_WAVE_ORDER();
        float s = 0.0f;
#pragma unroll 1
        for (int it = 0; it < 9; ++it) {
            const int k = lane + 64 * it;
            if (k <= M / 2) {
                const cf wk = make_float2(__fmaf_rn(wbase.x, c32[it], wbase.y * s32[it]), __fmaf_rn(wbase.y, c32[it], -(wbase.x * s32[it])));
                const int km = (M - k) & (M - 1);
                const cf zk = buf[k], zm = buf[km];
                const cf Fe = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)), Fo = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
                const cf T = make_float2(__fmaf_rn(wk.x, Fo.x, -(wk.y * Fo.y)), __fmaf_rn(wk.x, Fo.y, wk.y * Fo.x));
                s += bin_term(Fe.x + T.x, Fe.y + T.y, p.aw[k]);                         // bin k
                if (k != M / 2) s += bin_term(Fe.x - T.x, -(Fe.y - T.y), p.aw[M - k]);   // bin M - k (k = 512 is its own partner)
            }
        }
        s = wave_sum(s);
        if (lane == 0) p.out[unit] = s / (float)(M + 1);
        DDSP_WAVE_ORDER();
    }
}

template <int N>
hipError_t launch_pairs(const LoudParams &p, hipStream_t s)
{
    using U = PairUnit<N>;
    const long nunits = (p.npairs + U::BT - 1) / U::BT;
    const int blocks = (int)(nunits < kMaxBlocks ? nunits : kMaxBlocks);
    hipLaunchKernelGGL((loudness_pair_kernel<N>), dim3((unsigned)blocks), dim3(64), sizeof(float2) * U::BUF, s, p, nunits);
    return hipGetLastError();
}

}  // namespace

extern "C" int ddsp_loudness_supported(int n_fft) { return (n_fft >= 64 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0) ? 1 : 0; }

extern "C" int ddsp_loudness(const float *x, const double *a_weight, float *out, long B, long L, int n_fft, int hop, void *stream)
{
    if (B == 0) return 0;
    if (!x || !a_weight || !out || B < 0 || L <= 0 || n_fft <= 0 || hop <= 0) return DDSP_EINVAL;
    if (!ddsp_loudness_supported(n_fft) || L < n_fft) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    LoudParams p;
    p.x = x; p.aw = a_weight; p.out = out;
    p.B = B; p.L = L; p.F = 1 + (L - n_fft) / hop; p.hop = hop;
    p.PR = (p.F + 1) / 2;
    p.npairs = B * p.PR;
    switch (n_fft) {
    case 64: return (int)launch_pairs<64>(p, s);
    case 128: return (int)launch_pairs<128>(p, s);
    case 256: return (int)launch_pairs<256>(p, s);
    case 512: return (int)launch_pairs<512>(p, s);
    case 1024: return (int)launch_pairs<1024>(p, s);
    default: {
        const long nunits = B * p.F;
        const int blocks = (int)(nunits < kMaxBlocks ? nunits : kMaxBlocks);
        hipLaunchKernelGGL(loudness_2048_kernel, dim3((unsigned)blocks), dim3(64), sizeof(float2) * ddsp_wfft::buf_elems<16>(), s, p, nunits);
        return (int)hipGetLastError();
    }
    }
}
