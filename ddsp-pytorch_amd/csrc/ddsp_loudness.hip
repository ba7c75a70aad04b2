// A-weighted loudness (model/autoencoder/encoder.py:131-156) as ONE kernel from the waveform to one value per frame:
//   X = torch.stft(x, n_fft, hop, center=False, no window)       frame f = x[f hop .. f hop + n_fft)
//   loudness[b, f] = mean_k ((20 log10(|X[f, k]| + 1e-20) + a_weight[k]) / 90 + 1),   k = 0 .. n_fft / 2
// instead of torch.stft's framing copy and library FFT, the magnitude / log / add / scale passes over the whole spectrogram and
// the mean.  Transforms are the wavefront-private FFTs of ddsp_wave_fft.h (a wavefront owns its frames and shares nothing):
//   * n_fft = 64 ... 1024: frames 2q and 2q + 1 of one row are packed as one complex sequence a + i b (a row's last frame of an
//     odd count is paired with zeros); a wavefront takes 512 / n_fft pairs at a time (one for 1024).  Bin k of each frame comes
//     out of the Hermitian split A = (Z_k + conj Z_{n-k}) / 2, B = -i (Z_k - conj Z_{n-k}) / 2.  Pairing inside a row keeps every
//     row's result independent of the rest of the batch.  The two frames of a pair are equalised by powers of two
//     (ddsp_wave_fft.h: frame_scale): each is scaled by 2^-e, e the exponent of its largest |sample|, on load and by 2^e on the
//     split's outputs -- both exact, so |X| and everything after it round as they do for a frame transformed alone, and a quiet
//     frame (an onset after silence, a zero margin) does not carry its partner's rounding noise into its logarithms.  An
//     all-zero frame comes out as exact zeros (log10(1e-20) in every bin, the reference's value).  A frame with a NaN or an
//     infinite sample is NaN, as torch.stft makes it, and enters the transform as zeros: its partner is computed alone.
//   * n_fft = 2048: one real frame per wavefront through a 1024-point complex transform of z[m] = x[2m] + i x[2m+1] and the
//     real-split step (the one-frame form of ddsp_mss_fft.hip).
// The mean over bins is a per-lane sum in bin order and a fixed butterfly across the wavefront: deterministic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
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

// one bin's contribution, in the reference's operation order (encoder.py:148-151); |X| as a correctly rounded sqrt of |X|^2.
// The fp32 spectrum plus the float64 weight is rounded to fp32 once, as torch's in-place `stft += a_weight` does.
__device__ __forceinline__ float bin_term(float re, float im, double aw)
{
    const float mag = sqrtf(__fmaf_rn(re, re, im * im));
    const float db = (float)((double)(log10f(mag + 1e-20f) * 20.0f) + aw);
    return db / 90.0f + 1.0f;
}

// |x| for the frame's maximum; a NaN counts as infinite, so that fmaxf keeps it
__device__ __forceinline__ float abs_or_inf(float x) { return x != x ? __builtin_huge_valf() : fabsf(x); }

template <int N>
__global__ void __launch_bounds__(64) loudness_pair_kernel(LoudParams p, long nunits)
{
    using U = ddsp_wfft::PairUnit<N>;
    using ddsp_wfft::cf;
    constexpr int R1 = U::R1, PL = U::PL, BT = U::BT, STRIDE = U::STRIDE, BINS = U::BINS;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);
    const int lane = threadIdx.x;
    ddsp_wfft::PairFft<N> fft;
    fft.init(lane);

    for (long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        long frame[BT];
        int nvalid[BT];
        float outa[BT], outb[BT];                         // 2^e / 2 of the slot's two frames (0: an all-zero frame)
        bool deada[BT], deadb[BT];                        // a frame with a sample that is not finite
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
            float ma = 0.0f, mb = 0.0f;
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) {
                const float *r = p.x + start + 64 * n1 + lane;
                const float re = nvalid[b] > 0 ? r[0] : 0.0f;
                const float im = nvalid[b] > 1 ? r[p.hop] : 0.0f;
                v[b * R1 + n1] = make_float2(re, im);
                ma = fmaxf(ma, abs_or_inf(re));
                mb = fmaxf(mb, abs_or_inf(im));
            }
            ma = ddsp_wfft::wave_max(ma);
            mb = ddsp_wfft::wave_max(mb);
            const ddsp_wfft::FrameScale sa = ddsp_wfft::frame_scale_of(ma, 1.0f, 0.5f), sb = ddsp_wfft::frame_scale_of(mb, 1.0f, 0.5f);
            deada[b] = !(ma < __builtin_huge_valf());
            deadb[b] = !(mb < __builtin_huge_valf());
            outa[b] = sa.out;
            outb[b] = sb.out;
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) {
                const cf z = v[b * R1 + n1];
                v[b * R1 + n1] = make_float2(deada[b] ? 0.0f : z.x * sa.in, deadb[b] ? 0.0f : z.y * sb.in);
            }
        }
        fft.template run<false>(v, buf);
#pragma unroll
        for (int i = 0; i < PL; ++i) buf[fft.natural(i)] = v[i];
        DDSP_WAVE_ORDER();
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            const cf *zrow = buf + b * STRIDE;
            float sa = 0.0f, sb = 0.0f;
            for (int k = lane; k < BINS; k += 64) {
                const cf zk = zrow[k], zm = zrow[(N - k) & (N - 1)];
                const double aw = p.aw[k];
                sa += bin_term((zk.x + zm.x) * outa[b], (zk.y - zm.y) * outa[b], aw);     // the split's 1/2 is in outa, outb
                sb += bin_term((zk.y + zm.y) * outb[b], (zm.x - zk.x) * outb[b], aw);
            }
            sa = wave_sum(sa);
            sb = wave_sum(sb);
            if (lane == 0 && nvalid[b] > 0) {
                p.out[frame[b]] = deada[b] ? __builtin_nanf("") : sa / (float)BINS;
                if (nvalid[b] > 1) p.out[frame[b] + 1] = deadb[b] ? __builtin_nanf("") : sb / (float)BINS;
            }
        }
        DDSP_WAVE_ORDER();
    }
}

// n_fft = 2048: Z = FFT_1024(x[2m] + i x[2m+1]) and ddsp_wave_fft.h's real split (a lane owns bins k and M - k, k = 0 .. 512)
__global__ void __launch_bounds__(64) loudness_2048_kernel(LoudParams p, long nunits)
{
    using ddsp_wfft::cf;
    constexpr int M = 1024, R1 = 16;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);
    const int lane = threadIdx.x;
    ddsp_wfft::Twiddles<R1> tw;
    ddsp_wfft::make_twiddles<R1>(tw, lane);
    cf wbase;                                             // W_2048^lane: ddsp_wfft::lane_w2048 written out -- called, it costs
    {                                                     // this kernel 20 more SGPRs (same values, another schedule)
        float sn, cs;
        sincospif(2.0f * (float)lane / 2048.0f, &sn, &cs);
        wbase = make_float2(cs, -sn);
    }
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
                const cf wk = ddsp_wfft::twiddle2048(wbase, it);
                const int km = (M - k) & (M - 1);
                cf X1, X2;
                ddsp_wfft::split2048(buf[k], buf[km], wk, X1, X2);
                s += bin_term(X1.x, X1.y, p.aw[k]);                         // bin k
                if (k != M / 2) s += bin_term(X2.x, X2.y, p.aw[M - k]);     // bin M - k (k = 512 is its own partner)
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
    using U = ddsp_wfft::PairUnit<N>;
    const long nunits = (p.npairs + U::BT - 1) / U::BT;
    const int blocks = (int)(nunits < kMaxBlocks ? nunits : kMaxBlocks);
    hipLaunchKernelGGL((loudness_pair_kernel<N>), dim3((unsigned)blocks), dim3(64), sizeof(float2) * U::BUF, s, p, nunits);
    return hipGetLastError();
}

}  // namespace

extern "C" int ddsp_loudness_supported(int n_fft) { return ddsp_wfft::real_size_supported(n_fft) ? 1 : 0; }

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
