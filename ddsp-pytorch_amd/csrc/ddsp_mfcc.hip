// MFCC front end of the timbre encoder as ONE kernel from the waveform to the coefficients:
//   frame f = x[f hop .. f hop + n_fft) (no centring: LoudnessEncoder's frames), periodic Hann window w (fp64, rounded to fp32),
//   A[k]      = |FFT(w x)[k]| * scale                      (scale = 2 / sum w: a full-scale sine reads 1)
//   mel[m]    = sum_k band_w[m, k] A[k]                    (ascending k over the band's contiguous run of bins)
//   logmel[m] = log(mel[m] + floor)
//   mfcc[j]   = sum_m dct[j, m] logmel[m]                  (ascending m)
// instead of a framing copy, a library FFT and a magnitude, two GEMM and a log pass over a [B, F, n_fft / 2 + 1] spectrogram.
// The transforms and the packing of frames are ddsp_loudness.hip's (ddsp_wave_fft.h):
//   * n_fft = 64 ... 1024: frames 2q and 2q + 1 of one row as one complex sequence a + i b, 512 / n_fft pairs per wavefront (one for
//     1024), a row's last frame of an odd count paired with zeros.  Both frames are equalised by powers of two (frame_scale) on
//     load, and the power comes back with `scale` AFTER the square root: a quiet frame does not carry its partner's rounding
//     noise, and |X|^2 neither overflows nor underflows whatever the frame's level is.
//   * n_fft = 2048: one real frame per wavefront through the 1024-point transform and split2048, equalised the same way.
// A frame with a NaN or an infinite sample is NaN in every output and enters the transform as zeros: its partner is computed
// alone.  An all-zero frame has A = 0 exactly, so logmel = log(floor) in every band.
// Epilogue: the magnitudes of the unit's frames are parked in LDS, one row per frame; (frame, band) items are dealt to the lanes,
// each summing its own bins; the log-mel rows are parked in LDS; (frame, coefficient) items are dealt to the lanes, each summing
// its own DCT row.  No atomics, no cross-lane sums: every output's operations and their order are fixed by (n_fft, the tables)
// alone, whatever the batch or the grid.  A band whose sum is exactly 0 (an all-zero frame, a band without bins) reads
// fl32(log(floor)), formed once in fp64; every other band takes the fp32 logarithm.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_wave_fft.h"

namespace {

constexpr int kMaxBlocks = 8192;
constexpr int kMaxMels = 128;
constexpr int kMaxMfcc = 64;

struct MfccParams {
    const float *x;
    const int *band_start, *band_count;
    const float *band_w, *dct;
    float *mfcc, *logmel;          // logmel may be null
    long B, L, F, PR, npairs;      // PR = frame pairs per row = ceil(F / 2)
    int hop, n_mels, n_mfcc;
    float scale, floor;
};

// the band tables in LDS: first bin, bins, offset of the band's first weight in band_w (the exclusive prefix sum of the counts)
struct BandTable {
    int start[kMaxMels], count[kMaxMels], offset[kMaxMels], raw[kMaxMels];
};

// |x| for the frame's maximum; a NaN counts as infinite, so that fmaxf keeps it
__device__ __forceinline__ float abs_or_inf(float x) { return x != x ? __builtin_huge_valf() : fabsf(x); }

// periodic Hann, 0.5 - 0.5 cos(2 pi n / N) in fp64, rounded to fp32
__device__ __forceinline__ float hann(int n, int N) { return (float)(0.5 - 0.5 * cospi(2.0 * (double)n / (double)N)); }

// start and count clamped to the frame's bins: a malformed table reads nothing outside its magnitude row
__device__ __forceinline__ void load_bands(BandTable &t, const MfccParams &p, int bins, int lane)
{
    for (int m = lane; m < p.n_mels; m += 64) {
        const int c = p.band_count[m];
        t.raw[m] = c > 0 ? c : 0;
        const int s = min(max(p.band_start[m], 0), bins);
        t.start[m] = s;
        t.count[m] = min(max(c, 0), bins - s);
    }
    DDSP_WAVE_ORDER();
    for (int m = lane; m < p.n_mels; m += 64) {
        int o = 0;
        for (int i = 0; i < m; ++i) o += t.raw[i];
        t.offset[m] = o;
    }
    DDSP_WAVE_ORDER();
}

// What the epilogue reads of the parameters, held in VECTOR registers for the kernel's lifetime: every use is per lane anyway
// (an address, a product with the lane's item), and as scalars these values stay live across the transform, where the scalar
// file is full (the compiler then spills scalars; with them here it does not -- DESIGN.md section 10h, resources).
template <typename V>
__device__ __forceinline__ V in_vgpr(V v)
{
    asm volatile("" : "+v"(v));
    return v;
}

struct EpilogueArgs {
    const float *band_w, *dct;
    float *mfcc, *logmel;
    int n_mels, n_mfcc;
    float scale, floor, log_floor;

    __device__ __forceinline__ void init(const MfccParams &p)
    {
        band_w = in_vgpr(p.band_w);
        dct = in_vgpr(p.dct);
        mfcc = in_vgpr(p.mfcc);
        logmel = in_vgpr(p.logmel);
        n_mels = in_vgpr(p.n_mels);
        n_mfcc = in_vgpr(p.n_mfcc);
        scale = in_vgpr(p.scale);
        floor = in_vgpr(p.floor);
        log_floor = in_vgpr((float)log((double)p.floor));
    }
};

// Magnitude rows mag[nf][ms] -> log-mel rows lm[nf][n_mels] -> outputs.  fout[fi]: the frame's index in the outputs, -1 for a
// slot without a frame; fdead[fi]: a frame that is NaN.  The two sums are unrolled so that their loads are in flight together
// (the kernel is bound by latency: 0.87 -> 0.46 ms at 512 x 2 s); each stays ONE chain of fused multiply-adds in the definition's order.
__device__ __forceinline__ void epilogue(const EpilogueArgs &p, const BandTable &t, const float *mag, int ms, float *lm, const long *fout,
                                         const int *fdead, int nf, int lane)
{
    const int n_mels = p.n_mels, n_mfcc = p.n_mfcc;
    for (int it = lane; it < nf * n_mels; it += 64) {
        const int fi = it / n_mels, m = it - fi * n_mels;
        const float *row = mag + fi * ms + t.start[m];
        const float *w = p.band_w + t.offset[m];
        const int c = t.count[m];
        float acc = 0.0f;
#pragma unroll 4
        for (int i = 0; i < c; ++i) acc = __fmaf_rn(w[i], row[i], acc);
        const float v = acc == 0.0f ? p.log_floor : logf(acc + p.floor);
        lm[it] = v;
        const long fo = fout[fi];
        if (p.logmel && fo >= 0) p.logmel[fo * n_mels + m] = fdead[fi] ? __builtin_nanf("") : v;
    }
    DDSP_WAVE_ORDER();
    for (int it = lane; it < nf * n_mfcc; it += 64) {
        const int fi = it / n_mfcc, j = it - fi * n_mfcc;
        const float *d = p.dct + (long)j * n_mels;
        const float *row = lm + fi * n_mels;
        float acc = 0.0f;
#pragma unroll 8
        for (int m = 0; m < n_mels; ++m) acc = __fmaf_rn(d[m], row[m], acc);
        const long fo = fout[fi];
        if (fo >= 0) p.mfcc[fo * n_mfcc + j] = fdead[fi] ? __builtin_nanf("") : acc;
    }
    DDSP_WAVE_ORDER();
}

// LDS after the transform's buffer: magnitude rows, log-mel rows, band tables, per-frame records
template <int NF, int MS>
struct Tail {
    float mag[NF * MS];
    float lm[NF * kMaxMels];
    BandTable bands;
    long fout[NF];
    int fdead[NF];
};

template <int N>
__global__ void __launch_bounds__(64) mfcc_pair_kernel(MfccParams p, long nunits)
{
    using U = ddsp_wfft::PairUnit<N>;
    using ddsp_wfft::cf;
    constexpr int R1 = U::R1, PL = U::PL, BT = U::BT, STRIDE = U::STRIDE, BINS = U::BINS;
    using T = Tail<2 * BT, BINS>;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);
    T &tail = *reinterpret_cast<T *>(smem_f + 2 * U::BUF);
    const int lane = threadIdx.x;
    ddsp_wfft::PairFft<N> fft;
    fft.init(lane);
    float win[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) win[n1] = hann(64 * n1 + lane, N);
    load_bands(tail.bands, p, BINS, lane);
    EpilogueArgs ep;
    ep.init(p);

    for (long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        float outa[BT], outb[BT];                         // 2^e / 2 * scale of the slot's two frames (0: an all-zero frame)
        cf v[PL];
#pragma unroll
        for (int b = 0; b < BT; ++b) {                    // wave-uniform slot bookkeeping
            const long pair = in_vgpr(unit * BT + b);          // (the slot's bookkeeping in vector registers: see EpilogueArgs)
            int nvalid = 0;
            long frame = 0, start = 0;
            if (pair < p.npairs) {
                const long row = pair / p.PR, fa = 2 * (pair - row * p.PR);
                frame = row * p.F + fa;
                nvalid = (fa + 1 < p.F) ? 2 : 1;
                start = row * p.L + fa * p.hop;
            }
            float ma = 0.0f, mb = 0.0f;
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) {
                const float *r = p.x + start + 64 * n1 + lane;
                const float re = nvalid > 0 ? r[0] * win[n1] : 0.0f;
                const float im = nvalid > 1 ? r[p.hop] * win[n1] : 0.0f;
                v[b * R1 + n1] = make_float2(re, im);
                ma = fmaxf(ma, abs_or_inf(re));
                mb = fmaxf(mb, abs_or_inf(im));
            }
            ma = ddsp_wfft::wave_max(ma);
            mb = ddsp_wfft::wave_max(mb);
            const ddsp_wfft::FrameScale sa = ddsp_wfft::frame_scale_of(ma, 1.0f, 0.5f), sb = ddsp_wfft::frame_scale_of(mb, 1.0f, 0.5f);
            const bool deada = !(ma < __builtin_huge_valf()), deadb = !(mb < __builtin_huge_valf());
            outa[b] = sa.out * ep.scale;
            outb[b] = sb.out * ep.scale;
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) {
                const cf z = v[b * R1 + n1];
                v[b * R1 + n1] = make_float2(deada ? 0.0f : z.x * sa.in, deadb ? 0.0f : z.y * sb.in);
            }
            if (lane == 0) {
                tail.fout[2 * b] = nvalid > 0 ? frame : -1;
                tail.fout[2 * b + 1] = nvalid > 1 ? frame + 1 : -1;
                tail.fdead[2 * b] = deada;
                tail.fdead[2 * b + 1] = deadb;
            }
        }
        fft.template run<false>(v, buf);
#pragma unroll
        for (int i = 0; i < PL; ++i) buf[fft.natural(i)] = v[i];
        DDSP_WAVE_ORDER();
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            const cf *zrow = buf + b * STRIDE;
            float *ra = tail.mag + (2 * b) * BINS, *rb = ra + BINS;
            for (int k = lane; k < BINS; k += 64) {
                const cf zk = zrow[k], zm = zrow[(N - k) & (N - 1)];
                const float ar = zk.x + zm.x, ai = zk.y - zm.y, br = zk.y + zm.y, bi = zm.x - zk.x;   // the split's 1/2 is in outa, outb
                ra[k] = sqrtf(__fmaf_rn(ar, ar, ai * ai)) * outa[b];
                rb[k] = sqrtf(__fmaf_rn(br, br, bi * bi)) * outb[b];
            }
        }
        DDSP_WAVE_ORDER();
        epilogue(ep, tail.bands, tail.mag, BINS, tail.lm, tail.fout, tail.fdead, 2 * BT, lane);
    }
}

// n_fft = 2048: Z = FFT_1024(x[2m] + i x[2m+1]) and ddsp_wave_fft.h's real split (a lane owns bins k and M - k, k = 0 .. 512)
__global__ void __launch_bounds__(64) mfcc_2048_kernel(MfccParams p, long nunits)
{
    using ddsp_wfft::cf;
    constexpr int M = 1024, R1 = 16, BINS = M + 1;
    using T = Tail<1, BINS>;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);
    T &tail = *reinterpret_cast<T *>(smem_f + 2 * ddsp_wfft::buf_elems<R1>());
    const int lane = threadIdx.x;
    ddsp_wfft::Twiddles<R1> tw;
    ddsp_wfft::make_twiddles<R1>(tw, lane);
    const cf wbase = ddsp_wfft::lane_w2048(lane);
    cf win[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) win[n1] = make_float2(hann(2 * (64 * n1 + lane), 2 * M), hann(2 * (64 * n1 + lane) + 1, 2 * M));
    load_bands(tail.bands, p, BINS, lane);
    EpilogueArgs ep;
    ep.init(p);

    for (long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const long b = unit / p.F, fr = unit - b * p.F;
        const float *rs = p.x + b * p.L + fr * p.hop;
        cf v[R1];
        // (4-byte loads whatever the frame's alignment: a second, 8-byte form of this loop, as ddsp_loudness.hip has one, costs
        //  the scalar registers the rest of the kernel needs)
        float mx = 0.0f;
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) {
            v[n1] = make_float2(rs[2 * (64 * n1 + lane)] * win[n1].x, rs[2 * (64 * n1 + lane) + 1] * win[n1].y);
            mx = fmaxf(mx, fmaxf(abs_or_inf(v[n1].x), abs_or_inf(v[n1].y)));
        }
        mx = ddsp_wfft::wave_max(mx);
        const ddsp_wfft::FrameScale sc = ddsp_wfft::frame_scale_of(mx, 1.0f, 1.0f);
        const bool dead = !(mx < __builtin_huge_valf());
        const float out = sc.out * ep.scale;
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) v[n1] = dead ? make_float2(0.0f, 0.0f) : make_float2(v[n1].x * sc.in, v[n1].y * sc.in);
        if (lane == 0) {
            tail.fout[0] = unit;
            tail.fdead[0] = dead;
        }
        ddsp_wfft::fft_wave<R1, false, false>(v, tw, buf, lane);
        ddsp_wfft::store_natural<R1>(v, buf, lane);
        DDSP_WAVE_ORDER();
#pragma unroll 1
        for (int it = 0; it < 9; ++it) {
            const int k = lane + 64 * it;
            if (k <= M / 2) {
                const cf wk = ddsp_wfft::twiddle2048(wbase, it);
                const int km = (M - k) & (M - 1);
                cf X1, X2;
                ddsp_wfft::split2048(buf[k], buf[km], wk, X1, X2);
                tail.mag[k] = sqrtf(__fmaf_rn(X1.x, X1.x, X1.y * X1.y)) * out;                          // bin k
                if (k != M / 2) tail.mag[M - k] = sqrtf(__fmaf_rn(X2.x, X2.x, X2.y * X2.y)) * out;      // bin M - k
            }
        }
        DDSP_WAVE_ORDER();
        epilogue(ep, tail.bands, tail.mag, BINS, tail.lm, tail.fout, tail.fdead, 1, lane);
    }
}

template <int N>
hipError_t launch_pairs(const MfccParams &p, hipStream_t s)
{
    using U = ddsp_wfft::PairUnit<N>;
    const long nunits = (p.npairs + U::BT - 1) / U::BT;
    const int blocks = (int)(nunits < kMaxBlocks ? nunits : kMaxBlocks);
    const size_t lds = sizeof(float2) * U::BUF + sizeof(Tail<2 * U::BT, U::BINS>);
    hipLaunchKernelGGL((mfcc_pair_kernel<N>), dim3((unsigned)blocks), dim3(64), lds, s, p, nunits);
    return hipGetLastError();
}

}  // namespace

extern "C" int ddsp_mfcc(const float *x, const int *band_start, const int *band_count, const float *band_w, const float *dct, float *mfcc,
                         float *logmel, long B, long L, int n_fft, int hop, int n_mels, int n_mfcc, float scale, float floor,
                         void *stream)
{
    if (B < 0 || !ddsp_wfft::real_size_supported(n_fft) || hop < 1) return DDSP_EINVAL;
    if (n_mels < 1 || n_mels > kMaxMels || n_mfcc < 1 || n_mfcc > n_mels || n_mfcc > kMaxMfcc) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!x || !band_start || !band_count || !band_w || !dct || !mfcc || L < n_fft) return DDSP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    MfccParams p;
    p.x = x; p.band_start = band_start; p.band_count = band_count; p.band_w = band_w; p.dct = dct;
    p.mfcc = mfcc; p.logmel = logmel;
    p.B = B; p.L = L; p.F = 1 + (L - n_fft) / hop; p.hop = hop;
    p.PR = (p.F + 1) / 2;
    p.npairs = B * p.PR;
    p.n_mels = n_mels; p.n_mfcc = n_mfcc; p.scale = scale; p.floor = floor;
    switch (n_fft) {
    case 64: return (int)launch_pairs<64>(p, s);
    case 128: return (int)launch_pairs<128>(p, s);
    case 256: return (int)launch_pairs<256>(p, s);
    case 512: return (int)launch_pairs<512>(p, s);
    case 1024: return (int)launch_pairs<1024>(p, s);
    default: {
        const long nunits = B * p.F;
        const int blocks = (int)(nunits < kMaxBlocks ? nunits : kMaxBlocks);
        const size_t lds = sizeof(float2) * ddsp_wfft::buf_elems<16>() + sizeof(Tail<1, 1025>);
        hipLaunchKernelGGL(mfcc_2048_kernel, dim3((unsigned)blocks), dim3(64), lds, s, p, nunits);
        return (int)hipGetLastError();
    }
    }
}
