// Test hook: the pieces of ddsp_wave_fft.h on the caller's data, one wavefront per unit, so that tests/test_gpu_wave_fft.py can
// compare the transforms themselves with an fp64 DFT instead of seeing them through a loss, a logarithm or a random draw.
// Every kernel here loads its input in the layout the header documents, calls the header's function and stores the result in
// natural order; none does arithmetic of its own on the data.  The header is included, not changed.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_wave_fft.h"

namespace {

using ddsp_wfft::cf;

// PAIR: PairFft<N>::init, run<INV>, natural(i).  in, out [units, BT, N] complex (the STRIDE padding of the LDS rows is dropped)
template <int N, bool INV>
__global__ void __launch_bounds__(64) probe_pair_kernel(const cf *__restrict__ in, cf *__restrict__ out)
{
    using U = ddsp_wfft::PairUnit<N>;
    constexpr int R1 = U::R1, PL = U::PL, BT = U::BT, STRIDE = U::STRIDE;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);                       // U::BUF elements
    const int lane = threadIdx.x;
    ddsp_wfft::PairFft<N> fft;
    fft.init(lane);
    const cf *src = in + (long)blockIdx.x * BT * N;
    cf *dst = out + (long)blockIdx.x * BT * N;
    cf v[PL];
#pragma unroll
    for (int b = 0; b < BT; ++b)
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) v[b * R1 + n1] = src[b * N + 64 * n1 + lane];
    fft.template run<INV>(v, buf);
#pragma unroll
    for (int i = 0; i < PL; ++i) buf[fft.natural(i)] = v[i];
    DDSP_WAVE_ORDER();
#pragma unroll
    for (int b = 0; b < BT; ++b)
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) dst[b * N + 64 * n1 + lane] = buf[b * STRIDE + 64 * n1 + lane];
}

// WAVE: make_twiddles<R1>, fft_wave<R1, INV, HALFZERO>, store_natural<R1> (the noise kernels' route).  in [units, N] complex, or
// [units, N / 2] for HALFZERO with the upper registers zero; out [units, N] complex.
template <int R1, bool INV, bool HALFZERO>
__global__ void __launch_bounds__(64) probe_wave_kernel(const cf *__restrict__ in, cf *__restrict__ out)
{
    constexpr int N = 64 * R1, NIN = HALFZERO ? N / 2 : N;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);                       // buf_elems<R1>() >= N elements
    const int lane = threadIdx.x;
    ddsp_wfft::Twiddles<R1> tw;
    ddsp_wfft::make_twiddles<R1>(tw, lane);
    const cf *src = in + (long)blockIdx.x * NIN;
    cf *dst = out + (long)blockIdx.x * N;
    cf v[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) v[n1] = (!HALFZERO || n1 < R1 / 2) ? src[64 * n1 + lane] : make_float2(0.0f, 0.0f);
    ddsp_wfft::fft_wave<R1, INV, HALFZERO>(v, tw, buf, lane);
    ddsp_wfft::store_natural<R1>(v, buf, lane);
    DDSP_WAVE_ORDER();
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) dst[64 * n1 + lane] = buf[64 * n1 + lane];
}

// REAL2048 forward: in [units, 2048] real, out [units, 1025] complex.  The walk over the bins (k = lane + 64 it <= 512, the lane
// owns k and M - k, k = 0 yields bins 0 and M, k = 512 is its own partner) is NOT the header's: it mirrors the one in
// mss_wave2048_kernel and loudness_2048_kernel, whose own loops stay covered by their own tests.
__global__ void __launch_bounds__(64) probe_real2048_fwd_kernel(const float *__restrict__ in, cf *__restrict__ out)
{
    constexpr int M = 1024, R1 = 16;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);                       // buf_elems<16>() >= M elements
    const int lane = threadIdx.x;
    ddsp_wfft::Twiddles<R1> tw;
    ddsp_wfft::make_twiddles<R1>(tw, lane);
    const cf wbase = ddsp_wfft::lane_w2048(lane);
    const cf *src = reinterpret_cast<const cf *>(in) + (long)blockIdx.x * M;     // z[m] = x[2m] + i x[2m+1]
    cf *dst = out + (long)blockIdx.x * (M + 1);
    cf v[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) v[n1] = src[64 * n1 + lane];
    ddsp_wfft::fft_wave<R1, false, false>(v, tw, buf, lane);
    ddsp_wfft::store_natural<R1>(v, buf, lane);
    DDSP_WAVE_ORDER();
#pragma unroll 1
    for (int it = 0; it < 9; ++it) {
        const int k = lane + 64 * it;
        if (k <= M / 2) {
            cf X1, X2;
            ddsp_wfft::split2048(buf[k], buf[(M - k) & (M - 1)], ddsp_wfft::twiddle2048(wbase, it), X1, X2);
            dst[k] = X1;
            if (k != M / 2) dst[M - k] = X2;                        // k = 0: the Nyquist bin 1024
        }
    }
}

// REAL2048 inverse: in [units, 1025] complex (bins 0 and 1024 real, as a c2r transform takes them), out [units, 2048] real,
// unnormalised (2048 irfft).  The bin walk mirrors the users' (see above).
__global__ void __launch_bounds__(64) probe_real2048_inv_kernel(const cf *__restrict__ in, float *__restrict__ out)
{
    constexpr int M = 1024, R1 = 16;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    cf *buf = reinterpret_cast<cf *>(smem_f);
    const int lane = threadIdx.x;
    ddsp_wfft::Twiddles<R1> tw;
    ddsp_wfft::make_twiddles<R1>(tw, lane);
    const cf wbase = ddsp_wfft::lane_w2048(lane);
    const cf *src = in + (long)blockIdx.x * (M + 1);
    cf *dst = reinterpret_cast<cf *>(out) + (long)blockIdx.x * M;
#pragma unroll 1
    for (int it = 0; it < 9; ++it) {
        const int k = lane + 64 * it;
        if (k <= M / 2) {
            cf Y1, Y2;
            ddsp_wfft::pack2048(src[k], src[M - k], ddsp_wfft::twiddle2048(wbase, it), Y1, Y2);
            buf[k] = Y1;
            if (k != 0 && k != M / 2) buf[M - k] = Y2;
        }
    }
    DDSP_WAVE_ORDER();
    cf v[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) v[n1] = buf[64 * n1 + lane];
    DDSP_WAVE_ORDER();
    ddsp_wfft::fft_wave<R1, true, false>(v, tw, buf, lane);
    ddsp_wfft::store_natural<R1>(v, buf, lane);
    DDSP_WAVE_ORDER();
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) dst[64 * n1 + lane] = buf[64 * n1 + lane];
}

// TWIDDLES: every per-lane twiddle the header builds.  out [units, 64, DDSP_WFFT_TWIDDLE_COUNT] complex, per lane in this order:
//   Twiddles<8>: t1[8], t2[0][8];  Twiddles<16>: t1[16], t2[0][8], t2[1][8];  PairFft<128>::t1s[2];  PairFft<256>::t1s[4];
//   PairFft<64>, <128>, <256>::tw.t2[0][8];  lane_w2048(lane);  twiddle2048(lane_w2048(lane), it) for it = 0 .. 8.
template <int N>
__device__ __forceinline__ int dump_pair(cf *dst, int lane)
{
    ddsp_wfft::PairFft<N> fft;
    fft.init(lane);
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) dst[k2] = fft.tw.t2[0][k2];
    return 8;
}

__global__ void __launch_bounds__(64) probe_twiddles_kernel(cf *__restrict__ out)
{
    const int lane = threadIdx.x;
    cf *dst = out + ((long)blockIdx.x * 64 + lane) * DDSP_WFFT_TWIDDLE_COUNT;
    int o = 0;
    {
        ddsp_wfft::Twiddles<8> tw;
        ddsp_wfft::make_twiddles<8>(tw, lane);
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[o + k] = tw.t1[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[o + 8 + k] = tw.t2[0][k];
        o += 16;
    }
    {
        ddsp_wfft::Twiddles<16> tw;
        ddsp_wfft::make_twiddles<16>(tw, lane);
#pragma unroll
        for (int k = 0; k < 16; ++k) dst[o + k] = tw.t1[k];
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int k = 0; k < 8; ++k) dst[o + 16 + 8 * d + k] = tw.t2[d][k];
        o += 32;
    }
    {
        ddsp_wfft::PairFft<128> fft;
        fft.init(lane);
        dst[o] = fft.t1s[0]; dst[o + 1] = fft.t1s[1];
        o += 2;
    }
    {
        ddsp_wfft::PairFft<256> fft;
        fft.init(lane);
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[o + k] = fft.t1s[k];
        o += 4;
    }
    o += dump_pair<64>(dst + o, lane);
    o += dump_pair<128>(dst + o, lane);
    o += dump_pair<256>(dst + o, lane);
    const cf wbase = ddsp_wfft::lane_w2048(lane);
    dst[o++] = wbase;
#pragma unroll 1
    for (int it = 0; it < 9; ++it) dst[o + it] = ddsp_wfft::twiddle2048(wbase, it);
}

// SCALE: in [2 + n] floats (c_in, c_out, m[n]); out [n, 2]: frame_scale_of(m, c_in, c_out).in, .out
__global__ void __launch_bounds__(64) probe_scale_kernel(const float *__restrict__ in, float *__restrict__ out, long n)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const ddsp_wfft::FrameScale s = ddsp_wfft::frame_scale_of(in[2 + i], in[0], in[1]);
    out[2 * i] = s.in;
    out[2 * i + 1] = s.out;
}

// WAVEMAX: in, out [units, 64]: wave_max as every lane sees it
__global__ void __launch_bounds__(64) probe_wavemax_kernel(const float *__restrict__ in, float *__restrict__ out)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    out[i] = ddsp_wfft::wave_max(in[i]);
}

constexpr long kMaxUnits = 1L << 20;                                // far beyond any test; keeps every index inside 32-bit grids

template <int N, bool INV>
hipError_t launch_pair(const float *in, float *out, long units, hipStream_t s)
{
    hipLaunchKernelGGL((probe_pair_kernel<N, INV>), dim3((unsigned)units), dim3(64), sizeof(float2) * ddsp_wfft::PairUnit<N>::BUF, s,
                       reinterpret_cast<const cf *>(in), reinterpret_cast<cf *>(out));
    return hipGetLastError();
}

template <int R1, bool INV, bool HALFZERO>
hipError_t launch_wave(const float *in, float *out, long units, hipStream_t s)
{
    hipLaunchKernelGGL((probe_wave_kernel<R1, INV, HALFZERO>), dim3((unsigned)units), dim3(64), sizeof(float2) * ddsp_wfft::buf_elems<R1>(), s,
                       reinterpret_cast<const cf *>(in), reinterpret_cast<cf *>(out));
    return hipGetLastError();
}

// floats per unit (in, out) and floats in front of the units (SCALE's two constants); false for an unknown form
bool form_sizes(int form, long *in_unit, long *out_unit, long *in_head)
{
    *in_head = 0;
    if (form >= DDSP_WFFT_PAIR_FWD && form < DDSP_WFFT_PAIR_INV + 5) {
        *in_unit = *out_unit = 2 * 512 * (((form - DDSP_WFFT_PAIR_FWD) % 5) == 4 ? 2 : 1);       // BT * N complex: 512, or 1024 points
        return true;
    }
    switch (form) {
    case DDSP_WFFT_WAVE8_FWD: case DDSP_WFFT_WAVE8_INV: *in_unit = *out_unit = 2 * 512; return true;
    case DDSP_WFFT_WAVE8_HALFZERO: *in_unit = 2 * 256; *out_unit = 2 * 512; return true;
    case DDSP_WFFT_WAVE16_FWD: case DDSP_WFFT_WAVE16_INV: *in_unit = *out_unit = 2 * 1024; return true;
    case DDSP_WFFT_WAVE16_HALFZERO: *in_unit = 2 * 512; *out_unit = 2 * 1024; return true;
    case DDSP_WFFT_REAL2048_FWD: *in_unit = 2048; *out_unit = 2 * 1025; return true;
    case DDSP_WFFT_REAL2048_INV: *in_unit = 2 * 1025; *out_unit = 2048; return true;
    case DDSP_WFFT_TWIDDLES: *in_unit = 0; *out_unit = 2 * 64 * DDSP_WFFT_TWIDDLE_COUNT; return true;
    case DDSP_WFFT_SCALE: *in_unit = 1; *out_unit = 2; *in_head = 2; return true;
    case DDSP_WFFT_WAVEMAX: *in_unit = *out_unit = 64; return true;
    default: return false;
    }
}

}  // namespace

extern "C" int ddsp_wfft_probe_sizes(int form, long units, long *in_floats, long *out_floats)
{
    long iu, ou, head;
    if (!in_floats || !out_floats || units < 0 || units > kMaxUnits || !form_sizes(form, &iu, &ou, &head)) return DDSP_EINVAL;
    *in_floats = head + iu * units;
    *out_floats = ou * units;
    return 0;
}

extern "C" int ddsp_wfft_probe(int form, const float *in, float *out, long units, void *stream)
{
    if (!ddsp_hooks_on()) return DDSP_EPERM;
    long iu, ou, head;
    if (!in || !out || units < 0 || units > kMaxUnits || !form_sizes(form, &iu, &ou, &head)) return DDSP_EINVAL;
    if (units == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    switch (form) {
    case DDSP_WFFT_PAIR_FWD + 0: return (int)launch_pair<64, false>(in, out, units, s);
    case DDSP_WFFT_PAIR_FWD + 1: return (int)launch_pair<128, false>(in, out, units, s);
    case DDSP_WFFT_PAIR_FWD + 2: return (int)launch_pair<256, false>(in, out, units, s);
    case DDSP_WFFT_PAIR_FWD + 3: return (int)launch_pair<512, false>(in, out, units, s);
    case DDSP_WFFT_PAIR_FWD + 4: return (int)launch_pair<1024, false>(in, out, units, s);
    case DDSP_WFFT_PAIR_INV + 0: return (int)launch_pair<64, true>(in, out, units, s);
    case DDSP_WFFT_PAIR_INV + 1: return (int)launch_pair<128, true>(in, out, units, s);
    case DDSP_WFFT_PAIR_INV + 2: return (int)launch_pair<256, true>(in, out, units, s);
    case DDSP_WFFT_PAIR_INV + 3: return (int)launch_pair<512, true>(in, out, units, s);
    case DDSP_WFFT_PAIR_INV + 4: return (int)launch_pair<1024, true>(in, out, units, s);
    case DDSP_WFFT_WAVE8_FWD: return (int)launch_wave<8, false, false>(in, out, units, s);
    case DDSP_WFFT_WAVE8_INV: return (int)launch_wave<8, true, false>(in, out, units, s);
    case DDSP_WFFT_WAVE8_HALFZERO: return (int)launch_wave<8, false, true>(in, out, units, s);
    case DDSP_WFFT_WAVE16_FWD: return (int)launch_wave<16, false, false>(in, out, units, s);
    case DDSP_WFFT_WAVE16_INV: return (int)launch_wave<16, true, false>(in, out, units, s);
    case DDSP_WFFT_WAVE16_HALFZERO: return (int)launch_wave<16, false, true>(in, out, units, s);
    case DDSP_WFFT_REAL2048_FWD:
        hipLaunchKernelGGL(probe_real2048_fwd_kernel, dim3((unsigned)units), dim3(64), sizeof(float2) * ddsp_wfft::buf_elems<16>(), s, in,
                           reinterpret_cast<cf *>(out));
        return (int)hipGetLastError();
    case DDSP_WFFT_REAL2048_INV:
        hipLaunchKernelGGL(probe_real2048_inv_kernel, dim3((unsigned)units), dim3(64), sizeof(float2) * ddsp_wfft::buf_elems<16>(), s,
                           reinterpret_cast<const cf *>(in), out);
        return (int)hipGetLastError();
    case DDSP_WFFT_TWIDDLES:
        hipLaunchKernelGGL(probe_twiddles_kernel, dim3((unsigned)units), dim3(64), 0, s, reinterpret_cast<cf *>(out));
        return (int)hipGetLastError();
    case DDSP_WFFT_SCALE:
        hipLaunchKernelGGL(probe_scale_kernel, dim3((unsigned)((units + 63) / 64)), dim3(64), 0, s, in, out, units);
        return (int)hipGetLastError();
    default:   // DDSP_WFFT_WAVEMAX (form_sizes let nothing else through)
        hipLaunchKernelGGL(probe_wavemax_kernel, dim3((unsigned)units), dim3(64), 0, s, in, out);
        return (int)hipGetLastError();
    }
}
