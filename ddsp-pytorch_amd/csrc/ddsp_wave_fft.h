// Wavefront-private complex FFTs in registers + LDS exchanges (gfx950), and the real-signal pieces around them, shared by the
// filtered-noise FFT form (ddsp_noise_fft.hip), the spectral-loss scales (ddsp_mss_fft.hip), the encoder's loudness
// (ddsp_loudness.hip) and Griffin-Lim (ddsp_griffinlim.hip).  One wavefront owns its transforms and shares nothing with other
// wavefronts: LDS operations of one wavefront execute in order, so the stage hand-offs need no barrier (DDSP_WAVE_ORDER).
//
// FFT of N = 64 * R1 points on one wavefront: n = 64 n1 + 8 n2 + n3, k = k1 + R1 k2 + 8 R1 k3;
//   radix-R1 over n1 in registers (lane = 8 n2 + n3) -> twiddle W_N^(lane k1) -> LDS exchange -> radix-8 over n2
//   (lane = k1 + R1 n3') -> twiddle W_64^(n3 k2) -> LDS exchange -> radix-8 over n3 (lane = k1 + R1 k2).
// Twiddles live in registers; the exchange addresses are linear (lane base + immediate offsets) and padded against bank conflicts.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "ddsp_internal.h"

namespace ddsp_wfft {

typedef float2 cf;

__device__ __forceinline__ cf cadd(cf a, cf b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cf csub(cf a, cf b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cf cmul(cf a, cf b) { return make_float2(__fmaf_rn(a.x, b.x, -(a.y * b.y)), __fmaf_rn(a.x, b.y, a.y * b.x)); }
// a * w for the forward transform, a * conj(w) for the inverse (w always holds the FORWARD twiddle e^{-i theta})
template <bool INV>
__device__ __forceinline__ cf cmulw(cf a, cf w)
{
    if (!INV) return make_float2(__fmaf_rn(a.x, w.x, -(a.y * w.y)), __fmaf_rn(a.x, w.y, a.y * w.x));
    return make_float2(__fmaf_rn(a.x, w.x, a.y * w.y), __fmaf_rn(a.y, w.x, -(a.x * w.y)));
}
// times -i (forward) / +i (inverse)
template <bool INV>
__device__ __forceinline__ cf rot90(cf a) { return INV ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x); }
// times W8^1 = e^{-i pi/4} and W8^3 = e^{-3 i pi/4} (conjugated for the inverse)
template <bool INV>
__device__ __forceinline__ cf mul_w8_1(cf a)
{
    constexpr float r = 0.70710678118654752f;
    return INV ? make_float2((a.x - a.y) * r, (a.x + a.y) * r) : make_float2((a.x + a.y) * r, (a.y - a.x) * r);
}
template <bool INV>
__device__ __forceinline__ cf mul_w8_3(cf a)
{
    constexpr float r = 0.70710678118654752f;
    return INV ? make_float2(-(a.x + a.y) * r, (a.x - a.y) * r) : make_float2((a.y - a.x) * r, -(a.x + a.y) * r);
}

// natural order in, natural order out
template <bool INV>
__device__ __forceinline__ void dft4(cf &p0, cf &p1, cf &p2, cf &p3)
{
    const cf s0 = cadd(p0, p2), s1 = cadd(p1, p3), d0 = csub(p0, p2), d1 = rot90<INV>(csub(p1, p3));
    p0 = cadd(s0, s1); p1 = cadd(d0, d1); p2 = csub(s0, s1); p3 = csub(d0, d1);
}

template <bool INV>
__device__ __forceinline__ void dft8(cf (&v)[8])
{
    cf a0 = cadd(v[0], v[4]), a1 = cadd(v[1], v[5]), a2 = cadd(v[2], v[6]), a3 = cadd(v[3], v[7]);
    cf b0 = csub(v[0], v[4]), b1 = mul_w8_1<INV>(csub(v[1], v[5])), b2 = rot90<INV>(csub(v[2], v[6])), b3 = mul_w8_3<INV>(csub(v[3], v[7]));
    dft4<INV>(a0, a1, a2, a3);   // X[0], X[2], X[4], X[6]
    dft4<INV>(b0, b1, b2, b3);   // X[1], X[3], X[5], X[7]
    v[0] = a0; v[2] = a1; v[4] = a2; v[6] = a3;
    v[1] = b0; v[3] = b1; v[5] = b2; v[7] = b3;
}

// HALFZERO: v[8..15] are zero (a length-N/2 signal zero-padded to N): the first radix-2 layer costs only its twiddles
template <bool INV, bool HALFZERO>
__device__ __forceinline__ void dft16(cf (&v)[16])
{
    constexpr float C = 0.92387953251128674f, S = 0.38268343236508977f;   // cos, sin of pi/8
    const cf w1 = make_float2(C, -S), w3 = make_float2(S, -C), w5 = make_float2(-S, -C), w7 = make_float2(-C, -S);
    cf a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] = HALFZERO ? v[j] : cadd(v[j], v[j + 8]);
        b[j] = HALFZERO ? v[j] : csub(v[j], v[j + 8]);
    }
    b[1] = cmulw<INV>(b[1], w1);
    b[2] = mul_w8_1<INV>(b[2]);
    b[3] = cmulw<INV>(b[3], w3);
    b[4] = rot90<INV>(b[4]);
    b[5] = cmulw<INV>(b[5], w5);
    b[6] = mul_w8_3<INV>(b[6]);
    b[7] = cmulw<INV>(b[7], w7);
    dft8<INV>(a);   // X[2m]
    dft8<INV>(b);   // X[2m+1]
#pragma unroll
    for (int m = 0; m < 8; ++m) { v[2 * m] = a[m]; v[2 * m + 1] = b[m]; }
}

template <int R1, bool INV, bool HALFZERO>
__device__ __forceinline__ void dft_r1(cf (&v)[R1])
{
    if constexpr (R1 == 16) dft16<INV, HALFZERO>(v);
    else {
        if constexpr (HALFZERO) {
            // v[4..7] zero: a_j = v_j, b_j = v_j W8^j
            cf a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3];
            cf b0 = v[0], b1 = mul_w8_1<INV>(v[1]), b2 = rot90<INV>(v[2]), b3 = mul_w8_3<INV>(v[3]);
            dft4<INV>(a0, a1, a2, a3);
            dft4<INV>(b0, b1, b2, b3);
            v[0] = a0; v[2] = a1; v[4] = a2; v[6] = a3;
            v[1] = b0; v[3] = b1; v[5] = b2; v[7] = b3;
        } else {
            dft8<INV>(v);
        }
    }
}

// Per-wavefront twiddles of the 64*R1-point transform (forward values; the inverse conjugates on the fly).
template <int R1>
struct Twiddles {
    cf t1[R1];                 // W_N^(lane * k1)
    cf t2[R1 / 8][8];          // W_64^(n3 * k2) for the lane's n3 of step 2 (one per DFT the lane does there)
};

template <int R1>
__device__ __forceinline__ void make_twiddles(Twiddles<R1> &tw, int lane)
{
    constexpr int N = 64 * R1;
#pragma unroll
    for (int k1 = 0; k1 < R1; ++k1) {
        float s, c;
        sincospif(2.0f * (float)((lane * k1) & (N - 1)) / (float)N, &s, &c);
        tw.t1[k1] = make_float2(c, -s);
    }
#pragma unroll
    for (int d = 0; d < R1 / 8; ++d) {
        const int n3 = (lane / R1) + (64 / R1) * d;      // step-2 lane = k1 + R1 * (n3 mod (64/R1)), DFT d = n3 div (64/R1)
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) {
            float s, c;
            sincospif(2.0f * (float)((n3 * k2) & 63) / 64.0f, &s, &c);
            tw.t2[d][k2] = make_float2(c, -s);
        }
    }
}

// Exchange addresses (in float2 units inside one buffer of buf_elems<R1>() elements).  Both are SEPARABLE in their arguments --
// lane-dependent base + compile-time offset, so the unrolled loops address LDS with immediates -- and laid out so that b64
// accesses do not collide on banks (a b64 access of 32 lanes covers the 64 banks once):
// step 1 -> 2, R1 = 16: element (k1, n2, n3) at 136 n2 + 17 n3 + k1.  A write (lanes (n2, n3), one k1) touches
//   8 n2 + 17 n3 mod 32: 32 different residues; the step-2 reads (lanes k1 + 16 m) are consecutive apart from one pad per 16 lanes.
// step 1 -> 2, R1 = 8: element (k1, n2, n3) at 68 k1 + 8 n2 + n3.  A write (lanes 8 n2 + n3, one k1) is 64 CONSECUTIVE elements;
//   a step-2 read (lanes k1 + 8 n3, one n2) touches 4 k1 + n3 mod 32: 32 different residues per half wavefront.  (Rounds 2-3 used
//   81 n2 + 9 n3 + k1 here: both its writes and its reads were two-way conflicted -- a quarter to a third of the LDS cycles of the
//   spectral-loss scales below 1024 points, profiles/r03_mss_pmc.json.)
template <int R1>
__device__ __forceinline__ int addr1(int k1, int n2, int n3) { return (R1 == 16) ? 136 * n2 + 17 * n3 + k1 : 68 * k1 + 8 * n2 + n3; }
// step 2 -> 3: element (c = k1 + R1 k2, n3) at ROW2 n3 + c (R1 = 8: 72 = 8 mod 32 puts the four n3 of a half-wavefront write on
// different banks; R1 = 16: 128, the writes of a half wavefront are 2 x 16 consecutive elements 128 apart ... see fft_wave)
template <int R1>
__device__ __forceinline__ int addr2(int c, int n3) { return ((R1 == 16) ? 128 : 72) * n3 + c; }
template <int R1>
constexpr int buf_elems() { return (R1 == 16) ? 8 * 136 : 576; }

// 64*R1-point complex FFT of the wavefront's data.  In: v[n1] = x[64 n1 + lane].  Out: v[d * 8 + k3] = X[c + 8 R1 k3] with
// c = lane + 64 d (d < R1/8).  `buf`: N float2 of LDS, free to clobber.
template <int R1, bool INV, bool HALFZERO>
__device__ __forceinline__ void fft_wave(cf (&v)[R1], const Twiddles<R1> &tw, cf *buf, int lane)
{
    constexpr int ND = R1 / 8;                     // radix-8 DFTs per lane in steps 2 and 3
    // step 1: radix-R1 over n1, twiddle, scatter
    dft_r1<R1, INV, HALFZERO>(v);
    {
        const int n2 = lane >> 3, n3 = lane & 7;
#pragma unroll
        for (int k1 = 0; k1 < R1; ++k1) {
            const cf a = (k1 == 0) ? v[0] : cmulw<INV>(v[k1], tw.t1[k1]);
            buf[addr1<R1>(k1, n2, n3)] = a;
        }
    }
    DDSP_WAVE_ORDER();
    // step 2: radix-8 over n2, twiddle, scatter
    cf u[ND][8];
    {
        const int k1 = lane & (R1 - 1), m3 = lane / R1;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int n3 = m3 + (64 / R1) * d;
#pragma unroll
            for (int n2 = 0; n2 < 8; ++n2) u[d][n2] = buf[addr1<R1>(k1, n2, n3)];
        }
        DDSP_WAVE_ORDER();
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int n3 = m3 + (64 / R1) * d;
            dft8<INV>(u[d]);
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) {
                const cf a = (k2 == 0) ? u[d][0] : cmulw<INV>(u[d][k2], tw.t2[d][k2]);
                buf[addr2<R1>(k1 + R1 * k2, n3)] = a;
            }
        }
    }
    DDSP_WAVE_ORDER();
    // step 3: radix-8 over n3
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const int c = lane + 64 * d;
        cf t[8];
#pragma unroll
        for (int n3 = 0; n3 < 8; ++n3) t[n3] = buf[addr2<R1>(c, n3)];
        dft8<INV>(t);
#pragma unroll
        for (int k3 = 0; k3 < 8; ++k3) v[d * 8 + k3] = t[k3];
    }
    DDSP_WAVE_ORDER();
}

// natural-order store of the result layout of fft_wave
template <int R1>
__device__ __forceinline__ void store_natural(const cf (&v)[R1], cf *dst, int lane)
{
#pragma unroll
    for (int d = 0; d < R1 / 8; ++d)
#pragma unroll
        for (int k3 = 0; k3 < 8; ++k3) dst[lane + 64 * d + 8 * R1 * k3] = v[d * 8 + k3];
}


// ---- 512 points per wavefront as 8 / R1 independent transforms of N = 64 R1 points (R1 = 1, 2, 4, 8) -----------------------
// Eight points per lane whatever N is: step 1 is a radix-R1 butterfly per transform (nothing for R1 = 1) and its twiddle
// W_N^(lane k1); what is left are eight 64-point sequences (s = b R1 + k1) across the lanes -- exactly steps 2 and 3 of the
// 512-point transform above, with s in the role of k1.
//   In:  v[b R1 + n1] = x_b[64 n1 + lane].   Out: v[k3] = X_b[k1 + R1 (k2 + 8 k3)] on lane s + 8 k2, s = b R1 + k1.
// t1[k1] = W_N^(lane k1) (k1 < R1), t2[k2] = W_64^((lane >> 3) k2); `buf`: buf_elems<8>() float2 of LDS, free to clobber.
template <int R1, bool INV>
__device__ __forceinline__ void fft_wave_batched(cf (&v)[8], const cf *t1, const cf (&t2)[8], cf *buf, int lane)
{
    static_assert(R1 == 1 || R1 == 2 || R1 == 4 || R1 == 8, "transform sizes 64, 128, 256, 512");
    // step 1: radix-R1 over n1 inside each transform, twiddle, scatter
#pragma unroll
    for (int b = 0; b < 8 / R1; ++b) {
        if constexpr (R1 == 2) {
            const cf a0 = v[2 * b], a1 = v[2 * b + 1];
            v[2 * b] = cadd(a0, a1);
            v[2 * b + 1] = csub(a0, a1);
        } else if constexpr (R1 == 4) {
            dft4<INV>(v[4 * b], v[4 * b + 1], v[4 * b + 2], v[4 * b + 3]);
        } else if constexpr (R1 == 8) {
            dft8<INV>(v);
        }
    }
    {
        const int n2 = lane >> 3, n3 = lane & 7;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int k1 = s % R1;
            const cf a = (k1 == 0) ? v[s] : cmulw<INV>(v[s], t1[k1]);
            buf[addr1<8>(s, n2, n3)] = a;
        }
    }
    DDSP_WAVE_ORDER();
    // step 2: radix-8 over n2, twiddle, scatter
    cf u[8];
    {
        const int s = lane & 7, n3 = lane >> 3;
#pragma unroll
        for (int n2 = 0; n2 < 8; ++n2) u[n2] = buf[addr1<8>(s, n2, n3)];
        DDSP_WAVE_ORDER();
        dft8<INV>(u);
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) {
            const cf a = (k2 == 0) ? u[0] : cmulw<INV>(u[k2], t2[k2]);
            buf[addr2<8>(s + 8 * k2, n3)] = a;
        }
    }
    DDSP_WAVE_ORDER();
    // step 3: radix-8 over n3
#pragma unroll
    for (int n3 = 0; n3 < 8; ++n3) u[n3] = buf[addr2<8>(lane, n3)];
    dft8<INV>(u);
#pragma unroll
    for (int k3 = 0; k3 < 8; ++k3) v[k3] = u[k3];
    DDSP_WAVE_ORDER();
}


// ---- two real frames in one complex transform: the power-of-two equaliser ---------------------------------------------------
// A transform of a + i b (the filtered noise's, the loudness's) leaves in each frame an fp32-epsilon share of the other: harmless
// when they are equally loud, a relative error of eps * ratio in the quiet one when they are not (the reference transforms every
// frame alone).  Where everything between the load and the split is linear in the frame, the frame is scaled by 2^-e on the way
// in and by 2^e on the way out -- exact -- with e the exponent of its largest magnitude: both halves of a pair then sit in
// [0.5, 1).  An all-zero frame comes out as exact zeros (as the reference's does), not as its partner's rounding residue.
// `c_in`, `c_out`: the constants the two scalings fold into.
struct FrameScale { float in, out; };

// max over the 64 lanes, every lane gets it (fmaxf: a NaN lane is dropped, an infinite one wins)
__device__ __forceinline__ float wave_max(float m)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));
    return m;
}

// `m`: the frame's max |value| (wave_max).  Zero, infinite: e = 0.
__device__ __forceinline__ FrameScale frame_scale_of(float m, float c_in, float c_out)
{
    int e = 0;
    if (m > 0.0f && m < __builtin_huge_valf()) (void)frexpf(m, &e);
    e = max(-100, min(100, e));                         // 2^-e and 2^e stay normal numbers whatever the input holds
    FrameScale s;
    s.in = ldexpf(c_in, -e);
    s.out = (m == 0.0f) ? 0.0f : ldexpf(c_out, e);
    return s;
}

// `m`: the lane's own max |value|
__device__ __forceinline__ FrameScale frame_scale(float m, float c_in, float c_out) { return frame_scale_of(wave_max(m), c_in, c_out); }

// ---- real signals: n_fft a power of two in 64 .. 2048 -----------------------------------------------------------------------
constexpr bool real_size_supported(int n_fft) { return n_fft >= 64 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0; }

// n_fft = 64 ... 1024: two real frames a, b packed as one complex sequence a + i b.  One wavefront owns a unit of PL points per
// lane -- BT = 512 / n_fft frame pairs for n_fft <= 512, one pair for 1024 -- in the layout v[b R1 + n1] = z_b[64 n1 + lane];
// the spectra are parked in natural order in LDS, one row of STRIDE per pair.
template <int N>
struct PairUnit {
    static constexpr int R1 = N / 64;                            // 1, 2, 4, 8, 16
    static constexpr int PL = R1 < 8 ? 8 : R1;                   // points per lane
    static constexpr int BT = PL / R1;                           // frame pairs per unit
    static constexpr int STRIDE = N + (R1 < 8 ? 4 * R1 : 0);     // natural-order row of one pair's spectrum (pad: conflict-free stores)
    static constexpr int EXCH = buf_elems<(R1 < 8 ? 8 : R1)>();
    static constexpr int BUF = BT * STRIDE > EXCH ? BT * STRIDE : EXCH;
    static constexpr int BINS = N / 2 + 1;
};

// the lane's twiddles and the transforms of one unit (v[b R1 + n1] = z_b[64 n1 + lane] in, natural(i) out): fft_wave for 1024
// points, fft_wave_batched below
template <int N>
struct PairFft {
    static constexpr int R1 = PairUnit<N>::R1, PL = PairUnit<N>::PL;
    Twiddles<(R1 < 8 ? 8 : R1)> tw;                             // R1 = 16: the 1024-point transform's; smaller: t2 only
    cf t1s[R1 < 8 ? (R1 > 1 ? R1 : 1) : 1];
    int lane;

    __device__ __forceinline__ void init(int l)
    {
        lane = l;
        if constexpr (R1 >= 8) {
            make_twiddles<R1>(tw, lane);
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
    }
    template <bool INV>
    __device__ __forceinline__ void run(cf (&v)[PL], cf *buf)
    {
        if constexpr (R1 == 16) fft_wave<16, INV, false>(v, tw, buf, lane);
        else if constexpr (R1 == 8) fft_wave_batched<8, INV>(v, tw.t1, tw.t2[0], buf, lane);
        else fft_wave_batched<R1, INV>(v, t1s, tw.t2[0], buf, lane);
    }
    // result register i -> natural-order LDS address (pair's row * STRIDE + bin)
    __device__ __forceinline__ int natural(int i) const
    {
        if constexpr (R1 == 16) return lane + 64 * (i >> 3) + 128 * (i & 7);           // v[d * 8 + k3] = X[lane + 64 d + 128 k3]
        else {
            const int sq = lane & 7, k2 = lane >> 3;                                    // v[k3] = X_b[k1 + R1 (k2 + 8 k3)], s = b R1 + k1
            return (sq / R1) * PairUnit<N>::STRIDE + (sq % R1) + R1 * (k2 + 8 * i);
        }
    }
};

// n_fft = 2048: one REAL frame per wavefront through a 1024-point complex transform (the 2048 complex points of a frame pair
// exceed a wavefront's registers).  M = 1024; a lane owns the bins k and M - k, k = lane + 64 it <= 512 (k = 0: bins 0 and M).
// Forward: z[m] = x[2m] + i x[2m+1], Z = FFT_1024(z):  split2048.   Inverse (c2r): pack2048, then IFFT_1024(Y)[m] = 2048 (x[2m] + i x[2m+1]).

// W_2048^lane
__device__ __forceinline__ cf lane_w2048(int lane)
{
    float sn, cs;
    sincospif(2.0f * (float)lane / 2048.0f, &sn, &cs);
    return make_float2(cs, -sn);
}

// W_2048^k for k = lane + 64 it, = W_2048^lane * W_32^it: one product with an exact-to-the-ulp constant per trip (advancing a
// running twiddle by W_32 eight times costs 5e-7 of relative accuracy, which near-empty bins amplify a thousandfold)
__device__ __forceinline__ cf twiddle2048(cf wbase, int it)
{
    constexpr float c32[9] = {1.0f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f, 0.70710678118654752f,
                              0.55557023301960218f, 0.38268343236508977f, 0.19509032201612825f, 0.0f};
    constexpr float s32[9] = {0.0f, 0.19509032201612825f, 0.38268343236508977f, 0.55557023301960218f, 0.70710678118654752f,
                              0.83146961230254524f, 0.92387953251128674f, 0.98078528040323043f, 1.0f};
    // (wx + i wy)(c - i s)
    return make_float2(__fmaf_rn(wbase.x, c32[it], wbase.y * s32[it]), __fmaf_rn(wbase.y, c32[it], -(wbase.x * s32[it])));
}

// real-to-complex split, (Z[k], Z[M-k], W^k) -> (X[k], X[M-k]):
//   Fe = (Z[k] + conj Z[M-k]) / 2,  Fo = -i (Z[k] - conj Z[M-k]) / 2,  T = W^k Fo:   X[k] = Fe + T,  X[M-k] = conj(Fe - T)
__device__ __forceinline__ void split2048(cf zk, cf zm, cf wk, cf &xk, cf &xm)
{
    const cf Fe = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)), Fo = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
    const cf T = make_float2(__fmaf_rn(wk.x, Fo.x, -(wk.y * Fo.y)), __fmaf_rn(wk.x, Fo.y, wk.y * Fo.x));
    xk = make_float2(Fe.x + T.x, Fe.y + T.y);
    xm = make_float2(Fe.x - T.x, -(Fe.y - T.y));
}

// complex-to-real packing, (X[k], X[M-k], W^k) -> (Y[k], Y[M-k]):
//   S = X[k] + conj X[M-k],  D = X[k] - conj X[M-k]:   Y[k] = S + i conj(W^k) D,   Y[M-k] = conj(S) + i W^k conj(D)
__device__ __forceinline__ void pack2048(cf xk, cf xm, cf wk, cf &yk, cf &ym)
{
    const cf S = make_float2(xk.x + xm.x, xk.y - xm.y), D = make_float2(xk.x - xm.x, xk.y + xm.y);
    const cf cD = make_float2(__fmaf_rn(wk.x, D.x, wk.y * D.y), __fmaf_rn(wk.x, D.y, -(wk.y * D.x)));   // conj(w) D
    yk = make_float2(S.x - cD.y, S.y + cD.x);
    const cf wD = make_float2(__fmaf_rn(wk.x, D.x, wk.y * D.y), __fmaf_rn(wk.y, D.x, -(wk.x * D.y)));   // w conj(D)
    ym = make_float2(S.x - wD.y, -S.y + wD.x);
}

}  // namespace ddsp_wfft
