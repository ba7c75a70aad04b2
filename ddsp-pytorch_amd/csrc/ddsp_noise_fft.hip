// Filtered noise, in-LDS FFT form, for MI355X (gfx950): the same arithmetic contract as ddsp_noise.hip
// (model/ddsp/filtered_noise.py:7-53) for power-of-two hops R = 256 / 512, where the direct truncated convolution
// (R/2 multiply-adds per sample) is several times the cost of doing what the reference itself does (:25-32):
// zero-pad to N = 2R, multiply spectra, transform back, keep R samples.
//
// One WAVEFRONT owns a pair of frames (a, b) at a time and nothing is shared between wavefronts, so the kernel has no
// workgroup barrier at all (workgroup = 64 threads, 17 KB of LDS, eight per CU); LDS operations of one wavefront
// execute in order, which is all the hand-offs between the stages need.
//
//   1. impulse responses: irfft of the zero-phase magnitudes (:8-10).  For S = 512 the two frames' Hermitian spectra
//      are packed as H~a + i H~b and ONE 512-point complex inverse FFT yields z_a + i z_b (both real); other S take
//      the direct cosine sums of ddsp_noise.hip.  Periodic Hann window (:15), roll/pad/roll (:14,:19-20) -> kk = k_a + i k_b
//   2. noise: the injected draw or Philox4x32-10 with the SAME counter layout as the direct kernels -> xx = x_a + i x_b
//   3. two N-point complex FFTs, Cx = FFT(xx), Ck = FFT(kk) (inputs zero above R: the first radix-2 layer is free);
//      frames are paired signal-with-signal and kernel-with-kernel so that both halves of a packed transform have the
//      same magnitude (packing x with k would lose ~1e-6 of the kernel spectrum under the 13x larger noise spectrum)
//   4. Hermitian split + product + re-pack in one pass over the bins:
//         P[g] = [(A + B)(E + F) - i (A - B)(E - F)] / 4,  A = Cx[g], B = conj Cx[N-g], E = Ck[g], F = conj Ck[N-g]
//      = X_a K_a + i X_b K_b, then ONE N-point inverse FFT gives y_a + i y_b; the first R samples are kept (:31)
//   5. coalesced float4 stores (read-modify-write when accumulating into the oscillator's output, decoder.py:132)
// The transforms are ddsp_wave_fft.h's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_noise_common.h"
#include "ddsp_wave_fft.h"

using namespace ddsp_noise;

namespace {

using namespace ddsp_wfft;

// Two frames share every transform of this file (one in the real part, one in the imaginary part) and everything here is linear in
// a frame's magnitudes / gradient row: the pair is equalised by powers of two (ddsp_wave_fft.h: frame_scale).

struct FrameSrc {
    long frame;   // index into [B*T]
    bool valid;
};

// ---- the kernel ------------------------------------------------------------------------------------------------
// R1 = N / 64 = R / 32 (16: hop 512, 8: hop 256).  IRFFT: S == 512, impulse responses by one packed 512-point inverse
// FFT; otherwise direct cosine sums (any even S <= R).
// ACC: add to the output buffer's contents (harmonics + noise, decoder.py:132).
// Software pipeline over the frame pairs (round 3): the NEXT pair's filter magnitudes (IRFFT) and THIS pair's output lines (ACC)
// are read at the top of a pair's work and used a whole pair later / at its end -- an HBM read takes ~8000 cycles under this
// kernel's own load, two thirds of a pair's time -- and every global access sits in straight-line code, so that the compiler's
// vmcnt waits are counts, not drains.  An odd last frame is paired with itself (both halves compute and store the same values).
template <int R1, bool IRFFT, bool ACC>
__global__ void __launch_bounds__(64, 2) noise_fft_kernel(NoiseParams p, long npairs)
{
    constexpr int N = 64 * R1, R = N / 2;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    constexpr int NB = buf_elems<R1>();                 // N float2 + the exchange padding
    cf *bufA = reinterpret_cast<cf *>(smem_f);
    cf *bufB = bufA + NB;
    float *ctab = reinterpret_cast<float *>(bufB + NB); // [S] cos(2 pi m / S) (direct impulse responses only)
    const int lane = threadIdx.x;
    const int S = p.S, F = p.F, half = S >> 1;
    const long nframes = (long)p.B * p.T;

    Twiddles<R1> tw;
    make_twiddles<R1>(tw, lane);
    // 512-point transform of the packed impulse responses: its W_512^(lane k1) are the even entries of the N = 1024 table
    // (or the table itself when N = 512): no registers of their own; only its step-2 twiddles are new
    Twiddles<8> tw8;
    if (IRFFT) {
#pragma unroll
        for (int k1 = 0; k1 < 8; ++k1) tw8.t1[k1] = tw.t1[(R1 / 8) * k1];
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) {
            float sn, cs;
            sincospif(2.0f * (float)(((lane >> 3) * k2) & 63) / 64.0f, &sn, &cs);
            tw8.t2[0][k2] = make_float2(cs, -sn);
        }
    } else {
        for (int m = lane; m < S; m += 64) ctab[m] = cospif((float)(2 * m) / (float)S);
    }
    // cos, sin of 2 pi lane / 512 (for the window of z[lane + 64 k3]: 0.5 + 0.5 cos(2 pi lane / 512 + pi k3 / 4))
    const float win_c = tw.t1[(R1 / 8) * 1].x, win_s = -tw.t1[(R1 / 8) * 1].y;
    DDSP_WAVE_ORDER();
    const uint64_t base_off = p.offset + (p.offset_dev ? *p.offset_dev : 0ull);
    constexpr int quads = R >> 2;

    // the packed, Hermitian-extended spectra of a pair: h[n1] = (Ha[src], Hb[src]), bin f = 64 n1 + lane, src = f <= 256 ? f : 512 - f
    struct Mags { float a[8], b[8]; };
    auto load_mags = [&](long pr) {
        const long fa = 2 * pr, fb = (2 * pr + 1 < nframes) ? 2 * pr + 1 : 2 * pr;
        const float *Ha = p.Hm + fa * F, *Hb = p.Hm + fb * F;
        Mags m;
#pragma unroll
        for (int n1 = 0; n1 < 8; ++n1) {
            const int f = 64 * n1 + lane;
            const int src = f <= 256 ? f : 512 - f;
            m.a[n1] = Ha[src];
            m.b[n1] = Hb[src];
        }
        return m;
    };
    typedef float v4 __attribute__((ext_vector_type(4)));
    struct Lines { v4 v[2][R / 256]; };
    // impulse responses built beforehand (ddsp_noise_ir.hip; S < R only): z[n] S of a pair, n = lane + 64 e <= S/2, and the frames' max |H|
    constexpr int ZE = IRFFT ? 1 : R / 128 + 1;
    struct ZRows { float a[ZE], b[ZE], ma, mb; };
    auto load_zrows = [&](long pr) {
        const long fa = 2 * pr, fb = (2 * pr + 1 < nframes) ? 2 * pr + 1 : 2 * pr;
        const float *za = p.zrows + fa * p.zs, *zb = p.zrows + fb * p.zs;
        ZRows z;
#pragma unroll
        for (int e = 0; e < ZE; ++e) {
            const int n = min(lane + 64 * e, half);
            z.a[e] = za[n];
            z.b[e] = zb[n];
        }
        z.ma = za[p.zs - 4];
        z.mb = zb[p.zs - 4];
        return z;
    };
    const bool have_z = !IRFFT && p.zrows != nullptr;

    long pair = blockIdx.x;
    if (pair >= npairs) return;
    Mags hcur;
    if (IRFFT) hcur = load_mags(pair);
    ZRows zcur;
    if (have_z) zcur = load_zrows(pair);
    for (;;) {
        FrameSrc fr[2];
        fr[0].frame = 2 * pair;     fr[0].valid = true;
        fr[1].frame = (2 * pair + 1 < nframes) ? 2 * pair + 1 : 2 * pair;   // an odd last frame is paired with itself
        fr[1].valid = true;
        const long next = pair + gridDim.x;
        Lines yv;
        if (ACC) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int e = 0; e < R / 256; ++e) yv.v[q][e] = reinterpret_cast<const v4 *>(p.y + fr[q].frame * R)[lane + 64 * e];
        }
        Mags hnext;
        if (IRFFT) hnext = load_mags(next < npairs ? next : pair);            // (the last pair re-reads its own: no branch around the loads)
        ZRows znext;
        if (have_z) znext = load_zrows(next < npairs ? next : pair);

        // ---- 1. impulse responses -> kk[j] = k_a[j] + i k_b[j] in bufB[0, R) ----------------------------------
        cf h[8];
        FrameScale sca, scb;                                      // the pair's equalisers; .out carries the 1/(4N) of split + inverse transform
        constexpr float kOut = 1.0f / (4.0f * (float)N);
        if (IRFFT) {
            float ma = 0.0f, mb = 0.0f;
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) { ma = fmaxf(ma, fabsf(hcur.a[n1])); mb = fmaxf(mb, fabsf(hcur.b[n1])); }
            sca = frame_scale(ma, 1.0f, kOut);
            scb = frame_scale(mb, 1.0f, kOut);
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) h[n1] = make_float2(hcur.a[n1] * sca.in, hcur.b[n1] * scb.in);
        }
        if (IRFFT) {
            fft_wave<8, true, false>(h, tw8, bufB, lane);
            // z[n] = h[k3] at n = lane + 64 k3; S == R here: kk[n] = z[n] * window(n), window(n) = 0.5 + 0.5 cos(2 pi n / S)
            // (roll(+S/2), periodic Hann, roll(-S/2)); cos(2 pi lane / 512 + pi k3 / 4) from the lane's twiddle
            constexpr float r8 = 0.70710678118654752f;
            const float ck[8] = {1.0f, r8, 0.0f, -r8, -1.0f, -r8, 0.0f, r8}, sk[8] = {0.0f, r8, 1.0f, r8, 0.0f, -r8, -1.0f, -r8};
#pragma unroll
            for (int k3 = 0; k3 < 8; ++k3) {
                const int n = lane + 64 * k3;
                const int j = n < 256 ? n : n + (R - 512);
                const float wgt = __fmaf_rn(0.5f, win_c * ck[k3] - win_s * sk[k3], 0.5f) * (1.0f / 512.0f);
                bufB[j] = make_float2(h[k3].x * wgt, h[k3].y * wgt);
            }
            if constexpr (R > 512) {
                for (int j = 256 + lane; j < R - 256; j += 64) bufB[j] = make_float2(0.0f, 0.0f);
            }
        } else {
            // direct inverse real DFT (ddsp_noise.hip phase 1): z[n] and z[S/2 - n] from one pass over the bins.  The bins
            // are the same for every lane: they come straight from global memory (wave-uniform addresses -> scalar loads).
            const float *Ha = p.Hm + fr[0].frame * F;
            const float *Hb = p.Hm + (fr[1].valid ? fr[1].frame : fr[0].frame) * F;
            const float vb = fr[1].valid ? 1.0f : 0.0f;
            for (int j = lane; j < R; j += 64) bufB[j] = make_float2(0.0f, 0.0f);
            DDSP_WAVE_ORDER();
            if (have_z) {
                sca = frame_scale(zcur.ma, 1.0f / (float)S, kOut);
                scb = frame_scale(zcur.mb, 1.0f / (float)S, kOut);
            } else {
                float ma = 0.0f, mb = 0.0f;
                for (int k = lane; k < F; k += 64) { ma = fmaxf(ma, fabsf(Ha[k])); mb = fmaxf(mb, fabsf(Hb[k])); }
                sca = frame_scale(ma, 1.0f / (float)S, kOut);
                scb = frame_scale(mb, 1.0f / (float)S, kOut);
            }
            const float invSa = sca.in, invSb = scb.in;
            auto emit = [&](int nn, float za, float zb) {
#pragma unroll
                for (int wrap = 0; wrap < 2; ++wrap) {
                    int src;
                    if (!wrap) { if (nn == half) continue; src = nn + half; }
                    else       { if (nn == 0) continue;    src = half - nn; }
                    const float win = 0.5f - 0.5f * ctab[src];
                    const int jj = !wrap ? nn : (R - nn);       // S <= R: nn <= S/2 < R
                    bufB[jj] = make_float2(za * win, zb * vb * win);
                }
            };
            if (have_z) {
                // z S of both frames was built for the whole batch by one matrix product (ddsp_noise_ir.hip): window and place it
#pragma unroll
                for (int e = 0; e < ZE; ++e) {
                    const int n = lane + 64 * e;
                    if (n <= half) emit(n, zcur.a[e] * invSa, zcur.b[e] * invSb);
                }
            } else {
            const float h0a = Ha[0], hna = Ha[half], h0b = Hb[0], hnb = Hb[half];
            // n = 0 and n = S/2 need no cosines (plain and alternating sums): every lane takes the bins k = lane + 1 + 64 r
            {
                float ea = 0.0f, oa = 0.0f, eb = 0.0f, ob = 0.0f;
                for (int k = 1 + lane; k < half; k += 64) {
                    const float ha = Ha[k], hb = Hb[k];
                    if (k & 1) { oa += ha; ob += hb; } else { ea += ha; eb += hb; }
                }
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
                    ea += __shfl_xor(ea, m); oa += __shfl_xor(oa, m); eb += __shfl_xor(eb, m); ob += __shfl_xor(ob, m);
                }
                if (lane == 0) {
                    const float sg = (half & 1) ? -1.0f : 1.0f;
                    emit(0, __fmaf_rn(2.0f, ea + oa, h0a + hna) * invSa, __fmaf_rn(2.0f, eb + ob, h0b + hnb) * invSb);
                    emit(half, __fmaf_rn(2.0f, ea - oa, h0a + sg * hna) * invSa, __fmaf_rn(2.0f, eb - ob, h0b + sg * hnb) * invSb);
                }
            }
            // n = 1 .. S/4 paired with S/2 - n: cos(2 pi k (S/2 - n) / S) = (-1)^k cos(2 pi k n / S).  Bins two at a time
            // (odd, even), eight per unrolled step, so that the table reads of a step are in flight together.
            for (int n0 = 1; n0 <= half / 2; n0 += 64) {
                const int n = n0 + lane;
                const bool mine = n <= half / 2;
                const int nstep = mine ? n : 0;
                float ea = 0.0f, oa = 0.0f, eb = 0.0f, ob = 0.0f;
                int idx = 0;
                int k = 1;
#pragma unroll 1
                for (; k + 7 < half; k += 8) {
                    float c[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        idx += nstep;
                        if (idx >= S) idx -= S;
                        c[e] = ctab[idx];
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float ha = Ha[k + e], hb = Hb[k + e];
                        if ((e & 1) == 0) { oa = __fmaf_rn(ha, c[e], oa); ob = __fmaf_rn(hb, c[e], ob); }   // k odd (k starts at 1)
                        else              { ea = __fmaf_rn(ha, c[e], ea); eb = __fmaf_rn(hb, c[e], eb); }
                    }
                }
                for (; k < half; ++k) {
                    idx += nstep;
                    if (idx >= S) idx -= S;
                    const float c = ctab[idx];
                    const float ha = Ha[k], hb = Hb[k];
                    if (k & 1) { oa = __fmaf_rn(ha, c, oa); ob = __fmaf_rn(hb, c, ob); }
                    else       { ea = __fmaf_rn(ha, c, ea); eb = __fmaf_rn(hb, c, eb); }
                }
                if (mine) {
                    const int n2 = half - n;
                    const float sg1 = (n & 1) ? -1.0f : 1.0f, sg2 = (n2 & 1) ? -1.0f : 1.0f;
                    emit(n, __fmaf_rn(2.0f, ea + oa, h0a + sg1 * hna) * invSa, __fmaf_rn(2.0f, eb + ob, h0b + sg1 * hnb) * invSb);
                    if (n2 != n) emit(n2, __fmaf_rn(2.0f, ea - oa, h0a + sg2 * hna) * invSa, __fmaf_rn(2.0f, eb - ob, h0b + sg2 * hnb) * invSb);
                }
            }
            }
        }
        DDSP_WAVE_ORDER();

        // ---- 2. noise -> xx[m] = x_a[m] + i x_b[m] in bufA[0, R) -------------------------------------------------
        if (p.u) {
            const float *ua = p.u + fr[0].frame * R;
            const float *ub = p.u + (fr[1].valid ? fr[1].frame : fr[0].frame) * R;
#pragma unroll
            for (int e = 0; e < quads / 64; ++e) {
                const int q = lane + 64 * e;
                const float4 a = *reinterpret_cast<const float4 *>(ua + 4 * q);
                float4 b = *reinterpret_cast<const float4 *>(ub + 4 * q);
                if (!fr[1].valid) b = make_float4(0.5f, 0.5f, 0.5f, 0.5f);
                bufA[4 * q + 0] = make_float2(a.x * 2.0f - 1.0f, b.x * 2.0f - 1.0f);
                bufA[4 * q + 1] = make_float2(a.y * 2.0f - 1.0f, b.y * 2.0f - 1.0f);
                bufA[4 * q + 2] = make_float2(a.z * 2.0f - 1.0f, b.z * 2.0f - 1.0f);
                bufA[4 * q + 3] = make_float2(a.w * 2.0f - 1.0f, b.w * 2.0f - 1.0f);
            }
        } else {
#pragma unroll
            for (int e = 0; e < quads / 64; ++e) {
                const int q = lane + 64 * e;
                uint32_t ra[4], rb[4];
                const uint64_t ca = base_off + (uint64_t)fr[0].frame * (uint64_t)quads + (uint64_t)q;
                const uint64_t cb = base_off + (uint64_t)fr[1].frame * (uint64_t)quads + (uint64_t)q;
                philox4x32_10((uint32_t)ca, (uint32_t)(ca >> 32), (uint32_t)p.seed, (uint32_t)(p.seed >> 32), ra);
                philox4x32_10((uint32_t)cb, (uint32_t)(cb >> 32), (uint32_t)p.seed, (uint32_t)(p.seed >> 32), rb);
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) bufA[4 * q + c4] = make_float2(philox_to_sample(ra[c4]), philox_to_sample(rb[c4]));
            }
        }
        DDSP_WAVE_ORDER();

        // ---- 3. Cx = FFT_N(xx), Ck = FFT_N(kk), natural order in bufA / bufB ---------------------------------------
        cf v[R1];
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) v[n1] = (n1 < R1 / 2) ? bufA[64 * n1 + lane] : make_float2(0.0f, 0.0f);
        DDSP_WAVE_ORDER();
        fft_wave<R1, false, true>(v, tw, bufA, lane);
        store_natural<R1>(v, bufA, lane);
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) v[n1] = (n1 < R1 / 2) ? bufB[64 * n1 + lane] : make_float2(0.0f, 0.0f);
        DDSP_WAVE_ORDER();
        fft_wave<R1, false, true>(v, tw, bufB, lane);
        store_natural<R1>(v, bufB, lane);
        DDSP_WAVE_ORDER();

        // ---- 4. split, multiply, re-pack; inverse FFT ---------------------------------------------------------------
#pragma unroll
        for (int g1 = 0; g1 < R1; ++g1) {
            const int g = 64 * g1 + lane, gm = (g1 == 0) ? ((N - lane) & (N - 1)) : (N - lane) - 64 * g1;
            const cf A = bufA[g], Bc = bufA[gm], E = bufB[g], Fc = bufB[gm];
            const cf B = make_float2(Bc.x, -Bc.y), Fk = make_float2(Fc.x, -Fc.y);
            const cf m1 = cmul(cadd(A, B), cadd(E, Fk));          // 4 X_a K_a
            const cf m2 = cmul(csub(A, B), csub(E, Fk));          // -4 X_b K_b
            // P = (m1 - i m2) / 4 ; the 1/(4N) of split + inverse transform is applied at the output
            v[g1] = make_float2(m1.x + m2.y, m1.y - m2.x);
        }
        DDSP_WAVE_ORDER();
        fft_wave<R1, true, false>(v, tw, bufA, lane);

        // ---- 5. first R samples: y_a = Re, y_b = Im; staged through LDS for whole-line stores ----------------------
        float *ya = reinterpret_cast<float *>(bufB), *yb = ya + R;
        const float kScaleA = sca.out, kScaleB = scb.out;
#pragma unroll
        for (int d = 0; d < R1 / 8; ++d)
#pragma unroll
            for (int k3 = 0; k3 < 4; ++k3) {                      // n = c + 8 R1 k3 < R  <=>  k3 < 4
                const int n = lane + 64 * d + 8 * R1 * k3;
                ya[n] = v[d * 8 + k3].x * kScaleA;
                yb[n] = v[d * 8 + k3].y * kScaleB;
            }
        DDSP_WAVE_ORDER();
        // the next pair's magnitudes change registers HERE, before this pair's stores are issued: their loads are a whole pair old
        // (complete), whereas a wait placed after the stores -- where the compiler would sink these copies -- drains the stores too
        if (IRFFT) {
            hcur = hnext;
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) { asm volatile("" : "+v"(hcur.a[n1])); asm volatile("" : "+v"(hcur.b[n1])); }
        }
        if (have_z) {
            zcur = znext;
#pragma unroll
            for (int e = 0; e < ZE; ++e) { asm volatile("" : "+v"(zcur.a[e])); asm volatile("" : "+v"(zcur.b[e])); }
            asm volatile("" : "+v"(zcur.ma));
            asm volatile("" : "+v"(zcur.mb));
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            v4 *dst = reinterpret_cast<v4 *>(p.y + fr[q].frame * R);
            const v4 *src = reinterpret_cast<const v4 *>(q ? yb : ya);
#pragma unroll
            for (int e = 0; e < R / 256; ++e) {
                v4 o = src[lane + 64 * e];
                if (ACC) o += yv.v[q][e];
                dst[lane + 64 * e] = o;
            }
        }
        DDSP_WAVE_ORDER();
        if (next >= npairs) break;
        pair = next;
    }
}

// =====================================================================================================================
// Backward w.r.t. the filter magnitudes at hop 512 (autograd of filtered_noise.py:7-32; the draw is a constant of the graph),
// the mirror of the forward above, again one wavefront per frame pair and no workgroup barrier:
//   y[n] = sum_{m<=n} x[m] kern[n-m]   =>   d/dkern[j] = sum_d x[d] g[j+d]: a correlation, conj(X) G in the spectrum.
//   1. the SAME noise (Philox counters or the injected draw) -> xx = x_a + i x_b; the upstream gradient rows -> gg = g_a + i g_b
//   2. two N-point FFTs (N = 2R, inputs zero above R), natural order in LDS
//   3. per bin, with A = Cx[g], B = conj Cx[N-g], E = Cg[g], F = conj Cg[N-g]:
//         P[g] = [conj(A + B)(E + F) + i conj(A - B)(E - F)] / 4 = conj(X_a) G_a + i conj(X_b) G_b
//      and ONE inverse FFT gives dk_a + i dk_b; the first R lags are the taps' gradients
//   4. dz[n] = dk[n] window(n) lands exactly in the register layout a 512-point transform takes as input;
//      dH_k = c_k / S Re FFT_S(dz)[k] (z = irfft(H) is a cosine transform of the real, zero-phase H), both frames from ONE
//      packed transform: Re Z_a[k] = (Re Z[k] + Re Z[S-k]) / 2, Re Z_b[k] = (Im Z[k] + Im Z[S-k]) / 2.
// Only S == R = 512 (257 bands, BASELINE.json configs[2]).  Shorter impulse responses (195 bands, the reference's default) stay on
// the direct kernels: their dH step is F x S/2 cosine sums per frame either way, and a built and measured wavefront-per-pair
// version of it was slower than the lane-per-frame batched kernel (1.94 vs 1.36 ms at batch 512 x 375).
struct NoiseFftBwdParams {
    const float *g;      // [B, T*R] upstream gradient
    const float *u;      // [B, T, R] the forward's uniform draw (nullable -> Philox from seed / offset, as the forward)
    float *gH;           // [B, T, F]
    float *dz;           // ZOUT: the gradient of the impulse responses' unique taps, [B*T][zs], n = 0 .. S/2 (ddsp_noise_ir.hip finishes)
    int zs;
    int B, T, F, S;
    uint64_t seed, offset;
    const uint64_t *offset_dev;
};

// ZOUT (S < R: 195 bands, the reference's default): steps 1-3 as above, then dz[n] = dk[n] w(n + S/2) + dk[R - n] w(S/2 - n), n = 0 .. S/2
// (the adjoint of the forward's roll / window / pad / roll, filtered_noise.py:12-20), written -- with the 1/S of the inverse
// transform and the row's 2^e -- to the workspace; dH = dz C^T is then ONE matrix-core product for the whole batch (ddsp_noise_ir.hip)
// instead of F x S/2 cosine sums per frame.
template <bool ZOUT>
__global__ void __launch_bounds__(64, 2) noise_fft_bwd_kernel(NoiseFftBwdParams p, long npairs)
{
    constexpr int R1 = 16, N = 64 * R1, R = N / 2;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    constexpr int NB = buf_elems<R1>();
    cf *bufA = reinterpret_cast<cf *>(smem_f);
    cf *bufB = bufA + NB;
    const int lane = threadIdx.x;
    const int F = p.F;                                   // 257: S = 2 (F - 1) = R
    const long nframes = (long)p.B * p.T;

    Twiddles<R1> tw;
    make_twiddles<R1>(tw, lane);
    Twiddles<8> tw8;
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) tw8.t1[k1] = tw.t1[(R1 / 8) * k1];
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
        float sn, cs;
        sincospif(2.0f * (float)(((lane >> 3) * k2) & 63) / 64.0f, &sn, &cs);
        tw8.t2[0][k2] = make_float2(cs, -sn);
    }
    const float win_c = tw.t1[(R1 / 8) * 1].x, win_s = -tw.t1[(R1 / 8) * 1].y;     // cos, sin of 2 pi lane / 512
    DDSP_WAVE_ORDER();
    const uint64_t base_off = p.offset + (p.offset_dev ? *p.offset_dev : 0ull);
    constexpr int quads = R >> 2;

    // the upstream gradient rows of a pair, read a whole pair ahead (as the forward does with its magnitudes)
    typedef float v4 __attribute__((ext_vector_type(4)));
    struct Rows { v4 a[quads / 64], b[quads / 64]; };
    auto load_rows = [&](long pr) {
        const long ra = 2 * pr, rb = (2 * pr + 1 < nframes) ? 2 * pr + 1 : 2 * pr;
        Rows r;
#pragma unroll
        for (int e = 0; e < quads / 64; ++e) {
            r.a[e] = reinterpret_cast<const v4 *>(p.g + ra * R)[lane + 64 * e];
            r.b[e] = reinterpret_cast<const v4 *>(p.g + rb * R)[lane + 64 * e];
        }
        return r;
    };
    long pair = blockIdx.x;
    if (pair >= npairs) return;
    Rows gcur = load_rows(pair);
    for (;;) {
        const long fa = 2 * pair, fb = (2 * pair + 1 < nframes) ? 2 * pair + 1 : 2 * pair;   // an odd last frame is paired with itself
        const long next = pair + gridDim.x;
        // ---- 1. xx -> bufA[0, R), gg -> bufB[0, R) --------------------------------------------------------------------
        // (rows equalised by powers of two, frame_scale: a quiet frame's gradient does not drown in its partner's rounding)
        float ma = 0.0f, mb = 0.0f;
#pragma unroll
        for (int e = 0; e < quads / 64; ++e)
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) { ma = fmaxf(ma, fabsf(gcur.a[e][c4])); mb = fmaxf(mb, fabsf(gcur.b[e][c4])); }
        const float invS = 1.0f / (float)p.S;
        const FrameScale sca = frame_scale(ma, 1.0f, invS), scb = frame_scale(mb, 1.0f, invS);   // .out: the dH step's 1/S
        const float sa = sca.in, sb = scb.in;
#pragma unroll
        for (int e = 0; e < quads / 64; ++e) {
            const int q = lane + 64 * e;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) bufB[4 * q + c4] = make_float2(gcur.a[e][c4] * sa, gcur.b[e][c4] * sb);
        }
        const Rows gnext = load_rows(next < npairs ? next : pair);                 // (the last pair re-reads its own rows: no branch)
        if (p.u) {
            const float *ua = p.u + fa * R, *ub = p.u + fb * R;
#pragma unroll
            for (int e = 0; e < quads / 64; ++e) {
                const int q = lane + 64 * e;
                const float4 a = *reinterpret_cast<const float4 *>(ua + 4 * q);
                const float4 b = *reinterpret_cast<const float4 *>(ub + 4 * q);
                bufA[4 * q + 0] = make_float2(a.x * 2.0f - 1.0f, b.x * 2.0f - 1.0f);
                bufA[4 * q + 1] = make_float2(a.y * 2.0f - 1.0f, b.y * 2.0f - 1.0f);
                bufA[4 * q + 2] = make_float2(a.z * 2.0f - 1.0f, b.z * 2.0f - 1.0f);
                bufA[4 * q + 3] = make_float2(a.w * 2.0f - 1.0f, b.w * 2.0f - 1.0f);
            }
        } else {
#pragma unroll
            for (int e = 0; e < quads / 64; ++e) {
                const int q = lane + 64 * e;
                uint32_t ra[4], rb[4];
                const uint64_t ca = base_off + (uint64_t)fa * (uint64_t)quads + (uint64_t)q;
                const uint64_t cb = base_off + (uint64_t)fb * (uint64_t)quads + (uint64_t)q;
                philox4x32_10((uint32_t)ca, (uint32_t)(ca >> 32), (uint32_t)p.seed, (uint32_t)(p.seed >> 32), ra);
                philox4x32_10((uint32_t)cb, (uint32_t)(cb >> 32), (uint32_t)p.seed, (uint32_t)(p.seed >> 32), rb);
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) bufA[4 * q + c4] = make_float2(philox_to_sample(ra[c4]), philox_to_sample(rb[c4]));
            }
        }
        DDSP_WAVE_ORDER();

        // ---- 2. Cx = FFT_N(xx), Cg = FFT_N(gg), natural order in bufA / bufB ---------------------------------------------
        cf v[R1];
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) v[n1] = (n1 < R1 / 2) ? bufA[64 * n1 + lane] : make_float2(0.0f, 0.0f);
        DDSP_WAVE_ORDER();
        fft_wave<R1, false, true>(v, tw, bufA, lane);
        store_natural<R1>(v, bufA, lane);
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) v[n1] = (n1 < R1 / 2) ? bufB[64 * n1 + lane] : make_float2(0.0f, 0.0f);
        DDSP_WAVE_ORDER();
        fft_wave<R1, false, true>(v, tw, bufB, lane);
        store_natural<R1>(v, bufB, lane);
        DDSP_WAVE_ORDER();

        // ---- 3. split, correlate, re-pack; inverse FFT -----------------------------------------------------------------
#pragma unroll
        for (int g1 = 0; g1 < R1; ++g1) {
            const int g = 64 * g1 + lane, gm = (g1 == 0) ? ((N - lane) & (N - 1)) : (N - lane) - 64 * g1;
            const cf A = bufA[g], Bc = bufA[gm], E = bufB[g], Fc = bufB[gm];
            const cf U = make_float2(A.x + Bc.x, A.y - Bc.y), W = make_float2(E.x + Fc.x, E.y - Fc.y);      // A + B, E + F
            const cf U2 = make_float2(A.x - Bc.x, A.y + Bc.y), W2 = make_float2(E.x - Fc.x, E.y + Fc.y);    // A - B, E - F
            const cf s1 = make_float2(__fmaf_rn(U.x, W.x, U.y * W.y), __fmaf_rn(U.x, W.y, -(U.y * W.x)));   // conj(U) W
            const cf s2 = make_float2(__fmaf_rn(U2.x, W2.x, U2.y * W2.y), __fmaf_rn(U2.x, W2.y, -(U2.y * W2.x)));
            v[g1] = make_float2(s1.x - s2.y, s1.y + s2.x);        // s1 + i s2; the 1/(4N) is applied below
        }
        DDSP_WAVE_ORDER();
        fft_wave<R1, true, false>(v, tw, bufA, lane);
        constexpr float kScale = 1.0f / (4.0f * (float)N);

        if constexpr (ZOUT) {
            // ---- 4'. dk (both frames) through LDS; every lane folds the two wrapped positions of its taps -------------------
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int k3 = 0; k3 < 4; ++k3) bufB[lane + 64 * (d + 2 * k3)] = v[d * 8 + k3];
            DDSP_WAVE_ORDER();
            const int S = p.S, half = S >> 1;
            float *za = p.dz + fa * p.zs, *zb = p.dz + fb * p.zs;
            const float oa = sca.out * kScale, ob = scb.out * kScale;
#pragma unroll
            for (int e = 0; e < R / 128 + 1; ++e) {
                const int n = lane + 64 * e;
                if (n <= half) {
                    float da = 0.0f, db = 0.0f;
                    if (n < half) {
                        const float w = 0.5f - 0.5f * cospif((float)(2 * (n + half)) / (float)S);
                        const cf t = bufB[n];
                        da = t.x * w; db = t.y * w;
                    }
                    if (n > 0) {
                        const float w = 0.5f - 0.5f * cospif((float)(2 * (half - n)) / (float)S);
                        const cf t = bufB[R - n];
                        da = __fmaf_rn(t.x, w, da); db = __fmaf_rn(t.y, w, db);
                    }
                    za[n] = da * oa;
                    zb[n] = db * ob;
                }
            }
        } else {
            // ---- 4. dz[n] = dk[n] window(n), n = lane + 64 (d + 2 k3): exactly input n1 = d + 2 k3 of the 512-point transform
            constexpr float r8 = 0.70710678118654752f;
            const float ck[8] = {1.0f, r8, 0.0f, -r8, -1.0f, -r8, 0.0f, r8}, sk[8] = {0.0f, r8, 1.0f, r8, 0.0f, -r8, -1.0f, -r8};
            cf h[8];
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int k3 = 0; k3 < 4; ++k3) {
                    const int n1 = d + 2 * k3;
                    const float wgt = __fmaf_rn(0.5f, win_c * ck[n1] - win_s * sk[n1], 0.5f) * kScale;
                    h[n1] = make_float2(v[d * 8 + k3].x * wgt, v[d * 8 + k3].y * wgt);      // (still equalised: one more shared transform)
                }
            fft_wave<8, false, false>(h, tw8, bufB, lane);        // h[k3] = Z[lane + 64 k3]
#pragma unroll
            for (int k3 = 0; k3 < 8; ++k3) bufA[lane + 64 * k3] = h[k3];
            DDSP_WAVE_ORDER();
            float *Ha = p.gH + fa * F, *Hb = p.gH + fb * F;
#pragma unroll
            for (int k3 = 0; k3 < 4; ++k3) {
                const int k = lane + 64 * k3;
                const cf zm = bufA[(512 - k) & 511];
                const float half0 = (k == 0) ? 0.5f : 1.0f;
                Ha[k] = (h[k3].x + zm.x) * (half0 * sca.out);     // c_k / S and the row's 2^e
                Hb[k] = (h[k3].y + zm.y) * (half0 * scb.out);
            }
            if (lane == 0) { Ha[256] = h[4].x * sca.out; Hb[256] = h[4].y * scb.out; }   // c_k / (2 S) (Z[256] + Z[256]) with c_k = 1
        }
        DDSP_WAVE_ORDER();
        if (next >= npairs) break;
        gcur = gnext;
        pair = next;
    }
}

template <int R1, bool IRFFT>
hipError_t launch(const NoiseParams &p, hipStream_t s)
{
    const long nframes = (long)p.B * p.T;
    const long npairs = (nframes + 1) / 2;
    const size_t lds = sizeof(float2) * 2 * buf_elems<R1>() + (IRFFT ? 0 : sizeof(float) * (size_t)p.S);
    int cus = 0;
    const hipError_t e = ddsp_device_cus(&cus);
    if (e != hipSuccess) return e;
    // wavefronts a CU holds of this kernel: registers allow 2 (R1 = 16: 160-224 VGPRs) or 4 (R1 = 8: <= 120) per SIMD, LDS 160 KiB / lds
    const long by_regs = R1 == 16 ? 8 : 16, by_lds = (160 * 1024) / (long)lds;
    long per_cu = by_lds < by_regs ? by_lds : by_regs;
    if (per_cu > 4) per_cu -= per_cu % 4;    // the same number of wavefronts on each of the CU's four SIMDs (measured: 9 per CU is slower than 8)
    // tuning experiments (DDSP_TEST_HOOKS=1 processes only; read once)
    static const long env_waves = [] { const char *ev = getenv("DDSP_NOISE_FFT_WAVES"); return (ev && ddsp_hooks_on()) ? atol(ev) : 0L; }();
    if (env_waves > 0 && env_waves < per_cu) per_cu = env_waves;
    const long resident = (long)cus * per_cu;
    const long grid = npairs < resident ? npairs : resident;
    const int slot = ddsp_prof::begin(ddsp_prof::NOISE, s);
    if (p.accumulate) hipLaunchKernelGGL((noise_fft_kernel<R1, IRFFT, true>), dim3((unsigned)grid), dim3(64), lds, s, p, npairs);
    else hipLaunchKernelGGL((noise_fft_kernel<R1, IRFFT, false>), dim3((unsigned)grid), dim3(64), lds, s, p, npairs);
    ddsp_prof::end(slot, s);
    return hipGetLastError();
}

}  // namespace

namespace ddsp_noise {

hipError_t launch_noise_fft(const NoiseParams &p, hipStream_t s)
{
    if (p.R == 512) return (p.S == 512) ? launch<16, true>(p, s) : launch<16, false>(p, s);
    // hop 256 (N = 512) works and is tested through this entry, but measures no faster than the direct batched kernel there
    // (0.31-0.36 ms against 0.27-0.29 ms at batch 512 x 250 frames, F = 129): the direct form's 128 multiply-adds per sample are
    // already cheaper than three 512-point transforms.  Planned only on request (ddsp_noise_plan.h: kModeFftAtHop256).
    return launch<8, false>(p, s);
}

hipError_t launch_noise_fft_backward(const float *grad_y, const float *uniform, float *grad_H, int B, int T, int F, int hop, uint64_t seed,
                                     uint64_t offset, const uint64_t *offset_dev, void *workspace, hipStream_t s)
{
    NoiseFftBwdParams q;
    q.g = grad_y; q.u = uniform; q.gH = grad_H; q.B = B; q.T = T; q.F = F; q.S = 2 * (F - 1);
    q.dz = nullptr; q.zs = 0;
    q.seed = seed; q.offset = offset; q.offset_dev = offset_dev;
    const long nframes = (long)B * T, npairs = (nframes + 1) / 2;
    const size_t lds = sizeof(float2) * 2 * buf_elems<16>();
    int cus = 0;
    hipError_t e = ddsp_device_cus(&cus);
    if (e != hipSuccess) return e;
    const long resident = (long)cus * 8;                             // 17 KB of LDS each: eight wavefronts per CU
    const long grid = npairs < resident ? npairs : resident;
    if (workspace) {                                                 // 195 bands: dz to the workspace, dH = dz C^T as one product
        q.dz = ir_rows(workspace, F);
        q.zs = ir_row_stride(F);
        e = launch_ir_table(workspace, F, 1, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(noise_fft_bwd_kernel<true>, dim3((unsigned)grid), dim3(64), lds, s, q, npairs);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        return launch_ir_product(q.dz, q.zs, grad_H, F, nullptr, nframes, F, 1, workspace, s);
    }
    hipLaunchKernelGGL(noise_fft_bwd_kernel<false>, dim3((unsigned)grid), dim3(64), lds, s, q, npairs);   // 257 bands: dH inside the kernel
    return hipGetLastError();
}

}  // namespace ddsp_noise
