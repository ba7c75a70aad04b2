// Pitch decoders over CREPE's probabilities beyond the per-frame argmax of ddsp_pitch_decode:
//   pitch_centered_kernel  weighted average of the nine bins around a centre (the intent of encoder.py:95-118: every
//                          probability with its own bin's cents), the centre given or the frame's own torch argmax
//   pitch_viterbi_kernel   the maximum-score path over frames under a triangular +-11-bin transition: T dependent steps
//                          of a 360 x 23 max-plus and the backtrack, in one launch
// and what follows a decoder:
//   pitch_voicing_kernel   periodicity median and hysteresis, loudness gate, median-filtered voiced pitch, unvoiced gaps
//                          kept, held or interpolated: one wavefront per row, one launch
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"

namespace {

constexpr int kBins = 360;
constexpr int kHalf = 4;                        // the average takes bins c - 4 .. c + 4
constexpr int kBand = 11;                       // predecessors k with |k - j| <= 11
constexpr int kCand = 2 * kBand + 1;
constexpr int kThreads = 384;                   // six wavefronts, one thread per state (24 idle)
constexpr int kRow = kBins + 2 * kBand;         // a score row with -inf margins: no bounds test in the candidate loop
constexpr int kGroup = 8;                       // frames per prefetch group; the scores are re-centred once per group
constexpr int kChunk = 64;                      // frames of back-pointers staged in LDS by the workspace form's backtrack
constexpr int kScoreBytes = 2 * kThreads * 4;   // the two score rows open the dynamic LDS block (no static LDS beside it)
constexpr long kLdsBackBytes = 160 * 1024 - kScoreBytes;   // back-pointers stay in LDS up to this: T <= 446
static_assert(kRow <= kThreads, "every thread initialises one word of each score row");

// one wavefront per frame
__global__ void __launch_bounds__(256) pitch_centered_kernel(const float *__restrict__ probs, const int *__restrict__ center,
                                                             float *__restrict__ f0, float *__restrict__ harm,
                                                             float *__restrict__ ncents, int *__restrict__ bins_out, long N)
{
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;                                   // wave-uniform
    const float *p = probs + n * kBins;
    int c;
    if (center) {
        c = center[n];
        c = c < 0 ? 0 : (c >= kBins ? kBins - 1 : c);
    } else {                                              // torch.argmax, as pitch_decode_kernel takes it
        float best = 0.0f;
        c = kBins;
        for (int k = lane; k < kBins; k += 64) {
            const float v = p[k];
            if (c == kBins || takes_over(v, k, best, c)) { best = v; c = k; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int oi = __shfl_xor(c, o);
            if (oi != kBins && (c == kBins || takes_over(ov, oi, best, c))) { best = ov; c = oi; }
        }
    }
    const int k = c + lane - kHalf;
    const float w = (lane <= 2 * kHalf && k >= 0 && k < kBins) ? p[k] : 0.0f;
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int i = 0; i <= 2 * kHalf; ++i) {                // ascending offsets, one fixed order
        const float wi = __shfl(w, i);
        num += (float)(i - kHalf) * wi;
        den += wi;
    }
    const float at_centre = __shfl(w, kHalf);
    if (lane == 0) {
        // the offset is the fp32 quantity; what follows is one lane's work per frame, so it is done in fp64 and rounded once
        const double off = (double)(20.0f * (num / den));
        const double cents = ((double)(20 * c) + 1997.3794084376191) + off;
        f0[n] = (float)(10.0 * exp2(cents / 1200.0));
        ncents[n] = (float)(((double)(20 * c) + off) / 7180.0);   // (cents - cents_map(0)) / (cents_map(359) - cents_map(0))
        harm[n] = at_centre;
        if (bins_out) bins_out[n] = c;
    }
}

// The per-frame hand-off of the scores: only LDS is ordered, so the probabilities prefetched from global memory stay in
// flight across it (a __syncthreads() would drain them at every frame).
__device__ __forceinline__ void lds_handoff()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// One workgroup per row, thread j owns state j.  Frame t reads the scores of frame t - 1 from sc[t & 1] and writes its own
// to sc[(t & 1) ^ 1]: one barrier per frame.  Back-pointers (k - j, one signed byte) go to LDS (kLdsBack) or to the caller's
// workspace [T, 360] of this row.  Once per group of eight frames the maximum of the previous frame's scores is subtracted:
// every wavefront reduces the same row it is about to read, so the constant costs no barrier of its own.
// A CU holds one such workgroup at most, two wavefronts per SIMD: with waves_per_eu the compiler keeps the 23 reads of a
// frame in flight instead of saving registers for an occupancy the kernel cannot use.
template <bool kLdsBack>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 2)))
pitch_viterbi_kernel(const float *__restrict__ probs, const float *__restrict__ log_trans, const float *__restrict__ state_in,
                     float *__restrict__ state_out, int *__restrict__ bins, signed char *__restrict__ workspace, int T)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float (*sc)[kThreads] = (float (*)[kThreads])lds;
    signed char *back_s = (signed char *)lds + kScoreBytes;
    const int j = threadIdx.x;
    const int lane = j & 63;
    const bool live = j < kBins;
    const int jj = live ? j : kBins - 1;        // the idle threads load what thread 359 loads: every load is unconditional, so the
                                                // compiler counts the loads in flight instead of draining them at every frame
    const long row = blockIdx.x;
    const float *p = probs + row * T * kBins;
    signed char *back_g = workspace + (kLdsBack ? 0 : row * T * kBins);
    int *path = bins + row * T;
    const bool carried = state_in != nullptr;

    sc[0][j] = (carried && j >= kBand && j < kBand + kBins) ? state_in[row * kBins + j - kBand] : -INFINITY;
    sc[1][j] = -INFINITY;
    float lt[kCand];
#pragma unroll
    for (int d = 0; d < kCand; ++d) lt[d] = log_trans[jj * kCand + d];
    float pc[kGroup], pn[kGroup];
#pragma unroll
    for (int i = 0; i < kGroup; ++i) pc[i] = p[(long)(i < T ? i : T - 1) * kBins + jj];
    lds_handoff();

    float v = 0.0f;
    for (int t0 = 0; t0 < T; t0 += kGroup) {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const int tn = t0 + kGroup + i;
            pn[i] = p[(long)(tn < T ? tn : T - 1) * kBins + jj];
        }
        float m = 0.0f;
        if (t0 > 0 || carried) {
            m = -INFINITY;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int k = lane + 64 * q;
                if (k < kBins) m = fmaxf(m, sc[0][kBand + k]);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        }
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const int t = t0 + i;
            if (t < T) {                                                 // block-uniform
                if (live) {
                    const float e = logf(fmaxf(pc[i], 1e-30f));          // fmaxf drops a NaN: the frame is uninformative
                    if (t == 0 && !carried) {
                        v = e;                                           // uniform prior, its constant dropped
                    } else {
                        const float *prev = &sc[i & 1][j];
                        float pv[kCand];
#pragma unroll
                        for (int d = 0; d < kCand; ++d) pv[d] = prev[d];  // all reads in flight before the first compare
                        float best = pv[0] + lt[0];
                        int bd = 0;
#pragma unroll
                        for (int d = 1; d < kCand; ++d) {                // ascending: a tie keeps the lower predecessor
                            const float cand = pv[d] + lt[d];
                            if (cand > best) { best = cand; bd = d; }
                        }
                        if (i == 0) best -= m;
                        v = best + e;
                        if (kLdsBack) back_s[t * kBins + j] = (signed char)(bd - kBand);
                        else back_g[(long)t * kBins + j] = (signed char)(bd - kBand);
                    }
                    sc[(i & 1) ^ 1][kBand + j] = v;
                }
                lds_handoff();
            }
        }
        // The next group's probabilities are taken over here, eight frames after their loads were issued.  Making them opaque
        // at this point settles the wait for them once per group; otherwise every frame waits for all loads in flight,
        // the prefetch just issued included.
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            pc[i] = pn[i];
            asm volatile("" : "+v"(pc[i]));
        }
    }
    if (state_out && live) state_out[row * kBins + j] = v;

    // the last frame's best state (ties to the lower one), then the walk back by thread 0
    int s = 0;
    if (j < 64) {
        const float *last = &sc[T & 1][kBand];
        float best = last[lane];
        s = lane;
#pragma unroll
        for (int q = 1; q < 6; ++q) {
            const int k = lane + 64 * q;
            if (k < kBins && last[k] > best) { best = last[k]; s = k; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int os = __shfl_xor(s, o);
            if (ov > best || (ov == best && os < s)) { best = ov; s = os; }
        }
        if (j == 0) path[T - 1] = s;
    }
    if (kLdsBack) {
        if (j == 0) {
            for (int t = T - 1; t > 0; --t) {
                s += back_s[t * kBins + s];
                s = s < 0 ? 0 : (s >= kBins ? kBins - 1 : s);            // (only scores without any finite entry get here)
                path[t - 1] = s;
            }
        }
    } else {
        __syncthreads();                                                 // the workspace stores of every wavefront are visible
        for (int hi = T; hi > 1;) {                                      // frames [lo, hi) staged, walked from the top
            const int lo = hi - kChunk > 1 ? hi - kChunk : 1;
            const int *src = (const int *)(back_g + (long)lo * kBins);
            int *dst = (int *)back_s;
            for (int w = j; w < (hi - lo) * (kBins / 4); w += kThreads) dst[w] = src[w];
            __syncthreads();
            if (j == 0) {
                for (int t = hi - 1; t >= lo; --t) {
                    s += back_s[(t - lo) * kBins + s];
                    s = s < 0 ? 0 : (s >= kBins ? kBins - 1 : s);
                    path[t - 1] = s;
                }
            }
            __syncthreads();
            hi = lo;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ voicing
// ddsp_pitch_voicing: what follows a pitch decoder.  One wavefront per row, three sweeps over tiles
// of 64 frames with a wave-uniform carry from tile to tile:
//   A  forward   periodicity median, hysteresis (a scan over the maps set / clear / keep), gate -> m
//   B  forward   pitch median among the gated frames of the window -> the chosen frame u*, and the last voiced frame so far
//   C  backward  the next voiced frame, then every frame's outputs
// Between the sweeps a row keeps m (one byte per frame between zero margins of four, so that a window needs no bounds
// test), u* and the previous voiced frame (one int each) in LDS, or in the caller's workspace for rows beyond kVoiceLdsFrames.

constexpr int kVoiceHalf = 4;                   // the widest window reaches four frames either side
constexpr int kVoiceSlots = 2 * kVoiceHalf + 1;
constexpr int kVoiceLdsFrames = 4096;           // 9 bytes per frame: 36 KiB of LDS at most
constexpr int kNoFrame = 0x7fffffff;            // "no voiced frame after this one", and the index of a masked median entry
constexpr int kNoneBefore = -2;                 // "no voiced frame before this one"; -1 is the carried state's virtual frame
enum { kKeep = 0, kSet = 1, kClear = 2 };

struct VoiceKey {
    float v;
    int i;
};

__device__ __forceinline__ void key_order(VoiceKey &a, VoiceKey &b)
{
    const bool swap = b.v < a.v || (b.v == a.v && b.i < a.i);
    const VoiceKey lo = swap ? b : a, hi = swap ? a : b;
    a = lo;
    b = hi;
}

// Element (count - 1) div 2 of the nine keys in ascending (value, index) order; the 9 - count masked entries are
// (+inf, kNoFrame) and sort last.  A 25-exchange network; count >= 1 wherever the result is used.
__device__ __forceinline__ VoiceKey lower_median(VoiceKey (&s)[kVoiceSlots], int count)
{
    key_order(s[0], s[3]); key_order(s[1], s[7]); key_order(s[2], s[5]); key_order(s[4], s[8]);
    key_order(s[0], s[7]); key_order(s[2], s[4]); key_order(s[3], s[8]); key_order(s[5], s[6]);
    key_order(s[0], s[2]); key_order(s[1], s[3]); key_order(s[4], s[5]); key_order(s[7], s[8]);
    key_order(s[1], s[4]); key_order(s[3], s[6]); key_order(s[5], s[7]);
    key_order(s[0], s[1]); key_order(s[2], s[4]); key_order(s[3], s[5]); key_order(s[6], s[8]);
    key_order(s[2], s[3]); key_order(s[4], s[5]); key_order(s[6], s[7]);
    key_order(s[1], s[2]); key_order(s[3], s[4]); key_order(s[5], s[6]);
    const int r = (count - 1) >> 1;
    VoiceKey k = s[0];
#pragma unroll
    for (int i = 1; i <= kVoiceHalf; ++i)
        if (r == i) k = s[i];
    return k;
}

// a row's intermediates: two ints per frame, then the m bytes with their margins, rounded up to whole ints
__host__ __device__ __forceinline__ long voicing_row_bytes(long T) { return 8 * T + ((T + 2 * kVoiceHalf + 3) & ~3l); }

template <bool kLds>
__global__ void __launch_bounds__(64)
pitch_voicing_kernel(const float *__restrict__ f0, const float *__restrict__ ncents, const float *__restrict__ period,
                     const float *__restrict__ loud, const float *__restrict__ state_in, float *__restrict__ f0_out,
                     float *__restrict__ n_out, unsigned char *__restrict__ voiced_out, float *__restrict__ period_out,
                     float *__restrict__ state_out, unsigned char *__restrict__ workspace, int T, int half_p, int half_f,
                     float upper, float lower, float silence, int fill)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char voice_lds[];
    const int lane = threadIdx.x;
    const long row = blockIdx.x;
    unsigned char *store = kLds ? voice_lds : workspace + row * voicing_row_bytes(T);
    int *sel = (int *)store;                    // u* of a voiced frame, -1 for an unvoiced one
    int *prv = sel + T;                         // the last voiced frame at or before this one
    unsigned char *mm = store + 8l * T;         // m[t] at mm[t + 4]
    const float *p = period + row * T, *n = ncents + row * T, *f = f0 + row * T;
    const float *ld = loud ? loud + row * T : nullptr;
    const bool carried = state_in != nullptr;
    const float last_n = carried ? state_in[row * 3 + 1] : NAN;
    const float last_f = carried ? state_in[row * 3 + 2] : NAN;

    if (lane < 2 * kVoiceHalf) mm[lane < kVoiceHalf ? lane : T + lane] = 0;

    // A
    int v_carry = carried && state_in[row * 3] != 0.0f;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        VoiceKey s[kVoiceSlots];
        int count = 0;
#pragma unroll
        for (int j = 0; j < kVoiceSlots; ++j) {
            const int d = j - kVoiceHalf, u = t + d;
            const bool ok = in && u >= 0 && u < T && (d < 0 ? -d : d) <= half_p;
            float q = p[ok ? u : 0];
            q = q != q ? 0.0f : q;
            s[j].v = ok ? q : INFINITY;
            s[j].i = ok ? u : kNoFrame;
            count += ok;
        }
        const float ps = lower_median(s, count).v;
        int x = !in ? kKeep : (ps >= upper ? kSet : (ps < lower ? kClear : kKeep));
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {      // inclusive scan: second == keep ? first : second
            const int first = __shfl_up(x, o);
            if (lane >= o && x == kKeep) x = first;
        }
        const int v = x == kKeep ? v_carry : (x == kSet);
        v_carry = __shfl(v, 63);
        if (in) {
            const float nt = n[t];
            const bool m = v && fabsf(nt) < INFINITY && (!ld || ld[t] >= silence);   // a NaN compares false in both tests
            mm[t + kVoiceHalf] = m;
            voiced_out[row * T + t] = m;
            if (period_out) period_out[row * T + t] = ps;
        }
    }
    __syncthreads();

    // B
    int a_carry = (carried && last_n == last_n) ? -1 : kNoneBefore;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        const bool m = in && mm[t + kVoiceHalf];
        VoiceKey s[kVoiceSlots];
        int count = 0;
#pragma unroll
        for (int j = 0; j < kVoiceSlots; ++j) {
            const int d = j - kVoiceHalf, u = t + d;
            const bool ok = m && (d < 0 ? -d : d) <= half_f && mm[u + kVoiceHalf];     // the zero margins bound u
            const float nu = n[ok ? u : 0];
            s[j].v = ok ? nu : INFINITY;
            s[j].i = ok ? u : kNoFrame;
            count += ok;
        }
        const VoiceKey k = lower_median(s, count);
        int a = m ? t : kNoneBefore;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int before = __shfl_up(a, o);
            if (lane >= o) a = max(a, before);
        }
        a = max(a, a_carry);
        a_carry = __shfl(a, 63);
        if (in) {
            sel[t] = m ? k.i : -1;
            prv[t] = a;
        }
    }
    __syncthreads();

    if (state_out && lane == 0) {
        float sn = NAN, sf = NAN;
        if (a_carry >= 0) {
            const int u = sel[a_carry];
            sn = n[u];
            sf = f[u];
        } else if (a_carry == -1) {
            sn = last_n;
            sf = last_f;
        }
        state_out[row * 3] = v_carry ? 1.0f : 0.0f;
        state_out[row * 3 + 1] = sn;
        state_out[row * 3 + 2] = sf;
    }

    // C
    int b_carry = kNoFrame;
    for (int t0 = ((T - 1) >> 6) << 6; t0 >= 0; t0 -= 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        const int own = in ? sel[t] : -1;
        int b = own >= 0 ? t : kNoFrame;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int after = __shfl_down(b, o);
            if (lane + o < 64) b = min(b, after);
        }
        b = min(b, b_carry);
        b_carry = __shfl(b, 0);
        if (!in) continue;
        float nn, ff;
        if (own >= 0) {
            nn = n[own];
            ff = f[own];
        } else {
            const int a = prv[t];
            const bool has_a = a != kNoneBefore, has_b = b != kNoFrame;
            nn = n[t];
            ff = f[t];
            if (fill != DDSP_VOICING_FILL_NONE && (has_a || has_b)) {
                float na = last_n, fa = last_f, nb = 0.0f, fb = 0.0f;
                if (a >= 0) {
                    const int u = sel[a];
                    na = n[u];
                    fa = f[u];
                }
                if (has_b) {
                    const int u = sel[b];
                    nb = n[u];
                    fb = f[u];
                }
                if (fill == DDSP_VOICING_FILL_INTERPOLATE && has_a && has_b) {
                    const float w = (float)(t - a) / (float)(b - a);
                    const float step = (nb - na) * w;                        // three roundings: no contraction in this build
                    nn = na + step;
                    ff = (float)(10.0 * exp2((7180.0 * (double)nn + 1997.3794084376191) / 1200.0));
                } else {
                    nn = has_a ? na : nb;
                    ff = has_a ? fa : fb;
                }
            }
        }
        n_out[row * T + t] = nn;
        f0_out[row * T + t] = ff;
    }
}

}  // namespace

extern "C" int ddsp_pitch_centered(const float *probs, const int *center, float *f0, float *harmonicity, float *normalized_cents,
                                   int *bins_out, long N, void *stream)
{
    if (N == 0) return 0;
    if (!probs || !f0 || !harmonicity || !normalized_cents || N < 0) return DDSP_EINVAL;
    if ((N + 3) / 4 > 2147483647l) return DDSP_ERANGE;
    hipLaunchKernelGGL(pitch_centered_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, probs, center, f0,
                       harmonicity, normalized_cents, bins_out, N);
    return (int)hipGetLastError();
}

extern "C" size_t ddsp_pitch_viterbi_workspace_bytes(long B, long T)
{
    if (B <= 0 || T <= 0 || T * kBins <= kLdsBackBytes) return 0;
    return (size_t)B * (size_t)T * kBins;
}

extern "C" int ddsp_pitch_viterbi(const float *probs, const float *log_trans, const float *state_in, float *state_out, int *bins,
                                  void *workspace, long B, long T, void *stream)
{
    if (B == 0) return 0;
    if (!probs || !log_trans || !bins || B < 0 || T <= 0) return DDSP_EINVAL;
    if (B > 2147483647l || T > 2147483647l / kBins) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    if (T * kBins <= kLdsBackBytes) {
        static bool big_lds[64];
        const hipError_t e = ddsp_allow_big_lds((const void *)pitch_viterbi_kernel<true>, big_lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(pitch_viterbi_kernel<true>, dim3((unsigned)B), dim3(kThreads), (size_t)(kScoreBytes + T * kBins), s, probs, log_trans,
                           state_in, state_out, bins, (signed char *)nullptr, (int)T);
    } else {
        if (!workspace) return DDSP_EINVAL;
        hipLaunchKernelGGL(pitch_viterbi_kernel<false>, dim3((unsigned)B), dim3(kThreads), (size_t)(kScoreBytes + kChunk * kBins), s, probs, log_trans,
                           state_in, state_out, bins, (signed char *)workspace, (int)T);
    }
    return (int)hipGetLastError();
}

extern "C" size_t ddsp_pitch_voicing_workspace_bytes(long B, long T)
{
    if (B <= 0 || T <= kVoiceLdsFrames) return 0;
    return (size_t)B * (size_t)voicing_row_bytes(T);
}

extern "C" int ddsp_pitch_voicing(const float *f0, const float *normalized, const float *periodicity, const float *loudness,
                                  const float *state_in, float *f0_out, float *normalized_out, uint8_t *voiced_out,
                                  float *periodicity_out, float *state_out, void *workspace, long B, long T, int period_window,
                                  int pitch_window, float upper, float lower, float silence, int fill, void *stream)
{
    if (B == 0) return 0;
    if (!f0 || !normalized || !periodicity || !f0_out || !normalized_out || !voiced_out || B < 0 || T <= 0) return DDSP_EINVAL;
    const auto window = [](int w) { return w >= 1 && w <= kVoiceSlots && (w & 1); };
    if (!window(period_window) || !window(pitch_window) || upper < lower) return DDSP_EINVAL;
    if (fill != DDSP_VOICING_FILL_NONE && fill != DDSP_VOICING_FILL_HOLD && fill != DDSP_VOICING_FILL_INTERPOLATE) return DDSP_EINVAL;
    if (T >= (1l << 24) || B > 2147483647l / T) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    const int hp = (period_window - 1) / 2, hf = (pitch_window - 1) / 2;
    if (T <= kVoiceLdsFrames) {
        hipLaunchKernelGGL(pitch_voicing_kernel<true>, dim3((unsigned)B), dim3(64), (size_t)voicing_row_bytes(T), s,
                           f0, normalized, periodicity, loudness, state_in, f0_out, normalized_out, voiced_out, periodicity_out,
                           state_out, (unsigned char *)nullptr, (int)T, hp, hf, upper, lower, silence, fill);
    } else {
        if (!workspace) return DDSP_EINVAL;
        hipLaunchKernelGGL(pitch_voicing_kernel<false>, dim3((unsigned)B), dim3(64), 0, s, f0, normalized, periodicity, loudness,
                           state_in, f0_out, normalized_out, voiced_out, periodicity_out, state_out, (unsigned char *)workspace,
                           (int)T, hp, hf, upper, lower, silence, fill);
    }
    return (int)hipGetLastError();
}
