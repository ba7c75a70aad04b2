// Noise analysis, the inverse of the filtered noise: from a residual the band magnitudes H whose
// FilteredNoise frames have, in expectation, the residual's in-frame autocorrelation.  With M = 2 (F - 1), L = F - 1:
//   tables       AT [F][M], the M non-zero rows of the impulse-response map Amat transposed (row j: offset e = j below M / 2,
//                j - M above, sample d = e or hop + e), and CT [L][F], c_l g[l] cos(pi b l / L): fp64, rounded once.
//   measurement  one workgroup per (row, frame): the frame -> LDS; thread l owns lag l: r[l] = sum_n x[n] x[n + l], n ascending
//                (x[n] is a broadcast, x[n + l] consecutive words).
//   fixed point  one workgroup per four consecutive frames of the flattened [B T] axis, all iterations in one launch.  Every
//                operand is a float4 across the four frames in LDS, so a table entry or a weight is fetched once for four
//                multiply-adds:  rbar (thread l: the frames of the averaging window in ascending order, one division),
//                q = CT rbar (thread b), p = max(S q, 0), H0;  then per iteration  k = AT H (thread j, b ascending),
//                R[l] = 1/3 sum_d (hop - l - d) k[d] k[d + l] over the stored rows in their order (thread l), q = CT R, S, the
//                update.  A frame's arithmetic does not depend on which of the four slots it sits in, so a row's bits do not
//                depend on its batch.
// The two matrix products run on the VALU, one output per thread and four frames.  The matrix-core form was built and measured
// (DESIGN.md section 15): 16 frames per workgroup, both products on v_mfma_f32_16x16x4_f32 (an fp32 MFMA is a k-ordered chain
// of fp32 FMAs, so it gave the same bits), R(H) on the VALU: 2.08 ms against this form's 1.41 ms at 16 x 172 frames, hop 512,
// 195 bands, 16 iterations -- sixteen frames per workgroup leave 172 workgroups for 256 compute units.
//
// The overlap-add model (ddsp_noise_analysis_ola) inverts ddsp_noise_ola_forward with the same three launches.
// Its noise is stationary, so the model has no truncation weights and the measurement may cross frame boundaries (any hop >= 1):
//   tables       HT [F][P], the half response of unit vector b (hh[d] = h[+-d] = sum_b HT[b][d] H[b], P = F - 1: the sum
//                cos_sum_kernel<IR> of ddsp_noise_ola.hip forms), and the same CT.
//   measurement  one workgroup per (row, frame): hop + L - 1 samples -> LDS, zero beyond the row; thread l: r[l] = (hop / c) sum_n
//                x[n] x[n + l] over the c = min(hop, N - t hop - l) products inside the row, n ascending.
//   fixed point  the same tiling and the same rbar, spectrum and update; per iteration hh = HT^T H (thread d, b ascending), laid out
//                as the even response h[e] at e + P - 1, rho[l] = sum_e h[e] h[e + l] (thread l, e ascending: 2P - 1 - l terms),
//                R[l] = fl(hop / 3) rho[l].
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"

namespace {

constexpr int kMaxF = 257;                      // bands: one or two per thread
constexpr int kMaxHop = 1024;                   // frame samples: k of four frames is 16 KiB of LDS
constexpr int kThreads = 256;
constexpr int kTile = 4;                        // frames of one workgroup of the fixed point (the float4 lanes)
constexpr long kMaxGrid = 0x7fffffffl;
constexpr float kTiny = 1.17549435e-38f;        // the smallest normal

// AT[b M + j] and CT[l F + b]
__global__ void nana_tables_kernel(float *__restrict__ AT, float *__restrict__ CT, int F)
{
    const int L = F - 1, M = 2 * L;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const double inv = 1.0 / (double)L;
    if (i < (long)F * M) {
        const int b = (int)(i / M), j = (int)(i - (long)b * M);
        const int e = j < L ? j : j - M;
        const long turn = (((long)b * e) % M + M) % M;          // b e mod M: cos(2 pi b e / M) = cospi(turn / L)
        const double g = 0.5 + 0.5 * cospi((double)e * inv);
        const double cb = (b == 0 || b == F - 1) ? 1.0 : 2.0;
        AT[i] = (float)(g * (cb / (double)M) * cospi((double)turn * inv));
    }
    if (i < (long)L * F) {
        const int l = (int)(i / F), b = (int)(i - (long)l * F);
        const long turn = ((long)b * l) % M;
        const double g = 0.5 + 0.5 * cospi((double)l * inv);
        CT[i] = (float)((l == 0 ? 1.0 : 2.0) * g * cospi((double)turn * inv));
    }
}

// HT[b P + d] = (1/2 + 1/2 cos(pi d / P)) (c_b / M) cos(2 pi b d / M), and nana_tables_kernel's CT[l F + b]
__global__ void nana_ola_tables_kernel(float *__restrict__ HT, float *__restrict__ CT, int F)
{
    const int P = F - 1, M = 2 * P;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)F * P) return;
    const double inv = 1.0 / (double)P;
    {
        const int b = (int)(i / P), d = (int)(i - (long)b * P);
        const long turn = ((long)b * d) % M;
        const double g = 0.5 + 0.5 * cospi((double)d * inv);
        const double cb = (b == 0 || b == F - 1) ? 1.0 : 2.0;
        HT[i] = (float)(g * (cb / (double)M) * cospi((double)turn * inv));
    }
    const int l = (int)(i / F), b = (int)(i - (long)l * F);
    const long turn = ((long)b * l) % M;
    const double g = 0.5 + 0.5 * cospi((double)l * inv);
    CT[i] = (float)((l == 0 ? 1.0 : 2.0) * g * cospi((double)turn * inv));
}

// One workgroup per frame g of [B T]: r[g][l] = sum_{n < hop - l} x[n] x[n + l]
__global__ void __launch_bounds__(kThreads) nana_measure_kernel(const float *__restrict__ x, float *__restrict__ r, int hop, int L)
{
    __shared__ float xs[kMaxHop];
    const long g = blockIdx.x;
    const float *frame = x + g * hop;
    for (int n = threadIdx.x; n < hop; n += kThreads) xs[n] = frame[n];
    __syncthreads();
    for (int l = threadIdx.x; l < L; l += kThreads) {
        float acc = 0.0f;
        const int end = hop - l;
        for (int n = 0; n < end; ++n) acc = __fmaf_rn(xs[n], xs[n + l], acc);
        r[g * L + l] = acc;
    }
}

// One workgroup per frame g = row T + t of [B T]: r[g][l] = (hop / c) sum_{n < c} x[t hop + n] x[t hop + n + l], c = min(hop, N - t hop - l)
// the count of products inside the row (0 where there is none)
__global__ void __launch_bounds__(kThreads) nana_ola_measure_kernel(const float *__restrict__ x, float *__restrict__ r, long T, int hop,
                                                                    int L)
{
    __shared__ float xs[kMaxHop + kMaxF - 2];                   // hop + L - 1 samples from the frame's first on
    const long g = blockIdx.x;
    const long row = g / T, t = g - row * T;
    const long left = (T - t) * hop;                            // samples of the row from this frame on (>= hop)
    const float *src = x + (row * T + t) * hop;
    const int span = hop + L - 1;
    for (int i = threadIdx.x; i < span; i += kThreads) xs[i] = i < left ? src[i] : 0.0f;
    __syncthreads();
    for (int l = threadIdx.x; l < L; l += kThreads) {
        const long rest = left - l;
        const int c = rest < hop ? (rest > 0 ? (int)rest : 0) : hop;
        float acc = 0.0f;
        for (int n = 0; n < c; ++n) acc = __fmaf_rn(xs[n], xs[n + l], acc);
        r[g * L + l] = c > 0 ? acc * ((float)hop / (float)c) : 0.0f;
    }
}

__device__ __forceinline__ float4 fma4(float c, float4 v, float4 acc)
{
    return make_float4(__fmaf_rn(c, v.x, acc.x), __fmaf_rn(c, v.y, acc.y), __fmaf_rn(c, v.z, acc.z), __fmaf_rn(c, v.w, acc.w));
}

// acc += w (a * b), the product rounded on its own
__device__ __forceinline__ float4 wmul4(float w, float4 a, float4 b, float4 acc)
{
    return make_float4(__fmaf_rn(w, __fmul_rn(a.x, b.x), acc.x), __fmaf_rn(w, __fmul_rn(a.y, b.y), acc.y),
                       __fmaf_rn(w, __fmul_rn(a.z, b.z), acc.z), __fmaf_rn(w, __fmul_rn(a.w, b.w), acc.w));
}

// qs = CT Rs, then (all threads) S: P[b] = 1/4 (q[b - 1] + q[b + 1]) + 1/2 q[b] with mirrored ends, handed to `use(b, P)`
template <typename Use>
__device__ __forceinline__ void nana_spectrum(const float *__restrict__ CT, const float4 *Rs, float4 *qs, int F, int L, Use use)
{
    for (int b = threadIdx.x; b < F; b += kThreads) {
        float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int l = 0; l < L; ++l) q = fma4(CT[(long)l * F + b], Rs[l], q);
        qs[b] = q;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < F; b += kThreads) {
        const float4 lo = qs[b == 0 ? 1 : b - 1], hi = qs[b == F - 1 ? F - 2 : b + 1], q = qs[b];
        use(b, make_float4(__fmaf_rn(0.25f, lo.x + hi.x, 0.5f * q.x), __fmaf_rn(0.25f, lo.y + hi.y, 0.5f * q.y),
                           __fmaf_rn(0.25f, lo.z + hi.z, 0.5f * q.z), __fmaf_rn(0.25f, lo.w + hi.w, 0.5f * q.w)));
    }
    __syncthreads();
}

__device__ __forceinline__ float at_least(float v, float floor_) { return v < floor_ ? floor_ : v; }      // keeps a NaN

__device__ __forceinline__ float4 at_least4(float4 v, float f)
{
    return make_float4(at_least(v.x, f), at_least(v.y, f), at_least(v.z, f), at_least(v.w, f));
}

__device__ __forceinline__ float &lane_of(float4 &v, int f) { return f == 0 ? v.x : f == 1 ? v.y : f == 2 ? v.z : v.w; }

// Rs = rbar of the tile's frames g0 .. g0 + 3 (a slot past the last frame holds zeros and is not stored)
__device__ __forceinline__ void nana_rbar(const float *__restrict__ r, float4 *Rs, long g0, long nframes, long T, long half, int L)
{
    for (int l = threadIdx.x; l < L; l += kThreads) {
        float4 mean = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int f = 0; f < kTile; ++f) {
            const long g = g0 + f;
            if (g >= nframes) continue;
            const long row = g / T, t = g - row * T;
            const long lo = t - half < 0 ? 0 : t - half, hi = t + half > T - 1 ? T - 1 : t + half;      // (half <= T: no overflow)
            float acc = 0.0f;
            for (long u = lo; u <= hi; ++u) acc += r[(row * T + u) * L + l];
            lane_of(mean, f) = acc / (float)(hi - lo + 1);
        }
        Rs[l] = mean;
    }
}

// H and p of the tile's frames: consecutive threads, consecutive bands of one frame
__device__ __forceinline__ void nana_store(const float4 *Hs, const float4 *ps, float *__restrict__ H_out, float *__restrict__ p_out,
                                           long g0, long nframes, int F)
{
    for (int i = threadIdx.x; i < kTile * F; i += kThreads) {
        const int f = i / F, b = i - f * F;
        const long g = g0 + f;
        if (g >= nframes) break;
        float4 h = Hs[b], p = ps[b];
        H_out[g * F + b] = lane_of(h, f);
        if (p_out) p_out[g * F + b] = lane_of(p, f);
    }
}

__global__ void __launch_bounds__(kThreads) nana_fixed_point_kernel(const float *__restrict__ r, const float *__restrict__ AT,
                                                                    const float *__restrict__ CT, float *__restrict__ H_out,
                                                                    float *__restrict__ p_out, long T, long nframes, int F, int hop,
                                                                    long half, int iterations, float three_over_hop)
{
    __shared__ float4 ks[kMaxHop];                              // k of the four frames at sample d
    __shared__ float4 Hs[kMaxF], ps[kMaxF], qs[kMaxF], Rs[kMaxF - 1];
    const int L = F - 1, M = 2 * L;
    const int tid = threadIdx.x;
    const long g0 = (long)blockIdx.x * kTile;

    nana_rbar(r, Rs, g0, nframes, T, half, L);
    for (int d = tid; d < hop; d += kThreads) ks[d] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    __syncthreads();

    nana_spectrum(CT, Rs, qs, F, L, [&](int b, float4 P) {
        const float4 p = at_least4(P, 0.0f);
        ps[b] = p;
        Hs[b] = make_float4(sqrtf(p.x * three_over_hop), sqrtf(p.y * three_over_hop), sqrtf(p.z * three_over_hop),
                            sqrtf(p.w * three_over_hop));
    });

    for (int it = 0; it < iterations; ++it) {
        for (int j = tid; j < M; j += kThreads) {               // k = Amat H on the stored rows
            float4 k = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int b = 0; b < F; ++b) k = fma4(AT[(long)b * M + j], Hs[b], k);
            ks[j < L ? j : hop - M + j] = k;
        }
        __syncthreads();
        for (int l = tid; l < L; l += kThreads) {               // R(H)[l]; d + l < hop throughout
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int d = 0; d < L; ++d) acc = wmul4((float)(hop - l - d), ks[d], ks[d + l], acc);
            for (int d = hop - L; d < hop - l; ++d) acc = wmul4((float)(hop - l - d), ks[d], ks[d + l], acc);
            const float third = 1.0f / 3.0f;
            Rs[l] = make_float4(acc.x * third, acc.y * third, acc.z * third, acc.w * third);
        }
        __syncthreads();
        nana_spectrum(CT, Rs, qs, F, L, [&](int b, float4 P) {
            const float4 den = at_least4(P, kTiny), p = ps[b], h = Hs[b];
            Hs[b] = make_float4(h.x * sqrtf(p.x / den.x), h.y * sqrtf(p.y / den.y), h.z * sqrtf(p.z / den.z),
                                h.w * sqrtf(p.w / den.w));
        });
    }

    nana_store(Hs, ps, H_out, p_out, g0, nframes, F);
}

// acc += a * b, lane by lane
__device__ __forceinline__ float4 fmav4(float4 a, float4 b, float4 acc)
{
    return make_float4(__fmaf_rn(a.x, b.x, acc.x), __fmaf_rn(a.y, b.y, acc.y), __fmaf_rn(a.z, b.z, acc.z), __fmaf_rn(a.w, b.w, acc.w));
}

// The overlap-add model's fixed point: nana_fixed_point_kernel's tiling, rbar, spectrum and update around R_ola(H) = hop / 3 rho(H)
__global__ void __launch_bounds__(kThreads) nana_ola_fixed_point_kernel(const float *__restrict__ r, const float *__restrict__ HT,
                                                                        const float *__restrict__ CT, float *__restrict__ H_out,
                                                                        float *__restrict__ p_out, long T, long nframes, int F, long half,
                                                                        int iterations, float three_over_hop, float hop_over_three)
{
    __shared__ float4 hs[2 * kMaxF - 3];                        // h[e] of the four frames at e + P - 1, |e| < P
    __shared__ float4 Hs[kMaxF], ps[kMaxF], qs[kMaxF], Rs[kMaxF - 1];
    const int L = F - 1, P = F - 1;
    const int tid = threadIdx.x;
    const long g0 = (long)blockIdx.x * kTile;

    nana_rbar(r, Rs, g0, nframes, T, half, L);
    __syncthreads();

    nana_spectrum(CT, Rs, qs, F, L, [&](int b, float4 P_) {
        const float4 p = at_least4(P_, 0.0f);
        ps[b] = p;
        Hs[b] = make_float4(sqrtf(p.x * three_over_hop), sqrtf(p.y * three_over_hop), sqrtf(p.z * three_over_hop),
                            sqrtf(p.w * three_over_hop));
    });

    for (int it = 0; it < iterations; ++it) {
        for (int d = tid; d < P; d += kThreads) {               // hh = HT^T H, mirrored into the even response
            float4 k = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int b = 0; b < F; ++b) k = fma4(HT[(long)b * P + d], Hs[b], k);
            hs[P - 1 + d] = k;
            hs[P - 1 - d] = k;
        }
        __syncthreads();
        for (int l = tid; l < L; l += kThreads) {               // rho[l] over e = i - (P - 1) ascending; i + l <= 2P - 2
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const int end = 2 * P - 1 - l;
            for (int i = 0; i < end; ++i) acc = fmav4(hs[i], hs[i + l], acc);
            Rs[l] = make_float4(acc.x * hop_over_three, acc.y * hop_over_three, acc.z * hop_over_three, acc.w * hop_over_three);
        }
        __syncthreads();
        nana_spectrum(CT, Rs, qs, F, L, [&](int b, float4 P_) {
            const float4 den = at_least4(P_, kTiny), p = ps[b], h = Hs[b];
            Hs[b] = make_float4(h.x * sqrtf(p.x / den.x), h.y * sqrtf(p.y / den.y), h.z * sqrtf(p.z / den.z),
                                h.w * sqrtf(p.w / den.w));
        });
    }

    nana_store(Hs, ps, H_out, p_out, g0, nframes, F);
}


// false unless the sizes fit: B T frames within one grid, B T hop and B T F within 2^56 elements
bool nana_sizes(long B, long T, int F, int hop, long *frames)
{
    long n;
    if (__builtin_mul_overflow(B, T, frames) || *frames > kMaxGrid) return false;
    if (__builtin_mul_overflow(*frames, (long)(hop > F ? hop : F), &n) || n > (1l << 56)) return false;
    return true;
}

inline size_t nana_at_bytes(int F) { return align256((size_t)F * 2 * (F - 1) * sizeof(float)); }
inline size_t nana_ct_bytes(int F) { return align256((size_t)F * (F - 1) * sizeof(float)); }

}  // namespace

extern "C" size_t ddsp_noise_analysis_workspace_bytes(long B, long T, int F, int hop)
{
    long frames;
    if (B <= 0 || T <= 0 || F < 2 || F > kMaxF || hop < 2 * (F - 1) || hop > kMaxHop || !nana_sizes(B, T, F, hop, &frames)) return 0;
    return nana_at_bytes(F) + nana_ct_bytes(F) + align256((size_t)frames * (F - 1) * sizeof(float));
}

extern "C" int ddsp_noise_analysis(const float *x, float *H, float *power, void *workspace, long B, long T, int F, int hop,
                                   int average, int iterations, void *stream)
{
    if (B == 0) return 0;
    if (!x || !H || !workspace || B < 0 || T <= 0 || F < 2 || hop <= 0 || average < 1 || !(average & 1) || iterations < 0)
        return DDSP_EINVAL;
    if (((uintptr_t)workspace & 15) != 0) return DDSP_EINVAL;
    long frames;
    if (F > kMaxF || hop < 2 * (F - 1) || hop > kMaxHop || !nana_sizes(B, T, F, hop, &frames)) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    const int L = F - 1;
    float *AT = static_cast<float *>(workspace);
    float *CT = reinterpret_cast<float *>(static_cast<char *>(workspace) + nana_at_bytes(F));
    float *r = reinterpret_cast<float *>(static_cast<char *>(workspace) + nana_at_bytes(F) + nana_ct_bytes(F));
    const long entries = (long)F * 2 * L;
    hipLaunchKernelGGL(nana_tables_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, AT, CT, F);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(nana_measure_kernel, dim3((unsigned)frames), dim3(kThreads), 0, s, x, r, hop, L);
    if ((rc = (int)hipGetLastError())) return rc;
    long half = ((long)average - 1) / 2;
    half = half < T ? half : T;                                 // a window beyond the row is the whole row
    const long tiles = (frames + kTile - 1) / kTile;
    hipLaunchKernelGGL(nana_fixed_point_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, r, AT, CT, H, power, T, frames, F, hop,
                       half, iterations, (float)(3.0 / (double)hop));
    return (int)hipGetLastError();
}

namespace {

// the overlap-add range: ddsp_noise_ola_forward's (sample indices of a row are int there)
bool nana_ola_sizes(long B, long T, int F, int hop, long *frames)
{
    long n;
    if (F > kMaxF || hop > kMaxHop) return false;
    if (__builtin_mul_overflow(B, T, frames) || *frames > kMaxGrid) return false;
    return !__builtin_mul_overflow(T, (long)hop, &n) && n < (1l << 31) - 8192;
}

}  // namespace

extern "C" size_t ddsp_noise_analysis_ola_workspace_bytes(long B, long T, int F, int hop)
{
    long frames;
    if (B <= 0 || T <= 0 || F < 2 || hop <= 0 || !nana_ola_sizes(B, T, F, hop, &frames)) return 0;
    return 2 * nana_ct_bytes(F) + align256((size_t)frames * (F - 1) * sizeof(float));
}

extern "C" int ddsp_noise_analysis_ola(const float *x, float *H, float *power, void *workspace, long B, long T, int F, int hop,
                                       int average, int iterations, void *stream)
{
    if (B == 0) return 0;
    if (!x || !H || !workspace || B < 0 || T <= 0 || F < 2 || hop <= 0 || average < 1 || !(average & 1) || iterations < 0)
        return DDSP_EINVAL;
    if (((uintptr_t)workspace & 15) != 0) return DDSP_EINVAL;
    long frames;
    if (!nana_ola_sizes(B, T, F, hop, &frames)) return DDSP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    const int L = F - 1;
    float *HT = static_cast<float *>(workspace);                // [F][P] and [L][F]: F (F - 1) floats each
    float *CT = reinterpret_cast<float *>(static_cast<char *>(workspace) + nana_ct_bytes(F));
    float *r = reinterpret_cast<float *>(static_cast<char *>(workspace) + 2 * nana_ct_bytes(F));
    const long entries = (long)F * L;
    hipLaunchKernelGGL(nana_ola_tables_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, HT, CT, F);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(nana_ola_measure_kernel, dim3((unsigned)frames), dim3(kThreads), 0, s, x, r, T, hop, L);
    if ((rc = (int)hipGetLastError())) return rc;
    long half = ((long)average - 1) / 2;
    half = half < T ? half : T;
    const long tiles = (frames + kTile - 1) / kTile;
    hipLaunchKernelGGL(nana_ola_fixed_point_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, r, HT, CT, H, power, T, frames, F, half,
                       iterations, (float)(3.0 / (double)hop), (float)((double)hop / 3.0));
    return (int)hipGetLastError();
}
