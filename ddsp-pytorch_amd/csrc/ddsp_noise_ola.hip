// Filtered noise with overlap-add (include/ddsp_hip.h: ddsp_noise_ola_*) -- an opt-in beside the reference's
// truncated form of ddsp_noise.hip.  Every noise sample is filtered by the WHOLE windowed zero-phase response of its own frame:
//   x[b, t hop + j] = fl32(2u - 1)                                                  (philox_to_sample; the truncated form's draw)
//   h_t[e] = (1/2 + 1/2 cos(2 pi e / M)) (1/M) sum_{k<F} c_k H_t[k] cos(2 pi k e / M)    e in (-P, P), P = M/2 = F - 1
//   y[b, n] = sum_m h_{m / hop}[n - m] x[b, m]                                      over 0 <= m < N with |n - m| < P
//   q_t[e]  = sum_{j<hop} x[t hop + j] g[t hop + j + e],   dH_t[k] = (c_k/M) sum_e w(e) cos(2 pi k e / M) q_t[e]
// The tap e = -P has window weight 0 and is not evaluated at all, so a non-finite H_t or g[n] reaches what the other taps reach.
//
// Launches (no atomics, no allocation, no synchronisation; all capturable):
//   forward   cos_sum<IR>  H [frames][F] -> hh [frames][P] in the workspace (the distinct half of the even response)
//             ola_conv     one workgroup per (row, tile of 2048 outputs); a thread owns 8 consecutive outputs and walks the source
//                          samples m in ascending blocks of 8: 16 taps (4 x ds_read_b128, the same address for every lane whose block
//                          lies in the same frame) and 8 samples (2 x ds_read_b128, consecutive across lanes) feed 64 FMAs
//   backward  ola_corr     one workgroup per (row, group of frames); a thread owns 8 consecutive lags and walks j in ascending blocks
//                          of 8 (same register block); lags folded onto d = |e| and windowed -> Gs [frames][P] in the workspace
//             cos_sum<PROJ> Gs -> dH [frames][F]
//   stream    cos_sum<IR>, then ola_stream: ola_conv's tiles and chains over one block of frames, each chain started from the tail the
//             earlier blocks left and stored to the output (with the delayed dry signal) or to the new tail
// Orders (each output is ONE chain of fp32 FMAs from 0): y[n] over m ascending; q_t[e] over j ascending; the cosine sums over the
// inner index 1 .. P - 1 ascending, then the edge terms.  None depends on the batch, the tile or the run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"
#include "ddsp_noise_common.h"

using namespace ddsp_noise;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 8 * kThreads;     // outputs per workgroup of the convolution
constexpr int kMaxF = 257, kMaxHop = 1024;
constexpr size_t kLdsBudget = 64 * 1024;

__host__ __device__ inline int round_up8(int v) { return (v + 7) & ~7; }

// Geometry shared by host and device.  A thread's 8 outputs n0 .. n0 + 7 meet the source blocks m0 = n0 - Pa + 8 j, i.e. the tap
// offsets D = n0 - m0 = Pa, Pa - 8, ..., -Pb; a staged response row holds e in [-C, Pa + 8) at position e + C, zero for |e| >= P.
struct OlaGeom {
    int P, Pa, Pb, C, LEN, RS;
};
__host__ __device__ inline OlaGeom ola_geom(int F)
{
    OlaGeom g;
    g.P = F - 1;
    g.Pa = (g.P - 1 + 7) & ~7;          // >= P - 1
    g.Pb = ((g.P + 6) >> 3) << 3;       // the block that holds m = n0 + 7 + P - 1 starts at n0 + Pb
    g.C = g.Pb + 8;
    g.LEN = g.Pa + g.Pb + 16;
    g.RS = g.LEN + 4;
    return g;
}

// ---- the two cosine sums -----------------------------------------------------------------------------------------------------------
// IR   (in = H  [frames][P + 1], out = hh [frames][P]):     hh[d] = fl(fl(fma(2, S_d, H[0] + (-1)^d H[P])) / M) * w(d)
// PROJ (in = Gs [frames][P],     out = dH [frames][P + 1]): dH[k] = c_k (1/M) (Gs[0] + S_k)
// with S_o = sum_{i=1}^{P-1} in[i] cos(2 pi o i / M), ascending i, and w(d) = fma(0.5, cospif(2 d / M), 0.5): the window the batched
// truncated kernel forms.  16 frames per workgroup; a thread owns one output index of 4 frames.
constexpr int kCsFrames = 16, kCsStride = kCsFrames + 4;

template <bool IR>
__global__ void __launch_bounds__(kThreads) cos_sum_kernel(const float *__restrict__ in, float *__restrict__ out, long frames, int F)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int P = F - 1, M = 2 * P;
    const int NI = IR ? F : P, NO = IR ? P : F;
    float *ct = smem;                                   // [M] rounded up to a multiple of 4
    float *tile = ct + ((M + 3) & ~3);                  // [NI][kCsStride], transposed
    const int tid = threadIdx.x;
    const long frame0 = (long)blockIdx.x * kCsFrames;
    const int nf = (int)min((long)kCsFrames, frames - frame0);

    for (int m = tid; m < M; m += kThreads) ct[m] = cospif((float)(2 * m) / (float)M);
    for (int f = tid >> 6; f < kCsFrames; f += kThreads / 64)
        for (int i = tid & 63; i < NI; i += 64) tile[i * kCsStride + f] = (f < nf) ? in[(frame0 + f) * NI + i] : 0.0f;
    __syncthreads();

    const float invM = 1.0f / (float)M;
    for (int item = tid; item < NO * (kCsFrames / 4); item += kThreads) {
        const int fq = item / NO, o = item - fq * NO;   // o fastest: a wavefront's tile reads are broadcasts
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int idx = 0;
        const float *tp = tile + kCsStride + 4 * fq;
        for (int i = 1; i < P; ++i, tp += kCsStride) {
            idx += o;
            if (idx >= M) idx -= M;
            const float c = ct[idx];
            const float4 v = *reinterpret_cast<const float4 *>(tp);
            acc[0] = __fmaf_rn(v.x, c, acc[0]); acc[1] = __fmaf_rn(v.y, c, acc[1]);
            acc[2] = __fmaf_rn(v.z, c, acc[2]); acc[3] = __fmaf_rn(v.w, c, acc[3]);
        }
        const float4 v0 = *reinterpret_cast<const float4 *>(tile + 4 * fq);
        const float a0[4] = {v0.x, v0.y, v0.z, v0.w};
        if (IR) {
            const float4 vp = *reinterpret_cast<const float4 *>(tile + P * kCsStride + 4 * fq);
            const float ap[4] = {vp.x, vp.y, vp.z, vp.w};
            const float win = __fmaf_rn(0.5f, ct[o], 0.5f);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (4 * fq + q < nf) {
                    const float edge = a0[q] + ((o & 1) ? -ap[q] : ap[q]);
                    out[(frame0 + 4 * fq + q) * NO + o] = (__fmaf_rn(2.0f, acc[q], edge) * invM) * win;
                }
        } else {
            const float ck = (o == 0 || o == P) ? 1.0f : 2.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (4 * fq + q < nf) out[(frame0 + 4 * fq + q) * NO + o] = ck * invM * (a0[q] + acc[q]);
        }
    }
}

size_t cos_sum_lds(int F, bool ir)
{
    const int M = 2 * (F - 1);
    return (size_t)(((M + 3) & ~3) + (ir ? F : F - 1) * kCsStride) * sizeof(float);
}

// ---- the draw of one window of a row -------------------------------------------------------------------------------------------------
struct OlaDraw {
    const float *u;               // [B][T][hop] nullable
    uint64_t seed, offset;
    const uint64_t *offset_dev;
};

// xs[i] = x[row][first + i] for i in [0, count), 0 outside [0, N): the frames [fa, fb] hold every sample of the window inside the row
__device__ __forceinline__ void stage_draw(float *xs, const OlaDraw &d, long row, int T, int hop, int first, int count, int fa, int fb)
{
    const int tid = threadIdx.x;
    const int N = T * hop;
    if (d.u) {
        const float *ur = d.u + row * (long)N;
        for (int i = tid; i < count; i += kThreads) {
            const int m = first + i;
            xs[i] = (m >= 0 && m < N) ? ur[m] * 2.0f - 1.0f : 0.0f;
        }
        return;
    }
    for (int i = tid; i < count; i += kThreads) {
        const int m = first + i;
        if (m < 0 || m >= N) xs[i] = 0.0f;
    }
    const int quads = (hop + 3) >> 2;
    const uint64_t base = d.offset + (d.offset_dev ? *d.offset_dev : 0ull);
    const int items = (fb - fa + 1) * quads;
    for (int it = tid; it < items; it += kThreads) {
        const int fr = fa + it / quads, q = it - (fr - fa) * quads;
        const int m0 = fr * hop + 4 * q;
        if (m0 + 3 < first || m0 >= first + count) continue;
        const uint64_t ctr = base + (uint64_t)(row * (long)T + fr) * (uint64_t)quads + (uint64_t)q;
        uint32_t r[4];
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)d.seed, (uint32_t)(d.seed >> 32), r);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = m0 + e - first;
            if (4 * q + e < hop && i >= 0 && i < count) xs[i] = philox_to_sample(r[e]);
        }
    }
}

// rows[r][e + C] = h_{fa + r}[e] for e in [-C, Pa + 8), zero for |e| >= P: the even rows the fast path of ola_chains reads
__device__ __forceinline__ void stage_rows(float *rows, const float *hrow0, const OlaGeom &g, int fa, int nrows)
{
    for (int r = 0; r < nrows; ++r)
        for (int q = threadIdx.x; q < g.LEN; q += kThreads) {
            const int e = abs(q - g.C);
            rows[r * g.RS + q] = e < g.P ? hrow0[(long)(fa + r) * g.P + e] : 0.0f;
        }
}

// The chains of a thread's 8 outputs n0 .. n0 + 7 (n0 a multiple of 8, possibly negative) over the sources m in [0, N), ascending, on top
// of what acc holds.  xs[i] = x[xfirst + i]; fa: the frame of max(xfirst, 0), the first staged response row.
template <bool HLDS>
__device__ __forceinline__ void ola_chains(float (&acc)[8], const float *xs, const float *rows, const float *hrow0, const OlaGeom &g,
                                           int n0, int xfirst, int fa, int hop, int N)
{
    const int P = g.P;
    int f = fa, fnext = (fa + 1) * hop;                 // the frame of max(m0, 0), kept by stepping
    const int nblocks = (g.Pa + g.Pb) / 8 + 1;
    for (int j = 0; j < nblocks; ++j) {
        const int m0 = n0 - g.Pa + 8 * j, D = g.Pa - 8 * j;
        if (m0 + 7 < 0) continue;
        if (m0 >= N) break;
        while (fnext <= m0) { ++f; fnext += hop; }
        const float *xp = xs + (m0 - xfirst);
        if (HLDS && m0 >= 0 && m0 + 7 < fnext) {        // the whole block lies in frame f (always, when 8 divides the hop)
            const float *hp = rows + (f - fa) * g.RS + (g.C + D - 8);
            const float4 ha = *reinterpret_cast<const float4 *>(hp);
            const float4 hb = *reinterpret_cast<const float4 *>(hp + 4);
            const float4 hc = *reinterpret_cast<const float4 *>(hp + 8);
            const float4 hd = *reinterpret_cast<const float4 *>(hp + 12);
            const float4 xa = *reinterpret_cast<const float4 *>(xp);
            const float4 xb = *reinterpret_cast<const float4 *>(xp + 4);
            asm volatile("" ::"v"(ha.x));               // keep the (unused) first tap alive so the window stays 4 x ds_read_b128
            const float hw[16] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w, hc.x, hc.y, hc.z, hc.w, hd.x, hd.y, hd.z, hd.w};
            const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
            for (int v = 0; v < 8; ++v)
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = __fmaf_rn(hw[8 + u - v], xv[v], acc[u]);
        } else {
#pragma unroll 1
            for (int v = 0; v < 8; ++v) {
                const int m = m0 + v;
                if (m < 0 || m >= N) continue;
                const int fm = m / hop;
                const float x = xp[v];
                if (HLDS) {
                    const float *hp = rows + (fm - fa) * g.RS + (g.C + D - v);
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc[u] = __fmaf_rn(hp[u], x, acc[u]);
                } else {
                    const float *hp = hrow0 + (long)fm * P;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int e = abs(D + u - v);
                        acc[u] = __fmaf_rn(e < P ? hp[e] : 0.0f, x, acc[u]);
                    }
                }
            }
        }
    }
}

// ---- forward: the convolution --------------------------------------------------------------------------------------------------------
struct OlaConvParams {
    const float *hh;              // [B T][P]
    float *y;                     // [B][T hop]
    OlaDraw draw;
    int T, F, hop, accumulate;
    int rows_cap;                 // HLDS: response rows the LDS was sized for
};

// HLDS: the responses of the frames a tile touches are staged in LDS as zero-padded even rows.  Otherwise (small hops with many
// bands: the rows do not fit) every tap is read from the workspace; same chains, same bits.
template <bool HLDS>
__global__ void __launch_bounds__(kThreads) ola_conv_kernel(OlaConvParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const OlaGeom g = ola_geom(p.F);
    const int hop = p.hop, T = p.T, N = T * hop, P = g.P;
    const int tid = threadIdx.x;
    const int tiles = (N + kTile - 1) / kTile;
    const long row = blockIdx.x / tiles;
    const int tile0 = (int)(blockIdx.x - row * tiles) * kTile;
    const int xfirst = tile0 - g.Pa, xcount = kTile + g.Pa + g.Pb + 8;
    float *xs = smem;                                   // [xcount] (a multiple of 8)
    float *rows = xs + xcount;                          // HLDS: [nrows][RS]
    const int fa = max(xfirst, 0) / hop;
    const int fb = min(min(xfirst + xcount, N) - 1, N - 1) / hop;
    const float *hrow0 = p.hh + row * (long)T * P;

    stage_draw(xs, p.draw, row, T, hop, xfirst, xcount, fa, fb);
    if (HLDS) stage_rows(rows, hrow0, g, fa, min(fb - fa + 1, p.rows_cap));
    __syncthreads();

    const int n0 = tile0 + 8 * tid;
    if (n0 >= N) return;
    float acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.0f;
    ola_chains<HLDS>(acc, xs, rows, hrow0, g, n0, xfirst, fa, hop, N);
    float *dst = p.y + row * (long)N + n0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
        if (n0 + u < N) dst[u] = p.accumulate ? dst[u] + acc[u] : acc[u];
}

// ---- the stream: one block of frames, D = P - 1 samples late, with a carried tail ----------------------------------------------------------
// stream[i] = y[i - D] + dry[i - D] for i in [0, N) (include/ddsp_hip.h).  The block's sources m in [0, N) reach the outputs
// n in [-D, N + P - 1), i.e. the stream samples i = n + D in [0, N + M - 2): the first N leave, the other M - 2 are the new tail.
struct OlaStreamParams {
    const float *hh;              // [B T][P]
    const float *dry;             // [B][T hop] nullable
    float *out;                   // [B][T hop]
    const float *state_in;        // [B][3F - 6]: M - 2 of tail, then D of dry history (null when F == 2)
    float *state_out;
    OlaDraw draw;
    int T, F, hop;
    int rows_cap;
};

// ola_conv_kernel's tiles over n in [-Pa, N + P - 1): they start at a multiple of 8, so the source blocks stay aligned to the frames,
// and the outputs below -D are masked.  A chain starts from the tail's partial sum where there is one.
template <bool HLDS>
__global__ void __launch_bounds__(kThreads) ola_stream_kernel(OlaStreamParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const OlaGeom g = ola_geom(p.F);
    const int hop = p.hop, T = p.T, N = T * hop, P = g.P;
    const int delay = P - 1, L = 2 * P - 2;             // D and the tail's length M - 2
    const int tid = threadIdx.x;
    const int tiles = (N + P - 1 + g.Pa + kTile - 1) / kTile;
    const long row = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - row * tiles);
    const int tile0 = tile * kTile - g.Pa;
    const int xfirst = tile0 - g.Pa, xcount = kTile + g.Pa + g.Pb + 8;      // xfirst < N for every tile: Pa >= P - 1
    float *xs = smem;
    float *rows = xs + xcount;
    const int fa = max(xfirst, 0) / hop;
    const int fb = (min(xfirst + xcount, N) - 1) / hop;
    const float *hrow0 = p.hh + row * (long)T * P;
    const float *tail_in = p.state_in + row * (long)(L + delay), *hist_in = tail_in + L;
    float *tail_out = p.state_out + row * (long)(L + delay), *hist_out = tail_out + L;
    const float *dry = p.dry ? p.dry + row * (long)N : nullptr;

    stage_draw(xs, p.draw, row, T, hop, xfirst, xcount, fa, fb);
    if (HLDS) stage_rows(rows, hrow0, g, fa, min(fb - fa + 1, p.rows_cap));
    if (tile == 0)                                      // the dry history: the last D samples of (old history, this block's dry)
        for (int k = tid; k < delay; k += kThreads) {
            const int src = N - delay + k;
            hist_out[k] = src >= 0 ? (dry ? dry[src] : 0.0f) : hist_in[N + k];
        }
    __syncthreads();

    const int n0 = tile0 + 8 * tid, i0 = n0 + delay;
    if (i0 >= N + L) return;                            // (i0 >= -7: Pa - D < 8)
    float acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = (i0 + u >= 0 && i0 + u < L) ? tail_in[i0 + u] : 0.0f;
    ola_chains<HLDS>(acc, xs, rows, hrow0, g, n0, xfirst, fa, hop, N);
    float *dst = p.out + row * (long)N;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u;
        if (i < 0 || i >= N + L) continue;
        if (i >= N) tail_out[i - N] = acc[u];
        else if (dry) dst[i] = (i < delay ? hist_in[i] : dry[i - delay]) + acc[u];
        else dst[i] = acc[u];
    }
}

// ---- backward: the correlation, folded and windowed ------------------------------------------------------------------------------------
struct OlaCorrParams {
    const float *g;               // [B][T hop]
    float *Gs;                    // [B T][P]
    OlaDraw draw;
    int T, F, hop;
    int fw;                       // frames per workgroup
};

// A thread owns the lags e0 .. e0 + 7, e0 = -Pa + 8 c, of one frame; lags with |e| >= P are computed beside the others and dropped.
__global__ void __launch_bounds__(kThreads) ola_corr_kernel(OlaCorrParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const OlaGeom geo = ola_geom(p.F);
    const int hop = p.hop, T = p.T, N = T * hop, P = geo.P, Pa = geo.Pa;
    const int tid = threadIdx.x;
    const int groups = (T + p.fw - 1) / p.fw;
    const long row = blockIdx.x / groups;
    const int t0 = (int)(blockIdx.x - row * groups) * p.fw;
    const int nfr = min(p.fw, T - t0);
    const int NC = (2 * Pa) / 8 + 1;                    // lag chunks: e0 = -Pa .. Pa
    const int QS = 8 * NC + 1;                          // row stride of the lag buffer
    const int gfirst = t0 * hop - Pa, gcount = round_up8(nfr * hop) + 2 * Pa + 16;
    float *xs = smem;                                   // [fw hop + 8]: the frames' draws, contiguous
    float *gs = xs + round_up8(p.fw * hop) + 8;         // [gcount]: g[gfirst ..], 0 outside the row
    float *qs = gs + round_up8(p.fw * hop) + 2 * Pa + 16;   // [fw][QS]

    stage_draw(xs, p.draw, row, T, hop, t0 * hop, nfr * hop, t0, t0 + nfr - 1);
    const float *gr = p.g + row * (long)N;
    for (int i = tid; i < gcount; i += kThreads) {
        const int n = gfirst + i;
        gs[i] = (n >= 0 && n < N) ? gr[n] : 0.0f;
    }
    __syncthreads();

    for (int item = tid; item < nfr * NC; item += kThreads) {
        const int fr = item / NC, c = item - fr * NC;
        const int e0 = -Pa + 8 * c;
        const float *xp = xs + fr * hop;
        const float *gp = gs + fr * hop + (e0 + Pa);    // g[(t0 + fr) hop + j + e0] at gp[j]
        float acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = 0.0f;
        int j = 0;
        if ((hop & 3) == 0) {                           // 16-byte aligned rows: the register block of the forward
            for (; j + 7 < hop; j += 8) {
                const float4 xa = *reinterpret_cast<const float4 *>(xp + j);
                const float4 xb = *reinterpret_cast<const float4 *>(xp + j + 4);
                const float4 ga = *reinterpret_cast<const float4 *>(gp + j);
                const float4 gb = *reinterpret_cast<const float4 *>(gp + j + 4);
                const float4 gc = *reinterpret_cast<const float4 *>(gp + j + 8);
                const float4 gd = *reinterpret_cast<const float4 *>(gp + j + 12);
                asm volatile("" ::"v"(gd.w));           // keep the window as 4 x ds_read_b128
                const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
                const float gw[16] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w, gc.x, gc.y, gc.z, gc.w, gd.x, gd.y, gd.z, gd.w};
#pragma unroll
                for (int v = 0; v < 8; ++v)
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc[u] = __fmaf_rn(xv[v], gw[u + v], acc[u]);
            }
        }
#pragma unroll 1
        for (; j < hop; ++j) {
            const float x = xp[j];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] = __fmaf_rn(x, gp[j + u], acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) qs[fr * QS + 8 * c + u] = acc[u];
    }
    __syncthreads();

    // Gs[d] = w(d) (q[d] + q[-d]), Gs[0] = w(0) q[0]; q[e] sits at qs[e + Pa]
    const float M = (float)(2 * P);
    float *out = p.Gs + (row * (long)T + t0) * P;
    for (int item = tid; item < nfr * P; item += kThreads) {
        const int fr = item / P, d = item - fr * P;
        const float *q = qs + fr * QS + Pa;
        const float win = __fmaf_rn(0.5f, cospif((float)(2 * d) / M), 0.5f);
        out[(long)fr * P + d] = win * (d ? q[d] + q[-d] : q[0]);
    }
}

int corr_frames_per_group(int F, int hop)
{
    const OlaGeom g = ola_geom(F);
    const int NC = (2 * g.Pa) / 8 + 1;
    int fw = kThreads / NC;
    if (fw < 1) fw = 1;
    if (fw > 16) fw = 16;
    if (fw * hop > 4096) fw = 4096 / hop > 1 ? 4096 / hop : 1;      // (LDS: at most 4096 samples of draw and of gradient)
    return fw;
}

size_t corr_lds(int F, int hop, int fw)
{
    const OlaGeom g = ola_geom(F);
    const int NC = (2 * g.Pa) / 8 + 1, QS = 8 * NC + 1;
    const size_t span = (size_t)round_up8(fw * hop);
    return (span + 8 + span + 2 * (size_t)g.Pa + 16 + (size_t)fw * QS) * sizeof(float);
}

int conv_rows_cap(int F, int hop)
{
    const OlaGeom g = ola_geom(F);
    return (kTile + g.Pa + g.Pb + 8 + hop - 1) / hop + 1;
}

int validate(int B, int T, int F, int hop)
{
    if (F > kMaxF || hop > kMaxHop) return DDSP_ERANGE;
    if ((long)B * T >= (1L << 31) || (long)T * hop >= (1L << 31) - 4 * kTile) return DDSP_ERANGE;
    return 0;
}

}  // namespace

extern "C" size_t ddsp_noise_ola_workspace_bytes(int B, int T, int F, int hop)
{
    if (B <= 0 || T <= 0 || F < 2 || hop <= 0 || validate(B, T, F, hop)) return 0;
    return align256((size_t)B * T * (F - 1) * sizeof(float));
}

extern "C" int ddsp_noise_ola_forward(const float *Hmag, const float *uniform, float *y, int B, int T, int F, int hop, uint64_t seed,
                                      uint64_t offset, const uint64_t *counter_dev, int accumulate, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    if (uniform && counter_dev) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!Hmag || !y || B < 0 || T <= 0 || F < 2 || hop <= 0) return DDSP_EINVAL;
    const int rc = validate(B, T, F, hop);
    if (rc) return rc;
    if (!workspace || workspace_bytes < ddsp_noise_ola_workspace_bytes(B, T, F, hop) || ((uintptr_t)workspace % 4) != 0) return DDSP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long frames = (long)B * T;
    float *hh = (float *)workspace;
    hipLaunchKernelGGL(cos_sum_kernel<true>, dim3((unsigned)((frames + kCsFrames - 1) / kCsFrames)), dim3(kThreads), cos_sum_lds(F, true), s,
                       Hmag, hh, frames, F);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;

    const OlaGeom g = ola_geom(F);
    OlaConvParams p;
    p.hh = hh; p.y = y;
    p.draw = {uniform, seed, offset, counter_dev};
    p.T = T; p.F = F; p.hop = hop; p.accumulate = accumulate;
    p.rows_cap = conv_rows_cap(F, hop);
    const size_t xbytes = (size_t)(kTile + g.Pa + g.Pb + 8) * sizeof(float);
    const size_t staged = xbytes + (size_t)p.rows_cap * g.RS * sizeof(float);
    const long N = (long)T * hop;
    const long blocks = (long)B * ((N + kTile - 1) / kTile);
    if (blocks >= (1L << 31)) return DDSP_ERANGE;
    const dim3 grid((unsigned)blocks);
    if (staged <= kLdsBudget)
        hipLaunchKernelGGL(ola_conv_kernel<true>, grid, dim3(kThreads), staged, s, p);
    else
        hipLaunchKernelGGL(ola_conv_kernel<false>, grid, dim3(kThreads), xbytes, s, p);
    return (int)hipGetLastError();
}

extern "C" size_t ddsp_noise_ola_stream_state_floats(int F)
{
    return (F < 3 || F > kMaxF) ? 0 : (size_t)(3 * F - 6);
}

extern "C" int ddsp_noise_ola_stream(const float *Hmag, const float *uniform, const float *dry, float *out, const float *state_in,
                                     float *state_out, int B, int T, int F, int hop, uint64_t seed, uint64_t offset,
                                     const uint64_t *counter_dev, void *workspace, size_t workspace_bytes, void *stream)
{
    if (uniform && counter_dev) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!Hmag || !out || B < 0 || T <= 0 || F < 2 || hop <= 0) return DDSP_EINVAL;
    if (out == dry || (F > 2 && (!state_in || !state_out || state_in == state_out))) return DDSP_EINVAL;
    const int rc = validate(B, T, F, hop);
    if (rc) return rc;
    if (!workspace || workspace_bytes < ddsp_noise_ola_workspace_bytes(B, T, F, hop) || ((uintptr_t)workspace % 4) != 0) return DDSP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long frames = (long)B * T;
    float *hh = (float *)workspace;
    const OlaGeom g = ola_geom(F);
    const long N = (long)T * hop;
    const long blocks = (long)B * ((N + g.P - 1 + g.Pa + kTile - 1) / kTile);
    if (blocks >= (1L << 31)) return DDSP_ERANGE;
    hipLaunchKernelGGL(cos_sum_kernel<true>, dim3((unsigned)((frames + kCsFrames - 1) / kCsFrames)), dim3(kThreads), cos_sum_lds(F, true), s,
                       Hmag, hh, frames, F);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;

    OlaStreamParams p;
    p.hh = hh; p.dry = dry; p.out = out; p.state_in = state_in; p.state_out = state_out;
    p.draw = {uniform, seed, offset, counter_dev};
    p.T = T; p.F = F; p.hop = hop;
    p.rows_cap = conv_rows_cap(F, hop);
    const size_t xbytes = (size_t)(kTile + g.Pa + g.Pb + 8) * sizeof(float);
    const size_t staged = xbytes + (size_t)p.rows_cap * g.RS * sizeof(float);
    const dim3 grid((unsigned)blocks);
    if (staged <= kLdsBudget)
        hipLaunchKernelGGL(ola_stream_kernel<true>, grid, dim3(kThreads), staged, s, p);
    else
        hipLaunchKernelGGL(ola_stream_kernel<false>, grid, dim3(kThreads), xbytes, s, p);
    return (int)hipGetLastError();
}

extern "C" int ddsp_noise_ola_backward(const float *grad_y, const float *uniform, float *grad_H, int B, int T, int F, int hop, uint64_t seed,
                                       uint64_t offset, const uint64_t *counter_dev, void *workspace, size_t workspace_bytes, void *stream)
{
    if (uniform && counter_dev) return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!grad_y || !grad_H || B < 0 || T <= 0 || F < 2 || hop <= 0) return DDSP_EINVAL;
    const int rc = validate(B, T, F, hop);
    if (rc) return rc;
    if (!workspace || workspace_bytes < ddsp_noise_ola_workspace_bytes(B, T, F, hop) || ((uintptr_t)workspace % 4) != 0) return DDSP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long frames = (long)B * T;
    OlaCorrParams p;
    p.g = grad_y; p.Gs = (float *)workspace;
    p.draw = {uniform, seed, offset, counter_dev};
    p.T = T; p.F = F; p.hop = hop;
    p.fw = corr_frames_per_group(F, hop);
    const size_t lds = corr_lds(F, hop, p.fw);
    hipLaunchKernelGGL(ola_corr_kernel, dim3((unsigned)((long)B * ((T + p.fw - 1) / p.fw))), dim3(kThreads), lds, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(cos_sum_kernel<false>, dim3((unsigned)((frames + kCsFrames - 1) / kCsFrames)), dim3(kThreads), cos_sum_lds(F, false), s,
                       (const float *)workspace, grad_H, frames, F);
    return (int)hipGetLastError();
}
