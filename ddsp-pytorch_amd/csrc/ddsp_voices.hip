// Polyphony: V monophonic voices per score, each a row of the batch the decoder already handles.
//   voices_allocate_kernel  one wavefront per score row, the lanes are the voices.  The notes are walked in slot order; a tile of 64
//                           records is loaded once (lane j holds note j) and handed round by readlane, so the loop over the notes
//                           touches no memory but the winner's stores.  Each note costs one wave-wide minimum over int64 keys whose
//                           low 6 bits are the voice (a second one where a voice has to be stolen); the voice's state -- the end of
//                           its last note, that note's onset, pitch and level, its count -- stays in the lane's registers.  The rows
//                           are walked grid-strided from a capped grid.
//   voices_mix_kernel       B V rows of audio -> B rows (C channels): a workgroup per tile of up to 1024 samples of one score, a
//                           thread per 4 consecutive samples, the voices summed in ascending order in fp32.  With a gate the tile's
//                           frames (at most 34) get their envelope's numerator first, in LDS as 16-bit integers: a wavefront per
//                           voice looks back for the last active frame 64 frames at a time (a ballot), at most hold + fade frames,
//                           then one more ballot gives every frame of the tile its distance.  One launch, no workspace.
// Every record index is in [0, min(count, N)), every voice slot in [0, Nv), every frame in [0, T) and every sample in [0, L).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"

namespace {

constexpr int kMaxVoices = 64;
constexpr int kMaxRows = 2048;                  // allocate: workgroups in flight, the rows strided over them
constexpr long long kMaxDetune = 1ll << 30;
constexpr long kMaxGap = 1l << 24;
constexpr int kMixThreads = 256;
constexpr int kMixTile = 4 * kMixThreads;       // mix: samples of one workgroup at most
constexpr int kEnvFrames = 34;                  // mix: frames a tile can touch (tile / hop + 2 with the tile at most 32 hops)
constexpr long kMaxLookBack = 1l << 16;         // mix: hold + fade stays below it
constexpr long kMaxHop = 1l << 15;              // mix: fade * hop stays below 2^31

// the smallest key of the wavefront, in every lane
__device__ __forceinline__ long long wave_min(long long k)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long other = __shfl_xor(k, o);
        k = other < k ? other : k;
    }
    return k;
}

// fp32 -> uint32 in the order of the values; a NaN is the largest (a note without a level is never the quietest)
__device__ __forceinline__ unsigned level_order(float x)
{
    const unsigned u = __float_as_uint(x);
    if (x != x) return 0xFFFFFFFFu;
    return u & 0x80000000u ? ~u : u | 0x80000000u;
}

__global__ void __launch_bounds__(64)
voices_allocate_kernel(const int *__restrict__ onset_in, const int *__restrict__ frames_in, const int *__restrict__ pitch_in,
                       const int *__restrict__ detune_in, const float *__restrict__ level_in, const int *__restrict__ count_in,
                       int *__restrict__ onset_out, int *__restrict__ frames_out, int *__restrict__ pitch_out,
                       int *__restrict__ detune_out, float *__restrict__ level_out, int *__restrict__ count_out,
                       int *__restrict__ index_out, int *__restrict__ voice_out, int *__restrict__ slot_out, int *__restrict__ stats_out,
                       long B, int N, int V, int Nv, int assign, int steal, long long gap)
{
    const int lane = threadIdx.x;
    const bool mine = lane < V;
    for (long row = blockIdx.x; row < B; row += gridDim.x) {
        int n = count_in[row];
        n = n < 0 ? 0 : (n > N ? N : n);
        const long src0 = row * (long)N;
        const long dst0 = (row * V + lane) * (long)Nv;                          // (used by the lanes below V only)
        long long until = -(1ll << 31);                                         // the voice: the end of its last note,
        int last_onset = 0, last_pitch = -1, cnt = 0;                           // that note's onset and pitch (-1: never used), its notes
        float last_level = NAN;
        int stolen = 0, dropped = 0;

        for (int i0 = 0; i0 < N; i0 += 64) {
            const int i = i0 + lane;
            const bool in = i < n;
            const int o = in ? onset_in[src0 + i] : 0, f = in ? frames_in[src0 + i] : 0, p = in ? pitch_in[src0 + i] : 0,
                      d = in ? detune_in[src0 + i] : 0;
            const float lv = in ? level_in[src0 + i] : NAN;
            int my_voice = -1, my_slot = -1;
            const int m = n - i0 < 64 ? n - i0 : 64;                            // (<= 0 past the row's notes: only the -1s are written)
            for (int j = 0; j < m; ++j) {
                const int oj = __shfl(o, j), fj = __shfl(f, j), pj = __shfl(p, j);
                const long long dj = __shfl(d, j);
                const float lj = __shfl(lv, j);
                if (fj < 1 || oj < 0 || pj < 0 || pj > 127 || dj < -kMaxDetune || dj > kMaxDetune) continue;      // sounds nowhere
                const bool is_free = mine && until + gap <= (long long)oj;
                long long k = 0;                                                // 'lowest'
                if (assign == 1) {
                    k = until + (1ll << 31);                                    // 'oldest'
                } else if (assign == 2) {
                    const int dist = pj - last_pitch;
                    k = last_pitch < 0 ? 128 : (dist < 0 ? -dist : dist);       // 'nearest'
                }
                long long key = wave_min(is_free ? (k << 6) | lane : LLONG_MAX);
                bool steals = false;
                if (key == LLONG_MAX) {                                         // no voice is free (so every voice has a note)
                    if (steal == 2) {
                        ++dropped;
                        continue;
                    }
                    const long long sk = steal == 0 ? (long long)last_onset : (long long)level_order(last_level);
                    key = wave_min(mine ? (sk << 6) | lane : LLONG_MAX);
                    steals = true;
                    ++stolen;
                }
                const int w = (int)(key & 63);
                int s = -1;
                if (lane == w) {
                    if (steals && cnt > 0 && cnt - 1 < Nv) {                              // the stolen note ends where the new one begins
                        long long cut = (long long)oj - last_onset, had = until - last_onset;
                        cut = cut < had ? cut : had;
                        frames_out[dst0 + cnt - 1] = (int)(cut > 0 ? cut : 0);
                    }
                    if (cnt < Nv) {
                        s = cnt;
                        onset_out[dst0 + s] = oj;
                        frames_out[dst0 + s] = fj;
                        pitch_out[dst0 + s] = pj;
                        detune_out[dst0 + s] = (int)dj;
                        level_out[dst0 + s] = lj;
                        index_out[dst0 + s] = i0 + j;
                    }
                    ++cnt;
                    until = (long long)oj + fj;
                    last_onset = oj;
                    last_pitch = pj;
                    last_level = lj;
                }
                s = __shfl(s, w);
                if (lane == j) {
                    my_voice = w;
                    my_slot = s;
                }
            }
            if (i < N) {
                voice_out[src0 + i] = my_voice;
                slot_out[src0 + i] = my_slot;
            }
        }

        if (mine) count_out[row * V + lane] = cnt;
        for (int v = 0; v < V; ++v) {                                           // the voices' unused slots, a voice row at a time
            int c = __shfl(cnt, v);
            c = c < Nv ? c : Nv;
            const long base = (row * V + v) * (long)Nv;
            for (int s = c + lane; s < Nv; s += 64) {
                onset_out[base + s] = -1;
                frames_out[base + s] = 0;
                pitch_out[base + s] = INT_MIN;
                detune_out[base + s] = 0;
                level_out[base + s] = NAN;
                index_out[base + s] = -1;
            }
        }
        if (lane == 0) {
            stats_out[2 * row] = stolen;
            stats_out[2 * row + 1] = dropped;
        }
    }
}

template <bool kGated, int C>
__global__ void __launch_bounds__(kMixThreads)
voices_mix_kernel(const float *__restrict__ audio, const float *__restrict__ gains, const uint8_t *__restrict__ active,
                  float *__restrict__ out, long L, int V, int T, int hop, int hold, int fade, int S, long tiles, int vec)
{
    __shared__ unsigned short env[kGated ? kMaxVoices * kEnvFrames : 1];
    const long b = blockIdx.x / tiles;
    const long n0 = (long)(blockIdx.x % tiles) * S;
    const long n_end = n0 + S < L ? n0 + S : L;                                 // (n0 < L: tiles = ceil(L / S))
    [[maybe_unused]] int f0 = 0;
    if constexpr (kGated) {
        // the numerator of e[t], in units of 1 / max(fade, 1), for the frames f0 .. f1 the tile reads
        const long q0 = n0 / hop, q1 = (n_end - 1) / hop + 1;
        f0 = (int)(q0 < T - 1 ? q0 : T - 1);
        const int f1 = (int)(q1 < T - 1 ? q1 : T - 1);
        const int nf = f1 - f0 + 1;                                             // <= kEnvFrames: S <= 32 hop or hop >= 32, S <= 1024
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int W = hold + fade, F = fade > 0 ? fade : 1;
        for (int v = wave; v < V; v += kMixThreads / 64) {
            const uint8_t *act = active + (b * V + v) * (long)T;
            int d0 = W + 1;                                                     // frames since the last active one at or before f0
            for (int back = 0; back <= W; back += 64) {
                const int t = f0 - back - lane;
                const bool on = t >= 0 && back + lane <= W && act[t] != 0;
                const unsigned long long m = __ballot(on);
                if (m) {
                    d0 = back + __ffsll((long long)m) - 1;
                    break;
                }
                if (f0 - back - 63 <= 0) break;
            }
            const bool on = lane == 0 ? d0 == 0 : (lane < nf && act[f0 + lane] != 0);
            const unsigned long long m = __ballot(on);
            if (lane < nf) {
                const unsigned long long upto = m & ((2ull << lane) - 1);
                const int d = upto ? lane - (63 - __clzll((long long)upto)) : d0 + lane;
                env[v * kEnvFrames + lane] = (unsigned short)(d <= hold ? F : (d - hold < fade ? fade - (d - hold) : 0));
            }
        }
        __syncthreads();
    }

    const long n = n0 + 4l * threadIdx.x;
    if (n >= n_end) return;
    const bool whole = vec && n + 3 < n_end;                                    // four samples as one 16-byte access
    [[maybe_unused]] int i0[4], i1[4];
    [[maybe_unused]] unsigned r[4];
    [[maybe_unused]] unsigned FH = 0;
    [[maybe_unused]] float inv = 0.0f;
    if constexpr (kGated) {
        unsigned q = (unsigned)n / (unsigned)hop, rem = (unsigned)n - q * (unsigned)hop;     // (n < L < 2^31)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = q < (unsigned)(T - 1) ? (int)q : T - 1;
            i0[k] = t - f0;
            i1[k] = (t + 1 < T ? t + 1 : T - 1) - f0;
            r[k] = rem;
            if (n + k + 1 >= n_end) continue;                                   // (past the tile: the last sample's frames again)
            if (++rem == (unsigned)hop) {
                rem = 0;
                ++q;
            }
        }
        FH = (unsigned)(fade > 0 ? fade : 1) * (unsigned)hop;                   // < 2^31
        inv = 1.0f / (float)FH;
    }

    float acc[C][4];
    for (int v = 0; v < V; ++v) {
        const float *row = audio + (b * V + v) * L + n;
        float a[4];
        if (whole) {
            const float4 x = *reinterpret_cast<const float4 *>(row);
            a[0] = x.x;
            a[1] = x.y;
            a[2] = x.z;
            a[3] = x.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = n + k < n_end ? row[k] : 0.0f;
        }
        [[maybe_unused]] float g[4];
        if constexpr (kGated) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // g = (e0 (hop - r) + e1 r) / hop with e = num / F: an exact integer over F hop
                const unsigned num = env[v * kEnvFrames + i0[k]] * ((unsigned)hop - r[k]) + env[v * kEnvFrames + i1[k]] * r[k];
                g[k] = num == FH ? 1.0f : (float)num * inv;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float gn = gains[(b * V + v) * C + c];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float term;
                if constexpr (kGated) term = (gn * g[k]) * a[k]; else term = gn * a[k];
                acc[c][k] = v == 0 ? term : acc[c][k] + term;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float *dst = out + (b * C + c) * L + n;
        if (whole) {
            *reinterpret_cast<float4 *>(dst) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (n + k < n_end) dst[k] = acc[c][k];
        }
    }
}

}  // namespace

extern "C" int ddsp_voices_allocate(const int *onset, const int *frames, const int *pitch, const int *detune, const float *level,
                                    const int *count, int *v_onset, int *v_frames, int *v_pitch, int *v_detune, float *v_level,
                                    int *v_count, int *index, int *voice, int *slot, int *stats, long B, long N, int V, long Nv,
                                    int assign, int steal, long gap, void *stream)
{
    if (B < 0 || N < 0 || Nv < 0 || V < 1 || V > kMaxVoices || assign < 0 || assign > 2 || steal < 0 || steal > 2 || gap < 0 ||
        gap >= kMaxGap)
        return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!count || !v_count || !stats || (N > 0 && (!onset || !frames || !pitch || !detune || !level || !voice || !slot)) ||
        (Nv > 0 && (!v_onset || !v_frames || !v_pitch || !v_detune || !v_level || !index)))
        return DDSP_EINVAL;
    long total;
    if (__builtin_mul_overflow(B, N, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    if (__builtin_mul_overflow(B, (long)V, &total) || total >= (1l << 31) || __builtin_mul_overflow(total, Nv, &total) ||
        total >= (1l << 31))
        return DDSP_ERANGE;
    hipLaunchKernelGGL(voices_allocate_kernel, dim3((unsigned)(B < kMaxRows ? B : kMaxRows)), dim3(64), 0, (hipStream_t)stream, onset,
                       frames, pitch, detune, level, count, v_onset, v_frames, v_pitch, v_detune, v_level, v_count, index, voice, slot,
                       stats, B, (int)N, V, (int)Nv, assign, steal, (long long)gap);
    return (int)hipGetLastError();
}

extern "C" int ddsp_voices_mix(const float *audio, const float *gains, const uint8_t *active, float *out, long B, int V, int C, long L,
                               long T, long hop, long hold, long fade, void *stream)
{
    if (B < 0 || V < 1 || V > kMaxVoices || (C != 1 && C != 2) || L < 1 || hold < 0 || fade < 0 || hold >= kMaxLookBack ||
        fade >= kMaxLookBack || hold + fade >= kMaxLookBack || (active && (T < 1 || hop < 1)))
        return DDSP_EINVAL;
    if (B == 0) return 0;
    if (!audio || !gains || !out) return DDSP_EINVAL;
    if (L >= (1l << 31) || (active && (hop > kMaxHop || T >= (1l << 31)))) return DDSP_ERANGE;
    const int S = active && hop < 32 ? 32 * (int)hop : kMixTile;                // (a multiple of 4; at most kEnvFrames frames a tile)
    const long tiles = (L + S - 1) / S;
    long total;
    if (__builtin_mul_overflow(B, tiles, &total) || total >= (1l << 31)) return DDSP_ERANGE;
    if (__builtin_mul_overflow(B * (long)V, L, &total) || total >= (1l << 47)) return DDSP_ERANGE;      // (B V <= B tiles V < 2^37)
    if (active && (__builtin_mul_overflow(B * (long)V, T, &total) || total >= (1l << 47))) return DDSP_ERANGE;
    const int vec = L % 4 == 0 && (uintptr_t)audio % 16 == 0 && (uintptr_t)out % 16 == 0;
    auto kernel = active ? (C == 2 ? voices_mix_kernel<true, 2> : voices_mix_kernel<true, 1>)
                         : (C == 2 ? voices_mix_kernel<false, 2> : voices_mix_kernel<false, 1>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * tiles)), dim3(kMixThreads), 0, (hipStream_t)stream, audio, gains, active, out, L, V,
                       (int)T, (int)hop, (int)hold, (int)fade, S, tiles, vec);
    return (int)hipGetLastError();
}
