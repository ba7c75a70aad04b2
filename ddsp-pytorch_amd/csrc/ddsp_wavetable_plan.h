// How a wavetable call is laid out (ddsp_wavetable.hip: ddsp_wavetable_forward / ddsp_wavetable_backward), decided in one place:
// the bits of ddsp_wavetable_set_form, the limits, the LDS image of the tables, and the planner -- which form, how a row is cut
// into chunks and a chunk into iterations, the grid.  Everything that decides and nothing that launches.
// Plain C++ (no HIP), so that a host program can compile it on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ddsp_wavetable {

// ---- ddsp_wavetable_set_form (include/ddsp_hip.h): tests and A/B runs pass these as numbers ---------------------------------------
constexpr int kFormAuto = 0, kFormLds = 1, kFormGlobal = 2;      // bits 0-1
constexpr int kModeChunkShift = 8;      // bits 8-15: frames per chunk (0: the planner's), rounded up to whole iterations
constexpr int kModeIterShift = 16;      // bits 16-23: frames per iteration (0: as many as fit), at most the planner's

constexpr int kPlanERange = -2;                  // DDSP_ERANGE (ddsp_wavetable.hip asserts the equality)
constexpr size_t kMaxLdsBytes = 160 * 1024;      // a CU's LDS: the most one workgroup can ask for
constexpr int kThreads = 1024;                   // one workgroup: 16 wavefronts, a sample per thread and iteration
constexpr int kMaxGrid = 256;                    // most workgroups of a launch (an MI355X's CUs: one resident workgroup each; on a
                                                 // device with fewer the rest queue); a backward has one private grad_W table each
constexpr int kMaxChunksPerRow = 8;
constexpr int kMaxTables = 1024, kMaxTableSize = 65536, kMaxHop = kThreads;
constexpr long kMaxEntries = 1l << 18;           // N L
constexpr long kMaxSamples = 1l << 24;           // T hop: sample indices exact in fp32
constexpr size_t kHeadBytes = 256;               // LDS in front of the image: the wavefronts' fp64 totals
constexpr size_t kRecordBytes = 32;              // backward: one record per sample of an iteration

inline bool supported(long N, long L)
{
    return N >= 1 && N <= kMaxTables && L >= 2 && L <= kMaxTableSize && N * L <= kMaxEntries;
}

// ---- the LDS image: entry-major rows of 16-byte units, [L + 1] rows (row L repeats row 0) of pitch4 units ------------------------
// A lane reads the tables of ITS entry j as whole 16-byte units, four tables at a time; lanes on consecutive samples sit
// s = f0 L / sample_rate entries apart.  A 16-byte read is served in four groups of 16 lanes (not consecutive lanes, but each group
// holds every lane number modulo 16 once) over 64 banks, so a group wants 16 different units modulo 16.  The odd pitch makes
// consecutive entries differ; the skew (one more unit every 16 entries) makes entries 16 apart differ, which the pitch alone maps
// onto one bank group (s = 16 is 500 Hz at 16 kHz and L = 512).  Worked out for s = 1 and s = 16 only; not
// measured.
constexpr int pitch4(int N) { return ((N + 3) / 4) | 1; }
constexpr long image_unit(int j, int P4) { return (long)j * P4 + (j >> 4); }
inline size_t image_bytes(int N, int L) { return 16 * (size_t)(image_unit(L, pitch4(N)) + pitch4(N)); }

inline size_t forward_lds_bytes(int N, int L, bool lds_form) { return kHeadBytes + (lds_form ? image_bytes(N, L) : 0); }
// backward: the tables' image, the workgroup's private grad_W image, and the iteration's records
inline size_t backward_lds_bytes(int N, int L, int iter_samples, bool lds_form)
{
    return kHeadBytes + (lds_form ? 2 * image_bytes(N, L) : 0) + kRecordBytes * (size_t)iter_samples;
}

struct Plan {
    int form;            // kFormLds or kFormGlobal
    int iter_frames;     // whole frames per iteration: iter_frames * hop <= kThreads samples walk together
    int chunk_frames;    // frames per chunk, a multiple of iter_frames; a unit is one chunk of one row
    int chunks;          // per row
    long units;          // B * chunks
    int grid;            // workgroups: min(units, cap), each strides over the units
    int parts;           // backward: lanes that share one (frame, four tables) sum, a power of two <= 64
    size_t lds_bytes;
    int status;          // 0, or what the entry point returns instead of launching anything
};

// `live`: the call carries a phase per row in place, so a row is ONE unit (no other workgroup may still need the old phase).
// `grid_cap`: 0 = kMaxGrid (ddsp_wavetable_set_grid lowers it).
inline Plan plan(long B, long T, int N, int L, int hop, bool backward, bool live, int mode, int grid_cap)
{
    Plan pl = {kFormGlobal, 1, 1, 1, 0, 1, 1, 0, 0};
    const int fit = kThreads / hop;                                      // (hop <= kMaxHop: >= 1)
    int F = (long)fit < T ? fit : (int)T;
    const int want_f = (mode >> kModeIterShift) & 0xff;
    if (want_f > 0 && want_f < F) F = want_f;
    // backward: LDS atomics into the private table are worth shorter iterations (fewer records), where that makes the two images fit
    if (backward && (mode & 3) != kFormGlobal && backward_lds_bytes(N, L, hop, true) <= kMaxLdsBytes)
        while (F > 1 && backward_lds_bytes(N, L, F * hop, true) > kMaxLdsBytes) --F;
    pl.iter_frames = F;
    // chunks: enough units for every workgroup in flight, at most kMaxChunksPerRow (each one sums the row in front of it again)
    long S = live ? 1 : (kMaxGrid + B - 1) / B;
    if (S > kMaxChunksPerRow) S = kMaxChunksPerRow;
    long Tc = (T + S - 1) / S;
    const int want_c = (mode >> kModeChunkShift) & 0xff;
    if (want_c > 0 && !live) Tc = want_c;
    Tc = (Tc + F - 1) / F * F;
    if (Tc > T) Tc = (T + F - 1) / F * F;
    pl.chunk_frames = (int)Tc;
    pl.chunks = (int)((T + Tc - 1) / Tc);
    pl.units = B * pl.chunks;
    const long cap = grid_cap > 0 && grid_cap < kMaxGrid ? grid_cap : kMaxGrid;
    pl.grid = (int)(pl.units < cap ? pl.units : cap);
    // backward: items (frame, unit of four tables or the loudness, part); as many parts as fill the workgroup
    const long groups = (long)F * (pitch4(N) + 1);
    int parts = 1;
    while (parts < 64 && groups * (parts * 2) <= kThreads && parts * 2 <= hop) parts *= 2;
    pl.parts = parts;
    const int iter_samples = F * hop;
    const size_t lds = backward ? backward_lds_bytes(N, L, iter_samples, true) : forward_lds_bytes(N, L, true);
    const int want = mode & 3;
    if (want == kFormLds && lds > kMaxLdsBytes) pl.status = kPlanERange;
    pl.form = want == kFormGlobal || (want != kFormLds && lds > kMaxLdsBytes) ? kFormGlobal : kFormLds;
    pl.lds_bytes = pl.form == kFormLds ? lds
                                       : (backward ? backward_lds_bytes(N, L, iter_samples, false) : forward_lds_bytes(N, L, false));
    return pl;
}

// backward scratch: | part_c [B, T, 3, N] | part_a [B, T, 3] | private grad_W tables [grid][N, L] |, parts 256-byte aligned.
// `grid`: the workgroups of the backward's plan (at most kMaxGrid) -- a row that is one unit (a start phase) never has more.
inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }
inline size_t part_c_bytes(long B, long T, int N) { return round256(sizeof(float) * (size_t)B * T * 3 * N); }
inline size_t part_a_bytes(long B, long T) { return round256(sizeof(float) * (size_t)B * T * 3); }
inline size_t backward_scratch_bytes(long B, long T, int N, int L, int grid)
{
    return part_c_bytes(B, T, N) + part_a_bytes(B, T) + round256(sizeof(float) * (size_t)grid * N * L);
}

// ---- band-limited tables: Q + 1 = log2 L + 1 mip levels M [Q + 1, N, L], two of them read per sample ------
constexpr int kMipMinSize = 16, kMipMaxSize = 4096;                  // L: a power of two in this range
constexpr size_t kMipMaxPrivateBytes = (size_t)512 << 20;           // backward: the private grad_M tables of all workgroups together

inline bool mip_supported(long N, long L)
{
    return supported(N, L) && L >= kMipMinSize && L <= kMipMaxSize && (L & (L - 1)) == 0;
}
// Q + 1, or 0 for a table size that cannot be band-limited
inline int mip_levels(long L)
{
    if (L < kMipMinSize || L > kMipMaxSize || (L & (L - 1)) != 0) return 0;
    int Q = 0;
    while ((1l << Q) < L) ++Q;
    return Q + 1;
}

// The fit rule.  A unit (row, chunk) that hears the levels q_lo .. q_hi + 1 keeps one [L + 1][N] image (the layout above) of each
// behind the scan totals: in the forward the level itself, to read; in the backward the workgroup's private gradient of the level,
// to scatter into, with the iteration's records behind (it reads the levels from memory: images AND private copies of two levels
// are 166 KB at 16 tables of 512 points and fit nowhere).  `budget`: 0 = a CU's LDS.
inline size_t mip_lds_bytes(int N, int L, int levels, bool backward, int iter_samples)
{
    return kHeadBytes + (size_t)levels * image_bytes(N, L) + (backward ? kRecordBytes * (size_t)iter_samples : 0);
}
// the most levels a unit may stage: 0 .. Q + 1; below 2 no unit can take the LDS path (a sample reads two levels)
inline int mip_fit_levels(int N, int L, bool backward, int iter_samples, size_t budget)
{
    const size_t cap = budget > 0 && budget < kMaxLdsBytes ? budget : kMaxLdsBytes;
    const int all = mip_levels(L);
    int n = 0;
    while (n < all && mip_lds_bytes(N, L, n + 1, backward, iter_samples) <= cap) ++n;
    return n;
}

struct MipPlan {
    Plan walk;           // iterations, chunks, grid, parts as in the unlimited plan (its form and lds_bytes are replaced below)
    int levels;          // Q + 1
    int fit;             // levels a unit may stage (0: the memory path for every unit)
};

// mode: ddsp_wavetable_set_form's word.  Form 1 (LDS) wants EVERY level to fit, so that every unit takes the LDS path; form 2 none.
inline MipPlan plan_mip(long B, long T, int N, int L, int hop, bool backward, bool live, int mode, int grid_cap, size_t budget)
{
    MipPlan mp;
    mp.walk = plan(B, T, N, L, hop, backward, live, (mode & ~3) | kFormGlobal, grid_cap);     // (no shortened iterations)
    mp.levels = mip_levels(L);
    const int iter_samples = mp.walk.iter_frames * hop;
    const int want = mode & 3;
    mp.fit = want == kFormGlobal ? 0 : mip_fit_levels(N, L, backward, iter_samples, budget);
    if (mp.fit < 2) mp.fit = 0;
    if (mp.levels == 0 || (want == kFormLds && mp.fit < mp.levels)) mp.walk.status = kPlanERange;
    mp.walk.form = mp.fit ? kFormLds : kFormGlobal;
    mp.walk.lds_bytes = mip_lds_bytes(N, L, mp.fit, backward, iter_samples);
    if (backward) {     // one private [Q + 1, N, L] table per workgroup: fewer workgroups where those would pass kMipMaxPrivateBytes
        const size_t slice = sizeof(float) * (size_t)(mp.levels > 0 ? mp.levels : 1) * N * L;
        const long most = (long)(kMipMaxPrivateBytes / slice);
        if (mp.walk.grid > most) mp.walk.grid = most > 1 ? (int)most : 1;
    }
    return mp;
}

// band-limited backward scratch: | part_c | part_a | private grad_M tables [grid][Q + 1, N, L] | touched-level masks [grid] |
inline size_t mip_private_bytes(int N, int L, int levels, int grid) { return round256(sizeof(float) * (size_t)grid * levels * N * L); }
inline size_t mip_backward_scratch_bytes(long B, long T, int N, int L, int levels, int grid)
{
    return part_c_bytes(B, T, N) + part_a_bytes(B, T) + mip_private_bytes(N, L, levels, grid) + round256(sizeof(uint32_t) * (size_t)grid);
}

}  // namespace ddsp_wavetable
