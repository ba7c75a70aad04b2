// How a sinusoid-bank call is laid out (ddsp_sinusoids.hip: ddsp_sinusoids_forward / ddsp_sinusoids_backward), decided in one place:
// the bits of ddsp_sinusoids_set_form, the limits, the LDS a workgroup stages per iteration, and the planner -- how a row is cut
// into chunks of segments and a chunk into iterations, the grid, the scratch.  Everything that decides and nothing that launches
// (DESIGN.md section 5d).  Plain C++ (no HIP), so that a host program can compile it on its own.
//
// A row of T frames has T segments: segment s holds the hop samples whose phase increment is interpolated between the frames s and
// s + 1 (n = head + s hop + j, head = hop / 2); the last one has only hop - head samples, all at frame T - 1; the head samples in
// front (n < head) are walked with segment 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ddsp_sinusoids {

// ---- ddsp_sinusoids_set_form (include/ddsp_hip.h): tests and A/B runs pass these as numbers -------------------------------------
// There is one kernel form; what the planner decides are lengths, and the hook can force them.  Bits 0-7 are reserved (0).
constexpr int kModeChunkShift = 8;      // bits 8-15: segments per chunk (0: the planner's), rounded up to whole iterations
constexpr int kModeIterShift = 16;      // bits 16-23: segments per iteration (0: the planner's), at most the planner's
constexpr int kModeTileShift = 24;      // bits 24-30: backward, sample records per tile in units of 64 (0: as many as fit)

constexpr int kPlanERange = -2;                  // DDSP_ERANGE (ddsp_sinusoids.hip asserts the equality)
constexpr int kThreads = 256;                    // one workgroup: four wavefronts
constexpr int kMaxGrid = 2048;                   // most workgroups of a launch: eight per CU of an MI355X, each strides over the units
constexpr int kMaxChunksPerRow = 8;              // (each chunk sums the row's segment totals in front of it again: T K fp64 additions)
constexpr int kMaxPartials = 1024, kMaxHop = 1024;
constexpr long kMaxSamples = 1l << 24;           // T hop: sample indices exact in fp32
constexpr size_t kSmallLds = 64 * 1024;          // what the planner aims at: several workgroups share a CU
constexpr size_t kMaxLdsBytes = 160 * 1024;      // a CU's LDS
constexpr int kSlots = 4;                        // a segment's samples reach the frames s - 1 .. s + 2
constexpr size_t kRecordBytes = 32;              // backward: one record per sample of a tile
constexpr int kForwardSamples = 512;             // forward: samples per iteration the planner aims at (two per thread)

inline bool supported(long K, long hop) { return K >= 1 && K <= kMaxPartials && hop >= 1 && hop <= kMaxHop; }

// LDS of an iteration of F segments, in bytes.  Per partial: the carried phase and the row's start phase (fp64); per segment and
// partial its start phase and d / (2 hop) (fp64); g of the F + 1 frames s0 .. s0 + F (fp64); the weights of the F + 3 frames
// s0 - 1 .. s0 + F + 1 (fp32); 16 bytes in front for the highest audible partial, and room to align what follows to 64.
inline size_t staged_lds_bytes(int K, int F) { return (size_t)K * (16 + 16 * (size_t)F + 8 * ((size_t)F + 1) + 4 * ((size_t)F + 3)) + 128; }
// the backward adds grad_a's sums per (segment, slot, partial) and the tile's records
inline size_t backward_lds_bytes(int K, int F, int tile) { return staged_lds_bytes(K, F) + 4 * (size_t)kSlots * F * K + kRecordBytes * (size_t)tile; }

struct Plan {
    int iter_segments;   // F: whole segments that are staged and walked together
    int chunk_segments;  // segments per chunk, a multiple of F; a unit is one chunk of one row
    int chunks;          // per row
    long units;          // B * chunks
    int grid;            // workgroups: min(units, cap)
    int tile;            // backward: sample records in LDS at a time, a multiple of 64
    size_t lds_bytes;
    int status;          // 0, or what the entry point returns instead of launching anything
};

// `live`: the call carries a phase per row and partial in place, so a row is ONE unit (no other workgroup may still need the old
// phases).  `grid_cap`: 0 = kMaxGrid (ddsp_sinusoids_set_grid lowers it).
inline Plan plan(long B, long T, int K, int hop, bool backward, bool live, int mode, int grid_cap)
{
    Plan pl = {1, 1, 1, 0, 1, 64, 0, 0};
    // forward: a thread per sample; backward: a thread per (segment, partial), all of an iteration's in one round where K allows
    long F = backward ? kThreads / K : kForwardSamples / hop;
    if (F < 1) F = 1;
    if (F > T) F = T;
    if (F > 255) F = 255;
    const int want_f = (mode >> kModeIterShift) & 0xff;
    if (want_f > 0 && want_f < F) F = want_f;
    while (F > 1 && (backward ? backward_lds_bytes(K, (int)F, 64) : staged_lds_bytes(K, (int)F)) > kSmallLds) --F;
    pl.iter_segments = (int)F;
    if (backward) {
        const long all = (F * hop + hop / 2 + 63) / 64 * 64;
        long room = ((long)kSmallLds - (long)backward_lds_bytes(K, (int)F, 0)) / (long)kRecordBytes / 64 * 64;
        if (room < 64) room = 64;
        const int want_t = (mode >> kModeTileShift) & 0x7f;
        if (want_t > 0 && want_t * 64 < room) room = want_t * 64;
        pl.tile = (int)(room < all ? room : all);
        pl.lds_bytes = backward_lds_bytes(K, (int)F, pl.tile);
    } else {
        pl.lds_bytes = staged_lds_bytes(K, (int)F);
    }
    if (pl.lds_bytes > kMaxLdsBytes) pl.status = kPlanERange;            // (never within the limits: 84 KB at K = 1024, F = 1)
    long S = live ? 1 : (kMaxGrid + B - 1) / B;
    if (S > kMaxChunksPerRow) S = kMaxChunksPerRow;
    long Tc = (T + S - 1) / S;
    const int want_c = (mode >> kModeChunkShift) & 0xff;
    if (want_c > 0 && !live) Tc = want_c;
    Tc = (Tc + F - 1) / F * F;
    if (Tc > T) Tc = (T + F - 1) / F * F;
    pl.chunk_segments = (int)Tc;
    pl.chunks = (int)((T + Tc - 1) / Tc);
    pl.units = B * pl.chunks;
    const long cap = grid_cap > 0 && grid_cap < kMaxGrid ? grid_cap : kMaxGrid;
    pl.grid = (int)(pl.units < cap ? pl.units : cap);
    return pl;
}

// backward scratch: | part_c [B, T, kSlots, K] | part_a [B, T, kSlots] | part_f [B, T, 3, K] (only with grad_f) |, 256-byte aligned
inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }
inline size_t part_c_bytes(long B, long T, int K) { return round256(sizeof(float) * (size_t)B * T * kSlots * K); }
inline size_t part_a_bytes(long B, long T) { return round256(sizeof(float) * (size_t)B * T * kSlots); }
inline size_t part_f_bytes(long B, long T, int K) { return round256(sizeof(float) * (size_t)B * T * 3 * K); }
inline size_t backward_scratch_bytes(long B, long T, int K, bool grad_f)
{
    return part_c_bytes(B, T, K) + part_a_bytes(B, T) + (grad_f ? part_f_bytes(B, T, K) : 0);
}

}  // namespace ddsp_sinusoids
