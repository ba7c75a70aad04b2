// The trainer's batch fetch (train/train.py:48 of the reference: DataLoader(shuffle=True) + collate + host-to-device copy) for a
// training set that lives on the device:
//   gather_batch_kernel   row r of every static input tensor of a step <- row perm[*cursor + r] of the matching resident array,
//                         all arrays (f0, loudness, normalized_cents, audio) in ONE launch
//   advance_cursor_kernel *cursor += rows, behind it on the stream: a captured pair walks the permutation replay by replay
// A pure copy, written as one: the grid is sized by bytes (a row is cut into pieces of PIECE_BYTES, one workgroup per piece, so
// that 16 rows of 352 KB are 688 workgroups and not 16), 16-byte accesses when the row length and both bases allow, a 4-byte path
// otherwise, no LDS.  perm and cursor are device memory: nothing about the batch is known to the host at launch time, so an index
// is checked where it is read -- a position outside perm or an example outside [0, n_examples) is never turned into an address;
// the row is zero-filled and a bit of the error word is set instead.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ddsp_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int PIECE_BYTES = 8192;                       // per workgroup: two 16-byte loads in flight per thread
constexpr int PIECE_FLOATS = PIECE_BYTES / 4;
constexpr int MAX_ARRAYS = DDSP_GATHER_MAX_ARRAYS;

struct GatherPlan {                                     // by value in the kernel's arguments (a captured launch keeps it)
    const float *src[MAX_ARRAYS];
    float *dst[MAX_ARRAYS];
    long row_floats[MAX_ARRAYS];
    long pieces_per_row[MAX_ARRAYS];
    long first_block[MAX_ARRAYS];                       // workgroups of array a start here (arrays in ascending block order)
    int vec4[MAX_ARRAYS];                               // row length a multiple of 4 floats and both bases 16-byte aligned
    int n_arrays;
};

__global__ void __launch_bounds__(THREADS) gather_batch_kernel(GatherPlan plan, const long *__restrict__ perm,
                                                               const long *__restrict__ cursor, long perm_len, long n_examples,
                                                               unsigned *__restrict__ error)
{
    // which array this workgroup copies for: a compile-time walk over the plan (no run-time index into the kernel's arguments)
    const float *src = plan.src[0];
    float *dst = plan.dst[0];
    long n = plan.row_floats[0], per_row = plan.pieces_per_row[0], first = 0;
    int vec4 = plan.vec4[0];
#pragma unroll
    for (int k = 1; k < MAX_ARRAYS; ++k)
        if (k < plan.n_arrays && (long)blockIdx.x >= plan.first_block[k]) {
            src = plan.src[k], dst = plan.dst[k], n = plan.row_floats[k], per_row = plan.pieces_per_row[k];
            first = plan.first_block[k], vec4 = plan.vec4[k];
        }
    const long local = (long)blockIdx.x - first;
    const long r = local / per_row;
    const long piece = local - r * per_row;

    // the row's source: every workgroup of the row reads the same two words (broadcast loads, L2 hits after the first)
    const long c = *cursor;
    long e = -1;
    unsigned bad = 0;
    if (c < 0 || c > perm_len - 1 - r)                  // (r >= 0: no overflow in the subtraction for perm_len >= 0)
        bad = DDSP_GATHER_BAD_CURSOR;
    else {
        e = perm[c + r];
        if (e < 0 || e >= n_examples) bad = DDSP_GATHER_BAD_INDEX;
    }
    if (bad && piece == 0 && threadIdx.x == 0) atomicOr(error, bad);

    const long lo = piece * PIECE_FLOATS;
    const long hi = lo + PIECE_FLOATS < n ? lo + PIECE_FLOATS : n;
    float *__restrict__ out = dst + r * n;
    if (bad) {
        for (long i = lo + threadIdx.x; i < hi; i += THREADS) out[i] = 0.0f;
        return;
    }
    const float *__restrict__ in = src + e * n;
    if (vec4) {
        // lo, hi and n are multiples of 4 here (PIECE_FLOATS is, n is): whole float4s only
        const float4 *__restrict__ in4 = reinterpret_cast<const float4 *>(in);
        float4 *__restrict__ out4 = reinterpret_cast<float4 *>(out);
        const long i0 = lo / 4 + threadIdx.x, i1 = i0 + THREADS, end = hi / 4;
        float4 v0 = {0.0f, 0.0f, 0.0f, 0.0f}, v1 = v0;
        if (i0 < end) v0 = in4[i0];
        if (i1 < end) v1 = in4[i1];
        if (i0 < end) out4[i0] = v0;
        if (i1 < end) out4[i1] = v1;
    } else {
        for (long i = lo + threadIdx.x; i < hi; i += THREADS) out[i] = in[i];
    }
}

__global__ void advance_cursor_kernel(long *cursor, long rows)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *cursor += rows;
}

}  // namespace

extern "C" int ddsp_gather_batch(const void **src, void **dst, const long *row_floats, int n_arrays, const long *perm, long *cursor,
                                 long perm_len, long n_examples, int rows, int advance, unsigned *error, void *stream)
{
    if (n_arrays < 0 || n_arrays > MAX_ARRAYS || rows < 0 || perm_len < 0 || n_examples < 0) return DDSP_EINVAL;
    if (rows == 0 || n_arrays == 0) return 0;
    if (!src || !dst || !row_floats || !perm || !cursor || !error) return DDSP_EINVAL;
    GatherPlan plan;
    plan.n_arrays = n_arrays;
    long blocks = 0;
    for (int a = 0; a < MAX_ARRAYS; ++a) {
        const bool live = a < n_arrays;
        const long n = live ? row_floats[a] : 0;
        if (live && (!src[a] || !dst[a] || n <= 0)) return DDSP_EINVAL;
        if (live && (((uintptr_t)src[a] | (uintptr_t)dst[a]) & 3)) return DDSP_EINVAL;
        if (live && (n > LONG_MAX / 4 / (n_examples > rows ? n_examples : rows))) return DDSP_ERANGE;
        plan.src[a] = live ? (const float *)src[a] : nullptr;
        plan.dst[a] = live ? (float *)dst[a] : nullptr;
        plan.row_floats[a] = n;
        plan.pieces_per_row[a] = live ? (n + PIECE_FLOATS - 1) / PIECE_FLOATS : 1;
        plan.vec4[a] = live && n % 4 == 0 && ((((uintptr_t)src[a] | (uintptr_t)dst[a]) & 15) == 0);
        plan.first_block[a] = blocks;
        if (live) blocks += plan.pieces_per_row[a] * rows;
        if (blocks > INT_MAX) return DDSP_ERANGE;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gather_batch_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, plan, perm, (const long *)cursor, perm_len,
                       n_examples, error);
    if (advance) hipLaunchKernelGGL(advance_cursor_kernel, dim3(1), dim3(64), 0, s, cursor, (long)rows);
    return (int)hipGetLastError();
}
