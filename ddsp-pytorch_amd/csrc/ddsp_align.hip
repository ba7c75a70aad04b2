// Dynamic time warping of two feature sequences: the local costs, the recurrence with back-pointers, the
// walk back and the resampling of the path onto an output timeline, one launch, one wavefront per batch row.
//   The wavefront sweeps strips of 64 rows i of the cost matrix along j, skewed: at step n lane l works on the cell
//   (64 strip + l, n - l), so the 64 cells of a step lie on one anti-diagonal and are independent.  D(i, j - 1) is the lane's own
//   value of the step before, D(i - 1, j) the lower lane's (one shuffle), D(i - 1, j - 1) the value that shuffle brought a step
//   earlier.  Lane 0 takes them from `edge`, the last row of the strip above, which lane 63 overwrites in place 63 columns behind
//   lane 0's reads.  One wavefront needs no barrier: LDS operations of a wavefront execute in order (DDSP_WAVE_ORDER).
//   The lane's row of x_a stays in registers for the strip.  x_b goes through LDS as [j & 127][k] with a row stride of kD + 4
//   floats, an odd multiple of four: a lane reads its column as kD / 4 sixteen-byte reads (a [k][j] layout needs kD four-byte
//   reads, and the single wavefront waits out the latency of each group), the sixteen lanes such a read serves at a time are
//   on sixteen different four-bank groups, and the refill of 64 columns every 64 steps writes with lane = k, consecutive banks.
//   d(i, j) is the difference form, ascending k, one accumulator, every operation rounded on its own.
//   Back-pointers (a byte: 0 diagonal, 1 from (i - 1, j), 2 from (i, j - 1)) go to the workspace in the order they are made,
//   [strip][n][lane]: one 64-byte store per step.  Lane 0 walks back through them into LDS (the walk is bounded by i > 0 / j > 0
//   and never trusts a byte with more than the choice among steps that stay inside the matrix); then all lanes write the path
//   in forward order and resample it in fp64.
//   No feature value reaches an index: the costs are only compared.  No atomics, no allocation, no host synchronisation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddsp_hip.h"
#include "ddsp_internal.h"

namespace {

constexpr int kMaxT = 2048;                     // (analysis.DTW_KERNEL_MAX_FRAMES)
constexpr int kMaxD = 64;                       // (analysis.DTW_KERNEL_MAX_FEATURES)
constexpr int kWin = 128;                       // columns of x_b in LDS: the 64 of this refill and the 64 before

// kD: D rounded up to a multiple of 16.  The features D .. kD - 1 of both operands are zero (the window is cleared once and the
// refill writes k < D only), so they add (0 - 0)^2 = +0 to the accumulator, which changes no bit of it, and the loop over k
// needs no bound.
template <int kD>
__global__ void __launch_bounds__(64) dtw_kernel(const float *__restrict__ x_a, const float *__restrict__ x_b,
                                                 float *__restrict__ pos_a, float *__restrict__ pos_b, int *__restrict__ path,
                                                 int *__restrict__ length, float *__restrict__ cost,
                                                 unsigned char *__restrict__ workspace, int T_a, int T_b, int D, long T_out, long radius,
                                                 float penalty, double tau)
{
    __shared__ float edge[kMaxT];                               // D(64 strip - 1, j)
    constexpr int kStride = kD + 4;
    __shared__ __attribute__((aligned(16))) float bt[kWin * (kMaxD + 4)];   // x_b[j, k] at [j & 127][k], rows of kStride
    __shared__ short2 walk[2 * kMaxT - 1];                      // the path, backwards from the end of the array
    const int lane = threadIdx.x;
    const long row = blockIdx.x;
    const float *a = x_a + row * T_a * D, *b = x_b + row * T_b * D;
    const int strips = (T_a + 63) / 64, steps = T_b + 63, longest = T_a + T_b - 1;
    unsigned char *back = workspace + (size_t)row * strips * steps * 64;
    const long p = T_a - 1, q = T_b - 1, limit = radius * (p > q ? p : q);
    for (int e = lane; e < kWin * kStride; e += 64) bt[e] = 0.0f;

    float cur = INFINITY;
    for (int strip = 0; strip < strips; ++strip) {
        const int i = 64 * strip + lane;
        const bool alive = i < T_a;
        const float *mine = a + (long)(alive ? i : T_a - 1) * D;
        int width = D;
        asm volatile("" : "+s"(width));                         // formed here, not kept in scalar registers across the strips
        float xr[kD];
#pragma unroll
        for (int k = 0; k < kD; ++k) xr[k] = k < width ? mine[k] : 0.0f;
        // The row is taken over here, once: otherwise the first use inside the step loop waits for every memory operation in
        // flight, which from the second step on is the back-pointer store of the step before.
#pragma unroll
        for (int k = 0; k < kD; ++k) asm volatile("" : "+v"(xr[k]));
        float above = INFINITY, diag = INFINITY;
        cur = INFINITY;
        for (int n = 0; n < steps; ++n) {
            if ((n & 63) == 0) {                                // the next 64 columns of x_b; lane = k
                DDSP_WAVE_ORDER();
                for (int c = 0; c < 64; ++c) {
                    const int j = n + c;
                    if (j < T_b && lane < D) bt[(j & (kWin - 1)) * kStride + lane] = b[(long)j * D + lane];
                }
                DDSP_WAVE_ORDER();
            }
            const int j = n - lane;
            const bool valid = alive && j >= 0 && j < T_b;
            diag = above;
            above = __shfl_up(cur, 1);
            if (lane == 0) above = strip > 0 && j < T_b ? edge[j] : INFINITY;
            if (valid) {
                const float4 *col = reinterpret_cast<const float4 *>(bt + (j & (kWin - 1)) * kStride);
                float4 xb[kD / 4];
#pragma unroll
                for (int k = 0; k < kD / 4; ++k) xb[k] = col[k];           // all reads in flight before the first use
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < kD / 4; ++k) {
                    const float t0 = __fsub_rn(xr[4 * k], xb[k].x), t1 = __fsub_rn(xr[4 * k + 1], xb[k].y);
                    const float t2 = __fsub_rn(xr[4 * k + 2], xb[k].z), t3 = __fsub_rn(xr[4 * k + 3], xb[k].w);
                    acc = __fadd_rn(acc, __fmul_rn(t0, t0));
                    acc = __fadd_rn(acc, __fmul_rn(t1, t1));
                    acc = __fadd_rn(acc, __fmul_rn(t2, t2));
                    acc = __fadd_rn(acc, __fmul_rn(t3, t3));
                }
                float d = acc < INFINITY ? acc : INFINITY;      // a NaN too
                if (radius > 0) {
                    const long off = (long)i * q - (long)j * p;
                    if ((off < 0 ? -off : off) > limit) d = INFINITY;
                }
                const float up = __fadd_rn(above, penalty), left = __fadd_rn(cur, penalty);
                float best = 0.0f;
                unsigned char code = 0;
                if (i == 0) {
                    if (j > 0) { best = left; code = 2; }
                } else if (j == 0) {
                    best = up;
                    code = 1;
                } else {
                    best = diag;
                    if (up < best) { best = up; code = 1; }
                    if (left < best) { best = left; code = 2; }
                }
                cur = i == 0 && j == 0 ? d : __fadd_rn(d, best);
                back[((size_t)strip * steps + n) * 64 + lane] = code;
                if (lane == 63) edge[j] = cur;
            }
        }
    }
    const float total = __shfl(cur, (T_a - 1) & 63);            // the last strip's last live lane ended on (T_a - 1, T_b - 1)
    __threadfence();                                            // the walk reads what other lanes stored
    DDSP_WAVE_ORDER();

    int len = 0;
    if (lane == 0) {
        int i = T_a - 1, j = T_b - 1;
        for (; len < longest;) {
            walk[longest - 1 - len] = make_short2((short)i, (short)j);
            ++len;
            if (i == 0 && j == 0) break;
            const int l = i & 63;
            const unsigned char code = back[((size_t)(i >> 6) * steps + j + l) * 64 + l];
            if (i == 0) --j;
            else if (j == 0) --i;
            else if (code == 0) { --i; --j; }
            else if (code == 1) --i;
            else --j;
        }
    }
    DDSP_WAVE_ORDER();
    len = __shfl(len, 0);
    const short2 *pts = walk + (longest - len);                 // forward order
    int *out = path + row * longest * 2;
    for (int k = lane; k < longest; k += 64) {
        const bool on = k < len;
        out[2 * k] = on ? pts[k].x : -1;
        out[2 * k + 1] = on ? pts[k].y : -1;
    }
    if (lane == 0) {
        length[row] = len;
        cost[row] = total;
    }

    // the timeline: s_k = (1 - tau) i_k + tau j_k is non-decreasing along the path and ends at S
    const double wa = 1.0 - tau, wb = tau;
    const double S = wa * (double)p + wb * (double)q;
    for (long t = lane; t < T_out; t += 64) {
        double s = T_out > 1 ? (double)t * S / (double)(T_out - 1) : 0.0;
        if (s > S) s = S;
        int lo = 0, hi = len - 1;                               // the largest k with s_k <= s; s_0 = 0 <= s
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            const short2 e = pts[mid];
            if (wa * (double)e.x + wb * (double)e.y <= s) lo = mid;
            else hi = mid - 1;
        }
        const short2 e = pts[lo];
        double pi = (double)e.x, pj = (double)e.y;
        if (lo < len - 1) {
            const short2 f = pts[lo + 1];
            const double s0 = wa * pi + wb * pj, s1 = wa * (double)f.x + wb * (double)f.y;      // s0 <= s < s1
            const double lam = (s - s0) / (s1 - s0);
            pi += lam * (double)(f.x - e.x);                    // the steps are 0 or 1
            pj += lam * (double)(f.y - e.y);
        }
        pos_a[row * T_out + t] = (float)pi;
        pos_b[row * T_out + t] = (float)pj;
    }
}

bool in_range(long T_a, long T_b, int D) { return T_a <= kMaxT && T_b <= kMaxT && D <= kMaxD; }

}  // namespace

extern "C" size_t ddsp_dtw_workspace_bytes(long B, long T_a, long T_b)
{
    if (B <= 0 || T_a <= 0 || T_b <= 0 || !in_range(T_a, T_b, 1) || B > 0x7fffffffl) return 0;
    return (size_t)B * (size_t)((T_a + 63) / 64) * (size_t)(T_b + 63) * 64;
}

extern "C" int ddsp_dtw_align(const float *x_a, const float *x_b, float *pos_a, float *pos_b, int *path, int *length, float *cost,
                              void *workspace, size_t workspace_bytes, long B, long T_a, long T_b, int D, long T_out, long radius,
                              float penalty, double timing, void *stream)
{
    if (B == 0) return 0;
    if (!x_a || !x_b || !pos_a || !pos_b || !path || !length || !cost || !workspace || B < 0 || T_a <= 0 || T_b <= 0 || D <= 0 ||
        T_out <= 0 || radius < 0 || !(penalty >= 0.0f) || !(penalty < INFINITY) || !(fabs(timing) < INFINITY))
        return DDSP_EINVAL;
    if (!in_range(T_a, T_b, D) || B > 0x7fffffffl || T_out > 0x7fffffffl) return DDSP_ERANGE;
    if (workspace_bytes < ddsp_dtw_workspace_bytes(B, T_a, T_b)) return DDSP_EINVAL;
    const long widest = (T_a > T_b ? T_a : T_b) - 1;
    if (radius > widest) radius = 0;                            // such a band holds every cell
    const double tau = timing < 0.0 ? 0.0 : (timing > 1.0 ? 1.0 : timing);
    const auto kernel = D <= 16 ? dtw_kernel<16> : D <= 32 ? dtw_kernel<32> : D <= 48 ? dtw_kernel<48> : dtw_kernel<64>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, x_a, x_b, pos_a, pos_b, path, length, cost,
                       (unsigned char *)workspace, (int)T_a, (int)T_b, D, T_out, radius, penalty, tau);
    return (int)hipGetLastError();
}
