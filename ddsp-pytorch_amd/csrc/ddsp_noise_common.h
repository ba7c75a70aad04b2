// Shared by the four filtered-noise sources:
//   ddsp_noise.hip       the two entry points (validate -> plan -> launch) and the direct kernels (batched, one frame per workgroup)
//   ddsp_noise_fft.hip   in-LDS FFT form, forward and backward (hop 512; hop 256 on request)
//   ddsp_noise_wave.hip  wavefront-private form (hop 128, 65 bands), forward
//   ddsp_noise_ir.hip    impulse responses of the whole batch as one split-bf16 matrix product (195 bands at hop 512)
// Which of them a call runs is decided by ddsp_noise_plan.h alone; the launch_* functions below launch what they are told.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddsp_noise_plan.h"

namespace ddsp_noise {

struct NoiseParams {
    const float *Hm;
    const float *u;
    float *y;
    int B, T, F, R, S;
    uint64_t seed, offset;
    const uint64_t *offset_dev;  // nullable: the draw starts at offset + *offset_dev (a device counter: hipGraph replays)
    int accumulate;
    int lpf_log; // batched kernel: log2(lanes per frame) -> 64 >> lpf_log frames per workgroup
    const float *zrows;          // nullable (FFT form only): impulse responses already built by ddsp_noise_ir.hip, [B*T][zs]:
    int zs;                      //   z[n] * S at columns [0, S/2], max |H| of the frame at column zs - 4
};

// Philox4x32-10 (Salmon et al. 2011), counter = (c0,c1,0,0), key = seed.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
    uint32_t c[4] = {c0, c1, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        // (three-input xor as ONE instruction, v_bitop3_b32 with truth table 0x96: 20 instead of 40 xors per block)
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c[1], k0, 0x96);
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c[3], k1, 0x96);
        const uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}


// One U[0,1) draw of the in-kernel stream as x = 2u - 1, u = (r >> 8) 2^-24 (:44-45).  m = r >> 8 < 2^24 converts exactly, m 2^-23 is
// exact and so is the subtraction (a multiple of 2^-23 in [-1, 1)): ONE fused multiply-add gives the very bits of (u * 2) - 1.
__device__ __forceinline__ float philox_to_sample(uint32_t r) { return __fmaf_rn((float)(r >> 8), 1.0f / 8388608.0f, -1.0f); }

// Eight fp32 values as three bf16 terms each, hi + mid + lo == the value exactly: the operands of the split-bf16 matrix products
// (ddsp_noise_wave.hip, ddsp_noise_ir.hip).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
struct Split { bf16x8 p[3]; };
// x = hi + mid + lo with every term a bf16: both residuals are exact in fp32 (8 + 8 + 8 significand bits)
__device__ __forceinline__ void split3(float x, Split &d, int j)
{
    const __bf16 hi = (__bf16)x;
    const float r1 = x - (float)hi;
    const __bf16 mid = (__bf16)r1;
    const float r2 = r1 - (float)mid;
    d.p[0][j] = hi; d.p[1][j] = mid; d.p[2][j] = (__bf16)r2;
}

// ---- the launchers: each launches the form the plan named and returns the launch status ------------------------------------------
// FFT form, forward (hop 512, or hop 256; S <= hop; y and u 16-byte aligned); reads p.zrows instead of summing cosines when set.
hipError_t launch_noise_fft(const NoiseParams &p, hipStream_t s);

// FFT form, backward (hop 512; grad_y and uniform 16-byte aligned).  workspace == nullptr: 257 bands, dH inside the kernel; else
// (ir_workspace_bytes, the shapes of ir_product_shape) dz goes to the workspace and dH = dz C^T is one matrix product.
hipError_t launch_noise_fft_backward(const float *grad_y, const float *uniform, float *grad_H, int B, int T, int F, int hop, uint64_t seed,
                                     uint64_t offset, const uint64_t *offset_dev, void *workspace, hipStream_t s);

// Impulse responses as one split-bf16 matrix product for the whole batch (ddsp_noise_ir.hip), into the workspace
// (| cosine operand | z rows |): the forward's pair of launches leaves the z rows at ir_rows(workspace, F).
hipError_t launch_noise_ir(const float *Hmag, long frames, int F, void *workspace, hipStream_t s);
hipError_t launch_ir_table(void *workspace, int F, int transpose, hipStream_t s);
hipError_t launch_ir_product(const float *in, int in_stride, float *out, int out_stride, float *maxabs, long frames, int F, int transpose,
                             const void *workspace, hipStream_t s);

// Wavefront-private hop-128 / 65-band form on the first `frames` frames of p, a multiple of kWaveGroupFrames (y, Hm and u 16-byte
// aligned); the entry point runs a remainder through another kernel, with the Philox offset advanced.
hipError_t launch_noise_wave(const NoiseParams &p, long frames, hipStream_t s);

}  // namespace ddsp_noise
