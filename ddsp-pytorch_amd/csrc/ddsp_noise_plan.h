// Which kernel form a filtered-noise call takes (ddsp_noise.hip: ddsp_noise_forward_ws / ddsp_noise_backward_ws), decided in one
// place: the mode bits of ddsp_noise_set_generic, the fixed shapes the forms are built for, the LDS sizes, the thresholds, and the
// two planners.  Everything that decides a form and nothing that launches one.
// Plain C++ (no HIP), so that a host test can compile it on its own (tests/noise_plan_dump.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

namespace ddsp_noise {

// ---- ddsp_noise_set_generic (include/ddsp_hip.h): tests and A/B runs pass these as numbers ---------------------------------------
constexpr int kModeFrameKernels = 1;    // bit 0: the one-frame-per-workgroup kernels, whatever the shape
constexpr int kModeDirectForms = 2;     // bit 1: the direct (time-domain) forms where the in-LDS FFT form would run
constexpr int kModeFftAtHop256 = 4;     // bit 2: the FFT form at hop 256 too (correct there, not faster)
constexpr int kModeNoWaveForm = 8;      // bit 3: the batched kernel where the wavefront-private form would run
constexpr int kModeCosineSums = 16;     // bit 4: the cosine sums where a workspace would give the matrix product
constexpr int kModeLanesShift = 8;      // (l + 1) << 8: 64 >> l frames per workgroup in the batched forward kernel, l = 0..3

constexpr int kPlanERange = -2;                  // DDSP_ERANGE (ddsp_noise.hip asserts the equality)
constexpr size_t kMaxLdsBytes = 160 * 1024;      // a CU's LDS: the most one workgroup can ask for

// ---- the wavefront-private form (ddsp_noise_wave.hip): one shape, whole groups of frames ------------------------------------------
constexpr int kWaveHop = 128, kWaveBands = 65, kWaveGroupFrames = 16;

// ---- the whole-batch matrix product of the impulse responses (ddsp_noise_ir.hip) --------------------------------------------------
constexpr int kIrKT = 4;                // contraction steps of 32 per parity: S/4 + 1 <= 128
constexpr int kIrNT = 7;                // output tiles of 16 per parity:      S/4 + 1 in (96, 112]  <=>  F in [194, 225]
constexpr int kIrFR = 2 * kIrKT * 3;    // fragments of one output tile: (parity, step, term)
constexpr size_t kIrFragmentBytes = 64 * 16;     // 64 lanes x eight bf16
inline bool ir_product_shape(int F, int hop)
{
    const int S = 2 * (F - 1), NQ = (F - 1) / 2 + 1;
    return hop == 512 && S < hop && NQ > 16 * (kIrNT - 1) && NQ <= 16 * kIrNT;
}
inline int ir_row_stride(int F) { return 16 * ((F + 15) / 16) + 4; }    // z row: >= F columns + a 16-byte tail (max |H| in its first float)
inline size_t ir_table_bytes(int) { return (size_t)kIrNT * kIrFR * kIrFragmentBytes; }
// workspace: | cosine operand | z rows [frames][ir_row_stride] |
inline size_t ir_workspace_bytes(long frames, int F) { return ir_table_bytes(F) + (size_t)frames * ir_row_stride(F) * sizeof(float); }
inline float *ir_rows(void *workspace, int F) { return reinterpret_cast<float *>(static_cast<char *>(workspace) + ir_table_bytes(F)); }

// where the product pays for its extra launches (cosine operand + product; measured crossovers at 195 bands, hop 512: forward
// between 2 752 and 5 504 frames, backward below 688): the real-time callback's 4 frames and the reference's own training batch
// (16 x 172 frames) keep the cosine sums in the forward
constexpr long kIrProductMinFramesFwd = 4096, kIrProductMinFramesBwd = 512;

// ddsp_noise_workspace_bytes: 0 where no form uses a workspace
inline size_t noise_workspace_bytes(int B, int T, int F, int hop)
{
    if (B <= 0 || T <= 0 || F < 2 || hop <= 0) return 0;
    const long frames = (long)B * T;
    return (ir_product_shape(F, hop) && frames >= kIrProductMinFramesBwd) ? ir_workspace_bytes(frames, F) : 0;
}

// ---- dynamic LDS of the direct kernels (ddsp_noise.hip), R = hop -------------------------------------------------------------------
inline size_t batched_lds_bytes(int F, int R, int lpf_log)
{
    const int S = 2 * (F - 1), FB = 64 >> lpf_log;
    const size_t ua = (size_t)(FB + 4) * F, ub = (size_t)FB * (R + 12);
    const size_t un = ua > ub ? ua : ub;
    return sizeof(float) * (((S + 3) & ~3) + (size_t)FB * (R + 4) + un);
}
inline size_t bwd_batched_lds_bytes(int F, int R, int lpf_log)
{
    const int S = 2 * (F - 1), FB = 64 >> lpf_log;
    return sizeof(float) * (((S + 3) & ~3) + (size_t)FB * (R + 4) + (size_t)FB * (R + 12) + (size_t)(S / 2 + 1) * (FB + 4));
}
inline size_t frame_lds_bytes(int F, int R) { return sizeof(float) * ((size_t)F + 2 * (F - 1) + 2 * (size_t)R); }
inline size_t bwd_frame_lds_bytes(int F, int R) { return sizeof(float) * ((size_t)2 * (F - 1) + 2 * (size_t)R + (F - 1) + 1); }

// Lanes per frame (log2) of the batched forward kernel: 64 frames per workgroup when the tile fits in ~half the
// CU's LDS (two workgroups per CU), else 32 / 16 frames; -1 when even 8 frames do not fit (frame kernel then).
inline int pick_lpf_log(int F, int R, int mode)
{
    if (mode >> kModeLanesShift) return (mode >> kModeLanesShift) - 1;
    // measured (hop 128, F 65): 32 frames / 35 KB per workgroup (4 workgroups per CU) beats 64 frames / 70 KB by 14 %
    for (size_t limit : {(size_t)40 * 1024, (size_t)80 * 1024, kMaxLdsBytes})
        for (int l = 0; l <= 3; ++l)
            if (batched_lds_bytes(F, R, l) <= limit) return l;
    return -1;
}
inline int pick_bwd_lpf_log(int F, int R)
{
    for (size_t limit : {(size_t)48 * 1024, (size_t)80 * 1024, kMaxLdsBytes})
        for (int l = 0; l <= 3; ++l)
            if (bwd_batched_lds_bytes(F, R, l) <= limit) return l;
    return -1;
}

// ---- the planners -----------------------------------------------------------------------------------------------------------------
struct NoiseShape { int B, T, F, hop; };

// What the host knows of a call's pointers without the GPU.  "aligned": to 16 bytes.
struct NoiseFacts {
    bool y_aligned;                // forward: y; backward: grad_y
    bool hm_aligned;               // forward: Hmag (the backward does not look)
    bool u_given, u_aligned;       // a uniform draw is injected, and where it starts
    bool ws_present, ws_aligned;
    size_t ws_bytes;
};

// Fft: ddsp_noise_fft.hip, in-LDS FFT form (the backward's form A and, with ir_product, B); Wave: ddsp_noise_wave.hip, forward only;
// Batched, Frame: ddsp_noise.hip, 64 >> lpf_log frames / one frame per workgroup (the backward's C0..C3 and D)
enum class NoiseForm { None, Fft, Wave, Batched, Frame };

struct NoisePlan {
    NoiseForm form;       // takes every frame -- but Wave only the leading wave_frames
    bool ir_product;      // Fft: the impulse responses (forward, first) / dH from dz (backward, last) as the whole-batch product
    long wave_frames;     // Wave: whole groups of kWaveGroupFrames
    NoiseForm rest;       // Wave: Batched or Frame for the remainder of fewer than kWaveGroupFrames frames; None when there is none
    int lpf_log;          // of the Batched kernel, as `form` or as `rest`
    size_t lds_bytes;     // dynamic LDS of the Batched / Frame kernel, as `form` or as `rest` (the other forms know their own)
    int status;           // 0, or what the entry point returns instead of launching anything
};

inline bool workspace_fits(const NoiseFacts &f, long frames, int F)
{
    return f.ws_present && f.ws_aligned && f.ws_bytes >= ir_workspace_bytes(frames, F);
}
// What no faster form takes goes to a direct kernel: Batched where a tile fits in LDS (the forward's stores whole float4s, so not
// into a misaligned y), else Frame -- with DDSP_ERANGE where even one frame does not fit.  `slot`: pl.form or pl.rest.
inline void plan_direct(NoisePlan &pl, NoiseForm &slot, bool backward, int F, int hop, int mode, bool y_aligned)
{
    const int lpf_log = backward ? pick_bwd_lpf_log(F, hop) : pick_lpf_log(F, hop, mode);
    if (!(mode & kModeFrameKernels) && hop % 8 == 0 && lpf_log >= 0 && (backward || y_aligned)) {
        slot = NoiseForm::Batched;
        pl.lpf_log = lpf_log;
        pl.lds_bytes = backward ? bwd_batched_lds_bytes(F, hop, lpf_log) : batched_lds_bytes(F, hop, lpf_log);
        return;
    }
    slot = NoiseForm::Frame;
    pl.lds_bytes = backward ? bwd_frame_lds_bytes(F, hop) : frame_lds_bytes(F, hop);
    if (pl.lds_bytes > kMaxLdsBytes) pl.status = kPlanERange;
}

inline NoisePlan plan_noise_forward(const NoiseShape &sh, int mode, const NoiseFacts &f)
{
    const int F = sh.F, hop = sh.hop, S = 2 * (F - 1);
    const long frames = (long)sh.B * sh.T;
    const bool u_ok = !f.u_given || f.u_aligned;
    NoisePlan pl = {NoiseForm::None, false, 0, NoiseForm::None, 0, 0, 0};
    // hop 512 (and, asked for, hop 256) with an impulse response that is not cropped (S <= hop; S = 2 (F - 1) is even): the FFT form
    if (!(mode & (kModeFrameKernels | kModeDirectForms)) && S >= 4 && S <= hop && f.y_aligned && u_ok &&
        (hop == 512 || (hop == 256 && (mode & kModeFftAtHop256)))) {
        pl.form = NoiseForm::Fft;
        // 195 bands at hop 512 (the reference's default shape) with a workspace: the impulse responses of the whole batch as one
        // matrix product, which the FFT form then reads instead of summing cosines
        pl.ir_product = !(mode & kModeCosineSums) && ir_product_shape(F, hop) && frames >= kIrProductMinFramesFwd &&
                        workspace_fits(f, frames, F);
        return pl;
    }
    // hop 128 / 65 bands (the 16 kHz configurations): the wavefront-private form on the whole groups of 16 frames
    if (!(mode & (kModeFrameKernels | kModeNoWaveForm)) && hop == kWaveHop && F == kWaveBands && f.y_aligned && f.hm_aligned && u_ok &&
        frames >= kWaveGroupFrames) {
        pl.form = NoiseForm::Wave;
        pl.wave_frames = frames - frames % kWaveGroupFrames;
        if (pl.wave_frames < frames) plan_direct(pl, pl.rest, false, F, hop, mode, f.y_aligned);
        return pl;
    }
    plan_direct(pl, pl.form, false, F, hop, mode, f.y_aligned);
    return pl;
}

inline NoisePlan plan_noise_backward(const NoiseShape &sh, int mode, const NoiseFacts &f)
{
    const int F = sh.F, hop = sh.hop, S = 2 * (F - 1);
    const long frames = (long)sh.B * sh.T;
    NoisePlan pl = {NoiseForm::None, false, 0, NoiseForm::None, 0, 0, 0};
    // hop 512: the correlation in the in-LDS FFT form; its dH step is built for S == hop (257 bands) or, given a workspace, is one
    // matrix product at the shapes of ir_product_shape (195 bands)
    if (!(mode & (kModeFrameKernels | kModeDirectForms)) && hop == 512 && f.y_aligned && (!f.u_given || f.u_aligned)) {
        pl.ir_product = !(mode & kModeCosineSums) && ir_product_shape(F, hop) && frames >= kIrProductMinFramesBwd &&
                        workspace_fits(f, frames, F);
        if (pl.ir_product || S == hop) {
            pl.form = NoiseForm::Fft;
            return pl;
        }
    }
    plan_direct(pl, pl.form, true, F, hop, mode, f.y_aligned);
    return pl;
}

}  // namespace ddsp_noise
