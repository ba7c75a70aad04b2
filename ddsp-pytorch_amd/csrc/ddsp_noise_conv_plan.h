// Index plan of the hop-128 noise kernel's truncated convolution on the matrix cores (ddsp_noise_wave.hip):
// which taps and which noise samples every v_mfma_f32_4x4x1_16b_f32 of a group of 16 frames multiplies, which output window it adds
// to, and where those operands sit in the wavefront's two LDS tiles.  Everything the kernel indexes with and nothing that computes.
// Plain C++ (no HIP), so that a host test can compile it on its own (tests/noise_conv_plan_dump.cpp).
//
// The instruction is 16 independent 4 x 4 outer products, one per BLOCK; block b is frame b of the group.  Lane 4 b + i gives
// A[b][i], lane 4 b + j gives B[b][j], and D[b][i][j] comes back in register i of lane 4 b + j (measured:
// tools/microbench/int_mfma_rates.hip).  One STEP (c, n0) of frame b is
//     A[b][i] = k_b[c + i],   B[b][j] = x_b[n0 + 4 j - c],   D[b][i][j] += A B   =>   y_b[n0 + i + 4 j] += k_b[c + i] x_b[n0 + 4 j - c]:
// sixteen different outputs of the window of 16 samples at n0, each product a (tap, source) pair of y[n] = sum_{m <= n} k[m] x[n - m].
// Window o (n0 = 16 o, o = 0..7) needs c = -3 .. n0 + 12; taps and sources below 0 read zero padding, which is the causal truncation.
// With c = 16 a + mu, A depends on (mu, a) only and B on (mu, beta = o - a) only (n0 - c = 16 beta - mu): for one mu the kernel reads
// eight A and eight B operands and issues the 36 instructions a + beta = o <= 7; 16 mu x 36 = 576 instructions, 256 ds_read_b32.
#pragma once

namespace ddsp_noise {
namespace conv {

constexpr int kFrames = 16;              // blocks of the instruction = frames of a group
constexpr int kSamples = 128;            // taps, noise samples and outputs of a frame
constexpr int kWindow = 16;              // outputs of a frame that one instruction adds to
constexpr int kWindows = kSamples / kWindow;
constexpr int kMu = 16;                  // residues of c modulo 16
constexpr int kOperands = 8;             // A operands and B operands read per mu
constexpr int kStepsPerMu = kOperands * (kOperands + 1) / 2;      // 36
constexpr int kSteps = kMu * kStepsPerMu;                         // 576

// c = 16 a + mu runs from -3: the residues 13..15 start one sixteen lower and, c <= 16 o + 12, stop one lower as well
constexpr int a_first(int mu) { return mu >= 13 ? -1 : 0; }
constexpr int beta_first(int mu) { return mu >= 13 ? 1 : 0; }
// step (mu, r, s), r, s >= 0, r + s <= 7: a = a_first + r, beta = beta_first + s, window o = a + beta = r + s
constexpr int window_of(int r, int s) { return r + s; }
constexpr int tap_base(int mu, int a) { return 16 * a + mu; }              // tap of i = 0 (down to -3)
constexpr int src_base(int mu, int beta) { return 16 * beta - mu; }        // source sample of j = 0 (down to -12)

// ---- the tap tile: [kFrames][kTapStride], kTapPad zeros then the 128 taps ------------------------------------------------------------
// The A read of lane 4 b + i is at b kTapStride + i + const.  A ds_read_b32 serves lanes 0..31 and 32..63 in turn, bank = dword
// address mod 32: stride = 4 (mod 32) puts the eight frames x four i of a half on b 4 + i = 32 different banks.  The compiler
// pairs the reads of one lane base (a and a + 1, beta and beta + 1: constants 16 or 4 floats apart) into ds_read2_b32; that
// instruction is served as two ds_read_b32, one per dword, each over the same lane halves and banks, and each dword of a pair is
// one of the reads above with its own constant, so the argument holds per dword of the instruction that is emitted.
constexpr int kTapPad = 4;
constexpr int kTapStride = kTapPad + kSamples;                     // 132 = 4 (mod 32): exactly the padded row
constexpr int kTapFloats = kFrames * kTapStride;
constexpr int tap_slot(int b, int m) { return b * kTapStride + kTapPad + m; }          // tap m >= -kTapPad of frame b
constexpr int tap_offset(int mu, int a) { return kTapPad + tap_base(mu, a); }          // + b kTapStride + i

// ---- the noise tile: [4 phases][kFrames][kSrcRow] ------------------------------------------------------------------------------------
// The B read of lane 4 b + j is sample e + 4 j: a stride of four samples, which in a plain row would put the four j of a frame on
// banks 4 apart and leave only two frames' worth of different banks.  So a frame's samples are stored by PHASE: sample p (from
// -kSrcPad) sits in plane (p & 3) at index (p + kSrcPad) >> 2, and the four j of a read are four CONSECUTIVE floats of one plane.
// Row stride 36 = 4 (mod 32): b 4 + j, again 32 different banks per half.  The phase of a read depends on mu alone.
constexpr int kSrcPad = 16;                                        // zeros in front (12 are read; 16 keeps a plane's pad one float4)
constexpr int kSrcRow = (kSrcPad + kSamples) / 4;                  // 36 floats of one phase of one frame
constexpr int kSrcPlane = kFrames * kSrcRow;                       // 576
constexpr int kSrcFloats = 4 * kSrcPlane;                          // 2304
constexpr int src_slot(int b, int p) { return (p & 3) * kSrcPlane + b * kSrcRow + ((p + kSrcPad) >> 2); }   // sample p >= -kSrcPad
constexpr int src_offset(int mu, int beta) { return src_slot(0, src_base(mu, beta)); }                      // + b kSrcRow + j

static_assert(kTapStride % 32 == 4 && kSrcRow % 32 == 4, "bank-conflict-free operand reads");
static_assert(kTapStride % 4 == 0 && kSrcRow % 4 == 0 && kSrcPlane % 4 == 0, "16-byte aligned rows");
static_assert(tap_base(13, a_first(13)) == -3 && tap_offset(13, a_first(13)) >= 0, "the first step reads inside the tap padding");
static_assert(src_base(12, beta_first(12)) == -12 && kSrcPad + src_base(12, 0) >= 0, "the lowest source sample is inside the padding");

}  // namespace conv
}  // namespace ddsp_noise
