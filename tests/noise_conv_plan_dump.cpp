// Prints the index plan of the hop-128 noise convolution (csrc/ddsp_noise_conv_plan.h) as text, for tests/test_noise_conv_plan_host.py:
//   dims <frames> <samples> <steps> <tap_pad> <tap_stride> <tap_floats> <src_pad> <src_row> <src_plane> <src_floats>
//   step <mu> <a> <beta> <window> <tap_base> <src_base> <tap_offset> <src_offset>          one line per instruction, in issue order
// The LDS float a lane reads is tap_offset + b tap_stride + i for A (lane 4 b + i) and src_offset + b src_row + j for B (lane 4 b + j).
//   slot tap <b> <m> <float>  /  slot src <b> <p> <float>                                   where tap m / sample p of frame b is stored
#include <stdio.h>

#include "ddsp_noise_conv_plan.h"

namespace cp = ddsp_noise::conv;

int main()
{
    printf("dims %d %d %d %d %d %d %d %d %d %d\n", cp::kFrames, cp::kSamples, cp::kSteps, cp::kTapPad, cp::kTapStride, cp::kTapFloats,
           cp::kSrcPad, cp::kSrcRow, cp::kSrcPlane, cp::kSrcFloats);
    for (int mu = 0; mu < cp::kMu; ++mu)
        for (int r = 0; r < cp::kOperands; ++r)
            for (int s = cp::kOperands - 1 - r; s >= 0; --s) {
                const int a = cp::a_first(mu) + r, beta = cp::beta_first(mu) + s;
                printf("step %d %d %d %d %d %d %d %d\n", mu, a, beta, cp::window_of(r, s), cp::tap_base(mu, a), cp::src_base(mu, beta),
                       cp::tap_offset(mu, a), cp::src_offset(mu, beta));
            }
    for (int b = 0; b < cp::kFrames; ++b) {
        for (int m = -cp::kTapPad; m < cp::kSamples; ++m) printf("slot tap %d %d %d\n", b, m, cp::tap_slot(b, m));
        for (int p = -cp::kSrcPad; p < cp::kSamples; ++p) printf("slot src %d %d %d\n", b, p, cp::src_slot(b, p));
    }
    return 0;
}
