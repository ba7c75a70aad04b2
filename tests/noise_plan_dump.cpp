// Prints what the filtered-noise planner (csrc/ddsp_noise_plan.h) decides, as text, for tests/test_noise_plan_host.py.
//   usage: noise_plan_dump QUERY ...      one line of output per query
//   QUERY = dir:B:T:F:hop:mode:facts:ws
//     dir    f (forward), b (backward) or w (ddsp_noise_workspace_bytes only; the last three fields are ignored)
//     facts  five characters 0 / 1: y (backward: grad_y) aligned, Hmag aligned, uniform given, uniform aligned, workspace aligned
//     ws     "none", or the workspace's size as a signed offset from noise_workspace_bytes(B, T, F, hop) ("0": exactly that)
//   fwd B T F hop mode form=.. ir=.. wave=.. rest=.. lpf=.. lds=.. status=..
//   bwd B T F hop mode form=.. ir=.. lpf=.. lds=.. status=..
//   ws B T F hop bytes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ddsp_noise_plan.h"

using namespace ddsp_noise;

static const char *name(NoiseForm f)
{
    switch (f) {
        case NoiseForm::Fft: return "Fft";
        case NoiseForm::Wave: return "Wave";
        case NoiseForm::Batched: return "Batched";
        case NoiseForm::Frame: return "Frame";
        default: return "None";
    }
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        char dir = 0, facts[6] = "", ws[32] = "";
        int B = 0, T = 0, F = 0, hop = 0, mode = 0;
        if (sscanf(argv[a], "%c:%d:%d:%d:%d:%d:%5[01]:%31s", &dir, &B, &T, &F, &hop, &mode, facts, ws) != 8 || strlen(facts) != 5 ||
            !strchr("fbw", dir)) {
            fprintf(stderr, "bad query: %s\n", argv[a]);
            return 2;
        }
        const size_t need = noise_workspace_bytes(B, T, F, hop);
        if (dir == 'w') {
            printf("ws %d %d %d %d %zu\n", B, T, F, hop, need);
            continue;
        }
        NoiseFacts f = {facts[0] == '1', facts[1] == '1', facts[2] == '1', facts[3] == '1', false, facts[4] == '1', 0};
        if (strcmp(ws, "none") != 0) {
            const long delta = atol(ws);
            f.ws_present = true;
            f.ws_bytes = delta < 0 && (size_t)(-delta) > need ? 0 : need + delta;
        }
        const NoiseShape sh = {B, T, F, hop};
        if (dir == 'f') {
            const NoisePlan pl = plan_noise_forward(sh, mode, f);
            printf("fwd %d %d %d %d %d form=%s ir=%d wave=%ld rest=%s lpf=%d lds=%zu status=%d\n", B, T, F, hop, mode, name(pl.form),
                   pl.ir_product ? 1 : 0, pl.wave_frames, name(pl.rest), pl.lpf_log, pl.lds_bytes, pl.status);
        } else {
            const NoisePlan pl = plan_noise_backward(sh, mode, f);
            printf("bwd %d %d %d %d %d form=%s ir=%d lpf=%d lds=%zu status=%d\n", B, T, F, hop, mode, name(pl.form), pl.ir_product ? 1 : 0,
                   pl.lpf_log, pl.lds_bytes, pl.status);
        }
    }
    return 0;
}
