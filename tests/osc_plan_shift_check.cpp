// Checks the invariant the chunked oscillator's kernels compile in (csrc/ddsp_osc_plan.h: derived_shift) for
// tests/test_osc_plan_shift_host.py: in every plan that plan_slots accepts, a FILLED derived slot d has
// shift == derived_shift(K, d), and its parent's harmonic number times 2^shift is its own.
//   usage: osc_plan_shift_check Hmax K ...     (every K x G in {4, 8, 16} x H = 1..Hmax)
//   one line per K: "K <K> children <n> plans <accepted> filled <derived slots checked> padded <n> violations <n>",
//   then "shifts <K> : derived_shift of each derived slot"; a violation also prints a line "bad H K G lane slot h parent shift".
#include <stdio.h>
#include <stdlib.h>

#include "ddsp_osc_plan.h"

int main(int argc, char **argv)
{
    using namespace ddsp_osc;
    if (argc < 3) return 2;
    const int Hmax = atoi(argv[1]);
    for (int a = 2; a < argc; ++a) {
        const int K = atoi(argv[a]);
        long plans = 0, filled = 0, padded = 0, bad = 0;
        for (int G = 4; G <= 16; G *= 2)
            for (int H = 1; H <= Hmax; ++H) {
                SlotPlan pl;
                if (!plan_slots(H, K, G, pl)) continue;
                ++plans;
                for (int j = 0; j < G; ++j)
                    for (int d = 0; d < pl.KD; ++d) {
                        const int h = pl.t.h[j * K + pl.KR + d], t = pl.t.shift[j * K + pl.KR + d];
                        if (h == kNoHarmonic) {
                            ++padded;
                            continue;
                        }
                        ++filled;
                        const int ph = pl.t.h[j * K + derived_parent(K, d)];
                        const bool ok = t == derived_shift(K, d) && ph != kNoHarmonic && ((long)(ph + 1) << t) == (long)(h + 1);
                        if (!ok) {
                            ++bad;
                            printf("bad %d %d %d %d %d %d %d %d\n", H, K, G, j, d, h + 1, ph == kNoHarmonic ? 0 : ph + 1, t);
                        }
                    }
            }
        printf("K %d children %d plans %ld filled %ld padded %ld violations %ld\n", K, plan_derived(K), plans, filled, padded, bad);
        printf("shifts %d :", K);
        for (int d = 0; d < plan_derived(K); ++d) printf(" %d", derived_shift(K, d));
        printf("\n");
    }
    return 0;
}
