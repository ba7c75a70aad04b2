// Prints the chunked oscillator's slot plans as text for tests/test_osc_slot_plan_host.py:
//   usage: osc_slot_plan_dump H K G ...   (triples)
//   ks K ...                                     first line: the list of K the kernels are instantiated for (kOscKs)
//   plan H K G ok KR KD cls0 cls1 cls2 cls3      then one line per lane: "lane j : h/shift ..." (h 1-based, 0 = padding)
//   parents K : parent of each derived slot
#include <stdio.h>
#include <stdlib.h>

#include "ddsp_osc_plan.h"

int main(int argc, char **argv)
{
    using namespace ddsp_osc;
    printf("ks");
    for (int K : kOscKs) printf(" %d", K);
    printf("\n");
    for (int a = 1; a + 2 < argc; a += 3) {
        const int H = atoi(argv[a]), K = atoi(argv[a + 1]), G = atoi(argv[a + 2]);
        SlotPlan pl;
        const bool ok = plan_slots(H, K, G, pl);
        if (!ok) plan_all_roots(H, K, G, pl);
        printf("plan %d %d %d %d %d %d %d %d %d %d\n", H, K, G, ok ? 1 : 0, pl.KR, pl.KD, pl.cls_max[0], pl.cls_max[1], pl.cls_max[2], pl.cls_max[3]);
        printf("parents %d :", K);
        for (int d = 0; d < pl.KD; ++d) printf(" %d", derived_parent(K, d));
        printf("\n");
        for (int j = 0; j < G; ++j) {
            printf("lane %d :", j);
            for (int m = 0; m < K; ++m) {
                const int h = pl.t.h[j * K + m];
                printf(" %d/%d", h == kNoHarmonic ? 0 : h + 1, (int)pl.t.shift[j * K + m]);
            }
            printf("\n");
        }
    }
    return 0;
}
