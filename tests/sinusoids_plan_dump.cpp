// Prints the plans of csrc/ddsp_sinusoids_plan.h for the shapes on the command line: groups of "B T K hop backward live mode cap".
// The planner is plain C++, so tests/test_sinusoids_host.py compiles this on the host and holds the answers against its own
// arithmetic.
#include <stdio.h>
#include <stdlib.h>

#include "ddsp_sinusoids_plan.h"

int main(int argc, char **argv)
{
    using namespace ddsp_sinusoids;
    for (int i = 1; i + 7 < argc; i += 8) {
        const Plan p = plan(atol(argv[i]), atol(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]) != 0,
                            atoi(argv[i + 5]) != 0, atoi(argv[i + 6]), atoi(argv[i + 7]));
        printf("%d %d %d %ld %d %d %zu %d %zu\n", p.iter_segments, p.chunk_segments, p.chunks, p.units, p.grid, p.tile, p.lds_bytes,
               p.status, backward_scratch_bytes(atol(argv[i]), atol(argv[i + 1]), atoi(argv[i + 2]), true));
    }
    return 0;
}
