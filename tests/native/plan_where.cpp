// Where a workspace keeps the strips of its fit waves (csrc/layout.h: Layout.off_plan_strips / off_plan_count of the J-parameter
// plan, which the paired streams share), for tests/straight_worker.py to read them back:  plan_where H W n_views  prints
//   <byte offset of the StripEntry lists> <byte offset of the per-wave counts> <entries reserved per wave> <waves>
#define __host__
#define __device__
#include "layout.h"
#include <cstdio>
#include <cstdlib>
using namespace sucre;

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    Layout L;
    if (!make_layout(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), &L)) return 1;
    static_assert(sizeof(StripEntry) == 8, "strip, counts");
    std::printf("%zu %zu %zu %d %d\n", L.off_plan_strips[0], L.off_plan_count[0], L.plan_kmax[0], 4 * L.fit_blocks[0], kCountBits);
    return 0;
}
