// Host check of csrc/fit_math.h's scaled_b_ok (tests/test_scaled_b_host.py compiles it with hipcc, host side only, and runs it):
// the predicate that lets a fit launch run the B-scaled chunk arithmetic holds exactly on [kScaledBMin, kScaledBMax] in absolute
// value, in every channel, and nowhere else -- both edges and their float32 neighbours, 0, -0, a denormal, infinity, NaN.
// With a file name: the file holds float32 triples (B of the three channels); prints how many of them fail the predicate.
#include "fit_math.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
using namespace sucre;

int main(int argc, char **argv) {
    if (argc > 1) {
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        float b[3];
        long n = 0, fail = 0;
        while (std::fread(b, sizeof(float), 3, f) == 3) { ++n; fail += scaled_b_ok(b[0], b[1], b[2]) ? 0 : 1; }
        std::fclose(f);
        std::printf("%ld triples, %ld outside\n", n, fail);
        return fail != 0;
    }
    const float lo = kScaledBMin, hi = kScaledBMax, inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    struct Case { float b; bool ok; };
    const std::vector<Case> cases = {
        {0.1f, true}, {-0.05f, true}, {1.0f, true},
        {lo, true}, {-lo, true}, {std::nextafterf(lo, 0.f), false}, {-std::nextafterf(lo, 0.f), false}, {std::nextafterf(lo, 1.f), true},
        {hi, true}, {-hi, true}, {std::nextafterf(hi, inf), false}, {-std::nextafterf(hi, inf), false}, {std::nextafterf(hi, 0.f), true},
        {0.0f, false}, {-0.0f, false}, {std::numeric_limits<float>::denorm_min(), false}, {0x1p-127f, false}, {-0x1p-140f, false},
        {std::numeric_limits<float>::min(), false}, {std::numeric_limits<float>::max(), false}, {inf, false}, {-inf, false}, {nan, false}, {-nan, false},
    };
    int bad = 0, n = 0;
    const bool built = kScaledBBuilt;   // SUCRE_SCALED_B=0: never
    for (const Case &c : cases) {
        const bool want = built && c.ok;
        // alone in every channel next to two good ones, and in all three
        for (int ch = 0; ch < 4; ++ch) {
            const float b0 = (ch == 0 || ch == 3) ? c.b : 0.1f, b1 = (ch == 1 || ch == 3) ? c.b : 0.1f, b2 = (ch == 2 || ch == 3) ? c.b : 0.1f;
            if (scaled_b_ok(b0, b1, b2) != want) { ++bad; std::printf("B = %a in channel set %d: got %d\n", (double)c.b, ch, (int)!want); }
            ++n;
        }
    }
    if (!(lo > 0.f && lo <= 0.1f && 0.1f <= hi && std::isfinite(hi))) ++bad;   // fit_init's 0.1 is inside
    std::printf("%d cases, %d violations\n", n, bad);
    return bad != 0;
}
