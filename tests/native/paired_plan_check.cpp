// Host check of the item streams of a paired J-parameter iteration (csrc/layout.h: plan_thread, write_strip_items, kStreamL /
// kStreamF; tests/test_paired_host.py compiles and runs it): for hand-built strip tables, every store format, the plain deal of a
// small image and the weighted deal of the persistent grid, the plan kernel's own per-thread code is run for every (wave, k) and
//   - L's and F's streams name the same strips in the same order as plan 0 (and plan 0's the strips of its StripEntry list),
//     with plan 0's very chunk items;
//   - F's three start items -- J plane, G plane, moments -- precede its chunks; L has no moments item;
//   - every source range lies inside its region (state block, G plane, compact store);
//   - a wave's items, the trailing ones included, fit plan_stride / plan_stride_pair, and nothing is written behind them.
#define __host__
#define __device__
#include "layout.h"
#include <cstdio>
#include <vector>
using namespace sucre;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad < 20) std::printf("line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

static const PlanItem kPoison = {0xdeadbeefu, 0x3fffffffu};
static bool poison(const PlanItem &p) { return p.src64 == kPoison.src64 && p.shape == kPoison.shape; }

static void run_case(int H, int W, int n_views, int fmt, const std::vector<uint32_t> &levels_in) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) { ++bad; return; }
    const uint32_t n_strips = (uint32_t)L.n_strips, waves = (uint32_t)L.fit_blocks[0] * 4u;
    std::vector<StripMeta> meta(n_strips);
    uint64_t lv = 0;
    for (uint32_t s = 0; s < n_strips; ++s) {   // (the compaction sorts the heaviest strips first; the table is taken as given)
        const uint32_t l = levels_in[s % levels_in.size()] > (uint32_t)n_views ? (uint32_t)n_views : levels_in[s % levels_in.size()];
        meta[s] = StripMeta{lv, l, s % 3u == 0u ? l : l / 2u};
        lv += padded_levels(fmt, l);
    }
    const uint64_t lb = (uint64_t)level_bytes(fmt);
    CHECK(L.off_comp + lv * lb <= L.off_pcount);   // the table fits the store's region
    const size_t stride0 = L.plan_stride[0], strideP = L.plan_stride_pair, kmax = L.plan_kmax[0];
    std::vector<PlanItem> plan0(waves * stride0, kPoison), planL(waves * strideP, kPoison), planF(waves * strideP, kPoison);
    std::vector<StripEntry> strips(waves * kmax, StripEntry{0xffffffffu, 0u});
    std::vector<uint32_t> count(waves, 0xffffffffu);
    for (uint32_t wid = 0; wid < waves; ++wid)
        for (uint32_t k = 0; k < (uint32_t)kmax + 1u; ++k)   // (one thread slot beyond the wave's strips: it must write nothing)
            plan_thread(0, fmt, wid, k, waves, n_strips, meta.data(), plan0.data(), strips.data(), count.data(), (uint32_t)stride0, (uint32_t)kmax,
                        L.off_comp, L.off_state, planL.data(), planF.data(), (uint32_t)strideP, L.off_gplane);
    const uint64_t state_end = L.off_state + (uint64_t)n_strips * kStateFloats * 4, g_end = L.off_gplane + (uint64_t)n_strips * 3 * kStripPx * 4;
    auto inside = [&](const PlanItem &it, uint64_t lo, uint64_t hi) {
        const uint64_t a = (uint64_t)it.src64 << 6;
        return a >= lo && a + shape_bytes(it.shape, fmt) <= hi;
    };
    auto same = [](const PlanItem &a, const PlanItem &b) { return a.src64 == b.src64 && a.shape == b.shape; };
    std::vector<int> seen(n_strips, 0);
    for (uint32_t wid = 0; wid < waves; ++wid) {
        const uint32_t K = count[wid];
        CHECK(K <= kmax);
        if (K > kmax) continue;
        const PlanItem *p0 = &plan0[wid * stride0], *pL = &planL[wid * strideP], *pF = &planF[wid * strideP];
        size_t i0 = 0, iL = 0, iF = 0;
        for (uint32_t k = 0; k < K; ++k) {
            const StripEntry se = strips[wid * kmax + k];
            CHECK(se.strip < n_strips);
            if (se.strip >= n_strips) break;
            ++seen[se.strip];
            const uint32_t chunks = counts_unmasked(se.counts) + counts_masked(se.counts) + (counts_tail(se.counts) ? 1u : 0u);
            CHECK(chunks == (meta[se.strip].levels + 3u) / 4u);
            const uint64_t st = L.off_state + (uint64_t)se.strip * kStateFloats * 4;
            // the J plane opens the strip in all three streams
            CHECK(((uint64_t)p0[i0].src64 << 6) == st && same(pL[iL], p0[i0]) && same(pF[iF], p0[i0]));
            CHECK(shape_bytes(p0[i0].shape, fmt) == 3u * kStripPx * 4u && inside(p0[i0], L.off_state, state_end));
            ++i0; ++iL; ++iF;
            // F: the G plane and the moments before any chunk
            CHECK(((uint64_t)pF[iF].src64 << 6) == L.off_gplane + (uint64_t)se.strip * 3 * kStripPx * 4 && shape_bytes(pF[iF].shape, fmt) == 3u * kStripPx * 4u);
            CHECK(inside(pF[iF], L.off_gplane, g_end));
            ++iF;
            const PlanItem moments = pF[iF++];
            CHECK(((uint64_t)moments.src64 << 6) == st + 3 * kStripPx * 4 && shape_bytes(moments.shape, fmt) == 6u * kStripPx * 4u && inside(moments, L.off_state, state_end));
            for (uint32_t c = 0; c < chunks; ++c, ++i0, ++iL, ++iF) {
                CHECK(same(pL[iL], p0[i0]) && same(pF[iF], p0[i0]));
                CHECK(inside(p0[i0], L.off_comp + meta[se.strip].lvoff * lb, L.off_comp + (meta[se.strip].lvoff + meta[se.strip].levels) * lb));
                CHECK(((p0[i0].shape & kShapeFull) != 0u) == (c < meta[se.strip].levels / 4u));
            }
            CHECK(same(p0[i0], moments));   // plan 0 closes the strip with the moments; L has no such item
            ++i0;
        }
        if (K) {   // the trailing items: the wave's first J plane, marked, in all three streams; nothing behind them
            for (int j = 0; j < SUCRE_RING; ++j, ++i0, ++iL, ++iF) {
                CHECK((p0[i0].shape & kShapeTrail) && same(pL[iL], p0[i0]) && same(pF[iF], p0[i0]) && p0[i0].src64 == p0[0].src64);
                CHECK(inside(PlanItem{p0[i0].src64, p0[i0].shape & ~kShapeTrail}, L.off_state, state_end));
            }
        }
        CHECK(i0 <= stride0 && iL <= strideP && iF <= strideP && iF == i0 + K && iL + K == i0);
        for (size_t i = i0; i < stride0; ++i) CHECK(poison(p0[i]));
        for (size_t i = iL; i < strideP; ++i) CHECK(poison(pL[i]));
        for (size_t i = iF; i < strideP; ++i) CHECK(poison(pF[i]));
    }
    for (uint32_t s = 0; s < n_strips; ++s) CHECK(seen[s] == 1);
}

int main() {
    int cases = 0;
    // strips of 0 (nobody observes them), 1, 3, 4, 5 levels and more; many short ones back to back; one of every view
    const std::vector<std::vector<uint32_t>> tables = {
        {5, 4, 3, 1, 0}, {0, 0, 0, 0}, {1, 1, 1, 0, 1}, {8, 7, 4, 4, 3, 3, 1, 1, 0, 0, 0}, {4096, 17, 16, 15, 1, 0}, {65, 64, 63, 40, 12, 9, 5, 2},
    };
    struct Geo { int H, W, n; };
    // one tile (one workgroup of four waves), ragged small images on the plain deal, one whose grid has waves without a strip,
    // and the persistent grid with its weighted deal (1080p: 32640 strips over 5120 waves)
    const Geo geos[] = {{16, 16, 8}, {24, 40, 8}, {16, 80, 300}, {48, 64, 4096}, {360, 480, 17}, {1080, 1920, 65}};
    for (const Geo &g : geos)
        for (int fmt = 0; fmt < 4; ++fmt)
            for (size_t t = 0; t < tables.size(); ++t) {
                if (g.H == 1080 && (fmt == 1 || fmt == 2) && t != 5) continue;   // (the large grid: every format once, two formats on every table)
                run_case(g.H, g.W, g.n, fmt, tables[t]);
                ++cases;
            }
    std::printf("%d cases, %d violations\n", cases, bad);
    return bad != 0;
}
