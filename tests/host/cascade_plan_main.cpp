// cascade_plan_main.cpp — the sample cascade's plan (csrc/search_plan.h: cascade_geometry, cascade_plan, cascade_pick_d) on its own,
// for tests/test_cascade_plan.py: compiled with a host compiler (no HIP), reads one case per line from stdin as integers and prints
// one line of integers per case.  The first integer is the command:
//
//   1 G d ntiles                         the geometry as it is: "d G a0_first a0_stride a0_tiles a1_tiles b_step", then one line per
//                                        workgroup u < G of launch B: "first my_tiles" (the test enumerates the tiles itself)
//   2 G d ntiles_lo ntiles_hi            every ntiles in [lo, hi], tile by tile, through a coverage array filled from first / step /
//                                        my_tiles exactly as the tile programs walk them: "cases uncovered twice a0_in_a1 a0_outside
//                                        a0_repeated"
//   3 G want                             cascade_pick_d
//   4 mode want min_rounds G ntiles k ts_today family ts res sample_tiles    cascade_plan on a cosine index: "on d a0_tiles a0_stride"
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "search_plan.h"

using namespace codd;

namespace {

long long next() {
    long long v = 0;
    if (scanf("%lld", &v) != 1) {
        fprintf(stderr, "cascade_plan_main: a line ended early\n");
        exit(2);
    }
    return v;
}

}  // namespace

int main() {
    long long cmd;
    while (scanf("%lld", &cmd) == 1) {
        if (cmd == 1) {
            const int G = (int)next(), d = (int)next();
            const long long ntiles = next();
            const CascadePlan c = cascade_geometry(G, d, ntiles, G);
            printf("%d %d %lld %lld %lld %lld %lld\n", c.d, c.G, (long long)c.a0_first, (long long)c.a0_stride, (long long)c.a0_tiles, (long long)c.a1_tiles,
                   (long long)c.b_step);
            for (int u = 0; u < G; ++u) printf("%lld %lld\n", (long long)cascade_b_first(c, u), (long long)cascade_b_my_tiles(c, u, ntiles));
        } else if (cmd == 2) {
            const int G = (int)next(), d = (int)next();
            const long long lo = next(), hi = next();
            long long cases = 0, uncovered = 0, twice = 0, a0_in_a1 = 0, a0_outside = 0, a0_repeated = 0;
            for (long long ntiles = lo; ntiles <= hi; ++ntiles) {
                const CascadePlan c = cascade_geometry(G, d, ntiles, G);
                std::vector<int> seen((size_t)ntiles, 0);
                for (long long r = 0; r < c.a1_tiles; ++r) {   // A1: run-tile r is corpus tile r (d + 1)
                    const long long t = r * (d + 1);
                    if (t < ntiles) seen[(size_t)t]++;
                    else ++uncovered;   // (a run-tile past the corpus: counted as a fault of the plan)
                }
                for (int u = 0; u < G; ++u) {                  // B: one cursor, one step
                    long long t = cascade_b_first(c, u);
                    const long long mine = cascade_b_my_tiles(c, u, ntiles);
                    for (long long j = 0; j < mine; ++j, t += c.b_step) {
                        if (t < ntiles) seen[(size_t)t]++;
                        else ++uncovered;
                    }
                }
                for (long long t = 0; t < ntiles; ++t) {
                    if (seen[(size_t)t] == 0) ++uncovered;
                    if (seen[(size_t)t] > 1) ++twice;
                }
                std::vector<int> a0((size_t)ntiles, 0);
                for (long long u = 0; u < c.a0_tiles; ++u) {
                    const long long t = c.a0_first + u * c.a0_stride;
                    if (t < 0 || t >= ntiles) { ++a0_outside; continue; }
                    if (t % (d + 1) == 0) ++a0_in_a1;
                    if (a0[(size_t)t]++) ++a0_repeated;
                }
                if (c.a0_tiles < (ntiles >= 2 ? 1 : 0) || c.a0_tiles > G) ++a0_outside;
                ++cases;
            }
            printf("%lld %lld %lld %lld %lld %lld\n", cases, uncovered, twice, a0_in_a1, a0_outside, a0_repeated);
        } else if (cmd == 3) {
            const int G = (int)next(), want = (int)next();
            printf("%d\n", cascade_pick_d(G, want));
        } else if (cmd == 4) {
            FilterKnobs kn;
            kn.sample_cascade = (int)next();
            kn.cascade_d = (int)next();
            kn.cascade_min_rounds = (int)next();
            IndexShape s;
            s.num_cus = (int)next();
            const long long ntiles = next();
            const int k = (int)next();
            const long long ts_today = next();
            FilterProgram prog;
            prog.family = (FilterProgram::Family)next();
            prog.ts = (int)next();
            prog.res = (int)next();
            prog.el = 1;
            kn.sample_tiles = (int)next();
            const CascadePlan c = cascade_plan(kn, s, prog, ntiles, k, ts_today);
            printf("%d %d %lld %lld\n", c.on ? 1 : 0, c.d, (long long)c.a0_tiles, (long long)c.a0_stride);
        } else {
            fprintf(stderr, "cascade_plan_main: unknown command %lld\n", cmd);
            return 2;
        }
    }
    return 0;
}
