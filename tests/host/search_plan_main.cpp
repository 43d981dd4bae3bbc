// search_plan_main.cpp — csrc/search_plan.h on its own, for tests/test_search_plan.py: compiled with a host compiler (no HIP),
// reads one case per line from stdin as integers and prints one line of integers per case.  The first integer is the command:
//
//   0                                              the option table: one line "name default lo hi rejected(lo - 1) rejected(hi + 1)
//                                                  stored(lo) stored(hi)" per row (the one command that prints names)
//   1 KNOBS SHAPE B k cooling eps_micro wide       plan_search and the program of its first pass:
//                                                  "route use8 can8 per_block fused_prep family nbq ts res el sqd"
//   2 KNOBS ntiles k use8 nbq num_cus              sample_tile_count
//   3                                              the per_block enumeration: "cases disagreements"
//   4 op ...                                       one FilterWatch, kept between lines: 0 = reset; 1 q8 q16 = queries filtered;
//                                                  2 = sent(); 3 surv fb epoch = observe() with default knobs; prints
//                                                  "pending surv fb q8 q16 q8_sent q16_sent cooldown_left stat_cooldowns
//                                                  cooldown_surv8 cooldown_useless_epoch"
//   5 n                                            FilterWatch::due(n)
//   6 KNOBS SHAPE B k m                            mask_takes_dense
//
// KNOBS: the value of every row of kKnobTable, in its order, then filter, filter_min_rows, filter_min_rows_small, filter_min_batch.
// SHAPE: metric dtype dim count num_cus all_normalized (dpad = dim rounded up to 64, as codd_knn_create does).
#include <stdio.h>

#include <stdlib.h>

#include "search_plan.h"

using namespace codd;

namespace {

bool read_int(long long* v) { return scanf("%lld", v) == 1; }
long long next() {
    long long v = 0;
    if (!read_int(&v)) {
        fprintf(stderr, "search_plan_main: a line ended early\n");
        exit(2);
    }
    return v;
}

FilterKnobs read_knobs() {
    FilterKnobs kn;
    for (const KnobRow& row : kKnobTable) {
        const long long v = next();
        if (set_knob(kn, row, v)) {
            fprintf(stderr, "search_plan_main: %s = %lld is out of range\n", row.name, v);
            exit(2);
        }
    }
    kn.filter_enabled = next() != 0;
    kn.filter_min_rows = next();
    kn.filter_min_rows_small = next();
    kn.filter_min_batch = (int)next();
    return kn;
}

IndexShape read_shape() {
    IndexShape s;
    s.metric = (int)next();
    s.dtype = (int)next();
    s.dim = (int)next();
    s.dpad = (s.dim + 63) / 64 * 64;
    s.count = next();
    s.num_cus = (int)next();
    s.all_normalized = next() != 0;
    return s;
}

// the expression search_impl held before plan_search derived per_block from filter_program, verbatim but for the names
bool per_block_as_it_was(const FilterKnobs& ix, int nsteps8, int B) {
    return ix.i8v2 != 0 && nsteps8 >= 3 && B > 64 && (B <= 128 ? ix.i8v2_half != 0 : B <= kTileQ) && (ix.i8v2 == 2 || nsteps8 > 4 || !ix.resident_q);
}

void print_watch(const FilterWatch& w) {
    printf("%d %llu %llu %lld %lld %lld %lld %d %lld %lld %lld\n", w.pending ? 1 : 0, w.surv, w.fb, (long long)w.q8, (long long)w.q16, (long long)w.q8_sent,
           (long long)w.q16_sent, w.cooldown_left, (long long)w.stat_cooldowns, (long long)w.cooldown_surv8, (long long)w.cooldown_useless_epoch);
}

}  // namespace

int main() {
    FilterWatch watch;
    long long cmd;
    while (read_int(&cmd)) {
        if (cmd == 0) {
            for (const KnobRow& row : kKnobTable) {
                FilterKnobs kn;
                const int def = kn.*row.knob;
                const bool below = set_knob(kn, row, row.lo - 1) != nullptr && kn.*row.knob == def;
                const bool above = set_knob(kn, row, row.hi + 1) != nullptr && kn.*row.knob == def;
                const bool at_lo = set_knob(kn, row, row.lo) == nullptr && kn.*row.knob == row.lo;
                const bool at_hi = set_knob(kn, row, row.hi) == nullptr && kn.*row.knob == row.hi;
                printf("%s %d %lld %lld %d %d %d %d\n", row.name, def, (long long)row.lo, (long long)row.hi, below, above, at_lo, at_hi);
            }
        } else if (cmd == 1) {
            const FilterKnobs kn = read_knobs();
            const IndexShape s = read_shape();
            const int B = (int)next(), k = (int)next();
            const bool cooling = next() != 0;
            const float eps = (float)next() * 1e-6f;
            const long long wide = next();
            const SearchPlan p = plan_search(kn, s, B, k, cooling, eps, wide);
            const int nq = B < kTileQ ? B : kTileQ;
            const FilterProgram f = filter_program(kn, s, nq, p.use8 ? dpad8_of(s) / 128 : s.dpad / 64, p.use8);
            printf("%d %d %d %d %d %d %d %d %d %d %d\n", (int)p.route, p.use8, p.can8, p.per_block, p.fused_prep, (int)f.family, f.nbq, f.ts, f.res, f.el, f.sqd);
        } else if (cmd == 2) {
            const FilterKnobs kn = read_knobs();
            IndexShape s;
            const long long ntiles = next();
            const int k = (int)next();
            const bool use8 = next() != 0;
            const int nbq = (int)next();
            s.num_cus = (int)next();
            printf("%lld\n", (long long)sample_tile_count(kn, s, ntiles, k, use8, nbq));
        } else if (cmd == 3) {
            long long cases = 0, bad = 0;
            FilterKnobs kn;
            IndexShape s;  // a cosine index
            for (kn.i8v2 = 0; kn.i8v2 <= 2; ++kn.i8v2)
                for (kn.i8v2_half = 0; kn.i8v2_half <= 1; ++kn.i8v2_half)
                    for (kn.resident_q = 0; kn.resident_q <= 1; ++kn.resident_q)
                        for (int nsteps8 = 1; nsteps8 <= 32; ++nsteps8)
                            for (int B = 1; B <= 1024; ++B) {
                                s.dim = s.dpad = nsteps8 * 128;
                                const bool derived = B <= kTileQ && filter_program(kn, s, B, dpad8_of(s) / 128, true).family == FilterProgram::TILE;
                                ++cases;
                                if (derived != per_block_as_it_was(kn, nsteps8, B)) ++bad;
                            }
            printf("%lld %lld\n", cases, bad);
        } else if (cmd == 4) {
            const long long op = next();
            if (op == 0) watch = FilterWatch();
            else if (op == 1) { watch.q8 += next(); watch.q16 += next(); }
            else if (op == 2) watch.sent();
            else if (op == 3) {
                const unsigned long long surv = (unsigned long long)next(), fb = (unsigned long long)next();
                const long long epoch = next();
                watch.observe(surv, fb, epoch, FilterKnobs());
            }
            print_watch(watch);
        } else if (cmd == 5) {
            printf("%d\n", FilterWatch::due(next()) ? 1 : 0);
        } else if (cmd == 6) {
            const FilterKnobs kn = read_knobs();
            const IndexShape s = read_shape();
            const int B = (int)next(), k = (int)next();
            const long long m = next();
            printf("%d\n", mask_takes_dense(kn, s, B, k, m) ? 1 : 0);
        } else {
            fprintf(stderr, "search_plan_main: unknown command %lld\n", cmd);
            return 2;
        }
    }
    return 0;
}
