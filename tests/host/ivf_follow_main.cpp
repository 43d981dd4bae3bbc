// ivf_follow_main.cpp — csrc/ivf_follow.h on its own, for tests/test_ivf_follow_host.py: compiled with a host compiler (no HIP),
// reads one command per line from stdin as integers and prints one line of integers per command.  One PendingRows is kept between
// lines.  The first integer is the command:
//
//   0                               a fresh PendingRows: "count words"
//   1 count lo hi                   a range write [lo, hi) on an index of `count` rows (mark_written, slots = null):
//                                   "fresh pending words slot..." — the newly pending slots in the order appended
//   2 count n slot...               a scattered write of n slots (lo, hi: their hull, as codd_knn_upsert_host passes it): the same line
//   3 fold_rows ivf_count nlist pending    "threshold due"
//   4 num_cus B pending list_parts  delta_split
//   5                               clear (a fold): "count words bits_set"
//   6 slot                          test(slot)
//   7 have need                     pending_list_capacity
//   8 slots                         grow(slots): "words"
//   9 count lo                      pending_from
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ivf_follow.h"

using namespace codd;

namespace {

long long next() {
    long long v = 0;
    if (scanf("%lld", &v) != 1) {
        fprintf(stderr, "ivf_follow_main: a line ended early\n");
        exit(2);
    }
    return v;
}

void print_write(const PendingRows& p, const std::vector<uint32_t>& fresh, long long reported) {
    if (reported != (long long)fresh.size()) {
        fprintf(stderr, "ivf_follow_main: mark_written returned %lld for %zu fresh slots\n", reported, fresh.size());
        exit(3);
    }
    printf("%zu %lld %lld", fresh.size(), (long long)p.count, (long long)p.words());
    for (uint32_t s : fresh) printf(" %u", s);
    printf("\n");
}

}  // namespace

int main() {
    PendingRows p;
    long long cmd;
    while (scanf("%lld", &cmd) == 1) {
        switch (cmd) {
            case 0:
                p = PendingRows();
                printf("%lld %lld\n", (long long)p.count, (long long)p.words());
                break;
            case 1: {
                const long long count = next(), lo = next(), hi = next();
                std::vector<uint32_t> fresh;
                const long long r = mark_written(p, count, nullptr, hi - lo, lo, hi, fresh);
                print_write(p, fresh, r);
                break;
            }
            case 2: {
                const long long count = next(), n = next();
                std::vector<int64_t> slots((size_t)n);
                long long lo = 0, hi = 0;
                for (long long i = 0; i < n; ++i) {
                    slots[(size_t)i] = next();
                    if (i == 0 || slots[(size_t)i] < lo) lo = slots[(size_t)i];
                    if (i == 0 || slots[(size_t)i] + 1 > hi) hi = slots[(size_t)i] + 1;
                }
                std::vector<uint32_t> fresh;
                const long long r = mark_written(p, count, slots.data(), n, lo, hi, fresh);
                print_write(p, fresh, r);
                break;
            }
            case 3: {
                const long long fold_rows = next(), ivf_count = next(), nlist = next(), pending = next();
                const long long thr = fold_threshold(fold_rows, ivf_count, (int)nlist);
                printf("%lld %d\n", thr, fold_due(pending, thr) ? 1 : 0);
                break;
            }
            case 4: {
                const long long cus = next(), B = next(), pending = next(), parts = next();
                printf("%d\n", delta_split((int)cus, (int)B, pending, parts));
                break;
            }
            case 5: {
                p.clear();
                long long set = 0;
                for (uint32_t w : p.bits) set += __builtin_popcount(w);
                printf("%lld %lld %lld\n", (long long)p.count, (long long)p.words(), set);
                break;
            }
            case 6:
                printf("%d\n", p.test(next()) ? 1 : 0);
                break;
            case 7: {
                const long long have = next(), need = next();
                printf("%lld\n", (long long)pending_list_capacity(have, need));
                break;
            }
            case 8:
                p.grow(next());
                printf("%lld\n", (long long)p.words());
                break;
            case 9: {
                const long long count = next(), lo = next();
                printf("%lld\n", (long long)pending_from(count, lo));
                break;
            }
            default:
                fprintf(stderr, "ivf_follow_main: unknown command %lld\n", cmd);
                return 2;
        }
    }
    return 0;
}
