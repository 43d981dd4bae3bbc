// ivf_follow.h — the host bookkeeping of an IVF layout that follows writes (option "ivf_follow").  No HIP: plain
// C++17 like search_plan.h (tests/host/ivf_follow_main.cpp compiles it alone with a host compiler).  codd_knn.hip keeps one
// PendingRows per index beside the device bitmap and the device list of the same slots; everything the device work is sized by
// comes from here, so nothing is ever read back.
#pragma once
#include <stdint.h>

#include <vector>

namespace codd {

// The rows whose copy in the list layout is stale, or that the layout does not hold at all: one bit per row slot (the mirror of the
// device bitmap, as dead_host mirrors dead_bits) and the number of distinct slots set.
struct PendingRows {
    std::vector<uint32_t> bits;   // [ceil(slots covered / 32)]
    int64_t count = 0;            // distinct pending slots

    int64_t words() const { return (int64_t)bits.size(); }
    bool test(int64_t slot) const {
        return slot >= 0 && (slot >> 5) < words() && ((bits[(size_t)(slot >> 5)] >> (uint32_t)(slot & 31)) & 1u);
    }
    // the mirror covers `slots` row slots (contents kept, new words zero; never shrinks).  May throw std::bad_alloc.
    void grow(int64_t slots) {
        const int64_t need = (slots + 31) / 32;
        if (need > words()) bits.resize((size_t)need, 0u);
    }
    // marks one slot; true when it was not pending before (a slot written twice is pending once)
    bool mark(int64_t slot) {
        grow(slot + 1);
        uint32_t& word = bits[(size_t)(slot >> 5)];
        const uint32_t bit = 1u << (uint32_t)(slot & 31);
        if (word & bit) return false;
        word |= bit;
        ++count;
        return true;
    }
    // a fold: nothing is pending, the mirror keeps its length
    void clear() {
        for (uint32_t& w : bits) w = 0u;
        count = 0;
    }
};

// The gap rule: a write whose lowest slot lies above the count brings the slots in between into existence (zero rows, DESIGN.md
// §14).  The layout does not hold them either, so they are pending from the old count on.  Returns the first slot to mark for a
// write whose lowest slot is `lo` on an index of `count` rows.
inline int64_t pending_from(int64_t count, int64_t lo) { return lo > count ? count : lo; }

// One write: the slots it names (`slots`, n of them; null = the range [lo, hi)) and the gap below it.  Appends the slots that are
// newly pending to `fresh`, in the order met, and returns how many those are.  `count` is the row count BEFORE the write.
inline int64_t mark_written(PendingRows& p, int64_t count, const int64_t* slots, int64_t n, int64_t lo, int64_t hi, std::vector<uint32_t>& fresh) {
    const size_t before = fresh.size();
    if (hi > count) p.grow(hi);
    if (slots) {
        for (int64_t i = 0; i < n; ++i)
            if (p.mark(slots[i])) fresh.push_back((uint32_t)slots[i]);
        // ... and every slot from the old count up to the new one: the gap below a scattered write and the slots it leaves
        // unwritten between its own exist from now on as well
        for (int64_t s = count; s < hi; ++s)
            if (p.mark(s)) fresh.push_back((uint32_t)s);
    } else {
        for (int64_t s = pending_from(count, lo); s < hi; ++s)
            if (p.mark(s)) fresh.push_back((uint32_t)s);
    }
    return (int64_t)(fresh.size() - before);
}

// The fold threshold: a write folds before it returns when MORE than this many rows are pending.  "ivf_fold_rows" = 0 (the
// default) means one mean list, ceil(rows of the layout / lists): the pending scan then costs no more than one more probed list.
inline int64_t fold_threshold(int64_t fold_rows, int64_t ivf_count, int nlist) {
    if (fold_rows > 0) return fold_rows;
    if (nlist < 1) return 0;
    const int64_t mean = (ivf_count + nlist - 1) / nlist;
    return mean < 1 ? 1 : mean;
}
inline bool fold_due(int64_t pending, int64_t threshold) { return pending > threshold; }

// Parts the pending rows are cut into for the delta scan: the split rule of the masked list route (enough work items to fill the
// chip whatever the batch, no more parts than the list has workgroup steps of 16 rows), and no more parts than the probed lists
// have (`list_parts`, per query) — the delta's partial keys sit behind the lists' in one buffer with the lists' stride per query,
// so that ONE merge launch reads both.
inline int delta_split(int num_cus, int B, int64_t pending, int64_t list_parts) {
    const int64_t groups = (B + 3) / 4;
    int64_t split = (4 * (int64_t)num_cus + groups - 1) / groups;
    split = split < 1 ? 1 : (split > 256 ? 256 : split);
    if (split > (pending + 15) / 16) split = (pending + 15) / 16;
    if (split > list_parts) split = list_parts;
    return (int)(split < 1 ? 1 : split);
}

// the device list of pending slots grows by half, from 4,096 entries
inline int64_t pending_list_capacity(int64_t have, int64_t need) {
    int64_t cap = have > 0 ? have : 4096;
    while (cap < need) cap += cap / 2;
    return cap;
}

}  // namespace codd
