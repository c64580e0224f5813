// The reference side of tests/test_quadtree_primitives.py, built as a shared library at test time: the real std::sort (libstdc++) on the
// quadtree's 64-bit keys (count << 32 | x0 << 16 | index, comparator on key >> 16), the two classic inputs that drive std::sort into its
// heap-sort fallback, and a count of the ranges an input sends there (an instrumented copy of the introsort loop of
// csrc/libstdcxx_sort_model.h, itself pinned against std::sort by sort_model_test.cpp).
#include <algorithm>
#include <cstdint>
#include <vector>
#include "libstdcxx_sort_model.h"

namespace {
struct KeyLess { bool operator()(uint64_t a, uint64_t b) const { return (a >> 16) < (b >> 16); } };

// McIlroy, "A Killer Adversary for Quicksort" (1999): the comparator decides the values while std::sort runs.  Every item starts as "gas" (larger
// than every frozen value); when two gas items meet, the one that was not the last pivot candidate is frozen at the next value.  Sorting the
// values it ends with makes the same algorithm take the same comparisons again: every pivot is among the smallest of its range.
struct Adversary {
    std::vector<int> val; int gas, nsolid = 0, candidate = 0;
    explicit Adversary(int n) : val(n, n - 1), gas(n - 1) {}
    bool less(int x, int y) {
        if (val[x] == gas && val[y] == gas) { if (x == candidate) val[x] = nsolid++; else val[y] = nsolid++; }
        if (val[x] == gas) candidate = x; else if (val[y] == gas) candidate = y;
        return val[x] < val[y];
    }
};
}  // namespace

extern "C" {

void qsh_std_sort(uint64_t* keys, int n) { std::sort(keys, keys + n, KeyLess()); }

// counts[i] of the adversary sequence against std::sort itself (a permutation of 0 .. n-1)
void qsh_mcilroy_adversary(int* counts, int n) {
    if (n <= 0) return;
    Adversary adv(n);
    std::vector<int> items(n);
    for (int i = 0; i < n; i++) items[i] = i;
    std::sort(items.begin(), items.end(), [&adv](int x, int y) { return adv.less(x, y); });
    for (int i = 0; i < n; i++) counts[i] = adv.val[i];
}

// Musser's median-of-3 killer, as sort_model_test.cpp builds it
void qsh_musser_killer(int* counts, int n) {
    for (int i = 0; i < n; i++) counts[i] = 0;
    const int k = n / 2;
    for (int i = 1; i <= k; i++) {
        if (i % 2) { counts[i - 1] = i; if (i < n) counts[i] = k + i; }
        counts[k + i - 1] = 2 * i;
    }
}

// how many ranges std::sort's introsort loop heap-sorts on this input, and how many elements they hold
void qsh_heap_ranges(const uint64_t* keys, int n, int* nranges, long long* nelems) {
    *nranges = 0; *nelems = 0;
    if (n <= 0) return;
    std::vector<uint64_t> a(keys, keys + n);
    KeyLess less;
    int lg = 0;
    for (int t = n; t > 1; t >>= 1) lg++;
    struct Range { int first, last, depth; };
    std::vector<Range> stack(1, Range{0, n, lg * 2});
    while (!stack.empty()) {
        Range r = stack.back(); stack.pop_back();
        while (r.last - r.first > 16) {
            if (r.depth == 0) { orbx::sm_heap_sort(a.data(), r.first, r.last, less); ++*nranges; *nelems += r.last - r.first; break; }
            --r.depth;
            orbx::sm_move_median_to_first(a.data(), r.first, r.first + 1, r.first + (r.last - r.first) / 2, r.last - 1, less);
            const int cut = orbx::sm_unguarded_partition(a.data(), r.first + 1, r.last, r.first, less);
            stack.push_back(Range{cut, r.last, r.depth});
            r.last = cut;
        }
    }
}

}  // extern "C"
