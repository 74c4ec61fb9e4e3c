// view_lists.cpp -- TEST INFRASTRUCTURE: the rule of csrc/imt_view.hpp on the CPU, over lists built the way a view's
// build builds them (the index work of imt_rewind.hpp, the lists of imt_apply.hpp; tests/native/rewind_lists.cpp is the
// model).  tests/test_view_logic.py loads it as a library and checks every node against the oracle; built with
// -DVIEW_LISTS_MAIN it is a stand-alone program that runs the same grid over streams of its own against a brute-force
// restatement, for a sanitizer build.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>
#include "imt_apply.hpp"
#include "imt_rewind.hpp"
#include "imt_view.hpp"

extern "C" {

// nodes view_host classifies: level l = 0 .. depth, x = 0 .. ceil(M / 2^l) inclusive, in that order
uint64_t view_nodes(uint32_t M, unsigned depth) {
    uint64_t n = 0;
    for (unsigned l = 0; l <= depth; l++) n += imt::view::filled(M, l) + 1;
    return n;
}

// val [M][32], sorted [M]: the index of a tree of M leaves; s in [1, M]; l0 = min(ceil(log2(M)), depth).  cls / rank
// [view_nodes(M, depth)]: what view::classify says of every node as of size s; count [depth + 1] as prep::apply_lists
// leaves it.  s == M has no relinked leaf and no list (the library answers from the tree): every count is 0 and only the
// levels below l0 mean anything.  Returns R, the number of relinked leaves, or -1 for arguments the device code refuses.
int view_host(const uint8_t* val, const uint32_t* sorted, uint32_t M, uint32_t s, uint64_t base, unsigned l0, unsigned depth,
              uint8_t* cls, uint32_t* rank, uint64_t* count) {
    if (s == 0 || s > M || l0 > 31 || l0 > depth) return -1;
    std::vector<uint64_t> pos(M);
    uint64_t run = 0;
    for (uint32_t j = 0; j < M; j++) {
        pos[j] = run;
        run += imt::rewind::scan_flag(sorted, M, j, s);
    }
    uint32_t R = 0xffffffffu;
    std::vector<uint32_t> compact(s);
    for (uint32_t j = 0; j < M; j++) imt::rewind::compact_element(sorted, M, j, s, pos[j], compact.data(), &R);
    const uint32_t max_rows = std::min(M - s, s) + 1;
    const uint32_t rows = s == M ? 0 : R + 1;
    if (rows > max_rows || (s < M && l0 == 0)) return -1;
    std::vector<uint32_t> lists((size_t)std::max(l0, 1u) * max_rows, 0xffffffffu);
    for (unsigned l = 0; l <= depth; l++) count[l] = 0;
    if (s < M) {
        std::vector<uint32_t> key(rows, 0xffffffffu), row(rows, 0xffffffffu), rs(rows), re(rows), node(rows), time(rows);
        std::vector<uint8_t> pre((size_t)rows * 96);
        const imt::rewind::Table t{key.data(), row.data(), rs.data(), re.data(), pre.data(), rows};
        for (uint32_t j = 0; j < M; j++) imt::rewind::relink_element(val, sorted, compact.data(), M, j, s, pos[j], base, t);
        std::vector<uint32_t> ord(rows);
        std::iota(ord.begin(), ord.end(), 0u);
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        for (uint32_t x = 0; x < rows; x++) {
            node[x] = key[ord[x]];
            time[x] = row[ord[x]];
        }
        std::vector<uint32_t> src(max_rows);
        const imt::apply::Lists o{lists.data(), src.data(), count, max_rows};
        for (unsigned l = 0; l < l0; l++) {
            uint32_t p = 0;
            for (uint32_t x = 0; x < rows; x++) {
                imt::apply::scatter_element(node.data(), time.data(), re.data(), rows, x, l, p, l0, depth, o);
                p += imt::apply::head(node.data(), x, l);
            }
        }
    }
    const imt::view::Side sd{lists.data(), count, max_rows, l0, s, nullptr, nullptr};
    size_t k = 0;
    for (unsigned l = 0; l <= depth; l++)
        for (uint64_t x = 0; x <= imt::view::filled(M, l); x++, k++) {
            const imt::view::Where w = imt::view::classify(sd, l, x);
            cls[k] = (uint8_t)w.cls;
            rank[k] = w.rank;
        }
    return (int)R;
}

uint64_t view_filled(uint64_t s, unsigned l) { return imt::view::filled(s, l); }

}

#ifdef VIEW_LISTS_MAIN
#include <cstdio>
#include <cstring>
#include <set>

namespace {

// the same nodes from the definitions alone: relinked = kept leaves whose successor in value order is removed
int check(const std::vector<uint64_t>& v, uint32_t s, unsigned depth) {
    const uint32_t M = (uint32_t)v.size();
    std::vector<uint32_t> sorted(M);
    std::iota(sorted.begin(), sorted.end(), 0u);
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return v[a] < v[b]; });
    std::vector<uint8_t> val((size_t)M * 32, 0);
    for (uint32_t i = 0; i < M; i++) std::memcpy(&val[(size_t)i * 32], &v[i], 8);
    unsigned l0 = 0;
    while (((uint64_t)1 << l0) < M) l0++;
    l0 = std::min(l0, depth);
    const uint64_t n = view_nodes(M, depth);
    std::vector<uint8_t> cls(n, 0xee);
    std::vector<uint32_t> rank(n, 0xeeeeeeeeu);
    std::vector<uint64_t> count(depth + 1);
    const int R = view_host(val.data(), sorted.data(), M, s, 0, l0, depth, cls.data(), rank.data(), count.data());
    if (R < 0) return 1;
    std::set<uint64_t> level;
    if (s < M) {
        for (uint32_t j = 0; j + 1 < M; j++)
            if (sorted[j] < s && sorted[j + 1] >= s) level.insert(sorted[j]);
        if ((int)level.size() != R) return 2;
        level.insert(s);
    }
    size_t k = 0;
    for (unsigned l = 0; l <= depth; l++) {
        const std::vector<uint64_t> asc(level.begin(), level.end());
        for (uint64_t x = 0; x <= view_filled(M, l); x++, k++) {
            if (s == M && l >= l0) continue;
            int want = imt::view::STORED;
            uint32_t r = 0;
            const auto it = std::lower_bound(asc.begin(), asc.end(), x);
            if (x >= view_filled(s, l)) want = imt::view::EMPTY;
            else if (it != asc.end() && *it == x) { want = imt::view::SIDE; r = (uint32_t)(it - asc.begin()); }
            if (cls[k] != want || rank[k] != r) return 3;
        }
        std::set<uint64_t> up;
        for (uint64_t x : level) up.insert(x >> 1);
        level.swap(up);
    }
    return 0;
}

}  // namespace

int main() {
    uint64_t seed = 0x56494557;
    auto next = [&] { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (seed >> 11) | 1; };
    const uint32_t sizes[] = {2, 3, 18, 300, 1024, 1025};
    unsigned runs = 0;
    for (int kind = 0; kind < 3; kind++)
        for (uint32_t M : sizes)
            for (unsigned depth : {12u, 64u}) {
                if (depth == 64 && M > 18) continue;
                std::set<uint64_t> distinct;
                while (distinct.size() + 1 < M) distinct.insert(next());
                std::vector<uint64_t> v(distinct.begin(), distinct.end());       // ascending
                if (kind == 1) std::reverse(v.begin(), v.end());
                if (kind == 2)
                    for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[next() % i]);
                v.insert(v.begin(), 0);                                          // the sentinel
                std::set<uint32_t> cuts{1, 2, M - 1, M};
                for (uint32_t p = 2; p < M; p *= 2) { cuts.insert(p - 1); cuts.insert(p + 1); }
                for (uint32_t s : cuts) {
                    if (s < 1 || s > M) continue;
                    const int rc = check(v, s, depth);
                    if (rc) {
                        std::printf("view_lists: kind %d M %u s %u depth %u: check %d failed\n", kind, M, s, depth, rc);
                        return 1;
                    }
                    runs++;
                }
            }
    std::printf("view_lists: %u cuts ok\n", runs);
    return 0;
}
#endif
