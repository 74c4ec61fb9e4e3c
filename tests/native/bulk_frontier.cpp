// bulk_frontier.cpp -- TEST INFRASTRUCTURE: the frontier behind a bulk replay (csrc/imt_replay.hpp frontier_*) on the CPU.
// The device sweeps the n rewrites of stored low leaves level by level over the tables of imt_sweep.hpp and, between the
// level launches, keeps the final version of the one node per level that is a left-hand sibling of the first free slot S
// (k_bulk_frontier_base, k_bulk_frontier_level, the copy at the first upper level).  This file composes the same functions
// over the same tables with "versions" that are labels (level, event) instead of hashes (tests/test_bulk_frontier_rule.py).
// With -DBULK_FRONTIER_MAIN it is a program of its own that checks scripts against a linear walk, for a run under the
// host sanitizers.
#include <algorithm>
#include <cstdint>
#include <vector>
#include "imt_replay.hpp"

using namespace imt;

namespace {
unsigned ceil_log2(uint64_t x) {
    unsigned l = 0;
    while (l < 64 && ((uint64_t)1 << l) < x) l++;
    return l;
}
}  // namespace

extern "C" {

// S: the view's size (>= 1); low [n]: the low leaf of every event in event order, each < S.  Per level l < depth:
// cls[l] = replay::FRONTIER_ZERO / _VIEW / _VERSION, node[l] = the frontier's node of level l (0 for ZERO), event[l] = the
// event whose version it is (VERSION only, else 0xffffffff), hits[l] = how many slots of the level claimed the version (the
// device lets every such slot store: more than one would be a race).  Returns 0, or 1 for arguments it cannot take.
int bulk_frontier_host(uint64_t S, unsigned depth, const uint32_t* low, uint32_t n, int* cls, uint64_t* node, uint32_t* event,
                       uint32_t* hits) {
    if (S == 0 || depth == 0 || depth > 32 || n == 0) return 1;
    for (uint32_t k = 0; k < n; k++)
        if (low[k] >= S) return 1;
    const unsigned top = std::min(ceil_log2(S), depth);
    // the level-0 table as the preparation leaves it: the events sorted by (low leaf, event), runs of one leaf
    std::vector<uint64_t> keys(n);
    for (uint32_t k = 0; k < n; k++) keys[k] = ((uint64_t)low[k] << 32) | k;
    std::sort(keys.begin(), keys.end());
    std::vector<uint32_t> tab[2][4];
    for (auto& t : tab)
        for (auto& c : t) c.assign(n, 0);
    for (uint32_t s = 0; s < n; s++) {
        tab[0][0][s] = (uint32_t)(keys[s] >> 32);
        tab[0][1][s] = (uint32_t)keys[s];
    }
    for (uint32_t s = 0; s < n; s++) {
        uint32_t a = s, b = s + 1;
        while (a > 0 && tab[0][0][a - 1] == tab[0][0][s]) a--;
        while (b < n && tab[0][0][b] == tab[0][0][s]) b++;
        tab[0][2][s] = a;
        tab[0][3][s] = b;
    }
    // before the sweep: every row as no event had touched it
    for (unsigned l = 0; l < depth; l++) {
        cls[l] = replay::frontier_base(S, l);
        node[l] = cls[l] == replay::FRONTIER_VIEW ? replay::frontier_node(S, l) : 0;
        event[l] = 0xffffffffu;
        hits[l] = 0;
    }
    // the versions of level l by slot are labelled with the event that made them: time_l[slot]
    std::vector<uint32_t> time_l = tab[0][1], from(n), nodeb(n), timen(n);
    std::vector<int32_t> sibsrc(n);
    for (unsigned l = 0; l < top; l++) {
        const int a = l & 1, b = a ^ 1;
        const sweep::LevelTable in{tab[a][0].data(), time_l.data(), tab[a][2].data(), tab[a][3].data()};
        const sweep::LevelOut out{tab[b][0].data(), timen.data(), tab[b][2].data(), tab[b][3].data(), from.data(), sibsrc.data(),
                                  nodeb.data(), nullptr};
        for (uint32_t k = 0; k < n; k++) sweep::merge_element(in, out, k, n);
        for (uint32_t kp = 0; kp < n; kp++) {          // k_bulk_frontier_level: one thread per slot of level l + 1
            uint32_t slot;
            if (!replay::frontier_version(S, l, from[kp], nodeb[kp], slot) || slot >= n) continue;
            cls[l] = replay::FRONTIER_VERSION;
            event[l] = time_l[slot];
            hits[l]++;
        }
        time_l = timen;
    }
    uint32_t slot;                                     // from here up the versions are by event
    if (top < depth && replay::frontier_top_version(S, top, n, slot)) {
        cls[top] = replay::FRONTIER_VERSION;
        event[top] = slot;
        hits[top]++;
    }
    return 0;
}

}  // extern "C"

#ifdef BULK_FRONTIER_MAIN
#include <cstdio>
// The linear walk: writer[l][x] = the last event whose low leaf lies under node x of level l.  Row l of the frontier of
// slot S is then Z[l] where bit l of S is clear, the version of writer[l][(S >> l) - 1] if there is one, else the view's node.
namespace {
int check(uint64_t S, unsigned depth, const std::vector<uint32_t>& low) {
    const uint32_t n = (uint32_t)low.size();
    std::vector<int> cls(depth);
    std::vector<uint64_t> node(depth);
    std::vector<uint32_t> event(depth), hits(depth);
    if (bulk_frontier_host(S, depth, low.data(), n, cls.data(), node.data(), event.data(), hits.data())) return 1;
    for (unsigned l = 0; l < depth; l++) {
        if (!((S >> l) & 1)) {
            if (cls[l] != replay::FRONTIER_ZERO || hits[l]) return 2;
            continue;
        }
        const uint64_t y = (S >> l) - 1;
        int64_t writer = -1;
        for (uint32_t k = 0; k < n; k++)
            if (((uint64_t)low[k] >> l) == y) writer = k;
        if (node[l] != y) return 3;
        if (writer < 0 ? (cls[l] != replay::FRONTIER_VIEW || hits[l]) : (cls[l] != replay::FRONTIER_VERSION || hits[l] != 1 || event[l] != (uint32_t)writer))
            return 4;
    }
    return 0;
}
}  // namespace

int main() {
    unsigned long scripts = 0;
    for (uint64_t S = 1; S <= 12; S++)                  // every sequence of 1 .. 4 low leaves below S, at two depths
        for (unsigned n = 1; n <= 4; n++) {
            uint64_t count = 1;
            for (unsigned q = 0; q < n; q++) count *= S;
            for (uint64_t code = 0; code < count; code++) {
                std::vector<uint32_t> low;
                uint64_t c = code;
                for (unsigned q = 0; q < n; q++, c /= S) low.push_back((uint32_t)(c % S));
                for (unsigned depth : {4u, 9u}) {
                    const int rc = check(S, depth, low);
                    if (rc) {
                        std::printf("S %llu depth %u script %lu: mismatch %d\n", (unsigned long long)S, depth, scripts, rc);
                        return 1;
                    }
                    scripts++;
                }
            }
        }
    uint64_t x = 0x9E3779B97F4A7C15ull;                 // larger scripts: S up to 2^12, crowded and sparse
    auto next = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (unsigned it = 0; it < 4000; it++) {
        const uint64_t S = it % 7 == 0 ? (uint64_t)1 << (1 + next() % 12) : 1 + next() % 4096;
        const unsigned n = 1 + (unsigned)(next() % 200);
        const uint64_t span = it % 3 == 0 ? std::min<uint64_t>(S, 1 + next() % 8) : S;      // all of the batch in a few leaves
        const uint64_t base = next() % (S - span + 1);
        std::vector<uint32_t> low(n);
        for (auto& v : low) v = (uint32_t)(base + next() % span);
        const int rc = check(S, 14, low);
        if (rc) {
            std::printf("random script %u: mismatch %d\n", it, rc);
            return 1;
        }
        scripts++;
    }
    std::printf("bulk_frontier: %lu scripts agree with the linear walk\n", scripts);
    return 0;
}
#endif
