// replay_sources.cpp -- TEST INFRASTRUCTURE: where a replayed insertion reads its siblings (csrc/imt_replay.hpp), on the CPU.
// The view's lists are built the way a view's build builds them (tests/native/view_lists.cpp is the model), the sweep
// tables of the replayed events level by level with sweep::merge_element, and for every event and level below L0 the
// sibling's source is what replay::sibling_source -- the function k_sweep_view runs -- says.
// tests/test_replay_logic.py loads it as a library and checks every answer against the oracle; built with
// -DREPLAY_SOURCES_MAIN it is a stand-alone program that runs a grid of its own against a brute-force restatement, for a
// sanitizer build.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <numeric>
#include <vector>
#include "imt_apply.hpp"
#include "imt_replay.hpp"
#include "imt_rewind.hpp"
#include "imt_sweep.hpp"
#include "imt_view.hpp"

namespace {

typedef std::array<uint64_t, 4> Key;        // a value's limbs, most significant first: the array order is the value order
Key key_of(const uint8_t* v) {
    Key k;
    for (int i = 0; i < 4; i++) std::memcpy(&k[i], v + 8 * (3 - i), 8);
    return k;
}

unsigned ceil_log2(uint64_t x) {
    unsigned l = 0;
    while (l < 63 && ((uint64_t)1 << l) < x) l++;
    return l;
}

// the lists of a view at size s of the tree of M leaves (s < M): rows [top][stride] and the counts
struct ViewLists {
    std::vector<uint32_t> node;
    std::vector<uint64_t> count;
    uint32_t stride = 0;
    unsigned top = 0;
};
bool build_view(const uint8_t* val, const uint32_t* sorted, uint32_t M, uint32_t s, unsigned depth, ViewLists& out) {
    const unsigned l0 = std::min(ceil_log2(M), depth);
    if (l0 == 0 || l0 > 31) return false;
    std::vector<uint64_t> pos(M);
    uint64_t run = 0;
    for (uint32_t j = 0; j < M; j++) {
        pos[j] = run;
        run += imt::rewind::scan_flag(sorted, M, j, s);
    }
    uint32_t R = 0xffffffffu;
    std::vector<uint32_t> compact(s);
    for (uint32_t j = 0; j < M; j++) imt::rewind::compact_element(sorted, M, j, s, pos[j], compact.data(), &R);
    const uint32_t max_rows = std::min(M - s, s) + 1, rows = R + 1;
    if (rows > max_rows) return false;
    out.stride = max_rows;
    out.top = l0;
    out.node.assign((size_t)l0 * max_rows, 0xffffffffu);
    out.count.assign(depth + 1, 0);
    std::vector<uint32_t> key(rows, 0xffffffffu), row(rows, 0xffffffffu), rs(rows), re(rows), node(rows), time(rows);
    std::vector<uint8_t> pre((size_t)rows * 96);
    const imt::rewind::Table t{key.data(), row.data(), rs.data(), re.data(), pre.data(), rows};
    for (uint32_t j = 0; j < M; j++) imt::rewind::relink_element(val, sorted, compact.data(), M, j, s, pos[j], 0, t);
    std::vector<uint32_t> ord(rows);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    for (uint32_t x = 0; x < rows; x++) {
        node[x] = key[ord[x]];
        time[x] = row[ord[x]];
    }
    std::vector<uint32_t> src(max_rows);
    const imt::apply::Lists o{out.node.data(), src.data(), out.count.data(), max_rows};
    for (unsigned l = 0; l < l0; l++) {
        uint32_t p = 0;
        for (uint32_t x = 0; x < rows; x++) {
            imt::apply::scatter_element(node.data(), time.data(), re.data(), rows, x, l, p, l0, depth, o);
            p += imt::apply::head(node.data(), x, l);
        }
    }
    return true;
}

}  // namespace

extern "C" {

// val [M][32], sorted [M]: the index of a tree of M leaves.  The n insertions that followed size s (1 <= s, s + n <= M,
// n >= 1) are replayed against the view at s.  For event e (2i: the low leaf of insertion i rewritten, 2i + 1: leaf s + i
// written) and level l < L0 = min(ceil(log2(s + n)), depth): cls[l * 2n + e] = the source of its sibling and at[l * 2n + e]
// = the time of the event that made it (BATCH), its place in the level's list (SIDE) or 0.  low [n]: the low leaf of every
// insertion.  Returns L0, or -1 for arguments the library refuses.
int replay_sources(const uint8_t* val, const uint32_t* sorted, uint32_t M, uint32_t s, uint32_t n, unsigned depth, uint8_t* cls,
                   uint32_t* at, uint32_t* low) {
    if (s == 0 || n == 0 || (uint64_t)s + n > M || depth == 0 || depth > 64) return -1;
    ViewLists vl;
    if (!build_view(val, sorted, M, s, depth, vl)) return -1;
    const imt::view::Side side{vl.node.data(), vl.count.data(), vl.stride, vl.top, s, nullptr, nullptr};
    const unsigned L0 = std::min(ceil_log2((uint64_t)s + n), depth);
    const uint32_t E = 2 * n;
    // the low leaf of every replayed insertion: the greatest value below it among the leaves before it
    std::map<Key, uint32_t> stored;
    for (uint32_t i = 0; i < s; i++) stored[key_of(val + (size_t)i * 32)] = i;
    std::vector<uint64_t> keys(E);
    for (uint32_t i = 0; i < n; i++) {
        const Key k = key_of(val + (size_t)(s + i) * 32);
        auto it = stored.lower_bound(k);
        if (it == stored.begin() || (it != stored.end() && it->first == k)) return -1;
        low[i] = std::prev(it)->second;
        stored[k] = s + i;
        keys[2 * i] = ((uint64_t)low[i] << 32) | (2 * i);
        keys[2 * i + 1] = ((uint64_t)(s + i) << 32) | (2 * i + 1);
    }
    std::sort(keys.begin(), keys.end());
    std::vector<uint32_t> tab[2][4];
    for (auto& side_tabs : tab)
        for (auto& t : side_tabs) t.assign(E, 0xffffffffu);
    for (uint32_t k = 0; k < E;) {
        uint32_t j = k;
        while (j < E && (keys[j] >> 32) == (keys[k] >> 32)) j++;
        for (uint32_t x = k; x < j; x++) {
            tab[0][0][x] = (uint32_t)(keys[x] >> 32);
            tab[0][1][x] = (uint32_t)keys[x];
            tab[0][2][x] = k;
            tab[0][3][x] = j;
        }
        k = j;
    }
    std::vector<uint32_t> from(E), nodeb(E);
    std::vector<int32_t> sibsrc(E);
    for (unsigned l = 0; l < L0; l++) {
        const int a = l & 1, b = a ^ 1;
        const imt::sweep::LevelTable in{tab[a][0].data(), tab[a][1].data(), tab[a][2].data(), tab[a][3].data()};
        const imt::sweep::LevelOut o{tab[b][0].data(), tab[b][1].data(), tab[b][2].data(), tab[b][3].data(),
                                     from.data(), sibsrc.data(), nodeb.data(), nullptr};
        for (uint32_t k = 0; k < E; k++) imt::sweep::merge_element(in, o, k, E);
        for (uint32_t kp = 0; kp < E; kp++) {
            const uint32_t e = o.time[kp];
            const imt::replay::Source src = imt::replay::sibling_source(side, sibsrc[kp], l, (uint64_t)(nodeb[kp] ^ 1u));
            cls[(size_t)l * E + e] = (uint8_t)src.cls;
            at[(size_t)l * E + e] = src.cls == imt::replay::BATCH ? in.time[src.at] : src.at;
        }
    }
    return (int)L0;
}

}

#ifdef REPLAY_SOURCES_MAIN
#include <cstdio>
#include <set>

namespace {

// the same answers from the definitions alone
int check(const std::vector<uint64_t>& v, uint32_t s, uint32_t n, unsigned depth) {
    const uint32_t M = (uint32_t)v.size(), E = 2 * n;
    std::vector<uint32_t> sorted(M);
    std::iota(sorted.begin(), sorted.end(), 0u);
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return v[a] < v[b]; });
    std::vector<uint8_t> val((size_t)M * 32, 0);
    for (uint32_t i = 0; i < M; i++) std::memcpy(&val[(size_t)i * 32], &v[i], 8);
    const unsigned L0 = std::min(ceil_log2((uint64_t)s + n), depth);
    std::vector<uint8_t> cls((size_t)std::max(L0, 1u) * E, 0xee);
    std::vector<uint32_t> at((size_t)std::max(L0, 1u) * E, 0xeeeeeeeeu), low(n);
    if (replay_sources(val.data(), sorted.data(), M, s, n, depth, cls.data(), at.data(), low.data()) != (int)L0) return 1;
    std::vector<uint32_t> pos(E);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t best = 0;                              // the sentinel is below everything
        for (uint32_t j = 0; j < s + i; j++)
            if (v[j] < v[s + i] && v[j] >= v[best]) best = j;
        if (low[i] != best) return 2;
        pos[2 * i] = best;
        pos[2 * i + 1] = s + i;
    }
    std::set<uint64_t> level;                           // S_0: the kept leaves whose successor is removed, and slot s
    for (uint32_t j = 0; j + 1 < M; j++)
        if (sorted[j] < s && sorted[j + 1] >= s) level.insert(sorted[j]);
    level.insert(s);
    for (unsigned l = 0; l < L0; l++) {
        const std::vector<uint64_t> asc(level.begin(), level.end());
        for (uint32_t e = 0; e < E; e++) {
            const uint64_t y = ((uint64_t)pos[e] >> l) ^ 1;
            int want = imt::replay::STORED;
            uint32_t w = 0;
            bool batch = false;
            for (uint32_t f = e; f-- > 0;)
                if (((uint64_t)pos[f] >> l) == y) { batch = true; w = f; break; }
            const auto it = std::lower_bound(asc.begin(), asc.end(), y);
            if (batch) want = imt::replay::BATCH;
            else if (y >= imt::view::filled(s, l)) want = imt::replay::EMPTY;
            else if (it != asc.end() && *it == y) { want = imt::replay::SIDE; w = (uint32_t)(it - asc.begin()); }
            if (cls[(size_t)l * E + e] != want || at[(size_t)l * E + e] != w) return 3;
        }
        std::set<uint64_t> up;
        for (uint64_t x : level) up.insert(x >> 1);
        level.swap(up);
    }
    return 0;
}

}  // namespace

int main() {
    uint64_t seed = 0x5245504c;
    auto next = [&] { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (seed >> 11) | 1; };
    const uint32_t sizes[] = {2, 3, 18, 300, 1025};
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
                std::set<uint32_t> cuts{1, 2, M - 1};
                for (uint32_t p = 2; p < M; p *= 2) { cuts.insert(p - 1); cuts.insert(p + 1); }
                for (uint32_t s : cuts) {
                    if (s < 1 || s >= M) continue;
                    for (uint32_t n : std::set<uint32_t>{1, M - s, std::max(1u, (M - s) / 2)}) {
                        const int rc = check(v, s, n, depth);
                        if (rc) {
                            std::printf("replay_sources: kind %d M %u s %u n %u depth %u: check %d failed\n", kind, M, s, n, depth, rc);
                            return 1;
                        }
                        runs++;
                    }
                }
            }
    std::printf("replay_sources: %u replays ok\n", runs);
    return 0;
}
#endif
