// replay_mixed_rules.cpp -- TEST INFRASTRUCTURE: a mixed list replayed against the rows the tree stores
// (imt_itree_view_mixed_witness), on the CPU, through the functions the device runs: replay_op_class, read_neighbours,
// insert_is_duplicate and the nearest_* searches (csrc/imt_prep_logic.hpp) over arrays built the way prep::mixed_ranks /
// mixed_check_view build them, then sweep::merge_element for the tables of the events and replay::sibling_source -- what
// k_sweep_view_mixed asks -- for the source of every event's sibling at every level below L0.  The view's lists are built
// by tests/native/replay_sources.cpp's build_view, included as it is.  A stand-alone program: it reads cases from standard
// input and prints what the rules say; tests/test_replay_mixed_logic.py feeds it and compares with a plain walk over a
// sorted list and with set arithmetic.
//
// Input, repeated until end of file (values are 64 hex digits, most significant first):
//     C S M n depth
//     <M values: the tree's rows in leaf order, leaf 0 = the sentinel 0; the view is at S <= M>
//     <n lines: op value>            op: 0 = INSERT, 1 = READ
// Output per case, one of
//     range                          the list holds more INSERTs than the tree holds leaves beyond S
//     bad <p>                        the smallest offending position
//     ok <L0> <E>                    then n lines "kind low succ" (rows of the tree, succ -1 = none) and, when S < M, L0 lines
//                                    of E digits: the class of the sibling of event e at that level (0 EMPTY, 1 SIDE,
//                                    2 STORED, 3 BATCH); L0 is printed as 0 when S == M (no view is built then)
#include <cstdio>
#include "imt_prep_logic.hpp"
#include "replay_sources.cpp"

using namespace imt::prep;

namespace {

bool parse256(const char* hex, uint8_t* out) {
    if (std::strlen(hex) != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned b;
        if (std::sscanf(hex + 2 * i, "%2x", &b) != 1) return false;
        out[31 - i] = (uint8_t)b;                 // little-endian bytes
    }
    return true;
}

int levels_for(uint32_t n) {
    int k = 1;
    while ((1u << k) <= n) k++;
    return k;
}

}  // namespace

int main() {
    unsigned S, M, n, depth;
    char tag[8], hex[128];
    int cases = 0;
    while (std::scanf("%7s %u %u %u %u", tag, &S, &M, &n, &depth) == 5) {
        if (tag[0] != 'C' || S == 0 || S > M || n == 0 || depth == 0 || depth > 64) return 2;
        // 8-byte aligned rows: the rules read values as 64-bit limbs
        std::vector<uint64_t> val_store((size_t)M * 4), in_store((size_t)n * 4);
        uint8_t* val = reinterpret_cast<uint8_t*>(val_store.data());
        uint8_t* vals = reinterpret_cast<uint8_t*>(in_store.data());
        std::vector<uint8_t> op(n);
        for (unsigned i = 0; i < M; i++)
            if (std::scanf("%127s", hex) != 1 || !parse256(hex, val + (size_t)i * 32)) return 2;
        for (unsigned p = 0; p < n; p++) {
            unsigned o;
            if (std::scanf("%u %127s", &o, hex) != 2 || o > 1 || !parse256(hex, vals + (size_t)p * 32)) return 2;
            op[p] = (uint8_t)o;
        }
        cases++;
        auto by_value = [&](uint32_t a, uint32_t b) { return lt256(val + (size_t)a * 32, val + (size_t)b * 32); };
        std::vector<uint32_t> sorted_view(S), sorted_all(M);
        std::iota(sorted_view.begin(), sorted_view.end(), 0u);
        std::iota(sorted_all.begin(), sorted_all.end(), 0u);
        std::sort(sorted_view.begin(), sorted_view.end(), by_value);
        std::sort(sorted_all.begin(), sorted_all.end(), by_value);
        // mixed_ranks: flag, rank, the number of INSERTs; then the range, before any row beyond the tree is looked at
        std::vector<uint32_t> flag(n), rank(n), ipos(n), iota(n);
        uint32_t n_ins = 0;
        for (unsigned p = 0; p < n; p++) {
            flag[p] = op[p] == 0;
            rank[p] = n_ins;
            n_ins += flag[p];
        }
        if (n_ins > M - S) {
            std::printf("range\n");
            continue;
        }
        // mixed_check_view: k_mixed_match, then the checks of mixed_check over the STORED rows [S, S + n_ins)
        std::vector<int> err(n, 0);
        for (unsigned p = 0; p < n; p++) {
            err[p] |= replay_op_class(vals + (size_t)p * 32, flag[p] != 0, rank[p], val, S, 0, 0);
            if (!flag[p]) continue;
            iota[rank[p]] = S + rank[p];
            ipos[rank[p]] = p;
        }
        std::vector<uint32_t> bsorted(iota.begin(), iota.begin() + n_ins);
        std::sort(bsorted.begin(), bsorted.end(), [&](uint32_t a, uint32_t b) {
            const uint8_t *x = val + (size_t)a * 32, *y = val + (size_t)b * 32;
            return lt256(x, y) || (a < b && !lt256(y, x));
        });
        const int levels = levels_for(n_ins);
        std::vector<uint32_t> gap(n_ins), st((size_t)levels * n_ins + 1), low(n), succ(n);
        for (uint32_t j = 0; j < n_ins; j++) {
            gap[j] = count_below(val, sorted_view.data(), S, val + (size_t)bsorted[j] * 32);
            st[j] = bsorted[j] - S;
            if (insert_is_duplicate(val, sorted_view.data(), S, bsorted.data(), j, gap[j])) err[ipos[st[j]]] |= OP_DUPLICATE;
        }
        for (int k = 1; k < levels; k++)
            for (uint32_t j = 0; j + (1u << k) <= n_ins; j++)
                st[(size_t)k * n_ins + j] = std::min(st[(size_t)(k - 1) * n_ins + j], st[(size_t)(k - 1) * n_ins + j + (1u << (k - 1))]);
        for (uint32_t j = 0; j < n_ins; j++) {     // k_neighbours
            const uint32_t g = gap[j], t = st[j];
            const uint32_t jl = nearest_smaller_left(st.data(), n_ins, levels, j);
            const uint32_t jr = nearest_smaller_right(st.data(), n_ins, levels, j);
            low[t] = (jl < n_ins && gap[jl] == g) ? bsorted[jl] : sorted_view[g > 0 ? g - 1 : 0];
            succ[t] = (jr < n_ins && gap[jr] == g) ? bsorted[jr] : (g < S ? sorted_view[g] : OP_NONE);
        }
        for (unsigned p = 0; p < n; p++) {
            if (flag[p]) continue;
            const ReadAnswer a = read_neighbours(vals + (size_t)p * 32, rank[p], val, sorted_view.data(), S, bsorted.data(),
                                                 gap.data(), st.data(), n_ins, levels, 0, 0);
            err[p] |= a.err;
            low[n_ins + (p - rank[p])] = a.low;
            succ[n_ins + (p - rank[p])] = a.succ;
        }
        uint32_t bad = OP_NONE;
        for (unsigned p = 0; p < n; p++)
            if (err[p] && p < bad) bad = p;
        if (bad != OP_NONE) {
            std::printf("bad %u\n", bad);
            continue;
        }
        // accepted: the events (k_mixed_events' keys), their tables level by level, the source of every sibling
        const uint32_t E = n + n_ins;
        unsigned L0 = std::min(ceil_log2((uint64_t)S + n_ins), depth);
        ViewLists vl;
        if (S == M) L0 = 0;
        else if (!build_view(val, sorted_all.data(), M, S, depth, vl)) return 3;
        std::printf("ok %u %u\n", L0, E);
        std::vector<uint64_t> keys(E);
        for (unsigned p = 0; p < n; p++) {
            const uint32_t e = p + rank[p], at = flag[p] ? rank[p] : n_ins + (p - rank[p]);
            keys[e] = ((uint64_t)low[at] << 32) | e;
            if (flag[p]) keys[e + 1] = ((uint64_t)(S + rank[p]) << 32) | (e + 1);
            std::printf("%c %u %ld\n", flag[p] ? 'I' : 'R', low[at], succ[at] == OP_NONE ? -1L : (long)succ[at]);
        }
        if (L0 == 0) continue;
        const imt::view::Side side{vl.node.data(), vl.count.data(), vl.stride, vl.top, S, nullptr, nullptr};
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
        std::vector<char> line(E + 1, '\0');
        for (unsigned l = 0; l < L0; l++) {
            const int a = l & 1, b = a ^ 1;
            const imt::sweep::LevelTable in{tab[a][0].data(), tab[a][1].data(), tab[a][2].data(), tab[a][3].data()};
            const imt::sweep::LevelOut o{tab[b][0].data(), tab[b][1].data(), tab[b][2].data(), tab[b][3].data(),
                                         from.data(), sibsrc.data(), nodeb.data(), nullptr};
            for (uint32_t k = 0; k < E; k++) imt::sweep::merge_element(in, o, k, E);
            for (uint32_t kp = 0; kp < E; kp++) {
                const imt::replay::Source src = imt::replay::sibling_source(side, sibsrc[kp], l, (uint64_t)(nodeb[kp] ^ 1u));
                line[o.time[kp]] = (char)('0' + src.cls);
            }
            std::printf("%s\n", line.data());
        }
    }
    std::printf("cases %d ok\n", cases);
    return 0;
}
