// rewind_lists.cpp -- TEST INFRASTRUCTURE: the index work of imt_itree_rewind (csrc/imt_rewind.hpp) on the CPU.
// The device runs one exclusive scan of rewind::scan_flag, one compact_element and one relink_element per index entry, a
// sort of the emitted positions, and the list building of imt_apply.hpp over the sorted table; this file does the same
// with a sequential scan and std::stable_sort, over the same functions (tests/test_rewind_logic.py).
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>
#include "imt_apply.hpp"
#include "imt_rewind.hpp"

extern "C" {

// val [M][32], sorted [M]: the index of a tree of M leaves; s in [1, M].  Writes compact [s], and for s < M the table
// node / time [R + 1] (positions ascending and the preimage row of each), pre [R + 1][96], rs / re [R + 1],
// lists_node [l0][min(M - s, s) + 1] and count [depth + 1] as prep::apply_lists leaves them.  Arrays for the table hold
// min(M - s, s) + 1 rows.  Returns R, the number of relinked leaves, or -1 for arguments the device code refuses.
int rewind_host(const uint8_t* val, const uint32_t* sorted, uint32_t M, uint32_t s, uint64_t base, unsigned l0, unsigned depth,
                uint32_t* compact, uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re, uint8_t* pre,
                uint32_t* lists_node, uint64_t* count) {
    if (s == 0 || s > M) return -1;
    std::vector<uint64_t> pos(M);
    uint64_t run = 0;
    for (uint32_t j = 0; j < M; j++) {
        pos[j] = run;
        run += imt::rewind::scan_flag(sorted, M, j, s);
    }
    uint32_t R = 0xffffffffu;
    for (uint32_t j = 0; j < M; j++) imt::rewind::compact_element(sorted, M, j, s, pos[j], compact, &R);
    if (s == M) return (int)R;
    const uint32_t rows = R + 1, max_rows = std::min(M - s, s) + 1;
    if (rows > max_rows || l0 == 0 || l0 > 31 || l0 > depth) return -1;
    std::vector<uint32_t> key(rows, 0xffffffffu), row(rows, 0xffffffffu);
    const imt::rewind::Table t{key.data(), row.data(), rs, re, pre, rows};
    for (uint32_t j = 0; j < M; j++) imt::rewind::relink_element(val, sorted, compact, M, j, s, pos[j], base, t);
    std::vector<uint32_t> ord(rows);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    for (uint32_t x = 0; x < rows; x++) {
        node[x] = key[ord[x]];
        time[x] = row[ord[x]];
    }
    std::vector<uint32_t> src(max_rows);
    const imt::apply::Lists o{lists_node, src.data(), count, max_rows};
    for (unsigned l = 0; l < l0; l++) {
        uint32_t p = 0;
        for (uint32_t x = 0; x < rows; x++) {
            imt::apply::scatter_element(node, time, re, rows, x, l, p, l0, depth, o);
            p += imt::apply::head(node, x, l);
        }
    }
    for (uint32_t x = 0; x < rows; x++)
        if (src[x] != time[x]) return -1;       // one event per run: a leaf's final preimage is its only one
    return (int)R;
}

void rewind_refill_range(uint64_t s, uint64_t M, unsigned l, uint64_t* lo, uint64_t* hi) {
    imt::rewind::refill_range(s, M, l, lo, hi);
}

}
