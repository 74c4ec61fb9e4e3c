// apply_lists.cpp -- TEST INFRASTRUCTURE: the list building of imt_itree_apply_batch (csrc/imt_apply.hpp) on the CPU.
// The device runs one exclusive scan of apply::head per level and one scatter_element per (slot, level); this file
// does the same with a sequential scan, over the same functions (tests/test_apply_schedule.py).
#include <cstdint>
#include <vector>
#include "imt_apply.hpp"

extern "C" {

// node / time / re: the level-0 table ([total], events ordered by (position, time)).  Writes lists_node [l0][total],
// src [total], count [depth + 1]; returns 0, or -1 for arguments apply_lists refuses.
int apply_lists_host(const uint32_t* node, const uint32_t* time, const uint32_t* re, uint32_t total, unsigned l0,
                     unsigned depth, uint32_t* lists_node, uint32_t* src, uint64_t* count) {
    if (total == 0 || l0 == 0 || l0 > 31 || l0 > depth) return -1;
    const imt::apply::Lists o{lists_node, src, count, total};
    for (unsigned l = 0; l < l0; l++) {
        uint32_t pos = 0;
        for (uint32_t x = 0; x < total; x++) {
            imt::apply::scatter_element(node, time, re, total, x, l, pos, l0, depth, o);
            pos += imt::apply::head(node, x, l);
        }
    }
    return 0;
}

uint32_t apply_bound(uint32_t total, unsigned l0, unsigned l) { return imt::apply::bound(total, l0, l); }

}
