// resize_levels.cpp -- TEST INFRASTRUCTURE: the layout arithmetic of imt_itree_reserve (csrc/imt_resize.hpp) on the CPU.
// The device runs resize::source_of once per 16-byte half of every node of the new array (k_restride_levels); this file
// runs it once per node, sequentially, over the same functions (tests/test_resize_logic.py).  Built with
// -DRESIZE_LEVELS_MAIN it is a program of its own that re-lays a tagged array out and back and checks it, for a run
// under the host sanitizers.
#include <cstdint>
#include <cstring>
#include <vector>
#include "imt_resize.hpp"

extern "C" {

uint64_t resize_level_len(uint64_t cap, unsigned l) { return imt::resize::level_len(cap, l); }
uint64_t resize_level_off(uint64_t cap, unsigned l) { return imt::resize::level_off(cap, l); }
uint64_t resize_total_nodes(uint64_t cap, unsigned depth) { return imt::resize::total_nodes(cap, depth); }

// level and position of flat node `flat` of the layout (cap, depth); -1 if flat is outside it
int resize_locate(uint64_t cap, unsigned depth, uint64_t flat, unsigned* level, uint64_t* pos) {
    if (flat >= imt::resize::total_nodes(cap, depth)) return -1;
    std::vector<uint64_t> off(depth + 1);
    for (unsigned l = 0; l <= depth; l++) off[l] = imt::resize::level_off(cap, l);
    imt::resize::locate(off.data(), depth, flat, level, pos);
    return 0;
}

// old_nodes [total_nodes(old_cap, depth)][32] -> new_nodes [total_nodes(new_cap, depth)][32], zero [depth + 1][32];
// returns the number of nodes that came from `zero`
uint64_t resize_host(const uint8_t* old_nodes, uint64_t old_cap, uint8_t* new_nodes, uint64_t new_cap, unsigned depth,
                     const uint8_t* zero) {
    std::vector<uint64_t> old_off(depth + 1), old_len(depth + 1), new_off(depth + 1);
    for (unsigned l = 0; l <= depth; l++) {
        old_off[l] = imt::resize::level_off(old_cap, l);
        old_len[l] = imt::resize::level_len(old_cap, l);
        new_off[l] = imt::resize::level_off(new_cap, l);
    }
    const uint64_t total = imt::resize::total_nodes(new_cap, depth);
    uint64_t zeros = 0;
    for (uint64_t flat = 0; flat < total; flat++) {
        unsigned l;
        const uint64_t src = imt::resize::source_of(new_off.data(), old_off.data(), old_len.data(), depth, flat, &l);
        const bool z = src == ~(uint64_t)0;
        std::memcpy(new_nodes + flat * 32, z ? zero + (size_t)l * 32 : old_nodes + src * 32, 32);
        zeros += z;
    }
    return zeros;
}

}

#ifdef RESIZE_LEVELS_MAIN
#include <cstdio>
// node i of level l carries (l, i) in its 32 bytes, Z[l] carries (l, all ones)
static void tag(uint8_t* row, uint64_t l, uint64_t i) {
    const uint64_t w[4] = {l, i, ~l, ~i};
    std::memcpy(row, w, 32);
}
int main() {
    const unsigned depths[] = {1, 2, 5, 32, 33, 63, 64};
    unsigned long checked = 0;
    for (unsigned depth : depths) {
        std::vector<uint8_t> zero((depth + 1) * 32);
        for (unsigned l = 0; l <= depth; l++) tag(&zero[l * 32], l, ~(uint64_t)0);
        for (uint64_t a = 2; a <= 4096; a *= 2)
            for (uint64_t b = 2; b <= 4096; b *= 2) {
                if (depth < 63 && (a > ((uint64_t)1 << depth) || b > ((uint64_t)1 << depth))) continue;
                const uint64_t ta = imt::resize::total_nodes(a, depth), tb = imt::resize::total_nodes(b, depth);
                std::vector<uint8_t> from(ta * 32), to(tb * 32), want(32);
                for (unsigned l = 0; l <= depth; l++)
                    for (uint64_t i = 0; i < imt::resize::level_len(a, l); i++)
                        tag(&from[(imt::resize::level_off(a, l) + i) * 32], l, i);
                resize_host(from.data(), a, to.data(), b, depth, zero.data());
                for (unsigned l = 0; l <= depth; l++)
                    for (uint64_t i = 0; i < imt::resize::level_len(b, l); i++) {
                        tag(want.data(), l, i < imt::resize::level_len(a, l) ? i : ~(uint64_t)0);
                        if (std::memcmp(want.data(), &to[(imt::resize::level_off(b, l) + i) * 32], 32)) {
                            std::printf("depth %u: %llu -> %llu differs at level %u node %llu\n", depth, (unsigned long long)a,
                                        (unsigned long long)b, l, (unsigned long long)i);
                            return 1;
                        }
                        checked++;
                    }
            }
    }
    std::printf("resize_levels ok: %lu nodes\n", checked);
    return 0;
}
#endif
