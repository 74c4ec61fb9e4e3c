// load_values_rules.cpp -- host harness of imt_itree_load_values' check (tests/test_load_values_logic.py): the rank rule
// and the comparator of csrc/imt_prep_logic.hpp, driven the way imt_prep.hip drives them.
//
// stdin, per case:  "C n part_mod part_res", then n values as 64 hex digits (position q = line q).
// The first attempt orders the positions as the device's radix sort does -- by the top 64 bits, equal keys in input
// order -- and runs load_values_rank on every rank; the error bits are OR-ed and the smallest offending position kept.
// If a rank reports LOAD_TIE the positions are sorted with lv_pos_less and judged again, everything of the first attempt
// forgotten.  stdout, per case:  "bits bad attempts" and, if bits == 0, the order (n positions on one line).
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "imt_prep_logic.hpp"

using namespace imt::prep;

static bool parse_hex(const char* s, uint8_t* out) {
    if (std::strlen(s) != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned b;
        if (std::sscanf(s + 2 * (31 - i), "%2x", &b) != 1) return false;
        out[i] = (uint8_t)b;
    }
    return true;
}

int main() {
    char tag[8], line[128];
    unsigned long n_ul;
    unsigned part_mod, part_res;
    size_t cases = 0;
    while (std::scanf("%7s %lu %u %u", tag, &n_ul, &part_mod, &part_res) == 4) {
        if (std::strcmp(tag, "C") != 0 || n_ul == 0) return 2;
        const uint32_t n = (uint32_t)n_ul;
        // rows are 8-byte aligned for the limb reads of the rule
        std::vector<uint64_t> store((size_t)n * 4);
        uint8_t* vals = reinterpret_cast<uint8_t*>(store.data());
        for (uint32_t q = 0; q < n; q++) {
            if (std::scanf("%127s", line) != 1 || !parse_hex(line, vals + (size_t)q * 32)) return 2;
        }
        std::vector<uint32_t> ord(n);
        int bits = 0, attempts = 0;
        uint32_t bad = OP_NONE;
        for (int attempt = 0; attempt < 2; attempt++) {
            attempts++;
            for (uint32_t q = 0; q < n; q++) ord[q] = q;
            if (attempt == 0)
                std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return store[(size_t)a * 4 + 3] < store[(size_t)b * 4 + 3]; });
            else
                std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return lv_pos_less(vals, a, b); });
            bits = 0;
            bad = OP_NONE;
            for (uint32_t r = 0; r < n; r++) {
                const int e = load_values_rank(vals, ord.data(), r, part_mod, part_res);
                bits |= e;
                if (e & ~LOAD_TIE) bad = std::min(bad, ord[r]);
            }
            if (!(bits & LOAD_TIE)) break;
        }
        std::printf("%d %" PRId64 " %d\n", bits, bad == OP_NONE ? (int64_t)-1 : (int64_t)bad, attempts);
        if (bits == 0) {
            for (uint32_t r = 0; r < n; r++) std::printf(r ? " %u" : "%u", ord[r]);
            std::printf("\n");
        }
        cases++;
    }
    std::printf("cases %zu ok\n", cases);
    return 0;
}
