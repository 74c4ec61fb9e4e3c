// mixed_rules.cpp -- TEST INFRASTRUCTURE: the rules of a mixed batch (csrc/imt_prep_logic.hpp: read_neighbours,
// insert_is_duplicate, op_value_class, the nearest_* searches) on the CPU, over arrays built the way prep::mixed_ranks /
// mixed_check build them on the device.  A stand-alone program: it reads scripts from standard input and prints what the
// rules say of every operation; tests/test_mixed_logic.py feeds it and compares with a plain walk over a sorted list.
//
// Input, repeated until end of file (values are 64 hex digits, most significant first):
//     S M n
//     <M stored values in leaf order, leaf 0 = the sentinel 0>
//     <n lines: op value>            op: 0 = INSERT, 1 = READ
// Output per script: one line per operation "kind low succ err" (low / succ: rows of the value array, succ -1 = none; err:
// the OP_* bits of that operation), then "bad <smallest offending position or -1>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "imt_prep_logic.hpp"

using namespace imt::prep;

static bool parse256(const char* hex, uint8_t* out) {
    if (std::strlen(hex) != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned b;
        if (std::sscanf(hex + 2 * i, "%2x", &b) != 1) return false;
        out[31 - i] = (uint8_t)b;                 // little-endian bytes
    }
    return true;
}

static int levels_for(uint32_t n) {
    int k = 1;
    while ((1u << k) <= n) k++;
    return k;
}

int main() {
    unsigned M, n;
    char tag[8], hex[128];
    int scripts = 0;
    while (std::scanf("%7s %u %u", tag, &M, &n) == 3) {
        if (tag[0] != 'S' || M == 0) return 2;
        // 8-byte aligned rows: the rules read values as 64-bit limbs
        std::vector<uint64_t> val_store((size_t)(M + n) * 4), in_store((size_t)n * 4 + 4);
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
        std::vector<uint32_t> sorted_old(M);
        for (unsigned i = 0; i < M; i++) sorted_old[i] = i;
        std::sort(sorted_old.begin(), sorted_old.end(),
                  [&](uint32_t a, uint32_t b) { return lt256(val + (size_t)a * 32, val + (size_t)b * 32); });
        // mixed_ranks: flag, rank, the number of INSERTs
        std::vector<uint32_t> flag(n), rank(n), ipos(n), iota(n);
        uint32_t n_ins = 0;
        for (unsigned p = 0; p < n; p++) {
            flag[p] = op[p] == 0;
            rank[p] = n_ins;
            n_ins += flag[p];
        }
        // mixed_check: scatter, sort (value, then rank), gap / st, neighbours of the INSERTs, then the READs
        std::vector<int> err(n, 0);
        uint32_t bad = OP_NONE;
        for (unsigned p = 0; p < n; p++) {
            err[p] |= op_value_class(vals + (size_t)p * 32, 0, 0);
            if (!flag[p]) continue;
            std::memcpy(val + (size_t)(M + rank[p]) * 32, vals + (size_t)p * 32, 32);
            iota[rank[p]] = M + rank[p];
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
            gap[j] = count_below(val, sorted_old.data(), M, val + (size_t)bsorted[j] * 32);
            st[j] = bsorted[j] - M;
            if (insert_is_duplicate(val, sorted_old.data(), M, bsorted.data(), j, gap[j])) err[ipos[st[j]]] |= OP_DUPLICATE;
        }
        for (int k = 1; k < levels; k++)
            for (uint32_t j = 0; j + (1u << k) <= n_ins; j++)
                st[(size_t)k * n_ins + j] = std::min(st[(size_t)(k - 1) * n_ins + j], st[(size_t)(k - 1) * n_ins + j + (1u << (k - 1))]);
        for (uint32_t j = 0; j < n_ins; j++) {     // k_neighbours
            const uint32_t g = gap[j], t = st[j];
            const uint32_t jl = nearest_smaller_left(st.data(), n_ins, levels, j);
            const uint32_t jr = nearest_smaller_right(st.data(), n_ins, levels, j);
            low[t] = (jl < n_ins && gap[jl] == g) ? bsorted[jl] : sorted_old[g > 0 ? g - 1 : 0];
            succ[t] = (jr < n_ins && gap[jr] == g) ? bsorted[jr] : (g < M ? sorted_old[g] : OP_NONE);
        }
        for (unsigned p = 0; p < n; p++) {
            if (flag[p]) continue;
            const ReadAnswer a = read_neighbours(vals + (size_t)p * 32, rank[p], val, sorted_old.data(), M, bsorted.data(),
                                                 gap.data(), st.data(), n_ins, levels, 0, 0);
            err[p] |= a.err;
            low[n_ins + (p - rank[p])] = a.low;
            succ[n_ins + (p - rank[p])] = a.succ;
        }
        for (unsigned p = 0; p < n; p++) {
            const uint32_t at = flag[p] ? rank[p] : n_ins + (p - rank[p]);
            if (err[p] && p < bad) bad = p;
            std::printf("%c %u %ld %d\n", flag[p] ? 'I' : 'R', low[at], succ[at] == OP_NONE ? -1L : (long)succ[at], err[p]);
        }
        std::printf("bad %ld\n", bad == OP_NONE ? -1L : (long)bad);
        scripts++;
    }
    std::printf("scripts %d ok\n", scripts);
    return 0;
}
