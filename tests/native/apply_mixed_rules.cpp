// apply_mixed_rules.cpp -- TEST INFRASTRUCTURE: the event rule of a witness-free mixed block (csrc/imt_prep_logic.hpp:
// insert_event, insert_event_preimages -- the code the kernel of prep::mixed_insert_events runs) on the CPU, over the low /
// succ rows the mixed checks leave, built the way tests/native/mixed_rules.cpp builds them.  A stand-alone program: it
// reads scripts from standard input and prints the two events of every INSERT; tests/test_apply_mixed_logic.py feeds it and
// compares with a plain walk over the script with its READs removed.
//
// Input, repeated until end of file (values are 64 hex digits, most significant first):
//     S M n
//     <M stored values in leaf order, leaf 0 = the sentinel 0>
//     <n lines: op value>            op: 0 = INSERT, 1 = READ
// Output per script: one line per INSERT, in rank order, "E low succ key_low key_new <192 hex digits> <192 hex digits>" (low /
// succ: rows of the value array, succ -1 = none; the keys in decimal; the preimages of events 2r and 2r + 1 byte by byte
// as they lie in memory), then "bad <smallest position the checks refuse, or -1>".
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

static void print_hex(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; i++) std::printf("%02x", p[i]);
}

int main() {
    unsigned M, n;
    char tag[8], hex[128];
    int scripts = 0;
    while (std::scanf("%7s %u %u", tag, &M, &n) == 3) {
        if (tag[0] != 'S' || M == 0) return 2;
        // 16-byte aligned rows: the checks read values as 64-bit limbs, the event rule moves them as 16-byte words
        std::vector<Word128> val_store((size_t)(M + n) * 2), in_store((size_t)n * 2 + 2);
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
        // mixed_ranks, then mixed_check: scatter, sort (value, then rank), gap / st, neighbours of the INSERTs, the READs
        std::vector<uint32_t> flag(n), rank(n), ipos(n), iota(n);
        uint32_t n_ins = 0;
        for (unsigned p = 0; p < n; p++) {
            flag[p] = op[p] == 0;
            rank[p] = n_ins;
            n_ins += flag[p];
        }
        std::vector<int> err(n, 0);
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
        uint32_t bad = OP_NONE;
        for (unsigned p = 0; p < n; p++) {
            if (!flag[p]) {
                const ReadAnswer a = read_neighbours(vals + (size_t)p * 32, rank[p], val, sorted_old.data(), M, bsorted.data(),
                                                     gap.data(), st.data(), n_ins, levels, 0, 0);
                err[p] |= a.err;
                low[n_ins + (p - rank[p])] = a.low;
                succ[n_ins + (p - rank[p])] = a.succ;
            }
            if (err[p] && p < bad) bad = p;
        }
        // the event kernel, one INSERT per thread: exactly 2 n_ins preimage rows and keys, with a guard word behind each
        const uint64_t guard = 0xA5A5A5A5A5A5A5A5ull;
        std::vector<Word128> pre_store((size_t)2 * n_ins * 6 + 1, Word128{guard, guard});
        std::vector<uint64_t> keys((size_t)2 * n_ins + 1, guard);
        uint8_t* pre = reinterpret_cast<uint8_t*>(pre_store.data());
        if (bad == OP_NONE) {
            for (uint32_t r = 0; r < n_ins; r++) {
                const InsertEvent e = insert_event(r, M, low.data(), succ.data());
                insert_event_preimages(e, val, 0, pre + (size_t)(2 * r) * 96);
                keys[2 * r] = e.key_low;
                keys[2 * r + 1] = e.key_new;
                std::printf("E %u %ld %llu %llu ", e.low, e.succ == OP_NONE ? -1L : (long)e.succ, (unsigned long long)e.key_low,
                            (unsigned long long)e.key_new);
                print_hex(pre + (size_t)(2 * r) * 96, 96);
                std::printf(" ");
                print_hex(pre + (size_t)(2 * r + 1) * 96, 96);
                std::printf("\n");
            }
            if (pre_store.back().lo != guard || pre_store.back().hi != guard || keys.back() != guard) return 3;
        }
        std::printf("bad %ld\n", bad == OP_NONE ? -1L : (long)bad);
        scripts++;
    }
    std::printf("scripts %d ok\n", scripts);
    return 0;
}
