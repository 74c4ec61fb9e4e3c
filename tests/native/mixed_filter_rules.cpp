// mixed_filter_rules.cpp -- TEST INFRASTRUCTURE: the per-operation rule of imt_itree_mixed_filtered
// (csrc/imt_filter_logic.hpp: filter_class, mixed_pos_less, mixed_filter_rank) on the CPU, over arrays built the way
// prep::mixed_filter builds them on the device.  A stand-alone program: it reads scripts from standard input and prints
// what the rule says of every operation; tests/test_mixed_filter_logic.py feeds it and compares with a plain walk.
//
// Input, repeated until end of file (values are 64 hex digits, most significant first):
//     S M n
//     <M stored values in leaf order, leaf 0 = the sentinel 0>
//     <n lines: op value>            op: 0 = INSERT, 1 = READ
// Output per script: one line per operation "kind status aux" (aux: the stored leaf of a PRESENT value, f(v) of a
// REPEATED one, -1 otherwise), then "end".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "imt_filter_logic.hpp"

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

int main() {
    unsigned M, n;
    char tag[8], hex[128];
    int scripts = 0;
    while (std::scanf("%7s %u %u", tag, &M, &n) == 3) {
        if (tag[0] != 'S' || M == 0) return 2;
        // 8-byte aligned rows: the rules read values as 64-bit limbs
        std::vector<uint64_t> val_store((size_t)M * 4), in_store((size_t)n * 4 + 4);
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
        std::vector<uint32_t> sorted(M);
        for (unsigned i = 0; i < M; i++) sorted[i] = i;
        std::sort(sorted.begin(), sorted.end(),
                  [&](uint32_t a, uint32_t b) { return lt256(val + (size_t)a * 32, val + (size_t)b * 32); });
        // the class kernel, the sort, the rank kernel
        std::vector<uint8_t> cls(n), st(n);
        std::vector<uint32_t> ord(n);
        std::vector<long> aux(n, -1);
        for (unsigned p = 0; p < n; p++) {
            cls[p] = filter_class(vals + (size_t)p * 32, 0, 0);
            ord[p] = p;
        }
        std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return mixed_pos_less(vals, op.data(), a, b); });
        for (unsigned j = 0; j < n; j++) {
            const uint32_t p = ord[j];
            uint32_t a = 0;
            st[p] = mixed_filter_rank(vals, op.data(), ord.data(), j, cls[p], val, sorted.data(), M, &a);
            if (st[p] == VAL_PRESENT || st[p] == VAL_REPEATED) aux[p] = (long)a;
        }
        for (unsigned p = 0; p < n; p++) std::printf("%c %u %ld\n", op[p] ? 'R' : 'I', (unsigned)st[p], aux[p]);
        std::printf("end\n");
        scripts++;
    }
    std::printf("scripts %d ok\n", scripts);
    return 0;
}
