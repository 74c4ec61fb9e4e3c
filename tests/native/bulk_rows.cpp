// bulk_rows.cpp -- TEST INFRASTRUCTURE: the preparation of imt_itree_insert_bulk (csrc/imt_prep_logic.hpp bulk_row) on the
// CPU.  The device sorts the batch, counts the stored values below each value (k_gap) and runs bulk_row once per place of
// the sorted batch (k_bulk_events); this file does the same with std::sort over the same functions
// (tests/test_bulk_rows.py).  With -DBULK_ROWS_MAIN it is a program of its own that checks every small script against a
// linear walk, for a run under the host sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>
#include "imt_prep_logic.hpp"

using namespace imt::prep;

namespace {
void put_u64(uint8_t* dst, uint64_t v) {
    std::memset(dst, 0, 32);
    std::memcpy(dst, &v, 8);
}
}  // namespace

extern "C" {

// stored [M][32] (leaf order, row 0 the sentinel 0) and vals [n][32], canonical little-endian.  Returns the error bits
// (1: a value >= p, OP_ZERO, OP_DUPLICATE) and writes nothing, or 0 and: order / low_index [n], is_largest [n],
// low_leaf / rewritten [n][96] by row, new_leaf [n][96] in the caller's order, keys [n] = (position << 32) | row.
int bulk_rows_host(const uint8_t* stored, uint32_t M, const uint8_t* vals, uint32_t n, uint64_t* order, uint64_t* low_index,
                   uint8_t* is_largest, uint8_t* low_leaf, uint8_t* rewritten, uint8_t* new_leaf, uint64_t* keys) {
    std::vector<uint8_t> val((size_t)(M + n) * 32);
    std::memcpy(val.data(), stored, (size_t)M * 32);
    std::memcpy(val.data() + (size_t)M * 32, vals, (size_t)n * 32);
    const uint8_t* d_val = val.data();
    auto less = [&](uint32_t a, uint32_t b) { return lt256(d_val + (size_t)a * 32, d_val + (size_t)b * 32); };
    std::vector<uint32_t> sorted_old(M), bsorted(n), gap(n);
    for (uint32_t i = 0; i < M; i++) sorted_old[i] = i;
    for (uint32_t i = 0; i < n; i++) bsorted[i] = M + i;
    std::sort(sorted_old.begin(), sorted_old.end(), less);
    std::stable_sort(bsorted.begin(), bsorted.end(), less);
    int err = 0;
    for (uint32_t j = 0; j < n; j++) {
        const uint8_t* x = d_val + (size_t)bsorted[j] * 32;
        gap[j] = count_below(d_val, sorted_old.data(), M, x);
        if (lv_geq_p(x)) err |= 1;
        err |= op_value_class(x, 0, 0);
        if (bulk_is_duplicate(d_val, sorted_old.data(), M, bsorted.data(), n, j, gap[j])) err |= OP_DUPLICATE;
    }
    if (err) return err;
    for (uint32_t j = 0; j < n; j++) {
        const BulkRow r = bulk_row(sorted_old.data(), M, bsorted.data(), gap.data(), n, j);
        const uint8_t *v = d_val + (size_t)bsorted[j] * 32, *lv = d_val + (size_t)r.low * 32;
        uint8_t *before = low_leaf + (size_t)r.k * 96, *after = rewritten + (size_t)r.k * 96, *nl = new_leaf + (size_t)r.pos * 96;
        std::memcpy(nl, v, 32);
        if (r.succ != OP_NONE) {
            std::memcpy(nl + 32, d_val + (size_t)r.succ * 32, 32);
            put_u64(nl + 64, r.succ);
        } else {
            std::memset(nl + 32, 0, 64);
        }
        std::memcpy(before, lv, 32);
        std::memcpy(before + 32, nl + 32, 64);
        std::memcpy(after, lv, 32);
        std::memcpy(after + 32, v, 32);
        put_u64(after + 64, (uint64_t)M + r.pos);
        order[r.k] = r.pos;
        low_index[r.k] = r.low;
        is_largest[r.k] = r.succ == OP_NONE ? 1 : 0;
        keys[r.k] = ((uint64_t)r.low << 32) | r.k;
    }
    return 0;
}

}  // extern "C"

#ifdef BULK_ROWS_MAIN
#include <cstdio>
// Every stored list of 1 .. 5 leaves (the sentinel and up to four values of 1 .. 6 in every order) and every ordered
// batch of 1 .. 4 values of 0 .. 6, repeats and stored values included, against a
// walk that scans the whole list for every value: the largest first, the predecessor among the stored values, the
// pointers as the rewrites before left them.
namespace {
void row32(uint8_t* dst, uint64_t v) { put_u64(dst, v); }
uint64_t get_u64(const uint8_t* p) {
    uint64_t v;
    std::memcpy(&v, p, 8);
    return v;
}
int check(const std::vector<uint64_t>& st, const std::vector<uint64_t>& bv) {
    const uint32_t M = (uint32_t)st.size(), n = (uint32_t)bv.size();
    std::vector<uint8_t> stored((size_t)M * 32), vals((size_t)n * 32), lg(n), ll((size_t)n * 96), rw((size_t)n * 96), nl((size_t)n * 96);
    std::vector<uint64_t> order(n), low(n), keys(n);
    for (uint32_t i = 0; i < M; i++) row32(&stored[(size_t)i * 32], st[i]);
    for (uint32_t i = 0; i < n; i++) row32(&vals[(size_t)i * 32], bv[i]);
    const int err = bulk_rows_host(stored.data(), M, vals.data(), n, order.data(), low.data(), lg.data(), ll.data(), rw.data(),
                                   nl.data(), keys.data());
    bool bad = false;
    for (uint32_t i = 0; i < n; i++) {
        if (bv[i] == 0) bad = true;
        for (uint32_t j = 0; j < M; j++) bad |= st[j] == bv[i];
        for (uint32_t j = 0; j < i; j++) bad |= bv[j] == bv[i];
    }
    if (bad != (err != 0)) return 1;
    if (bad) return 0;
    std::vector<uint64_t> nv(M), ni(M);                 // the stored leaves' pointers as the walk goes on
    for (uint32_t i = 0; i < M; i++) {
        nv[i] = ni[i] = 0;
        for (uint32_t j = 0; j < M; j++)
            if (st[j] > st[i] && (nv[i] == 0 || st[j] < nv[i])) { nv[i] = st[j]; ni[i] = j; }
    }
    std::vector<bool> done(n, false);
    for (uint32_t k = 0; k < n; k++) {
        uint32_t i = n;
        for (uint32_t j = 0; j < n; j++)
            if (!done[j] && (i == n || bv[j] > bv[i])) i = j;
        done[i] = true;
        uint32_t lo = 0;
        for (uint32_t j = 0; j < M; j++)
            if (st[j] < bv[i] && st[j] >= st[lo]) lo = j;
        const uint8_t *b = &ll[(size_t)k * 96], *a = &rw[(size_t)k * 96], *w = &nl[(size_t)i * 96];
        if (order[k] != i || low[k] != lo || lg[k] != (nv[lo] == 0) || keys[k] != (((uint64_t)lo << 32) | k)) return 2;
        if (get_u64(b) != st[lo] || get_u64(b + 32) != nv[lo] || get_u64(b + 64) != ni[lo]) return 3;
        if (get_u64(a) != st[lo] || get_u64(a + 32) != bv[i] || get_u64(a + 64) != M + i) return 4;
        if (get_u64(w) != bv[i] || get_u64(w + 32) != nv[lo] || get_u64(w + 64) != ni[lo]) return 5;
        nv[lo] = bv[i];
        ni[lo] = M + i;
    }
    return 0;
}
}  // namespace

int main() {
    const unsigned U = 7;                               // values 0 .. 6
    auto digits = [&](unsigned code, unsigned len) {
        std::vector<uint64_t> v;
        for (unsigned q = 0; q < len; q++, code /= U) v.push_back(code % U);
        return v;
    };
    auto pow_u = [&](unsigned len) {
        unsigned r = 1;
        while (len--) r *= U;
        return r;
    };
    unsigned long scripts = 0;
    for (unsigned m = 0; m <= 4; m++)                   // stored values beside the sentinel, in every leaf order
        for (unsigned sc = 0; sc < pow_u(m); sc++) {
            std::vector<uint64_t> st{0};
            bool ok = true;
            for (uint64_t v : digits(sc, m)) {
                ok = ok && v != 0 && std::find(st.begin(), st.end(), v) == st.end();
                st.push_back(v);
            }
            if (!ok) continue;
            for (unsigned n = 1; n <= 4; n++)           // every ordered batch, the refused ones included
                for (unsigned bc = 0; bc < pow_u(n); bc++) {
                    const int rc = check(st, digits(bc, n));
                    if (rc) {
                        std::printf("script %lu: mismatch %d\n", scripts, rc);
                        return 1;
                    }
                    scripts++;
                }
        }
    std::printf("bulk_rows: %lu scripts agree with the linear walk\n", scripts);
    return 0;
}
#endif
