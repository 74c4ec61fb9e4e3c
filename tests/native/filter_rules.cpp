// Host build of the classification rule of imt_itree_insert_filtered / imt_itree_lookup_batch (csrc/imt_filter_logic.hpp,
// the code the kernels of imt_prep.hip run), composed the way prep::filter composes it on the device: per-value class,
// sort of the input positions by (value, position), filter_rank over that order, exclusive scan of the accepted flags,
// filter_leaf + compaction in input order.  Used by tests/test_filter_rules.py:
//   filter_rules IN OUT
// IN:  u32 batches, then per batch: u32 M, u32 n, u32 part_mod, u32 part_res, u64 base, M stored values (leaf order,
//      leaf 0 = 0) and n batch values, 32 bytes each (little-endian)
// OUT: per batch: n status bytes, n u64 leaf indices, u32 accepted count, the accepted values (32 bytes each), then n
//      lookup status bytes and n u64 lookup leaf indices
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>
#include "imt_filter_logic.hpp"

using namespace imt::prep;

template <class T> static bool rd(FILE* f, T* p, size_t n = 1) { return fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE* f, const T* p, size_t n = 1) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t batches = 0;
    if (!rd(in, &batches)) return 3;
    std::vector<uint8_t> val, vals, acc, st, lst;
    std::vector<uint32_t> sorted, idx, ord, aux, flag, rank;
    std::vector<uint64_t> leaf, lleaf;
    for (uint32_t b = 0; b < batches; b++) {
        uint32_t M, n, pm, pr;
        uint64_t base;
        if (!rd(in, &M) || !rd(in, &n) || !rd(in, &pm) || !rd(in, &pr) || !rd(in, &base)) return 3;
        val.resize((size_t)M * 32);
        vals.resize((size_t)n * 32);
        if ((M && !rd(in, val.data(), val.size())) || (n && !rd(in, vals.data(), vals.size()))) return 3;
        // the stored index: leaf indices in value order
        sorted.resize(M);
        std::iota(sorted.begin(), sorted.end(), 0u);
        std::sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t c) { return lt256(&val[a * 32], &val[c * 32]); });
        // k_filter_class
        st.assign(n, 0);
        idx.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            st[i] = filter_class(&vals[(size_t)i * 32], pm, pr);
            idx[i] = i;
        }
        // the merge sort (any sort: the order is total)
        ord = idx;
        std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t c) { return pos_less(vals.data(), a, c); });
        // k_filter_rank
        aux.assign(n, 0);
        flag.assign(n, 0);
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t i = ord[j];
            uint32_t a = 0;
            const uint8_t s = filter_rank(vals.data(), ord.data(), j, st[i], val.data(), sorted.data(), M, &a);
            st[i] = s;
            aux[i] = a;
            flag[i] = s == VAL_NEW;
        }
        // the exclusive scan
        rank.assign(n, 0);
        for (uint32_t i = 1; i < n; i++) rank[i] = rank[i - 1] + flag[i - 1];
        const uint32_t count = n ? rank[n - 1] + flag[n - 1] : 0;
        // k_filter_compact
        leaf.assign(n, 0);
        acc.assign((size_t)count * 32, 0);
        for (uint32_t i = 0; i < n; i++) {
            if (st[i] == VAL_NEW) std::memcpy(&acc[(size_t)rank[i] * 32], &vals[(size_t)i * 32], 32);
            leaf[i] = filter_leaf(st[i], aux[i], rank.data(), i, base, M);
        }
        // k_lookup
        lst.assign(n, 0);
        lleaf.assign(n, 0);
        for (uint32_t i = 0; i < n; i++)
            lst[i] = lookup_one(&vals[(size_t)i * 32], val.data(), sorted.data(), M, base, pm, pr, &lleaf[i]);
        wr(out, st.data(), n);
        wr(out, leaf.data(), n);
        wr(out, &count);
        wr(out, acc.data(), acc.size());
        wr(out, lst.data(), n);
        wr(out, lleaf.data(), n);
    }
    fclose(out);
    fclose(in);
    return 0;
}
