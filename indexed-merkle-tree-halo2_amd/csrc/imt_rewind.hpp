// imt_rewind.hpp -- going back: the tree as it was when it held s leaves, from the tree that holds M >= s.
//
// The tree is append-only and stores no leaf preimage: a preimage is derived from val[] (values in leaf order) and
// sorted[] (leaf indices in value order).  The tree of size s is therefore a function of val[0 .. s), which the tree
// of size M still holds, and going back k = M - s insertions is three pieces of index arithmetic and a few hashes:
//   index   the sorted index of the earlier tree is the stable compaction of sorted[0 .. M) to the entries < s;
//   leaves  the only kept leaves whose preimage changes are those whose successor in value order is removed (the
//           RELINKED leaves, at most min(k, s)); their new successor is the next kept entry, none for the new largest;
//   nodes   the stored nodes [ceil(s / 2^l), ceil(M / 2^l)) of level l become the empty subtree Z[l] again, and the
//           nodes to hash are S_0 = relinked + {s}, S_(l+1) = { x >> 1 : x in S_l }: slot s is empty (its preimage is
//           all zero, H(0,0,0) = Z[0]) and its ancestors are exactly the nodes that straddle the cut.
// S_0 with one preimage row per position, positions ascending, is a level-0 table of the form imt_apply.hpp reads (one
// event per run), so the lists of every level and the hashing are those of imt_itree_apply_batch.
// Host and device run the functions below (tests/native/rewind_lists.cpp runs them on the CPU).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define IMT_RW_HD __host__ __device__ __forceinline__
#else
#define IMT_RW_HD inline
#endif

namespace imt {
namespace rewind {

// ---- 32-byte rows: two 16-byte words on the device (rows are 16-byte aligned there), bytes on the host ----
struct alignas(16) Row16 { uint32_t x, y, z, w; };
IMT_RW_HD void row_copy(uint8_t* dst, const uint8_t* src) {
#if defined(__HIP_DEVICE_COMPILE__)
    const Row16* s = reinterpret_cast<const Row16*>(src);
    Row16* d = reinterpret_cast<Row16*>(dst);
    d[0] = s[0];
    d[1] = s[1];
#else
    std::memcpy(dst, src, 32);
#endif
}
IMT_RW_HD void row_u64(uint8_t* dst, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    Row16* d = reinterpret_cast<Row16*>(dst);
    d[0] = Row16{(uint32_t)v, (uint32_t)(v >> 32), 0, 0};
    d[1] = Row16{0, 0, 0, 0};
#else
    std::memset(dst, 0, 32);
    std::memcpy(dst, &v, 8);
#endif
}

// entry j of the index stays in the tree of size s
IMT_RW_HD bool kept(const uint32_t* sorted, uint32_t j, uint32_t s) { return sorted[j] < s; }
// ... and its successor in value order does not: its preimage changes
IMT_RW_HD bool relinked(const uint32_t* sorted, uint32_t M, uint32_t j, uint32_t s) {
    return sorted[j] < s && j + 1 < M && sorted[j + 1] >= s;
}
// What one scan counts for both: kept entries in the low word, relinked ones in the high word.  Its exclusive scan at
// j is (rank of entry j among the relinked leaves) << 32 | (place of entry j in the compacted index).
IMT_RW_HD uint64_t scan_flag(const uint32_t* sorted, uint32_t M, uint32_t j, uint32_t s) {
    return (uint64_t)kept(sorted, j, s) | ((uint64_t)relinked(sorted, M, j, s) << 32);
}

// compaction: entry j into the other index buffer.  The last entry also leaves the number of relinked leaves.
IMT_RW_HD void compact_element(const uint32_t* sorted, uint32_t M, uint32_t j, uint32_t s, uint64_t pos, uint32_t* out,
                               uint32_t* n_relinked) {
    if (kept(sorted, j, s)) out[(uint32_t)pos] = sorted[j];
    if (j + 1 == M) *n_relinked = (uint32_t)((pos + scan_flag(sorted, M, j, s)) >> 32);
}

// The level-0 table and the preimage rows, unsorted: row r < R belongs to the r-th relinked leaf in value order, row R
// to the empty slot s.  key = leaf position, row = which preimage, re = r + 1 and rs = r (every run is one event; they
// do not move with the sort).  `compact` is the index compact_element wrote (s entries), `base` the tree's index base:
// next_idx is hashed, so it is global.
struct Table {
    uint32_t* key;      // [R + 1] positions, to be sorted ascending together with `row`
    uint32_t* row;      // [R + 1]
    uint32_t* rs;       // [R + 1]
    uint32_t* re;       // [R + 1]
    uint8_t* pre;       // [R + 1][96] canonical preimages {val, next_val, next_idx}
    uint32_t rows;      // R + 1 as the caller sized the arrays: a row beyond it is not written
};
IMT_RW_HD void table_slot(const Table& t, uint32_t r, uint32_t position) {
    t.key[r] = position;
    t.row[r] = r;
    t.rs[r] = r;
    t.re[r] = r + 1;
}
IMT_RW_HD void relink_element(const uint8_t* val, const uint32_t* sorted, const uint32_t* compact, uint32_t M, uint32_t j,
                              uint32_t s, uint64_t pos, uint64_t base, const Table& t) {
    if (j + 1 == M) {                                   // the empty slot s: the all-zero preimage, H(0,0,0) = Z[0]
        const uint32_t R = (uint32_t)((pos + scan_flag(sorted, M, j, s)) >> 32);
        if (R >= t.rows) return;
        uint8_t* e = t.pre + (size_t)R * 96;
        row_u64(e, 0);
        row_u64(e + 32, 0);
        row_u64(e + 64, 0);
        table_slot(t, R, s);
    }
    if (!relinked(sorted, M, j, s)) return;
    const uint32_t r = (uint32_t)(pos >> 32), place = (uint32_t)pos;
    if (r >= t.rows) return;
    const uint32_t leaf = sorted[j];
    uint8_t* e = t.pre + (size_t)r * 96;
    row_copy(e, val + (size_t)leaf * 32);
    if (place + 1 < s) {                                // the next kept entry is the new successor
        const uint32_t su = compact[place + 1];
        row_copy(e + 32, val + (size_t)su * 32);
        row_u64(e + 64, base + su);
    } else {                                            // the new largest value
        row_u64(e + 32, 0);
        row_u64(e + 64, 0);
    }
    table_slot(t, r, leaf);
}

// the stored nodes of level l (l < 32) that the tree of size s no longer fills: [lo, hi)
IMT_RW_HD void refill_range(uint64_t s, uint64_t M, unsigned l, uint64_t* lo, uint64_t* hi) {
    const uint64_t r = ((uint64_t)1 << l) - 1;
    *lo = (s + r) >> l;
    *hi = (M + r) >> l;
}

}  // namespace rewind
}  // namespace imt
