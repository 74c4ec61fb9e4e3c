// imt_prep_logic.hpp -- per-element logic of the GPU batch preparation (imt_prep.hip), kept free of
// HIP types so tests/native/ can run it on the host against a brute force.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IMT_PL_HD __host__ __device__ __forceinline__
#else
#define IMT_PL_HD inline
#endif

namespace imt {
namespace prep {

// 256-bit little-endian integers stored as 32 bytes
IMT_PL_HD bool lt256(const uint8_t* a, const uint8_t* b) {
    const uint64_t* x = reinterpret_cast<const uint64_t*>(a);
    const uint64_t* y = reinterpret_cast<const uint64_t*>(b);
    for (int i = 3; i >= 0; i--)
        if (x[i] != y[i]) return x[i] < y[i];
    return false;
}
IMT_PL_HD bool eq256(const uint8_t* a, const uint8_t* b) {
    const uint64_t* x = reinterpret_cast<const uint64_t*>(a);
    const uint64_t* y = reinterpret_cast<const uint64_t*>(b);
    return x[0] == y[0] && x[1] == y[1] && x[2] == y[2] && x[3] == y[3];
}

// (256-bit little-endian integer) mod m, m < 2^32
IMT_PL_HD uint32_t mod_small(const uint8_t* a, uint32_t m) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a);
    uint64_t r = 0;
    for (int i = 7; i >= 0; i--) r = ((r << 32) | w[i]) % m;
    return (uint32_t)r;
}

// number of stored values (sorted[0..M) indexes val) strictly below x
IMT_PL_HD uint32_t count_below(const uint8_t* val, const uint32_t* sorted, uint32_t M, const uint8_t* x) {
    uint32_t lo = 0, hi = M;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lt256(val + (uint64_t)sorted[mid] * 32, x)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Sparse min-table st[k][j] = min(t[j .. j + 2^k)), rows of length n (entries with j + 2^k > n unused).
// Nearest position left of j whose value is < t[j]; returns n ("none") if there is none.
IMT_PL_HD uint32_t nearest_smaller_left(const uint32_t* st, uint32_t n, int levels, uint32_t j) {
    const uint32_t t = st[j];
    uint32_t p = j;                       // invariant: every entry in [p, j) is > t
    for (int k = levels - 1; k >= 0; k--) {
        const uint32_t w = 1u << k;
        if (p >= w && st[(uint64_t)k * n + (p - w)] > t) p -= w;
    }
    return p > 0 ? p - 1 : n;
}
IMT_PL_HD uint32_t nearest_smaller_right(const uint32_t* st, uint32_t n, int levels, uint32_t j) {
    const uint32_t t = st[j];
    uint32_t p = j + 1;                   // invariant: every entry in (j, p) is > t
    for (int k = levels - 1; k >= 0; k--) {
        const uint32_t w = 1u << k;
        if (p + w <= n && st[(uint64_t)k * n + p] > t) p += w;
    }
    return p < n ? p : n;
}

// ---- mixed batches (imt_itree_mixed_batch): READs between the INSERTs of one batch -------------------------------
// The INSERTs of the batch in value order, equal values by rank: bsorted[j] = M + rank of the j-th smallest (its row of
// val), gap[j] = stored values below it, st = the sparse min-table over their ranks (row 0 = bsorted[j] - M, row stride
// n_ins).  An operation's rank R is the number of INSERTs before it, so "an INSERT with a smaller position" is "an INSERT
// of rank < R" for an INSERT and a READ alike.  A READ is a query point of that table and nothing else: it is in none of
// these arrays, so it is nobody's neighbour.
constexpr uint8_t OP_INSERT = 0, OP_READ = 1, OP_MEMBER = 2;      // include/imt.h IMT_OP_*
// Nearest position left of j0 (right: at or right of j0) whose rank is < thr; n if there is none.
IMT_PL_HD uint32_t nearest_below_left(const uint32_t* st, uint32_t n, int levels, uint32_t j0, uint32_t thr) {
    uint32_t p = j0;                      // invariant: every entry in [p, j0) is >= thr
    for (int k = levels - 1; k >= 0; k--) {
        const uint32_t w = 1u << k;
        if (p >= w && st[(uint64_t)k * n + (p - w)] >= thr) p -= w;
    }
    return p > 0 ? p - 1 : n;
}
IMT_PL_HD uint32_t nearest_below_right(const uint32_t* st, uint32_t n, int levels, uint32_t j0, uint32_t thr) {
    uint32_t p = j0;                      // invariant: every entry in [j0, p) is >= thr
    for (int k = levels - 1; k >= 0; k--) {
        const uint32_t w = 1u << k;
        if (p + w <= n && st[(uint64_t)k * n + p] >= thr) p += w;
    }
    return p < n ? p : n;
}
// number of the batch's INSERT values strictly below x
IMT_PL_HD uint32_t batch_below(const uint8_t* val, const uint32_t* bsorted, uint32_t n_ins, const uint8_t* x) {
    uint32_t lo = 0, hi = n_ins;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lt256(val + (uint64_t)bsorted[mid] * 32, x)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// What is wrong with an operation's value (the bits of prep::ERR_ZERO / ERR_DUPLICATE / ERR_FOREIGN): each refuses the
// batch with IMT_ERR_VALUE, and the smallest position that has one is *bad_op.
constexpr int OP_ZERO = 2, OP_DUPLICATE = 4, OP_FOREIGN = 8;
constexpr uint32_t OP_NONE = 0xffffffffu;
IMT_PL_HD int op_value_class(const uint8_t* x, uint32_t part_mod, uint32_t part_res) {
    const uint64_t* w = reinterpret_cast<const uint64_t*>(x);
    int e = 0;
    if ((w[0] | w[1] | w[2] | w[3]) == 0) e |= OP_ZERO;
    if (part_mod > 1 && mod_small(x, part_mod) != part_res) e |= OP_FOREIGN;
    return e;
}
// The INSERT at place j of the value order is a duplicate iff its value is stored or the INSERT before it in that order
// has the same value -- that one has the smaller rank, so the walk would have refused THIS one.
IMT_PL_HD bool insert_is_duplicate(const uint8_t* val, const uint32_t* sorted_old, uint32_t M, const uint32_t* bsorted,
                                   uint32_t j, uint32_t g) {
    const uint8_t* x = val + (uint64_t)bsorted[j] * 32;
    if (g < M && eq256(val + (uint64_t)sorted_old[g] * 32, x)) return true;
    return j > 0 && eq256(val + (uint64_t)bsorted[j - 1] * 32, x);
}
// A READ of x behind R INSERTs.  Duplicate iff x is stored or an INSERT of rank < R has the same value (the first of an
// equal run has the smallest rank); an equal INSERT of rank >= R comes later and is none of its business.  Its low leaf
// is the nearest INSERT to the left with rank < R if no stored value lies between (same gap), else the stored
// predecessor; its successor likewise to the right, OP_NONE if x is above everything.  Always in bounds, also for the
// refused value 0 (g == 0).
struct ReadAnswer {
    uint32_t low, succ;     // rows of val
    int err;                // OP_* bits
};
IMT_PL_HD ReadAnswer read_neighbours(const uint8_t* x, uint32_t R, const uint8_t* val, const uint32_t* sorted_old, uint32_t M,
                                     const uint32_t* bsorted, const uint32_t* gap, const uint32_t* st, uint32_t n_ins,
                                     int levels, uint32_t part_mod, uint32_t part_res) {
    ReadAnswer a;
    a.err = op_value_class(x, part_mod, part_res);
    const uint32_t g = count_below(val, sorted_old, M, x);
    if (g < M && eq256(val + (uint64_t)sorted_old[g] * 32, x) && g > 0) a.err |= OP_DUPLICATE;
    const uint32_t j0 = batch_below(val, bsorted, n_ins, x);
    if (j0 < n_ins && st[j0] < R && eq256(val + (uint64_t)bsorted[j0] * 32, x)) a.err |= OP_DUPLICATE;
    const uint32_t jl = nearest_below_left(st, n_ins, levels, j0, R);
    const uint32_t jr = nearest_below_right(st, n_ins, levels, j0, R);
    a.low = (jl < n_ins && gap[jl] == g) ? bsorted[jl] : sorted_old[g > 0 ? g - 1 : 0];
    a.succ = (jr < n_ins && gap[jr] == g) ? bsorted[jr] : (g < M ? sorted_old[g] : OP_NONE);
    return a;
}
// number of the batch's INSERT values at or below x
IMT_PL_HD uint32_t batch_not_above(const uint8_t* val, const uint32_t* bsorted, uint32_t n_ins, const uint8_t* x) {
    uint32_t lo = 0, hi = n_ins;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lt256(x, val + (uint64_t)bsorted[mid] * 32)) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// A MEMBER of x behind R INSERTs (IMT_OP_MEMBER, IMT_MEMBER_OPS): the presence read.  Its leaf is the one that holds x as
// of its place -- the stored hit, or the first INSERT of an equal run if that one has rank < R (an accepted block has at
// most one of the two: an INSERT of a value that is there is a duplicate) -- and OP_ABSENT says there is none: x is not
// stored and no INSERT of rank < R put it in; an equal INSERT of rank >= R comes later and does not help.  Its successor
// is what that leaf points at as of R: the nearest INSERT of rank < R strictly above x if no stored value lies between
// (the gap right of x: g + 1 behind a stored hit, which count_below counts for everything above it), else the stored
// successor, OP_NONE if x is above everything.  Always in bounds, also for the refused value 0 and for an absent x, whose
// `low` is the READ's low leaf.  `low` and `succ` go where a READ's go: to the sweep a MEMBER is a READ of another leaf.
constexpr int OP_ABSENT = 2048;
IMT_PL_HD ReadAnswer member_neighbours(const uint8_t* x, uint32_t R, const uint8_t* val, const uint32_t* sorted_old, uint32_t M,
                                       const uint32_t* bsorted, const uint32_t* gap, const uint32_t* st, uint32_t n_ins,
                                       int levels, uint32_t part_mod, uint32_t part_res) {
    ReadAnswer a;
    a.err = op_value_class(x, part_mod, part_res);
    const uint32_t g = count_below(val, sorted_old, M, x);
    const bool stored = g < M && eq256(val + (uint64_t)sorted_old[g] * 32, x);
    const uint32_t j0 = batch_below(val, bsorted, n_ins, x);
    const bool put_in = j0 < n_ins && st[j0] < R && eq256(val + (uint64_t)bsorted[j0] * 32, x);
    if (stored) a.low = sorted_old[g];
    else if (put_in) a.low = bsorted[j0];
    else {
        a.err |= OP_ABSENT;
        const uint32_t jl = nearest_below_left(st, n_ins, levels, j0, R);
        a.low = (jl < n_ins && gap[jl] == g) ? bsorted[jl] : sorted_old[g > 0 ? g - 1 : 0];
    }
    const uint32_t gs = stored ? g + 1 : g;
    const uint32_t j1 = batch_not_above(val, bsorted, n_ins, x);
    const uint32_t jr = nearest_below_right(st, n_ins, levels, j1, R);
    a.succ = (jr < n_ins && gap[jr] == gs) ? bsorted[jr] : (gs < M ? sorted_old[gs] : OP_NONE);
    return a;
}

// ---- witness-free mixed blocks (imt_itree_apply_mixed): the events of the INSERTs alone ---------------------------------
// Behind the checks low[r] / succ[r] hold, for the INSERT of rank r, its low leaf and that leaf's successor as of its
// place in the block (rows of val, OP_NONE: no successor).  A READ changes no leaf, so the block's effect on the tree is
// that of its INSERTs in order, and the INSERT of rank r has the two events an insertion-only batch of those values
// gives it: event 2r rewrites the low leaf {low.val, v, base + M + r}, event 2r + 1 writes the new leaf M + r, which
// inherits the low leaf's old pointers {v, succ.val, base + succ} ({v, 0, 0} above everything).  A key is
// (leaf << 32) | event: sorted, the events of one leaf are a run in the order of the block.
struct InsertEvent {
    uint32_t low, succ;             // rows of val
    uint32_t leaf;                  // the new leaf's row, M + r
    uint64_t key_low, key_new;      // of events 2r and 2r + 1
};
IMT_PL_HD InsertEvent insert_event(uint32_t r, uint32_t M, const uint32_t* low, const uint32_t* succ) {
    InsertEvent e;
    e.low = low[r];
    e.succ = succ[r];
    e.leaf = M + r;
    e.key_low = ((uint64_t)e.low << 32) | (uint64_t)(2 * r);
    e.key_new = ((uint64_t)e.leaf << 32) | (uint64_t)(2 * r + 1);
    return e;
}
// the two preimages of that INSERT, [2][3][32] canonical at `pre`.  Rows move as two 16-byte words, like every row the
// preparation moves: val and pre are 16-byte aligned.
struct alignas(16) Word128 { uint64_t lo, hi; };
IMT_PL_HD void insert_event_preimages(const InsertEvent& e, const uint8_t* val, uint64_t base, uint8_t* pre) {
    const Word128* v = reinterpret_cast<const Word128*>(val + (uint64_t)e.leaf * 32);
    const Word128* lv = reinterpret_cast<const Word128*>(val + (uint64_t)e.low * 32);
    Word128* o = reinterpret_cast<Word128*>(pre);       // 12 words: {low.val, v, leaf} {v, succ.val, succ}
    const Word128 v0 = v[0], v1 = v[1], zero = {0, 0};
    o[0] = lv[0];
    o[1] = lv[1];
    o[2] = v0;
    o[3] = v1;
    o[4] = Word128{base + e.leaf, 0};
    o[5] = zero;
    o[6] = v0;
    o[7] = v1;
    if (e.succ != OP_NONE) {
        const Word128* sv = reinterpret_cast<const Word128*>(val + (uint64_t)e.succ * 32);
        o[8] = sv[0];
        o[9] = sv[1];
        o[10] = Word128{base + e.succ, 0};
    } else {
        o[8] = zero;
        o[9] = zero;
        o[10] = zero;
    }
    o[11] = zero;
}

// ---- a mixed list replayed against the rows the tree stores (imt_itree_view_mixed_witness) ---------------------------
// The list is the block as it went in at size S: its INSERT of rank r must be the value the tree holds at leaf S + r.
// What is wrong with the operation at one position on its own: the op_value_class bits of its value and, for an INSERT,
// OP_MISMATCH unless its value is row S + r of val.  Everything else that can refuse an operation (a READ of a stored value
// or of one an earlier INSERT put in) is judged by read_neighbours / insert_is_duplicate over the STORED rows [S, S + n_ins),
// which are the list's own INSERTs at every position before the first mismatch -- so the smallest offending position
// over all of these bits is the smallest position at which the walk refuses or the list differs from the tree.
constexpr int OP_MISMATCH = 1024;
IMT_PL_HD int replay_op_class(const uint8_t* x, bool insert, uint32_t r, const uint8_t* val, uint32_t S, uint32_t part_mod,
                              uint32_t part_res) {
    int e = op_value_class(x, part_mod, part_res);
    if (insert && !eq256(val + (uint64_t)(S + r) * 32, x)) e |= OP_MISMATCH;
    return e;
}

// ---- snapshot check (imt_itree_load): the leaves, visited in value order, must be ONE linked list ----------------
// pre = [n][3][32] canonical {val, next_val, next_idx}; idx[r] = leaf index of the r-th smallest val (candidate order:
// sorted by the top 64 bits at least).  Rank r checks leaf idx[r] against its successor idx[r + 1]: strictly larger
// val (equal: duplicate; smaller under an equal top limb: the candidate order was too coarse, LOAD_TIE -> the caller
// re-sorts with the full comparator), next_val = the successor's val, next_idx = base + its index; the last leaf points
// to {0, 0}; rank 0 is leaf 0 = the {0,..} sentinel (the reference's first leaf, src/indexed_merkle_tree.rs:710-713).
constexpr int LOAD_SENTINEL = 16, LOAD_LINK = 32, LOAD_LAST = 64, LOAD_TIE = 128, LOAD_DUP = 4;
IMT_PL_HD bool is_u64_256(const uint8_t* a, uint64_t v) {
    const uint64_t* x = reinterpret_cast<const uint64_t*>(a);
    return x[0] == v && (x[1] | x[2] | x[3]) == 0;
}
IMT_PL_HD int load_check_rank(const uint8_t* pre, uint32_t n, uint64_t base, const uint32_t* idx, uint32_t r) {
    const uint32_t i = idx[r];
    const uint8_t* p = pre + (uint64_t)i * 96;
    int e = 0;
    if (r == 0 && (i != 0 || !is_u64_256(p, 0))) e |= LOAD_SENTINEL;
    if (r + 1 < n) {
        const uint32_t j = idx[r + 1];
        const uint8_t* q = pre + (uint64_t)j * 96;
        if (eq256(p, q)) return e | LOAD_DUP;
        if (!lt256(p, q)) return e | LOAD_TIE;
        if (!eq256(p + 32, q) || !is_u64_256(p + 64, base + j)) e |= LOAD_LINK;
    } else if (!is_u64_256(p + 32, 0) || !is_u64_256(p + 64, 0)) {
        e |= LOAD_LAST;
    }
    return e;
}

// ---- value log check (imt_itree_load_values): which position would one-by-one insertion stop at ---------------------
// vals = [n][32] the inserted values in insertion order: position q becomes leaf q + 1.  The sentinel's 0 of leaf 0 is not
// among them: it is the smallest value at the smallest leaf, so it is rank 0 of the tree's order whatever the values are,
// and "equal to the sentinel" is "is 0".  ord[r] = the position of the r-th smallest value, equal values by position (the
// candidate order of the radix sort: by the top 64 bits, equal keys in input order).  Rank r judges position ord[r]
// against its predecessor ord[r - 1]: a smaller value, or an equal one at a larger position, says the candidate order
// is not the order (LOAD_TIE: the caller re-sorts with lv_pos_less and the other bits of this attempt mean nothing); an
// equal value at a smaller position was inserted earlier, so the walk refuses THIS one.  Together with what is wrong
// with the value alone (>= p, 0, a foreign residue) these are all the refusals of the walk, and the smallest position
// that has one is where it stops.
constexpr int LV_NONCANONICAL = 1;      // the other bits: OP_ZERO / OP_DUPLICATE / OP_FOREIGN, LOAD_TIE
// three-way comparison, the most significant differing limb decides (the form of cmp256, imt_filter_logic.hpp)
IMT_PL_HD int lv_cmp256(const uint8_t* a, const uint8_t* b) {
    const uint64_t* x = reinterpret_cast<const uint64_t*>(a);
    const uint64_t* y = reinterpret_cast<const uint64_t*>(b);
    int c = 0;
    for (int i = 0; i < 4; i++) {
        const int d = (int)(x[i] > y[i]) - (int)(x[i] < y[i]);
        c = d ? d : c;
    }
    return c;
}
// the order of the fallback sort: by value, then by position -- total, and written without a branch
IMT_PL_HD bool lv_pos_less(const uint8_t* vals, uint32_t a, uint32_t b) {
    const int c = lv_cmp256(vals + (uint64_t)a * 32, vals + (uint64_t)b * 32);
    return c < 0 || (c == 0 && a < b);
}
IMT_PL_HD bool lv_geq_p(const uint8_t* v) {
    const uint64_t P[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
    const uint64_t* x = reinterpret_cast<const uint64_t*>(v);
    for (int i = 3; i >= 0; i--)
        if (x[i] != P[i]) return x[i] > P[i];
    return true;
}
// the error bits of position ord[r]; 0 = the walk inserts it (if it gets that far)
IMT_PL_HD int load_values_rank(const uint8_t* vals, const uint32_t* ord, uint32_t r, uint32_t part_mod, uint32_t part_res) {
    const uint32_t q = ord[r];
    const uint8_t* x = vals + (uint64_t)q * 32;
    int e = op_value_class(x, part_mod, part_res);
    if (lv_geq_p(x)) e |= LV_NONCANONICAL;
    if (r > 0) {
        const uint32_t pq = ord[r - 1];
        const int c = lv_cmp256(vals + (uint64_t)pq * 32, x);
        if (c > 0 || (c == 0 && pq > q)) e |= LOAD_TIE;
        else if (c == 0) e |= OP_DUPLICATE;
    }
    return e;
}

// ---- bulk insertion (imt_itree_insert_bulk): the batch in DESCENDING value order, one low-leaf rewrite per value ----
// The batch in ascending value order is bsorted[0 .. n) (rows of val, row M + i = the caller's value i) with gap[j] = the
// stored values below the j-th smallest.  Row k of the witness is the k-th LARGEST value, place j = n - 1 - k.  Every
// value of gap g has the stored leaf sorted_old[g - 1] as its low leaf -- never a leaf of the batch -- and what that leaf
// points at as of step k is the neighbour above in the sorted batch if it shares the gap (it was row k - 1), else the
// stored successor sorted_old[g], else nothing.  That neighbour is also the value's successor in the final tree, so the
// low leaf's pointer before row k and the new leaf's final pointer are the same pair.  Always in bounds, also for the
// refused value 0 (g == 0).
struct BulkRow {
    uint32_t k;             // the row: n - 1 - j
    uint32_t pos;           // the caller's position of the value: bsorted[j] - M
    uint32_t low;           // row of val of the low leaf (a stored leaf)
    uint32_t succ;          // row of val the low leaf points at before the rewrite = the new leaf's successor; OP_NONE: none
};
IMT_PL_HD BulkRow bulk_row(const uint32_t* sorted_old, uint32_t M, const uint32_t* bsorted, const uint32_t* gap, uint32_t n,
                           uint32_t j) {
    const uint32_t g = gap[j];
    BulkRow r;
    r.k = n - 1 - j;
    r.pos = bsorted[j] - M;
    r.low = sorted_old[g > 0 ? g - 1 : 0];
    r.succ = (j + 1 < n && gap[j + 1] == g) ? bsorted[j + 1] : (g < M ? sorted_old[g] : OP_NONE);
    return r;
}
// place j of the sorted batch is refused as a duplicate: its value is stored, or the place above holds the same value.
// On the device k_gap makes these two comparisons for every batch (imt_prep.hip); this is their statement for a host
// driver (tests/native/bulk_rows.cpp).
IMT_PL_HD bool bulk_is_duplicate(const uint8_t* val, const uint32_t* sorted_old, uint32_t M, const uint32_t* bsorted, uint32_t n,
                                 uint32_t j, uint32_t g) {
    const uint8_t* x = val + (uint64_t)bsorted[j] * 32;
    if (g < M && eq256(val + (uint64_t)sorted_old[g] * 32, x)) return true;
    return j + 1 < n && eq256(val + (uint64_t)bsorted[j + 1] * 32, x);
}

}  // namespace prep
}  // namespace imt
