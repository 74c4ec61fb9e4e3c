// imt_filter_logic.hpp -- the per-value rule of imt_itree_insert_filtered and imt_itree_lookup_batch and the
// per-operation rule of imt_itree_mixed_filtered (include/imt.h), kept free of HIP types like imt_prep_logic.hpp: the
// kernels of imt_prep.hip and host builds (tests/test_filter_rules.py, tests/test_mixed_filter_logic.py) include the
// same code.
//
// The filtered batch is the reference's sequence of insert_leaf calls with the rejected ones skipped.  Every value has
// one status; when several apply the first in this order wins: ZERO, FOREIGN, PRESENT, REPEATED, NEW.  ZERO and FOREIGN
// depend on the value alone, PRESENT on the stored index, REPEATED on the batch in value order (ties by input position,
// a total order, so the outcome does not depend on how the sort breaks ties): the head of a run of equal values is its
// first occurrence, the rest repeat it.
#pragma once
#include <cstdint>
#include "imt_prep_logic.hpp"

namespace imt {
namespace prep {

// include/imt.h IMT_VAL_*
constexpr uint8_t VAL_NEW = 0, VAL_ZERO = 1, VAL_PRESENT = 2, VAL_REPEATED = 3, VAL_FOREIGN = 4;
constexpr uint64_t LEAF_NONE = ~(uint64_t)0;

// what a value is by itself: ZERO, FOREIGN, or NEW (not decided yet).  0 is the sentinel whatever the partition.
IMT_PL_HD uint8_t filter_class(const uint8_t* v, uint32_t part_mod, uint32_t part_res) {
    const uint64_t* x = reinterpret_cast<const uint64_t*>(v);
    if ((x[0] | x[1] | x[2] | x[3]) == 0) return VAL_ZERO;
    if (part_mod > 1 && mod_small(v, part_mod) != part_res) return VAL_FOREIGN;
    return VAL_NEW;
}

// the batch order: by value, equal values by input position
IMT_PL_HD bool pos_less(const uint8_t* vals, uint32_t a, uint32_t b) {
    const uint8_t* x = vals + (uint64_t)a * 32;
    const uint8_t* y = vals + (uint64_t)b * 32;
    if (lt256(x, y)) return true;
    if (lt256(y, x)) return false;
    return a < b;
}

// Status of the value at rank j of the batch order (ord[r] = input position of rank r; cls = its filter_class), against
// the stored index (val / sorted[0..M), imt_prep.hpp).  *aux = the stored leaf (PRESENT, local index) or the input
// position of the first occurrence (REPEATED); untouched otherwise.
IMT_PL_HD uint8_t filter_rank(const uint8_t* vals, const uint32_t* ord, uint32_t j, uint8_t cls, const uint8_t* val,
                              const uint32_t* sorted, uint32_t M, uint32_t* aux) {
    if (cls != VAL_NEW) return cls;
    const uint8_t* x = vals + (uint64_t)ord[j] * 32;
    const uint32_t g = count_below(val, sorted, M, x);
    if (g < M && eq256(val + (uint64_t)sorted[g] * 32, x)) {
        *aux = sorted[g];
        return VAL_PRESENT;
    }
    uint32_t lo = 0, hi = j;                // first rank whose value is >= x: the head of x's run
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lt256(vals + (uint64_t)ord[mid] * 32, x)) lo = mid + 1; else hi = mid;
    }
    if (lo < j) {
        *aux = ord[lo];
        return VAL_REPEATED;
    }
    return VAL_NEW;
}

// Leaf index reported for input position i.  rank = exclusive scan of the accepted flags in input order, M = leaves
// before the batch, base = the placement (imt_itree_set_placement).
IMT_PL_HD uint64_t filter_leaf(uint8_t st, uint32_t aux, const uint32_t* rank, uint32_t i, uint64_t base, uint64_t M) {
    switch (st) {
        case VAL_NEW: return base + M + rank[i];
        case VAL_REPEATED: return base + M + rank[aux];
        case VAL_PRESENT: return base + aux;
        case VAL_ZERO: return base;
        default: return LEAF_NONE;
    }
}

// ---- imt_itree_mixed_filtered: the same statuses over a block of INSERTs (op 0) and READs (any other byte) ----
// The walk skips an operation whose value is 0 (ZERO), was stored before the call (PRESENT) or was put in by an earlier
// INSERT of the block (REPEATED), whichever kind the operation is; every other operation is carried out (NEW).  With
// f(v) the smallest position whose operation is an INSERT of v, position p is REPEATED iff p > f(v): only an accepted
// INSERT puts v in, and the first INSERT of a value that is neither 0 nor stored is accepted.

// the batch order: by value, equal values INSERT before READ, then by input position -- a total order.  The head of a
// run of equal values is f(v) if the run holds an INSERT, a READ otherwise.
// Written without a branch: one three-way comparison of the values, then (kind, position) as one 32-bit key (positions
// are below 2^30, imt.h).  The form of pos_less -- lt256(x, y), then lt256(y, x), then the tie -- handed to
// rocprim::merge_sort as the comparator of this order came back from gfx950 with positions lost and others doubled
// whenever equal values had to change places; pos_less never asks for that, its ties are in input order.
IMT_PL_HD int cmp256(const uint8_t* a, const uint8_t* b) {         // -1 / 0 / 1, the most significant differing limb decides
    const uint64_t* x = reinterpret_cast<const uint64_t*>(a);
    const uint64_t* y = reinterpret_cast<const uint64_t*>(b);
    int c = 0;
    for (int i = 0; i < 4; i++) {
        const int d = (int)(x[i] > y[i]) - (int)(x[i] < y[i]);
        c = d ? d : c;
    }
    return c;
}
IMT_PL_HD bool mixed_pos_less(const uint8_t* vals, const uint8_t* op, uint32_t a, uint32_t b) {
    const int c = cmp256(vals + (uint64_t)a * 32, vals + (uint64_t)b * 32);
    const uint32_t ka = ((uint32_t)(op[a] != 0) << 31) | a, kb = ((uint32_t)(op[b] != 0) << 31) | b;
    return c < 0 || (c == 0 && ka < kb);
}

// Status of the operation at rank j of that order (ord / cls / val / sorted / M as in filter_rank).  *aux = the stored
// leaf (PRESENT, local index) or f(v) (REPEATED); untouched otherwise.  Two binary searches, whatever the length of
// the run.
IMT_PL_HD uint8_t mixed_filter_rank(const uint8_t* vals, const uint8_t* op, const uint32_t* ord, uint32_t j, uint8_t cls,
                                    const uint8_t* val, const uint32_t* sorted, uint32_t M, uint32_t* aux) {
    if (cls != VAL_NEW) return cls;
    const uint32_t p = ord[j];
    const uint8_t* x = vals + (uint64_t)p * 32;
    const uint32_t g = count_below(val, sorted, M, x);
    if (g < M && eq256(val + (uint64_t)sorted[g] * 32, x)) {
        *aux = sorted[g];
        return VAL_PRESENT;
    }
    uint32_t lo = 0, hi = j;                // first rank whose value is >= x: the head of x's run
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lt256(vals + (uint64_t)ord[mid] * 32, x)) lo = mid + 1; else hi = mid;
    }
    const uint32_t h = ord[lo];
    if (op[h] == 0 && h < p) {
        *aux = h;
        return VAL_REPEATED;
    }
    return VAL_NEW;
}

// Leaf index reported for position p, except for an accepted READ (its low leaf is known once the accepted operations
// have been checked).  rank_ins = exclusive scan of the accepted-INSERT flags in input order.
IMT_PL_HD uint64_t mixed_filter_leaf(uint8_t st, uint32_t aux, const uint32_t* rank_ins, uint32_t p, uint64_t base,
                                     uint64_t M) {
    switch (st) {
        case VAL_NEW: return base + M + rank_ins[p];
        case VAL_REPEATED: return base + M + rank_ins[aux];
        case VAL_PRESENT: return base + aux;
        case VAL_ZERO: return base;
        default: return LEAF_NONE;
    }
}

// ---- MEMBERs in a filtered block (IMT_MEMBER_OPS) ----
// The status says what the VALUE is at that place, whichever kind the operation is, so mixed_pos_less and
// mixed_filter_rank take a MEMBER as they take a READ (any byte but 0).  What is carried out depends on the kind: an
// INSERT or a READ iff the value is not there (NEW), a MEMBER iff it is -- stored before the call (PRESENT) or put in by
// the INSERT at f(v) < p (REPEATED), which is then NEW and carried out itself.
IMT_PL_HD bool mixed_carried(uint8_t op, uint8_t st) {
    return op == OP_MEMBER ? (st == VAL_PRESENT || st == VAL_REPEATED) : st == VAL_NEW;
}
// mixed_filter_leaf for an operation of any kind: a MEMBER of a value that is not there (NEW, skipped) names no leaf; a
// carried-out one gets the leaf that holds its value, which is what its status reports already.
IMT_PL_HD uint64_t mixed_filter_op_leaf(uint8_t op, uint8_t st, uint32_t aux, const uint32_t* rank_ins, uint32_t p, uint64_t base,
                                        uint64_t M) {
    if (op == OP_MEMBER && st == VAL_NEW) return LEAF_NONE;
    return mixed_filter_leaf(st, aux, rank_ins, p, base, M);
}

// imt_itree_lookup_batch: status of one candidate against the stored index; *leaf = the stored leaf (PRESENT), the low
// leaf (NEW: greatest stored value below x), the sentinel (ZERO) or LEAF_NONE (FOREIGN)
IMT_PL_HD uint8_t lookup_one(const uint8_t* x, const uint8_t* val, const uint32_t* sorted, uint32_t M, uint64_t base,
                             uint32_t part_mod, uint32_t part_res, uint64_t* leaf) {
    const uint8_t cls = filter_class(x, part_mod, part_res);
    if (cls == VAL_ZERO) { *leaf = base; return cls; }
    if (cls == VAL_FOREIGN) { *leaf = LEAF_NONE; return cls; }
    const uint32_t g = count_below(val, sorted, M, x);      // >= 1: the sentinel 0 is stored and x > 0
    if (g < M && eq256(val + (uint64_t)sorted[g] * 32, x)) { *leaf = base + sorted[g]; return VAL_PRESENT; }
    *leaf = base + sorted[g > 0 ? g - 1 : 0];
    return VAL_NEW;
}

}  // namespace prep
}  // namespace imt
