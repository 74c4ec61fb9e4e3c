// imt_view.hpp -- reading the tree as it was when it held s leaves, while it stays the tree of M >= s leaves.
//
// imt_rewind.hpp: the tree of size s is a function of val[0 .. s), and it differs from the stored tree of size M only in
//   the nodes of S_0 = relinked + {s}, S_(l+1) = { x >> 1 : x in S_l }   -- a few hashes, which a view keeps in a SIDE
//                                                                           table instead of writing them into the tree,
//   the nodes wholly at or beyond the cut, x >= ceil(s / 2^l)              -- the empty subtree Z[l],
//   and nothing else                                                        -- the stored node as it is.
// So node x of level l as of size s is, in this order,
//     EMPTY   iff x >= ceil(s / 2^l);
//     SIDE    iff x is in S_l: its place in the level's ascending list (imt_apply.hpp builds the lists) is its place in
//             the side table.  From level `top` up (2^top >= M, or top = depth) the list is node 0 alone: one chain;
//     STORED  otherwise.
// Every reader of a view -- the hash kernels that fill the side table from the level below, the proof gather -- goes
// through classify() below, and so does tests/native/view_lists.cpp on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define IMT_VW_HD __host__ __device__ __forceinline__
#else
#define IMT_VW_HD inline
#endif

namespace imt {
namespace view {

enum : int { EMPTY = 0, SIDE = 1, STORED = 2 };
constexpr uint32_t NOT_LISTED = 0xffffffffu;

// ceil(s / 2^l): the nodes of level l a tree of s leaves fills, for any l (a shift by 64 or more is not one)
IMT_VW_HD uint64_t filled(uint64_t s, unsigned l) {
    if (l >= 64) return s ? 1 : 0;
    return (s >> l) + ((s & (((uint64_t)1 << l) - 1)) ? 1 : 0);
}

// place of x in the ascending list[0 .. n), NOT_LISTED if it is not there
IMT_VW_HD uint32_t find(const uint32_t* list, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (list[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && list[lo] == x ? lo : NOT_LISTED;
}

// The lists of one build (apply::Lists as prep::apply_lists leaves them) and the values hashed for them.
struct Side {
    const uint32_t* node;   // [top][stride]: row l = S_l ascending
    const uint64_t* count;  // [depth + 1]: |S_l| for l < top, 1 from there up
    size_t stride;
    unsigned top;           // lists exist below this level; from here to the depth the chain of node 0
    uint64_t size;          // s
    const uint8_t* val;     // [top][stride][32]: val[l][j] = node node[l][j] of level l as of size s (stored format)
    const uint8_t* chain;   // [depth + 1][32]: chain[l] = node 0 of level l >= top as of size s
};

struct Where {
    int cls;
    uint32_t rank;          // SIDE: the place in the level's list (0 on the chain)
};

IMT_VW_HD Where classify(const Side& sd, unsigned l, uint64_t x) {
    if (x >= filled(sd.size, l)) return {EMPTY, 0};
    if (l >= sd.top) return {SIDE, 0};                  // below ceil(s / 2^l) <= 1: node 0, on the chain
    const uint64_t n = sd.count[l];
    const uint32_t r = find(sd.node + (size_t)l * sd.stride, n < sd.stride ? (uint32_t)n : (uint32_t)sd.stride, x);
    if (r != NOT_LISTED) return {SIDE, r};
    return {STORED, 0};
}

// where a SIDE node's 32 bytes are
IMT_VW_HD const uint8_t* side_row(const Side& sd, unsigned l, uint32_t rank) {
    return l >= sd.top ? sd.chain + (size_t)l * 32 : sd.val + ((size_t)l * sd.stride + rank) * 32;
}

// Node x of level l as of size s.  stored_l: the stored level l with len_l nodes, zero_l: Z[l], both in the stored format.
// A STORED node lies below ceil(s / 2^l) <= len_l by construction; one that does not reads as Z[l], never out of bounds.
IMT_VW_HD const uint8_t* node_row(const Side& sd, unsigned l, uint64_t x, const uint8_t* stored_l, uint64_t len_l,
                                  const uint8_t* zero_l) {
    const Where w = classify(sd, l, x);
    if (w.cls == SIDE) return side_row(sd, l, w.rank);
    if (w.cls == STORED && x < len_l) return stored_l + x * 32;
    return zero_l;
}

}  // namespace view
}  // namespace imt
