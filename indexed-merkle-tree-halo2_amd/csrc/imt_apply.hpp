// imt_apply.hpp -- the second schedule of a batch insertion: the tree AFTER the batch and nothing else.
//
// The level sweep (imt_sweep.hpp) hashes every version of every touched node, because a witness needs the tree as it was
// between any two insertions: two events per insertion, one hash per event per level.  A caller who only keeps the tree
// current needs the final version alone, and that is one hash per DISTINCT node the batch touches:
//     S_0 = { low_idx(i) } + { size + i },   S_(l+1) = { x >> 1 : x in S_l },
// the final preimage of every leaf of S_0, then level by level every node of S_(l+1) from the final values of its two
// children, which are already in the stored tree when the level below has been written.
//
// The lists are index arithmetic over the level-0 table the prepare stage leaves behind (events ordered by (position,
// time), `node` = position, ascending): slot x starts a new node of level l iff it is the first slot or
// node[x] >> l differs from node[x - 1] >> l.  An exclusive scan of that flag is the node's place in the list of level l,
// so every list is one scan of the same table and all of them exist before the first hash.  Above l0 (2^l0 >= size
// after the batch) the only touched node of a level is node 0 and its right sibling is the empty subtree.
// Host and device build the lists from the functions below (tests/native/apply_lists.cpp runs them on the CPU).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define IMT_AP_HD __host__ __device__ __forceinline__
#else
#define IMT_AP_HD inline
#endif

namespace imt {
namespace apply {

// 1 iff slot x of the level-0 table starts a node of level l (l < 32)
IMT_AP_HD uint32_t head(const uint32_t* node, uint32_t x, unsigned l) {
    return (x == 0 || (node[x] >> l) != (node[x - 1] >> l)) ? 1u : 0u;
}

struct Lists {
    uint32_t* node;     // [l0][stride]: row l = the touched nodes of level l, ascending
    uint32_t* src;      // [stride]: the event whose preimage is the final one of leaf node[0][j]
    uint64_t* count;    // [depth + 1]: touched nodes per level = hashes per level
    size_t stride;
};

// What slot x adds to the list of level l < l0; pos = exclusive scan of head(node, ., l) at x.  The last slot also
// writes the level's count, and slot 0 of level 0 the counts of the levels from l0 up (one node each).
IMT_AP_HD void scatter_element(const uint32_t* node, const uint32_t* time, const uint32_t* re, uint32_t total, uint32_t x,
                               unsigned l, uint32_t pos, unsigned l0, unsigned depth, const Lists& o) {
    const uint32_t h = head(node, x, l);
    if (h) {
        o.node[(size_t)l * o.stride + pos] = node[x] >> l;
        if (l == 0) o.src[pos] = time[re[x] - 1];       // a leaf's final preimage is its run's last event
    }
    if (x == total - 1) o.count[l] = (uint64_t)pos + h;
    if (x == 0 && l == 0)
        for (unsigned k = l0; k <= depth; k++) o.count[k] = 1;
}

// most nodes a batch of `total` events can touch at level l <= l0: what the launches are sized by (the count itself
// stays on the device)
inline uint32_t bound(uint32_t total, unsigned l0, unsigned l) {
    const uint64_t w = (uint64_t)1 << (l0 - l);
    return w < total ? (uint32_t)w : total;
}

}  // namespace apply
}  // namespace imt
