// imt_resize.hpp -- another capacity for a tree that exists: the layout of the stored nodes, and where each node of the
// new layout comes from.
//
// The nodes of an indexed tree of capacity C (a power of two) lie in one array, level after level: level l holds
// level_len(C, l) = max(1, C >> l) nodes at offset level_off(C, l) = sum of the lengths below it.  A level is a filled
// prefix -- node i of level l exists for i < level_len -- and every node outside the prefix reads as the empty subtree
// Z[l].  The tree of another capacity that holds the same leaves therefore stores, at node i of level l,
//     the old node i of level l   where the old layout has one (from_old),
//     Z[l]                        where it has not,
// and nothing is hashed: a node the old layout lacks has no leaf below it (the size fits both capacities), and a node
// only the old layout has is dropped where it was Z[l] already.
// imt_itree_new lays its tree out with level_len, k_restride_levels (imt_kernels.hip) moves the nodes with locate /
// from_old, and tests/native/resize_levels.cpp runs the same functions on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define IMT_RS_HD __host__ __device__ __forceinline__
#else
#define IMT_RS_HD inline
#endif

namespace imt {
namespace resize {

// nodes stored for level l at capacity cap; a 64-bit shift by 64 or more is not defined, and cap <= 2^31 anyway
IMT_RS_HD uint64_t level_len(uint64_t cap, unsigned l) {
    const uint64_t n = l < 63 ? cap >> l : 0;
    return n ? n : 1;
}
// nodes stored below level l; level_off(cap, depth + 1) is the whole array
IMT_RS_HD uint64_t level_off(uint64_t cap, unsigned l) {
    uint64_t off = 0;
    for (unsigned k = 0; k < l; k++) off += level_len(cap, k);
    return off;
}
IMT_RS_HD uint64_t total_nodes(uint64_t cap, unsigned depth) { return level_off(cap, depth + 1); }

// Level and position of flat node `flat` < total of a layout given by its offsets off[0 .. depth].  The lengths halve,
// so half of all nodes stop at level 0 and three quarters by level 1.
IMT_RS_HD void locate(const uint64_t* off, unsigned depth, uint64_t flat, unsigned* level, uint64_t* pos) {
    unsigned l = 0;
    while (l < depth && flat >= off[l + 1]) l++;
    *level = l;
    *pos = flat - off[l];
}

// node i of level l of the new layout is the old layout's node i (true) or Z[l] (false)
IMT_RS_HD bool from_old(const uint64_t* old_len, unsigned l, uint64_t i) { return i < old_len[l]; }

// One node of the new array, as the kernel's lanes do it 16 bytes at a time: which 32-byte row it is a copy of.
// Returns the row's index in the old array, or ~0 for Z[level].
IMT_RS_HD uint64_t source_of(const uint64_t* new_off, const uint64_t* old_off, const uint64_t* old_len, unsigned depth,
                             uint64_t flat, unsigned* level) {
    uint64_t i;
    locate(new_off, depth, flat, level, &i);
    return from_old(old_len, *level, i) ? old_off[*level] + i : ~(uint64_t)0;
}

}  // namespace resize
}  // namespace imt
