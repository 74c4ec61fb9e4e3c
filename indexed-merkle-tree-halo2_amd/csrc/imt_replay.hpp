// imt_replay.hpp -- the witnesses of insertions the tree has already made (imt_itree_view_insert_witness).
//
// The n insertions that followed size s are replayed against the tree AS OF s (imt_view.hpp) with the level sweep of
// imt_sweep.hpp, and nothing is written back.  The sweep's tables are those of the original batch -- they depend on the
// values and on s alone -- so the only thing that differs from imt_itree_insert_batch is where an event finds a sibling
// that no earlier event of the replay has written (sibsrc < 0).  The inserting sweep reads it from the stored tree, which
// is the tree as of s at that moment.  The replay's stored tree has moved on to M >= s + n leaves, so that sibling is
// node y of level l as of size s by the view's rule:
//     BATCH   sibsrc >= 0: the newest version of y an earlier event of the replay made, slot sibsrc one level down;
//     EMPTY   y >= ceil(s / 2^l);
//     SIDE    y is in S_l: the side table's entry, at its rank in the level's list;
//     STORED  otherwise: the node the tree of M leaves stores.  It equals the node as of s because every node that
//             differs between the two trees is in S_l or beyond the cut (imt_rewind.hpp).
// k_sweep_view / k_sweep_view_coop go through sibling_source() below, and so does tests/native/replay_sources.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include "imt_view.hpp"

namespace imt {
namespace replay {

enum : int { EMPTY = view::EMPTY, SIDE = view::SIDE, STORED = view::STORED, BATCH = 3 };

struct Source {
    int cls;
    uint32_t at;            // BATCH: the slot one level down; SIDE: the place in the level's list; 0 otherwise
};

// where the sibling `node` (= own node ^ 1) of level l comes from, for an event whose table entry says sibsrc
IMT_VW_HD Source sibling_source(const view::Side& sd, int32_t sibsrc, unsigned l, uint64_t node) {
    if (sibsrc >= 0) return {BATCH, (uint32_t)sibsrc};
    const view::Where w = view::classify(sd, l, node);
    return {w.cls, w.rank};
}

// its 32 bytes.  val_in: the replay's versions of level l by slot; stored_l / len_l / zero_l as in view::node_row, and
// as there a STORED node the level cannot hold reads as the empty subtree, never out of bounds.
IMT_VW_HD const uint8_t* sibling_row(const view::Side& sd, int32_t sibsrc, unsigned l, uint64_t node, const uint8_t* val_in,
                                     const uint8_t* stored_l, uint64_t len_l, const uint8_t* zero_l) {
    const Source src = sibling_source(sd, sibsrc, l, node);
    if (src.cls == BATCH) return val_in + (size_t)src.at * 32;
    if (src.cls == SIDE) return view::side_row(sd, l, src.at);
    if (src.cls == STORED && node < len_l) return stored_l + node * 32;
    return zero_l;
}

}  // namespace replay
}  // namespace imt
