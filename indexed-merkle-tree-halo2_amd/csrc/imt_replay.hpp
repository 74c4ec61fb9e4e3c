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
#include "imt_sweep.hpp"
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

// ---- the frontier behind a bulk replay (imt_itree_view_bulk_witness) ----
// append_sib[l] of a bulk witness is row l of the proof of the first free slot s AFTER the n rewrites of stored low leaves:
// Z[l] where the sibling lies to the right (bit l of s clear), otherwise node y = (s >> l) - 1 of level l.  The live call
// reads that node from the stored tree behind its write-back; a replay writes nothing back, so the node is
//     VERSION  the level-l version the LAST event below y made, if any event's low_index >> l == y.  Below the first
//              upper level that is the slot the write-back would store (sweep::LAST_BIT of `from`, node_below == y), picked
//              up between the level launches while the versions of level l are still there; at the first upper level
//              (s a power of two, y = 0: every event lies below it) it is the last event's value;
//     VIEW     otherwise: view::node_row as of s.
// k_bulk_frontier_base / k_bulk_frontier_level and the host driver of the replay go through the functions below, and so
// does tests/native/bulk_frontier.cpp.
enum : int { FRONTIER_ZERO = 0, FRONTIER_VIEW = 1, FRONTIER_VERSION = 2 };

// bit l of s: the sibling of slot s at level l lies to the left, i.e. it exists
IMT_VW_HD bool frontier_left(uint64_t s, unsigned l) { return l < 64 && ((s >> l) & 1u); }
// ... and is this node of level l
IMT_VW_HD uint64_t frontier_node(uint64_t s, unsigned l) { return (s >> l) - 1; }
// what row l is before any event is looked at
IMT_VW_HD int frontier_base(uint64_t s, unsigned l) { return frontier_left(s, l) ? FRONTIER_VIEW : FRONTIER_ZERO; }
// Slot kp of the table of level l + 1 (from / node_below: row l of the per-level tables), l below the first upper level:
// true iff the event there carries the final version of the frontier node of level l; `slot` = where that version lies
// among the versions of level l.  At most one kp of a level says so: a node has one last version.
IMT_VW_HD bool frontier_version(uint64_t s, unsigned l, uint32_t from, uint32_t node_below, uint32_t& slot) {
    if (!frontier_left(s, l) || !(from & sweep::LAST_BIT) || (uint64_t)node_below != frontier_node(s, l)) return false;
    slot = from & ~sweep::LAST_BIT;
    return true;
}
// The first upper level `top` = min(ceil_log2(s), depth) of a replay of `events` > 0 events: true iff the frontier has a
// left-hand sibling there -- s = 2^top, node 0, which every event lies below; `slot` = the last event's (values are by
// event from here up).  Above `top` bit l of s is clear.
IMT_VW_HD bool frontier_top_version(uint64_t s, unsigned top, uint32_t events, uint32_t& slot) {
    if (top >= 64 || s != ((uint64_t)1 << top) || events == 0) return false;
    slot = events - 1;
    return true;
}

}  // namespace replay
}  // namespace imt
