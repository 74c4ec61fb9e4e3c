// imt_launch.hpp -- host-callable launchers of the gfx950 kernels (imt_kernels.hip).
// Everything is asynchronous on `stream`; pointers are device pointers.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include "imt_consts.hpp"
#include "imt_sweep.hpp"
#include "imt_view.hpp"
#include "imt_replay.hpp"

namespace imt {
namespace launch {

// sibling array addressing in units of 32-byte elements:
//   element(level, item) = sib + (level * level_stride + item * item_stride) * 32
struct SibLayout {
    uint64_t level_stride, item_stride;
};

// description of a stored tree: level l has `len[l]` nodes at nodes + off[l]*32; nodes
// outside [0, len[l]) read as zero[l] (the empty-subtree hash of that height)
struct TreeView {
    const uint8_t* nodes;        // device format
    const uint64_t* off;         // [depth+1] device array
    const uint64_t* len;         // [depth+1] device array
    const uint8_t* zero;         // [depth+1][32] device format, may be NULL when never needed
    uint64_t index_base = 0;     // leaf indices handed to gather_proof are global: local = index - index_base
};

hipError_t upload_consts(const dev::PoseidonConsts& pc);
hipError_t upload_trace_consts(const dev::TraceConsts& tc);

// f1: every witness of hash_fix_len_array for n_items hashes of `arity` inputs.  The items form blocks of n_per (the
// levels of a path; a single block otherwise); block l occupies rows [row0 + l * rows, ...) of a trace of rows_total
// rows per item column, row-major [rows_total][n_per] or item-major [n_per][rows_total].
void hash_trace(hipStream_t s, const uint8_t* in, size_t n_items, int arity, uint8_t* trace, size_t n_per, size_t row0,
                size_t rows_total, bool item_major, unsigned fmt_in, unsigned fmt_out, int* err);
// The same for up to eight groups of hashes in ONE launch (blockIdx.y = group): the 3 leaf hashes and 4 paths of an
// insert_leaf call do not depend on each other once the path inputs are known, and for a few items one thread per hash
// leaves the chip empty -- seven launches in a row would cost seven times one hash's 0.9 ms.
struct TraceJobs {
    struct Job {
        const uint8_t* in;       // [n_items][arity][32]
        size_t n_items;          // item q -> block q / n_per (rows row0 + (q / n_per) * rows(arity) ...) of column q % n_per
        int arity;
        size_t row0;
        unsigned fmt_in;
    } j[8];
    int n_jobs;
    uint8_t* trace;
    size_t n_per, rows_total;
    int item_major;
    int* err;
};
void hash_trace_jobs(hipStream_t s, const TraceJobs& a, unsigned fmt_out);
// {low.val, new.val, new_index} per item -> new_low [n][3][32], and the zero-leaf hash -> zero_leaf [n][32] (fmt)
void insert_trace_inputs(hipStream_t s, const uint8_t* low_leaf, const uint8_t* new_leaf, const uint64_t* new_index,
                         size_t n, uint8_t* new_low, uint8_t* zero_leaf, unsigned fmt, int* err);
// the (left, right) inputs of every hash2 along n paths, for up to four chains in one launch:
// chain k writes pairs[depth][n][2][32] (device format) and optionally its roots
struct PathChains {
    struct Chain {
        const uint8_t* leaf;      // [n][32], or
        const uint8_t* leaf3;     // [n][3][32]: the chain starts from H(leaf3)
        const uint64_t* index;
        const uint8_t* sib;
        uint8_t* pairs;
        uint8_t* root_out;        // or NULL
    } c[4];
    int n_chains;
    SibLayout lay;
    unsigned depth;
    size_t n;
    unsigned fmt_in, fmt_out;
    int* err;
};
void path_pairs(hipStream_t s, const PathChains& a, uint32_t coop_max);

void hash_batch(hipStream_t s, const uint8_t* in, uint8_t* out, size_t n, int arity, unsigned fmt_in,
                unsigned fmt_out, int* err, uint32_t coop_max = 0);
// imt_hash_n.hip: the hash of `len` = 1..16 inputs per item, in[n][len][32].  That translation unit keeps its own copies
// of the two tables (upload_hash_n_consts, once per context).  coop_max as for hash_batch.
hipError_t upload_hash_n_consts(const dev::PoseidonConsts& pc, const dev::TraceConsts& tc);
void hash_n_batch(hipStream_t s, const uint8_t* in, unsigned len, uint8_t* out, size_t n, unsigned fmt_in, unsigned fmt_out,
                  int* err, uint32_t coop_max);
// ... and its witness trace: `rows` = imt_hash_n_trace_rows(len) rows per hash, [rows][n] or item-major [n][rows]
void hash_n_trace(hipStream_t s, const uint8_t* in, unsigned len, size_t n, uint8_t* trace, size_t rows, bool item_major,
                  unsigned fmt_in, unsigned fmt_out, int* err);
void permute_batch(hipStream_t s, const uint8_t* in, uint8_t* out, size_t n, unsigned fmt_in,
                   unsigned fmt_out, int* err);
void convert(hipStream_t s, const uint8_t* in, uint8_t* out, size_t n, unsigned fmt_in,
             unsigned fmt_out, int* err);

// `blocks` x 256 threads, each 8 x `iters` multiply-adds
void mad_peak(hipStream_t s, uint32_t* out, unsigned blocks, int iters);
void split128(hipStream_t s, const uint8_t* vals, uint8_t* q, uint8_t* r, size_t n, unsigned fmt, int* err);

// Path recompute.  leaf3 != NULL: the start value is hash3(leaf3[i]) ([n][3][32]);
// otherwise leaf[i].  index bit l (or ~helper_mask bit l when is_helper) = node is a right
// child at level l.  expect (optional, stride 0 or 32 bytes) -> ok_out[i].
void path_root(hipStream_t s, const uint8_t* leaf, const uint8_t* leaf3, const uint64_t* index,
               bool is_helper, const uint8_t* sib, SibLayout lay, unsigned depth, size_t n,
               uint8_t* root_out, const uint8_t* expect, unsigned expect_stride, uint8_t* ok_out,
               unsigned fmt_in, unsigned fmt_out, int* err, uint32_t coop_max = 0);

void non_membership(hipStream_t s, const uint8_t* root, unsigned root_stride, const uint8_t* low_leaf,
                    const uint64_t* low_index, const uint8_t* sib, SibLayout lay, unsigned depth,
                    const uint8_t* new_val, const uint8_t* is_largest, size_t n, uint8_t* fail_out,
                    uint8_t* root_out, unsigned fmt_in, unsigned fmt_out, int* err, uint32_t coop_max);

// 4 chains per item; trace [7][n][32] (device buffer, required), then the check kernel
void insert_witness(hipStream_t s, const uint8_t* old_root, const uint8_t* low_leaf,
                    const uint64_t* low_index, const uint8_t* low_sib, const uint8_t* new_root,
                    const uint8_t* new_leaf, const uint64_t* new_index, const uint64_t* new_path_index,
                    const uint8_t* new_sib, SibLayout lay, const uint8_t* is_largest, unsigned depth, size_t n,
                    uint8_t* fail_out, uint8_t* trace, unsigned fmt_in, unsigned fmt_out, int* err, uint32_t coop_max);

// next[i] = hash2(prev[2i], prev[2i+1]), device format
void tree_level(hipStream_t s, const uint8_t* prev, uint8_t* next, size_t n_parents, uint32_t coop_max = 0);
// stored level 0 from the device index (val[M][32] canonical, sorted[M]): node sorted[r] = H(val[sorted[r]],
// val[sorted[r + 1]], base + sorted[r + 1]), the last rank H(val, 0, 0); tree0 in device format.  A value >= p sets *err.
void index_leaves(hipStream_t s, const uint8_t* val, const uint32_t* sorted, uint32_t M, uint64_t base, uint8_t* tree0,
                  int* err);
// chain: out[l+1] = hash2(out[l], out[l]) for l < depth, out[0] = H(0,0,0); one thread
void zero_chain(hipStream_t s, uint8_t* out, unsigned depth);
// cur = hash2(cur, zero[l]) for l in [from, to): extends a subtree root up the left spine
void extend_root(hipStream_t s, uint8_t* cur, const uint8_t* zero, unsigned from, unsigned to);

// siblings of `index[i]` at every level of a stored tree
void gather_proof(hipStream_t s, TreeView tv, const uint64_t* index, size_t n, unsigned depth,
                  uint8_t* out, SibLayout lay, unsigned fmt_out);
// helper[l] = 1 iff (index >> l) is even, as field elements (get_proof, src/utils.rs:79)
void write_helpers(hipStream_t s, uint64_t index, unsigned depth, uint8_t* out, unsigned fmt_out);


// ---- batch insertion level sweep (imt_sweep.hpp) ----
// argument block of k_sweep, the one hash kernel behind sweep_leaves / sweep_level / sweep_upper
enum : int { SWEEP_LEAVES = 0, SWEEP_LEVEL = 1 };
struct SweepArgs {
    int mode;
    uint32_t begin, count;                // slots [begin, begin + count)
    // LEAVES
    const uint8_t* pre;
    const uint32_t* time0;
    unsigned fmt_in;
    int* err;
    // LEVEL
    const uint8_t* val_in;
    uint8_t* val_out;                     // (LEAVES writes it too)
    const uint32_t* from;                 // NULL at and above l0: slot = event, node 0, sibling = zero_l
    const int32_t* sibsrc;
    const uint32_t* node_below;
    const uint32_t* time_next;
    const uint8_t* tree_l;
    uint64_t len_l;
    const uint8_t* zero_l;
    unsigned level;
    uint32_t last_event;                  // the event whose node goes back to the stored tree (above l0), or ~0
    uint8_t *node_in, *node_out;          // where its input / output value is stored (device format), or NULL
    uint8_t *low_sib, *new_sib;           // proof rows
    SibLayout lay;
    unsigned fmt_out;
};
void fill_level(hipStream_t s, uint8_t* nodes, size_t n, const uint8_t* zero_l);
// imt_itree_reserve (imt_resize.hpp): every node of the new layout -- new_total nodes, levels at new_off [depth+1] --
// from the node at the same level and position of the old layout (old_off / old_len [depth+1]) or, where that has none,
// from zero [depth+1][32].  All offset arrays are device arrays; the two node arrays do not overlap.
void restride_levels(hipStream_t s, const uint8_t* old_nodes, const uint64_t* old_off, const uint64_t* old_len,
                     uint8_t* new_nodes, const uint64_t* new_off, uint64_t new_total, const uint8_t* zero, unsigned depth);
// coop_max: launches of at most this many events use the latency form of the kernel (a quad of lanes per event,
// imt_coop_device.hpp); 0 = never
void sweep_leaves(hipStream_t s, const uint8_t* pre, const uint32_t* time0, uint8_t* val0, uint32_t k_begin,
                  uint32_t k_count, unsigned fmt_in, int* err, uint32_t coop_max);
void merge_level(hipStream_t s, sweep::LevelTable in, sweep::LevelOut out, uint32_t total);
// hashes slots [k_begin, k_begin + k_count) of level `level`+1 (a rank's share when sharded)
void sweep_level(hipStream_t s, const uint8_t* val_in, uint8_t* val_out, const uint32_t* from, const int32_t* sibsrc,
                 const uint32_t* node_below, const uint32_t* time_next, const uint8_t* tree_l, uint64_t len_l,
                 const uint8_t* zero_l, uint32_t k_begin, uint32_t k_count, uint8_t* low_sib, uint8_t* new_sib,
                 SibLayout lay, unsigned level, unsigned fmt_out, uint32_t coop_max);
void writeback(hipStream_t s, const uint8_t* val_l, const uint32_t* from, const uint32_t* node_below, uint8_t* tree_l,
               uint32_t total);
// level l >= l0 for events [e_begin, e_begin + e_count): val indexed by event id, sibling = zero_l; the values
// of `last_event` go to node_in (its input, i.e. the node at level l) / node_out (the node at level l + 1)
void sweep_upper(hipStream_t s, const uint8_t* val_in, uint8_t* val_out, const uint8_t* zero_l, uint32_t e_begin,
                 uint32_t e_count, uint32_t last_event, uint8_t* node_in, uint8_t* node_out, uint8_t* low_sib,
                 uint8_t* new_sib, SibLayout lay, unsigned level, unsigned fmt_out, uint32_t coop_max);
// roots per event from the top values (no hashing); sharded mode: roots_dev[e] in device format
void emit_roots(hipStream_t s, const uint8_t* val, uint32_t e_begin, uint32_t e_count, uint32_t total, uint8_t* old_root,
                uint8_t* interim_root, uint8_t* new_root, unsigned fmt_out, uint8_t* roots_dev, uint8_t* node_store);

// ---- witness-free batch insertion (imt_apply.hpp): one hash per touched node, straight into the stored tree ----
// argument block of k_apply_level.  The launch is sized by `bound`; the number of listed nodes is read on the device.
enum : int { APPLY_LEAVES = 0, APPLY_LEVEL = 1 };
struct ApplyArgs {
    int mode;
    const uint64_t* count;                // device word: listed nodes (<= bound)
    uint32_t bound;
    const uint32_t* list;                 // [count] nodes of the level that is written, ascending
    uint8_t* tree_out;                    // that stored level (device format) and its length
    uint64_t len_out;
    // LEAVES: node list[j] = H(preimage of event src[j])
    const uint32_t* src;
    const uint8_t* pre;
    unsigned fmt_in;
    int* err;
    // LEVEL: node p = hash2(children 2p, 2p + 1 of the stored level below; outside its prefix: zero_in)
    const uint8_t* tree_in;
    uint64_t len_in;
    const uint8_t* zero_in;
};
// coop_max as for the sweep: a launch of at most that many nodes (by its bound) takes the quad form
void apply_leaves(hipStream_t s, const uint64_t* count, uint32_t bound, const uint32_t* list, const uint32_t* src,
                  const uint8_t* pre, unsigned fmt_in, int* err, uint8_t* tree0, uint64_t len0, uint32_t coop_max);
void apply_level(hipStream_t s, const uint64_t* count, uint32_t bound, const uint32_t* list, const uint8_t* tree_in,
                 uint64_t len_in, const uint8_t* zero_in, uint8_t* tree_out, uint64_t len_out, uint32_t coop_max);
// levels [from, to), from = l0 - 1: stored node 0 of level l + 1 = hash2(stored node 0 of level l, its right sibling):
// stored node 1 at level `from`, zero[l] above.  off / len: the tree's device arrays.  One quad.
void apply_top(hipStream_t s, uint8_t* nodes, const uint64_t* off, const uint64_t* len, const uint8_t* zero, unsigned from,
               unsigned to);
// the same chain into rows from + 1 .. to of `chain` ([depth + 1][32], the caller's) with nothing written to the tree,
// and rows [from, to] of such a chain into node 0 of stored levels from .. to, row `to` also into root[32]
// (imt_itree_apply_pipelined: the hashes of consecutive batches overlap, only the store is ordered)
void apply_chain(hipStream_t s, const uint8_t* nodes, const uint64_t* off, const uint64_t* len, const uint8_t* zero,
                 uint8_t* chain, unsigned from, unsigned to);
void apply_chain_store(hipStream_t s, const uint8_t* chain, uint8_t* nodes, const uint64_t* off, unsigned from, unsigned to,
                       uint8_t* root);

// ---- a view of the tree at an earlier size (imt_view.hpp): the same hashes into a side table, the tree only read ----
// argument block of k_view_level: ApplyArgs with another store address -- listed node j goes to out + j * 32 -- and, for a
// LEVEL launch, the children read through view::node_row.
struct ViewArgs {
    int mode;                             // APPLY_LEAVES / APPLY_LEVEL
    const uint64_t* count;                // device word: listed nodes of the level that is hashed (<= bound)
    uint32_t bound;                       // <= the side table's stride: rank j < bound stays inside row `out`
    const uint32_t* list;                 // [count] those nodes, ascending
    uint8_t* out;                         // the side table's row of that level
    uint64_t len_out;                     // nodes the level can hold: a listed node beyond it is never hashed
    // LEAVES: as ApplyArgs
    const uint32_t* src;
    const uint8_t* pre;
    unsigned fmt_in;
    int* err;
    // LEVEL: node p = hash2(children 2p, 2p + 1 of level `level_in` as of the view's size)
    view::Side side;
    unsigned level_in;
    const uint8_t* tree_in;               // the stored level below, its length and its empty subtree
    uint64_t len_in;
    const uint8_t* zero_in;
};
void view_leaves(hipStream_t s, const uint64_t* count, uint32_t bound, const uint32_t* list, const uint32_t* src,
                 const uint8_t* pre, unsigned fmt_in, int* err, uint8_t* out, uint64_t len0, uint32_t coop_max);
// row level_in + 1 of the side table from level level_in
void view_level(hipStream_t s, const view::Side& side, unsigned level_in, uint32_t bound, const uint8_t* tree_in,
                uint64_t len_in, const uint8_t* zero_in, uint8_t* out, uint64_t len_out, uint32_t coop_max);
// chain[l + 1] = hash2(node 0 of level l, its right sibling) for l in [from, to), from = side.top - 1: both through the
// rule at level `from`, chain[l] and zero[l] above.  tv: the stored tree.  One quad.
void view_top(hipStream_t s, const view::Side& side, TreeView tv, uint8_t* chain, unsigned from, unsigned to);
// gather_proof with every sibling read as of the view's size
void view_gather_proof(hipStream_t s, const view::Side& side, TreeView tv, const uint64_t* index, size_t n, unsigned depth,
                       uint8_t* out, SibLayout lay, unsigned fmt_out);

// ---- witnesses of insertions already made (imt_replay.hpp): the level sweep against a view, nothing written back ----
// argument block of k_sweep_view: a LEVEL launch of k_sweep below l0 (from .. time_next required, no node_in / node_out)
// and the view whose size the base siblings are read as of.  tree_l / len_l / zero_l: the stored level, as for k_sweep.
struct SweepViewArgs {
    SweepArgs sweep;
    view::Side side;
};
// hashes slots [0, k_count) of level `level` + 1; coop_max as for the sweep
void sweep_view_level(hipStream_t s, const view::Side& side, const uint8_t* val_in, uint8_t* val_out, const uint32_t* from,
                      const int32_t* sibsrc, const uint32_t* node_below, const uint32_t* time_next, const uint8_t* tree_l,
                      uint64_t len_l, const uint8_t* zero_l, uint32_t k_count, uint8_t* low_sib, uint8_t* new_sib, SibLayout lay,
                      unsigned level, unsigned fmt_out, uint32_t coop_max);

// ---- mixed batches (imt_itree_mixed_batch): the sweep with READ events among the INSERTs' ----
// erow[e] = (row << 2) | kind for every event (prep::ROW_*): whose proof rows and root event e's are.  read_sib: the READs'
// low_sib (NULL: not wanted), dimensioned like the INSERTs' sibling arrays.  The leaf hashes and the index phase of a
// mixed batch are the ordinary ones; these are its LEVEL launches (below l0: all slots; above: all events, the last
// event's nodes to node_in / node_out) and its roots.  coop_max as for the sweep.
struct MixedRoute {
    const uint32_t* erow;
    uint8_t* read_sib;
};
struct SweepMixedArgs {                   // argument block of k_sweep_mixed: a LEVEL launch of k_sweep and the route
    SweepArgs sweep;
    const uint32_t* erow;
    uint8_t* read_sib;
};
void sweep_level_mixed(hipStream_t s, const MixedRoute& r, const uint8_t* val_in, uint8_t* val_out, const uint32_t* from,
                       const int32_t* sibsrc, const uint32_t* node_below, const uint32_t* time_next, const uint8_t* tree_l,
                       uint64_t len_l, const uint8_t* zero_l, uint32_t k_count, uint8_t* low_sib, uint8_t* new_sib, SibLayout lay,
                       unsigned level, unsigned fmt_out, uint32_t coop_max);
void sweep_upper_mixed(hipStream_t s, const MixedRoute& r, const uint8_t* val_in, uint8_t* val_out, const uint8_t* zero_l,
                       uint32_t e_count, uint8_t* node_in, uint8_t* node_out, uint8_t* low_sib, uint8_t* new_sib, SibLayout lay,
                       unsigned level, unsigned fmt_out, uint32_t coop_max);
void emit_roots_mixed(hipStream_t s, const MixedRoute& r, const uint8_t* val, uint32_t total, uint32_t n_ins, uint8_t* old_root,
                      uint8_t* interim_root, uint8_t* new_root, uint8_t* read_root, unsigned fmt_out, uint8_t* node_store);

// ---- bulk insertion (imt_itree_insert_bulk): one low-leaf rewrite per value, then all new leaves at once ----
// The sweep of a bulk batch is a mixed one whose events are all prep::ROW_LOW (rows of low_sib); these are its roots --
// root_after[k] = the top value of event k = root_before[k + 1] -- and, behind its last write-back, the proof of the first
// free slot with zero[l] at every right-hand level.  The append itself is the witness-free schedule (apply_leaves /
// apply_level / apply_top) over the dense list of the new leaves.
void emit_roots_bulk(hipStream_t s, const uint8_t* val, uint32_t total, uint8_t* root_before, uint8_t* root_after,
                     unsigned fmt_out, uint8_t* node_store);
void gather_frontier(hipStream_t s, TreeView tv, uint64_t index, unsigned depth, uint8_t* out, unsigned fmt_out);
// The stateless form (imt_frontier_append_root): n nodes of level 0 at start .. start + n - 1 hashed upwards on scratch rows
// until one node is left at level `top`, then two paths.  frontier_rows says where row l lies (in nodes) and how many
// nodes it has; frontier_bounds writes the boundary slots, the frontier with its right-hand rows forced to zero[l], and
// the two path indices (k_frontier_bounds).
constexpr unsigned FRONTIER_MAX_DEPTH = 64;       // IMT_MAX_DEPTH (imt_ctx.hpp)
struct FrontierArgs {
    const uint8_t* sib;                  // [depth][32] the caller's, fmt_in
    unsigned fmt_in;
    int* err;
    uint64_t start, n;
    unsigned depth, top;                  // top: the first level at which the range is one node
    const uint8_t* zero;                  // [depth + 1][32] device format
    uint8_t* rows;                        // scratch of frontier_rows(...) nodes
    uint64_t off[FRONTIER_MAX_DEPTH + 1];     // row l starts at rows + off[l] * 32
    uint8_t* fsib;                        // [depth][32] device format
    uint64_t* idx;                        // [2]
};
// fills a.top and a.off from a.start / a.n / a.depth; returns the nodes `rows` must hold
uint64_t frontier_rows(FrontierArgs& a);
void frontier_bounds(hipStream_t s, const FrontierArgs& a);
// The builder both callers share (imt_frontier_append_root, imt_itree_view_bulk_witness), with a.rows / a.fsib / a.idx the
// caller's scratch: the leaves into row 0 -- hash3 of leaf[n][3][32] if leaf3, else leaf[n][32] as they are, fmt_leaf --,
// the boundary slots, one tree_level per level until one node is left, then that node's path into root_after and (unless
// NULL) the path of Z[0] from `start` into root_before, both fmt_out.  Host code over the launchers above, nothing else.
inline void frontier_append(hipStream_t s, const FrontierArgs& a, const uint8_t* leaf, bool leaf3, unsigned fmt_leaf,
                            uint8_t* root_before, uint8_t* root_after, unsigned fmt_out, uint32_t coop_max) {
    constexpr unsigned dev = 2u;      // the resident format of stored nodes (FMT_DEVICE, imt_device.hpp)
    auto row = [&](unsigned l) { return a.rows + (a.off[l] + ((a.start >> l) & 1)) * 32; };   // the first node of the range at level l
    if (leaf3) hash_batch(s, leaf, row(0), a.n, 3, fmt_leaf, dev, a.err, coop_max);
    else convert(s, leaf, row(0), a.n, fmt_leaf, dev, a.err);
    frontier_bounds(s, a);
    for (unsigned l = 0; l < a.top; l++) {
        const uint64_t parents = ((a.start + a.n - 1) >> (l + 1)) - (a.start >> (l + 1)) + 1;
        tree_level(s, a.rows + a.off[l] * 32, row(l + 1), parents, coop_max);
    }
    const SibLayout one{1, 1};
    if (root_before)
        path_root(s, a.zero, nullptr, a.idx, false, a.fsib, one, a.depth, 1, root_before, nullptr, 0, nullptr, dev,
                  fmt_out, a.err, coop_max);
    path_root(s, row(a.top), nullptr, a.idx + 1, false, a.fsib + (size_t)a.top * 32, one, a.depth - a.top, 1, root_after, nullptr, 0,
              nullptr, dev, fmt_out, a.err, coop_max);
}
// ---- the frontier behind a bulk replay (imt_itree_view_bulk_witness; the rule is in imt_replay.hpp) ----
// out: [depth][32] device format.  bulk_frontier_base before the sweep: row l = the node as of the view's size where bit l
// of side.size is set, zero[l] elsewhere.  bulk_frontier_level behind the launch that made the versions val_l of level l
// (from / node_below: row l of the per-level tables, `total` slots) and before the launch after next overwrites them: the
// final version of the frontier's node of level l into out_l, if an event made one; nothing where bit l of size is clear.
void bulk_frontier_base(hipStream_t s, const view::Side& side, TreeView tv, unsigned depth, uint8_t* out);
void bulk_frontier_level(hipStream_t s, uint64_t size, unsigned level, const uint8_t* val_l, const uint32_t* from,
                         const uint32_t* node_below, uint32_t total, uint8_t* out_l);

// ---- witnesses of a mixed block already applied (imt_itree_view_mixed_witness): both of the above at once ----
// argument block of k_sweep_view_mixed: k_sweep_view's (a LEVEL launch below l0 and the view the base siblings are read as
// of) with k_sweep_mixed's route.  The levels from l0 up are sweep_upper_mixed with both node stores NULL, the roots
// emit_roots_mixed with node_store NULL: nothing goes back to the stored tree.
struct SweepViewMixedArgs {
    SweepArgs sweep;
    view::Side side;
    const uint32_t* erow;
    uint8_t* read_sib;
};
// hashes slots [0, k_count) of level `level` + 1; coop_max as for the sweep
void sweep_view_level_mixed(hipStream_t s, const view::Side& side, const MixedRoute& r, const uint8_t* val_in, uint8_t* val_out,
                            const uint32_t* from, const int32_t* sibsrc, const uint32_t* node_below, const uint32_t* time_next,
                            const uint8_t* tree_l, uint64_t len_l, const uint8_t* zero_l, uint32_t k_count, uint8_t* low_sib,
                            uint8_t* new_sib, SibLayout lay, unsigned level, unsigned fmt_out, uint32_t coop_max);

// ---- subtree placement: lift subtree-level witnesses to the depth of the enclosing tree ----
// top[j] (device format, j < levels) = sibling of this subtree's ancestor at height sub_depth + j;
// bit j of pos_bits = that ancestor is a RIGHT child.  Roots are lifted in place (format fmt):
// interim_root[i], new_root[i] and old_root[i] climb `levels` hashes each; with new_root and old_root
// both given, old_root[i + 1] is written from new_root[i] and only old_root[0] climbs on its own.
void lift_roots(hipStream_t s, uint8_t* old_root, uint8_t* interim_root, uint8_t* new_root, uint32_t n,
                const uint8_t* top, uint64_t pos_bits, unsigned levels, unsigned fmt, int* err);
// rows [first_level, first_level + levels) of a sibling array = top[j], for all n items
void fill_sib_rows(hipStream_t s, uint8_t* sib, SibLayout lay, unsigned first_level, unsigned levels, uint32_t n,
                   const uint8_t* top, unsigned fmt_out);
// mixed[r] = r < self ? after[r] : before[r]   (device format out, fmt_in in)
void mix_roots(hipStream_t s, const uint8_t* before, const uint8_t* after, uint8_t* mixed, uint32_t n_sub, uint32_t self,
               unsigned fmt_in, int* err);
// top[j] = node (j, (self >> j) ^ 1) of the tree over `mixed` for j < k, then zero[sub_depth + j] for j >= k
void pick_top(hipStream_t s, const uint8_t* levels_buf, uint32_t n_sub, uint32_t self, unsigned k, unsigned levels,
              const uint8_t* zero, unsigned sub_depth, uint8_t* top);

// ---- sharded single-list batch (imt_itree_batch_*) ----
void slot0(hipStream_t s, const uint32_t* time0, uint32_t* slot0_out, uint32_t total);
struct ExtractParams {
    const uint8_t* const* val;   // device array of l0 + 1 device pointers
    const uint32_t* slot;
    const int32_t* sibsrc;
    const uint32_t* node_below;
    size_t stride;
    const uint8_t* tree_nodes;
    const uint64_t* tree_off;
    const uint64_t* tree_len;
    const uint8_t* zero;
    const uint8_t* roots;
    unsigned l0, depth;
    uint32_t ins_begin, ins_count, n_total;
    uint8_t *old_root, *interim_root, *new_root, *low_sib, *new_sib;
    SibLayout lay;
    unsigned fmt_out;
};
void extract(hipStream_t s, const ExtractParams& p);
// time-sliced single list: the (node, value) pairs k_writeback would write, packed behind an atomic counter (at most
// `cap` of them), and their application to a replica's stored level
void pack_writeback(hipStream_t s, const uint8_t* val_l, const uint32_t* from, const uint32_t* node_below, uint32_t total,
                    uint8_t* tree_l, uint8_t* out_vals, uint32_t* out_nodes, uint32_t* counter, uint32_t cap,
                    hipEvent_t done = nullptr);
void apply_packed(hipStream_t s, const uint8_t* vals, const uint32_t* nodes, const uint32_t* counter, uint32_t cap,
                  uint8_t* tree_l, uint64_t len_l);
// every payload of one all-gather applied by one launch (imt_itree_slice_apply_gathered)
struct ApplyJobs {
    struct Job {
        const uint8_t* payload;          // header 128 B | values [cap][32] | node ids [cap]
        int pairs;                       // 1: (node, value) pairs for stored level tree_l; 0: the header's nodes
        uint32_t cap;
        uint8_t* tree_l;
        uint64_t len_l;
        uint8_t *node_in, *node_out, *root;     // header targets (any may be NULL)
    } j[16];
    int n_jobs;
    const uint32_t* poison;              // device-visible word (may be NULL): non-zero = a transport gave up waiting for a
                                         // payload of this gather, nothing is applied (imt_flags.hip)
};
// done (here and in pack_writeback): the event the kernel's own completion signals (hipExtLaunchKernelGGL's stop event) --
// what a hipEventRecord right behind the launch would mark, without the marker packet
void apply_gathered(hipStream_t s, const ApplyJobs& a, hipEvent_t done = nullptr);
void store_top_path(hipStream_t s, const uint8_t* top_path, uint8_t* tree_nodes, const uint64_t* tree_off, unsigned l0,
                    unsigned depth);

}  // namespace launch
}  // namespace imt
