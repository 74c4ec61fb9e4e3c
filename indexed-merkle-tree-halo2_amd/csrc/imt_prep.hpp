// imt_prep.hpp -- GPU-side preparation of a batch insertion ("GPU low-leaf
// search"): everything imt_itree.cpp otherwise does on the host between receiving the values and
// launching the hash sweep -- the low-leaf search of update_idx_leaf
// (/root/reference/src/indexed_merkle_tree.rs:639-658), the event preimages and the
// (position, time) order of the events -- as device kernels over a device-resident index.
//
// Device index of a tree: val[cap][32] (canonical integers, leaf order) and sorted[size] (leaf
// indices in ascending value order).  Leaf indices ARE insertion times, so "the low leaf of v at
// the time it is inserted" is the nearest element to the left of v, in value order, with a
// smaller leaf index: an all-nearest-smaller-values problem, solved per batch with a sparse
// min-table over the batch in value order plus the gap (number of stored values below) of each
// new value.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include "imt_apply.hpp"

namespace imt {
namespace prep {

constexpr uint32_t NONE = 0xffffffffu;
// error bits written by the kernels
constexpr int ERR_NONCANONICAL = 1, ERR_ZERO = 2, ERR_DUPLICATE = 4, ERR_FOREIGN = 8;
// 16 / 32 / 64 / 128: LOAD_SENTINEL / LOAD_LINK / LOAD_LAST / LOAD_TIE of the snapshot check (imt_prep_logic.hpp)
constexpr int ERR_RANGE = 256;

struct Workspace {            // per plan set, sized for `cap_n` insertions
    size_t cap_n = 0;
    uint32_t part_mod = 0, part_res = 0;   // value partition: accept only v % part_mod == part_res (0/1 = everything)
    uint32_t* iota = nullptr;      // [n]   M+i
    uint32_t* bsorted = nullptr;   // [n]   new leaf indices in value order
    uint32_t* gap = nullptr;       // [n]   stored values below each new value
    uint32_t* st = nullptr;        // [levels][n] sparse min-table of insertion times
    uint32_t* low = nullptr;       // [n]   by insertion time
    uint32_t* succ = nullptr;      // [n]
    uint64_t* keys = nullptr;      // [2n]  (position << 32) | event
    uint64_t* keys_sorted = nullptr;
    void* tmp = nullptr;           // rocPRIM temporary storage
    size_t tmp_bytes = 0;
    int* err = nullptr;            // device word
    // hash-free outputs kept for imt_itree_batch_extract (sharded mode)
    uint64_t* o_low = nullptr;     // [n]
    uint8_t* o_largest = nullptr;  // [n]
    uint8_t* o_lowleaf = nullptr;  // [n][96]
    uint8_t* o_newleaf = nullptr;  // [n][96]
};

size_t temp_bytes_needed(size_t n, size_t max_size);

// Everything up to (and including) the level-0 tables and the new sorted index.
//   vals      [n][32] canonical, device
//   d_val     device index values; rows [M, M+n) are written
//   sorted_old[M] -> sorted_new[M+n]
//   pre       [2n][96] event preimages (canonical)
//   node/time/rs/re  level-0 tables [2n]
//   o_* user outputs (device pointers, any may be NULL): low_index u64[n], is_largest u8[n],
//        low_leaf / new_leaf [n][3][32] canonical
//   base      added to every leaf index that leaves the tree: the next_idx fields of the preimages and
//             o_low_index (a tree placed as a subtree of a deeper one, imt_itree_set_placement)
// Errors are OR-ed into ws.err (ERR_*); nothing outside rows [M, M+n) of d_val, sorted_new and the
// workspace is written, so a failed batch leaves the tree untouched.  Returns the first failure of a
// rocPRIM call or kernel launch (hipErrorInvalidValue if the workspace is too small for (n, M)).
// All 32-byte rows (vals, d_val, pre, o_*_leaf) must be 16-byte aligned: they move as two 16-byte words.
// vals == NULL: the values are rows [M, M + n) of d_val already (a replay of insertions the tree has made,
// imt_itree_view_insert_witness).  Then no row of d_val is written, not even with the bytes it holds, and the checks of
// the values themselves (non-canonical, zero, foreign) are skipped: stored values passed them when they went in.
hipError_t run(hipStream_t s, Workspace& ws, const uint8_t* vals, uint8_t* d_val, const uint32_t* sorted_old,
               uint32_t* sorted_new, uint32_t M, uint32_t n, uint64_t base, uint8_t* pre, uint32_t* node, uint32_t* time,
               uint32_t* rs, uint32_t* re, uint64_t* o_low_index, uint8_t* o_is_largest, uint8_t* o_low_leaf,
               uint8_t* o_new_leaf);

// The index part of run() alone -- values into rows [M, M+n) of d_val, the checks (non-canonical, zero, duplicate),
// sorted_old[M] -> sorted_new[M+n] -- for values whose hashing is another GPU's share (imt_itree_slice_prepare): needs
// only iota / bsorted / gap / st[n] / tmp / err of the workspace.
hipError_t index_only(hipStream_t s, Workspace& ws, const uint8_t* vals, uint8_t* d_val, const uint32_t* sorted_old,
                      uint32_t* sorted_new, uint32_t M, uint32_t n);

// ---- mixed batches (imt_itree_mixed_batch): INSERTs and READs in one ordered list (imt_prep_logic.hpp) ----
// An operation at position p that R INSERTs precede has the events p + R (the low leaf: rewritten by an INSERT, rewritten
// with the bytes it holds by a READ) and, an INSERT, p + R + 1 (the new leaf): E = 2 n_ins + n_reads events whose ids keep
// the order of the operations.  erow[e] says whose rows event e's proof elements and root are.
constexpr int ERR_OP = 512;                  // an op byte above the greatest the call takes (max_op below)
constexpr int ERR_ABSENT = 2048;             // a MEMBER whose value is not there as of its place (OP_ABSENT, imt_prep_logic.hpp)
constexpr uint32_t ROW_LOW = 0, ROW_NEW = 1, ROW_READ = 2;      // erow[e] = (row << 2) | one of these
struct MixedWs {              // scratch of one mixed batch of n operations, beside the Workspace
    uint32_t* flag = nullptr;      // [n]   1 = INSERT
    uint32_t* rank = nullptr;      // [n]   INSERTs before the operation
    uint32_t* ipos = nullptr;      // [n]   position of the r-th INSERT
    uint32_t* word = nullptr;      // [2]   number of INSERTs, smallest offending position (0xffffffff: none)
    uint32_t* erow = nullptr;      // [2n]  indexed by event
};
struct ReadOut {              // device pointers, any may be NULL: row q belongs to the q-th operation that is no INSERT
    uint64_t* low_index;
    uint8_t* is_largest;
    uint8_t* low_leaf;             // [..][3][32] canonical
};
// 1. ranks and the number of INSERTs (mx.word[0]); ERR_OP into ws.err for a byte above max_op -- 1 (READ), or 2 (MEMBER)
// for a call that takes presence reads (IMT_MEMBER_OPS).  op: [n] device.
hipError_t mixed_ranks(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* op, uint32_t n, uint8_t max_op);
// 2. behind it, n_ins read back and M + n_ins within the capacity: the INSERT values into rows [M, M + n_ins) of d_val,
// every check of the values (ERR_* into ws.err, the smallest offending position into mx.word[1]) and the neighbours of
// every operation (ws.low / ws.succ: INSERTs by rank, then READs and MEMBERs by rank among the two -- a MEMBER's `low` is the
// leaf that holds its value, ERR_ABSENT if none does).  op: the bytes mixed_ranks read.  Writes nothing else of the tree,
// no output.
hipError_t mixed_check(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* vals, const uint8_t* op, uint8_t* d_val,
                       const uint32_t* sorted_old, uint32_t M, uint32_t n, uint32_t n_ins);
// 2'. the same for a list replayed against a view (imt_itree_view_mixed_witness): sorted_view[S] is the view's index, and
// the INSERT of rank r must be the value row S + r of d_val holds (S + n_ins <= the tree's size: the caller has checked).
// Writes NO row of d_val: the value is compared instead, ERR_MISMATCH into ws.err and the position into mx.word[1] like
// every other offender (replay_op_class, imt_prep_logic.hpp); the remaining checks run over the stored rows.
constexpr int ERR_MISMATCH = 1024;
hipError_t mixed_check_view(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* vals, const uint8_t* op,
                            const uint8_t* d_val, const uint32_t* sorted_view, uint32_t S, uint32_t n, uint32_t n_ins);
// 3. behind it, the batch accepted: what run() leaves -- preimages pre[E][96] by event, the level-0 tables [E],
// sorted_new[M + n_ins] (untouched if n_ins == 0), the hash-free outputs of both kinds -- and mx.erow.
hipError_t mixed_events(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* d_val, const uint32_t* sorted_old,
                        uint32_t* sorted_new, uint32_t M, uint32_t n, uint32_t n_ins, uint64_t base, uint8_t* pre,
                        uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re, uint64_t* o_low_index,
                        uint8_t* o_is_largest, uint8_t* o_low_leaf, uint8_t* o_new_leaf, const ReadOut& rd);
// 3'. instead of 3, for a block that is applied without witnesses (imt_itree_apply_mixed), n_ins > 0: the events of the
// INSERTs alone -- byte for byte the preimages pre[2 n_ins][96], level-0 tables [2 n_ins] and sorted_new[M + n_ins] that
// run() leaves for an insertion-only batch of the INSERT values in their order, which is what apply_lists reads.  A READ
// has no event; no output of either kind is written.
hipError_t mixed_insert_events(hipStream_t s, Workspace& ws, const uint8_t* d_val, const uint32_t* sorted_old, uint32_t* sorted_new,
                               uint32_t M, uint32_t n_ins, uint64_t base, uint8_t* pre, uint32_t* node, uint32_t* time,
                               uint32_t* rs, uint32_t* re);

// ---- bulk insertion (imt_itree_insert_bulk): the batch in descending value order, one event per value ----
struct BulkOut {              // device pointers, any may be NULL; rows k in processing order except new_leaf (caller's order)
    uint64_t* order;
    uint64_t* low_index;
    uint8_t* is_largest;
    uint8_t* low_leaf;             // [n][3][32] canonical
    uint8_t* new_leaf;             // [n][3][32] canonical
};
// 1. the values into rows [M, M + n) of d_val, the batch sorted (ws.bsorted), its gaps (ws.gap) and every check of the
// values into ws.err, by the kernels run() checks an insertion batch with.  Writes nothing else of the tree, no output.
// vals == NULL, as for run(): the values are rows [M, M + n) of d_val already (imt_itree_view_bulk_witness) -- no row of
// d_val is written, and stored values leave the error word as it is.
hipError_t bulk_check(hipStream_t s, Workspace& ws, const uint8_t* vals, uint8_t* d_val, const uint32_t* sorted_old, uint32_t M,
                      uint32_t n);
// 2. behind it, the batch accepted (bulk_row, imt_prep_logic.hpp): event k = row k's rewrite of its low leaf -- preimages
// pre[0 .. n), the level-0 tables [n], erow[k] = (k << 2) | ROW_LOW --, the new leaves' final preimages pre[n + i] in the
// caller's order, sorted_new[M + n] and the hash-free outputs.  pre: [2n][96].
hipError_t bulk_events(hipStream_t s, Workspace& ws, const uint8_t* d_val, const uint32_t* sorted_old, uint32_t* sorted_new,
                       uint32_t M, uint32_t n, uint8_t* pre, uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re,
                       uint32_t* erow, const BulkOut& o);
// 3. the level-0 table apply_lists reads for the append of leaves M .. M + n - 1 (runs of one, preimage row n + i)
hipError_t append_table(hipStream_t s, uint32_t M, uint32_t n, uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re);

// ---- witness-free insertion (imt_itree_apply_batch): the touched nodes of every level (imt_apply.hpp) ----
// From the level-0 tables run() left ([total] each): lists.node rows 0 .. l0-1, lists.src and lists.count[0 .. depth].
// pos = [l0][lists.stride] scratch for the scans; tmp as in the workspace (temp_bytes_needed covers it).
// the temporary storage apply_lists needs for `total` events, for a caller without a Workspace (a view's build)
size_t apply_lists_tmp_bytes(size_t total);
hipError_t apply_lists(hipStream_t s, void* tmp, size_t tmp_bytes, const uint32_t* node, const uint32_t* time,
                       const uint32_t* re, uint32_t total, unsigned l0, unsigned depth, uint32_t* pos,
                       const apply::Lists& lists);

// ---- going back (imt_itree_rewind): the index, the relinked leaves and the emptied nodes (imt_rewind.hpp) ----
// ws: rewind_ws_bytes(M, rows) bytes of device memory, 256-byte aligned, the same block for both calls (rows: the most
// table rows rewind_table will be asked for; 1 if only rewind_compact runs).
size_t rewind_ws_bytes(size_t M, size_t rows);
// sorted_new[0 .. s) = the entries < s of sorted_old[0 .. M) in their order (1 <= s < M); *n_relinked = a device word
// inside ws that holds the number R of relinked leaves when the stream gets there.  Writes nothing but ws and sorted_new.
hipError_t rewind_compact(hipStream_t st, void* ws, size_t ws_bytes, const uint32_t* sorted_old, uint32_t* sorted_new,
                          uint32_t M, uint32_t s, const uint32_t** n_relinked);
// Behind rewind_compact, rows = R + 1: the preimages pre[rows][96] of the relinked leaves and of the empty slot s, and
// the level-0 table apply_lists reads -- node (positions ascending), time (the preimage row of each), rs / re (runs of
// one).  key / row: [rows] scratch for the unsorted table.  Writes nothing of the tree.
hipError_t rewind_table(hipStream_t st, void* ws, size_t ws_bytes, const uint8_t* d_val, const uint32_t* sorted_old,
                        const uint32_t* sorted_new, uint32_t M, uint32_t s, uint64_t base, uint32_t rows, uint32_t* key,
                        uint32_t* row, uint8_t* pre, uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re);
// stored nodes [ceil(s / 2^l), ceil(M / 2^l)) of every level l < l0 (2^l0 >= M) = zero[l], one launch; nodes / off / len:
// the tree's node array and its per-level offsets and lengths (device), zero: [l0][32] in the stored format
void rewind_refill(hipStream_t st, uint8_t* nodes, const uint64_t* off, const uint64_t* len, const uint8_t* zero, uint64_t s,
                   uint64_t M, unsigned l0);

// ---- filtered insertion (imt_itree_insert_filtered): which values of a batch are inserted ----
struct FilterWs {             // per plan set, sized for `cap_n` values
    size_t cap_n = 0;
    uint32_t* idx = nullptr;       // [n]   input positions
    uint32_t* ord = nullptr;       // [n]   input positions in batch order (value, then position)
    uint8_t* st = nullptr;         // [n]   class, then status (input order)
    uint32_t* aux = nullptr;       // [n]   stored leaf (PRESENT) / first occurrence (REPEATED)
    uint32_t* flag = nullptr;      // [n]   1 = accepted
    uint32_t* rank = nullptr;      // [n]   exclusive scan of flag
    uint32_t* count = nullptr;     // [2]   accepted values; mixed_filter: accepted INSERTs, accepted READs
    uint8_t* acc = nullptr;        // [n][32] accepted values in input order (canonical)
    uint8_t* aop = nullptr;        // [n]   mixed_filter: op bytes of the accepted operations, beside acc
    uint32_t* apos = nullptr;      // [n]   mixed_filter: input position of the k-th accepted operation
    uint8_t* status = nullptr;     // [n]   staging of the status for host-pointer callers
    uint64_t* leaf = nullptr;      // [n]   ... and of the leaf indices
    void* tmp = nullptr;           // rocPRIM temporary storage
    size_t tmp_bytes = 0;
};
size_t filter_temp_bytes(size_t n);

// Classifies vals [n][32] (canonical, device) against the stored index (d_val, sorted[M]; imt_filter_logic.hpp):
// status[i] / leaf[i] (leaf may be NULL; global with `base`), the accepted values compacted into ws.acc in input order,
// their number into *ws.count.  ERR_NONCANONICAL is OR-ed into *err.  Writes nothing but ws, status, leaf and err.
hipError_t filter(hipStream_t s, FilterWs& ws, const uint8_t* vals, uint32_t n, const uint8_t* d_val,
                  const uint32_t* sorted, uint32_t M, uint64_t base, uint32_t part_mod, uint32_t part_res,
                  uint8_t* status, uint64_t* leaf, int* err);

// ---- filtered mixed batches (imt_itree_mixed_filtered): which operations of a block are carried out ----
// Classifies the operations (vals [n][32] canonical, op [n], both device) against the stored index of a tree that is
// neither placed nor partitioned (mixed_filter_rank, imt_filter_logic.hpp): status[i]; leaf[i] (may be NULL) for every
// operation but an accepted READ; the accepted operations compacted in input order -- values into ws.acc, op bytes into
// ws.aop, positions into ws.apos -- and their numbers into ws.count[0] (INSERTs) and ws.count[1] (READs and MEMBERs).
// max_op as in mixed_ranks; which operations are accepted: mixed_carried, imt_filter_logic.hpp.
// ERR_NONCANONICAL / ERR_OP are OR-ed into *err.  Writes nothing but ws, status, leaf and err.  ws.flag / rank / idx / ord /
// aux are scratch: MixedWs may be laid over them afterwards, ws.acc / aop / apos stay.
hipError_t mixed_filter(hipStream_t s, FilterWs& ws, const uint8_t* vals, const uint8_t* op, uint32_t n, uint8_t max_op,
                        const uint8_t* d_val, const uint32_t* sorted, uint32_t M, uint64_t base, uint8_t* status, uint64_t* leaf,
                        int* err);
// Behind mixed_ranks + mixed_check of (ws.acc, ws.aop, n_acc): leaf[ws.apos[k]] = base + the low leaf of the k-th accepted
// operation, for the READs among them.
hipError_t mixed_filter_reads(hipStream_t s, const FilterWs& ws, const Workspace& prep_ws, const MixedWs& mx, uint32_t n_acc,
                              uint32_t n_ins, uint64_t base, uint64_t* leaf);

// imt_itree_lookup_batch: status and leaf index (may be NULL) of every candidate (lookup_one, imt_filter_logic.hpp)
void lookup(hipStream_t s, const uint8_t* vals, const uint8_t* d_val, const uint32_t* sorted, uint32_t M, uint32_t n,
            uint64_t base, uint32_t part_mod, uint32_t part_res, uint8_t* status, uint64_t* leaf, int* err);

// non-membership witness: low leaf index, its preimage {val, next_val, next_idx} (canonical) and the
// is_largest flag of every candidate; any output may be NULL.  part_mod > 1: candidates with v % part_mod != part_res
// belong to another subtree's list (ERR_FOREIGN)
void nm_witness(hipStream_t s, const uint8_t* vals, const uint8_t* d_val, const uint32_t* sorted, uint32_t M, uint32_t n,
                uint64_t base, uint32_t part_mod, uint32_t part_res, uint64_t* low_index, uint8_t* low_leaf,
                uint8_t* is_largest, int* err);

// predecessor search only (imt_itree_find_low_batch): low[i] = leaf index of the greatest value < vals[i]
void find_low(hipStream_t s, const uint8_t* vals, const uint8_t* d_val, const uint32_t* sorted, uint32_t M, uint32_t n,
              uint64_t base, uint32_t part_mod, uint32_t part_res, uint64_t* low_index, int* err);

// ---- snapshot (imt_itree_load, imt_itree_get_leaves): the tree's list checked and read on the device ----
// load_check: pre = [n][3][32] canonical leaf preimages in index order.  Orders the leaves by val (radix sort on the top
// 64 bits; full_sort: merge sort with the 256-bit comparator -- the caller's second attempt after LOAD_TIE) and checks
// every rank (load_check_rank, imt_prep_logic.hpp); error bits are OR-ed into *err, the smallest leaf index with a broken
// link into **bad (0xffffffff if none).  *sorted = the leaf indices in value order, inside `ws` (load_ws_bytes(n) bytes of
// device memory).  Writes nothing but ws / err.
size_t load_ws_bytes(size_t n);
hipError_t load_check(hipStream_t s, const uint8_t* pre, uint32_t n, uint64_t base, uint32_t part_mod, uint32_t part_res,
                      void* ws, size_t ws_bytes, bool full_sort, int* err, uint32_t** bad, const uint32_t** sorted);
// d_val[i] = pre[i].val
void load_commit(hipStream_t s, const uint8_t* pre, uint32_t n, uint8_t* d_val);
// out[i] = canonical preimage of leaf index[i] (index == NULL: first + i), all-zero for an empty slot below `cap`;
// ERR_RANGE for an index outside [base, base + cap)
void leaves(hipStream_t s, const uint64_t* index, uint64_t first, uint32_t n, const uint8_t* d_val, const uint32_t* sorted,
            uint32_t M, uint64_t cap, uint64_t base, uint8_t* out, int* err);


// ---- value log (imt_itree_load_values, imt_itree_get_values): a tree from its values in leaf order ----
// load_values_check: vals = [n][32] canonical, position q = the value of leaf q + 1 (the sentinel is not passed).  Orders
// the positions by value, equal values by position (radix sort on the top 64 bits; full_sort: merge sort with
// lv_pos_less -- the caller's second attempt after LOAD_TIE) and judges every rank (load_values_rank, imt_prep_logic.hpp):
// error bits are OR-ed into *err, the smallest offending position into *bad (atomicMin: the caller sets it to 0xffffffff).  *order = the positions
// in that order, inside `ws` (load_values_ws_bytes(n) bytes of device memory).  Writes nothing but ws / err.
size_t load_values_ws_bytes(size_t n);
hipError_t load_values_check(hipStream_t s, const uint8_t* vals, uint32_t n, uint32_t part_mod, uint32_t part_res, void* ws,
                             size_t ws_bytes, bool full_sort, int* err, uint32_t* bad, const uint32_t** order);
// raw = [n][32] in ANY format, before it is converted: every format refuses the encodings >= p.  ERR_NONCANONICAL into
// *err and the smallest such position into *bad, which the caller has set (atomicMin).
void first_noncanonical(hipStream_t s, const uint8_t* raw, uint32_t n, int* err, uint32_t* bad);
// d_val rows [0, n] = {0, vals}; sorted[0 .. n] = {0, order + 1}: the index of the tree that holds exactly these values
void load_values_commit(hipStream_t s, const uint8_t* vals, const uint32_t* order, uint32_t n, uint8_t* d_val, uint32_t* sorted);

}  // namespace prep
}  // namespace imt
