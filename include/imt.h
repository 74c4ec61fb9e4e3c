/*
 * imt.h -- C ABI of libimt_hip.so: the MI355X (gfx950) indexed-Merkle-tree hot path.
 *
 * Drop-in boundary for the one data-parallel path of
 * aerius-labs/indexed-merkle-tree-halo2 (reference @ /root/reference): the Poseidon
 * (T=3, RATE=2, R_F=8, R_P=57 over bn256::Fr) hashes and the depth-d Merkle-path
 * recomputes behind
 *     src/utils.rs                  IndexedMerkleTree::{new,get_root,get_proof,verify_proof}
 *     src/indexed_merkle_tree.rs    verify_non_inclusion (:127), insert_leaf (:231),
 *                                   compute_merkle_root (:78), and the test module's
 *                                   update_idx_leaf / hash_nullifier_pre_images (:632-671)
 * Each entry point names the reference interface it replaces.  INTEGRATION.md shows the
 * Rust `extern "C"` binding a maintainer would add.
 *
 * Conventions
 *  - every function returns IMT_OK (0) or a negative IMT_ERR_* code; nothing throws or
 *    aborts across the ABI.  imt_last_error(ctx) gives a message for the last failure.
 *  - a field element is 32 bytes.  IMT_FMT_CANONICAL: little-endian integer < p
 *    (halo2curves Fr::to_repr()).  IMT_FMT_MONT256: the in-memory [u64;4] of a
 *    halo2curves bn256::Fr (Montgomery, R = 2^256), for zero-copy from Rust.
 *    IMT_FMT_DEVICE: the library's own resident format (Montgomery R = 2^261, reduced,
 *    packed 8 x u32); only meaningful for buffers produced by this library.
 *  - buffers are caller-allocated.  By default pointers are HOST pointers and the call
 *    is synchronous.  With IMT_DEVICE_PTRS all data pointers are device pointers on the
 *    context's device, the work is enqueued on the context's stream and the call returns
 *    without synchronising; input errors are then reported by imt_ctx_sync().
 *  - sibling arrays are LEVEL-MAJOR by default: sib[level][item] (coalesced on the
 *    device).  IMT_SIB_ITEM_MAJOR selects sib[item][level], the order of the reference's
 *    per-proof Vec<F> (src/utils.rs:63-85).
 *  - an imt_ctx belongs to one host thread at a time (the reference's objects are
 *    single-owner through &mut borrows: src/utils.rs:6-10).
 *  - there is NO CPU fallback: without a usable HIP device imt_ctx_create fails with
 *    IMT_ERR_NO_DEVICE.
 */
#ifndef IMT_H
#define IMT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMT_OK 0
#define IMT_ERR_NO_LEAVES (-1)    /* "Cannot create Merkle Tree with no leaves"  src/utils.rs:24-26 */
#define IMT_ERR_ODD_LEAVES (-2)   /* "Leaves must be even"                       src/utils.rs:34-36 */
#define IMT_ERR_NOT_POW2 (-3)     /* the index panic at src/utils.rs:45 for an even non-power-of-two */
#define IMT_ERR_RANGE (-4)        /* an index / depth / capacity out of range (reference: slice panic) */
#define IMT_ERR_NONCANONICAL (-5) /* a field element >= p (Fr::from_repr would return None) */
#define IMT_ERR_ALLOC (-6)
#define IMT_ERR_NO_DEVICE (-7)    /* no HIP device / runtime: this library has no CPU path */
#define IMT_ERR_HIP (-8)          /* a HIP call failed; see imt_last_error */
#define IMT_ERR_ARG (-9)          /* NULL pointer or inconsistent arguments */
#define IMT_ERR_VALUE (-10)       /* value 0 or already present: the reference's circuit panics at
                                     src/indexed_merkle_tree.rs:190 for such an insertion */
#define IMT_ERR_FULL (-11)        /* indexed tree capacity exhausted */
#define IMT_ERR_INTERNAL (-12)
#define IMT_ERR_TIMEOUT (-13)     /* a host-side wait inside imt_sliced_* ran into the world's watchdog (a peer died or
                                     hangs); the world's state has been written to stderr, see IMT_SLICED_OPT_WATCHDOG_MS.
                                     AFTER IT: something of the world may still run on the device and may never end (a
                                     collective whose peer is gone has no time limit of its own).  imt_sliced_destroy and
                                     imt_transport_destroy then return without waiting for the device -- the world's device
                                     buffers, streams and communicators are LEFT ALLOCATED -- but imt_itree_destroy /
                                     imt_ctx_destroy / hipFree would wait.  The process should report and EXIT non-zero
                                     (without those calls) and recovery (reload from a checkpoint) should happen in a
                                     freshly started process -- never by exec'ing over one that has touched the GPU. */

/* flags */
#define IMT_FMT_CANONICAL 0u
#define IMT_FMT_MONT256 1u
#define IMT_FMT_DEVICE 2u
#define IMT_FMT_MASK 3u
#define IMT_DEVICE_PTRS 0x10u
#define IMT_SIB_ITEM_MAJOR 0x20u
#define IMT_ROOT_PER_ITEM 0x40u   /* root argument is root[n][32] instead of one root[32] */
#define IMT_HOST_PREP 0x100u      /* imt_itree_insert_batch: do the low-leaf search, the event preimages and the
                                     event ordering on the host instead of on the GPU (the default keeps a
                                     device-resident sorted index and the host only launches kernels).
                                     Same results either way; the two can be mixed on one tree. */
#define IMT_PIPELINE 0x80u        /* imt_itree_insert_batch with IMT_DEVICE_PTRS only: consecutive batches run on
                                     internal streams (up to four in flight) one tree level apart, so their hash
                                     kernels share the GPU.
                                     The outputs of such a batch are ordered by imt_ctx_sync() (or by the next
                                     imt_itree_root / get_proof / non-pipelined call on the tree), not by
                                     the context's stream. */

#define IMT_MEMBER_OPS 0x400u     /* the mixed-block calls: op byte IMT_OP_MEMBER is legal -- see "PRESENCE READS" at
                                     imt_itree_mixed_batch.  Without it the calls take op bytes 0 and 1 only, as ever. */
#define IMT_INPUTS_READY 0x200u   /* imt_itree_insert_batch with IMT_DEVICE_PTRS: `vals` and the hash-free output buffers
                                     (low_index, is_largest, low_leaf, new_leaf) are idle -- nothing enqueued on the
                                     context's stream still writes `vals` or reads those outputs.  Without it the
                                     batch's preparation is ordered behind the context's stream first, which costs
                                     nothing unless that stream holds long-running work. */

/* failure bits written per item by the relation checkers; each is one constraint or
 * assert of the reference (src/indexed_merkle_tree.rs) */
#define IMT_F_RANGE_PRED 0x01   /* select(is_largest, next_val==0, new<next_val) == 1   :182-191 */
#define IMT_F_LOW_IN_ROOT 0x02  /* low leaf hashes up to the given root                  :196-204 */
#define IMT_F_LOW_LT_NEW 0x04   /* low_leaf.val < new value                             :206-228 */
#define IMT_F_ZERO_SLOT 0x08    /* the zero leaf sits at the new slot of the interim root :286-294 */
#define IMT_F_NEXT_VAL 0x10     /* new_leaf.next_val == low_leaf.next_val               :296 */
#define IMT_F_NEXT_IDX 0x20     /* new_leaf.next_idx == low_leaf.next_idx               :297 */
#define IMT_F_NEW_ROOT 0x40     /* new root recomputes                                  :305-313 */
#define IMT_F_BAD_BIT 0x80      /* a flag that must be 0/1 is not (gate.assert_bit      :41,54) */

typedef struct imt_ctx imt_ctx;
typedef struct imt_tree imt_tree;     /* dense tree: IndexedMerkleTree<'a,F,T,RATE> src/utils.rs:6-10 */
typedef struct imt_itree imt_itree;   /* depth-d append-only indexed tree (sparse storage) */

/* ---- context ------------------------------------------------------------------- */
/* Builds the Poseidon tables (Poseidon::<Fr,3,2>::new(8,57), src/indexed_merkle_tree.rs:370)
 * and uploads them to `device`.  device < 0 or no GPU -> IMT_ERR_NO_DEVICE. */
int imt_ctx_create(int device, imt_ctx **out);
void imt_ctx_destroy(imt_ctx *ctx);
const char *imt_last_error(const imt_ctx *ctx);
/* Use an existing hipStream_t (e.g. PyTorch's current stream); NULL = the context's own. */
int imt_ctx_set_stream(imt_ctx *ctx, void *hip_stream);
/* Wait for the stream and report deferred input errors (IMT_ERR_NONCANONICAL, ...). */
int imt_ctx_sync(imt_ctx *ctx);
/* Page-locked host memory that the device can address (hipHostMalloc).  A pointer from here may be
 * passed wherever IMT_DEVICE_PTRS expects a device pointer: the kernels then read the values and
 * write the roots and proofs straight into the caller's memory over PCIe, asynchronously and
 * pipelined like any device-pointer call, and the data is valid on the host after imt_ctx_sync().
 * This is how a host-language caller (the Rust shim of INTEGRATION.md) gets its witnesses without a
 * staging copy: measured at the same insertion rate as HBM-resident outputs.
 * Plain host pointers (no IMT_DEVICE_PTRS) stay supported and are synchronous. */
int imt_host_alloc(imt_ctx *ctx, size_t bytes, void **out);
int imt_host_free(imt_ctx *ctx, void *ptr);
/* Tuning knobs.  IMT_OPT_COOP_MAX_EVENTS: batch-insertion launches of at most this many events (2 per insertion) use
 * the latency form of the hash kernel -- four lanes per hash, 0.55x the time per launch, 2x the lane-instructions --
 * which pays while a launch leaves most of the chip idle; likewise plain hashes (imt_hash2/3_batch), path recomputes (imt_path_root_batch,
 * imt_compute_merkle_root_batch, imt_verify_proof_batch, imt_non_membership_batch, the path inputs of the trace calls)
 * of at most a quarter as many paths and imt_insert_witness_batch of at most a sixteenth as many items.  Default 16384
 * (one wave per SIMD); 0 = never.  Results are bit-identical either way. */
#define IMT_OPT_COOP_MAX_EVENTS 1
int imt_ctx_set_option(imt_ctx *ctx, int option, uint64_t value);
/* ABI / build identification, e.g. "imt-hip gfx950 r4" */
const char *imt_version(void);
/* Per-kernel timing with HIP events recorded on the context's stream around the launches of
 * imt_itree_insert_batch (used by bench.py for the roofline line; off by default).
 * imt_profile_read synchronises the stream, adds up the finished intervals, writes
 * out[2*c] = total milliseconds and out[2*c+1] = number of launches / calls for class c
 * (IMT_PROF_*), and resets the counters. */
#define IMT_PROF_LEAVES 0      /* k_sweep, leaf launches: the 3-input leaf hashes */
#define IMT_PROF_INDEX 1       /* k_merge_level + table copies: index phase, no hashing */
#define IMT_PROF_LEVEL 2       /* k_sweep, the levels below the highest meeting point: one hash per event per level */
#define IMT_PROF_TOP 3         /* k_sweep, the levels above it (every event against the empty subtree) */
#define IMT_PROF_WRITEBACK 4   /* k_writeback */
#define IMT_PROF_HOST 5        /* host side of imt_itree_insert_batch (wall time, waits excluded) */
#define IMT_PROF_CLASSES 6
/* The classes of imt_itree_apply_batch, behind the six above: imt_profile_read writes the first IMT_PROF_CLASSES only
 * (its callers' arrays are that long), imt_profile_read_all all IMT_PROF_ALL_CLASSES; either resets every counter. */
#define IMT_PROF_APPLY_LISTS 6   /* the scans and the scatter that list every level's touched nodes: no hashing */
#define IMT_PROF_APPLY_LEAVES 7  /* k_apply_level, leaf launch: one 3-input hash per touched leaf */
#define IMT_PROF_APPLY_LEVEL 8   /* k_apply_level, the levels below l0 - 1: one hash per touched node */
#define IMT_PROF_APPLY_TOP 9     /* k_apply_top: the chain from level l0 - 1 to the root */
#define IMT_PROF_ALL_CLASSES 10
/* Measures the device's v_mad_u64_u32 issue rate (8 independent chains per lane, 8 waves per SIMD): the
 * ceiling of the VALU roofline bench.py reports.  *gmads = 10^9 lane multiply-adds per second. */
int imt_measure_mad_peak(imt_ctx *ctx, double *gmads);
int imt_profile_enable(imt_ctx *ctx, int on);
int imt_profile_read(imt_ctx *ctx, double *out /*[2*IMT_PROF_CLASSES]*/);
int imt_profile_read_all(imt_ctx *ctx, double *out /*[2*IMT_PROF_ALL_CLASSES]*/);

/* ---- a1 / a10: batched hashes -------------------------------------------------- */
/* out[i] = Poseidon::update(&[in[i][0], in[i][1]]) ; squeeze_and_reset()
 * replaces src/utils.rs:46-47,96-100 and hash_fix_len_array at indexed_merkle_tree.rs:92 */
int imt_hash2_batch(imt_ctx *ctx, const void *in /*[n][2][32]*/, void *out /*[n][32]*/, size_t n,
                    unsigned flags);
/* 3-input leaf hash [val, next_val, next_idx]: indexed_merkle_tree.rs:193-194,271-275,299-303,663-668 */
int imt_hash3_batch(imt_ctx *ctx, const void *in /*[n][3][32]*/, void *out /*[n][32]*/, size_t n,
                    unsigned flags);
/* the bare permutation on [n][3] states (test hook for the round schedule) */
int imt_permute_batch(imt_ctx *ctx, const void *in /*[n][3][32]*/, void *out /*[n][3][32]*/, size_t n,
                      unsigned flags);

/* ---- f1: the witness trace of PoseidonHasher::hash_fix_len_array ---------------- */
/* The circuit recomputes every Poseidon on the CPU while it assigns (hasher.hash_fix_len_array at
 * src/indexed_merkle_tree.rs:92, :194, :271-275, :299-303).  These calls produce, on the GPU, every NEW advice value
 * the gadget assigns for a hash -- both permutations' absorb cells, S-box intermediates x^2, x^4, x^5 + c and the
 * running sums of every MDS row -- in assignment order ("trace rows"), so a chip can assign instead of recompute.
 * Order and cell structure follow the published halo2-lib v0.4.x gadget (poseidon/hasher/state.rs over GateChip's
 * vertical gate); halo2-base is not vendored in the reference, so this order is UNPINNED BY THE REFERENCE.  What pins
 * it: the output row is the hash (reference KAT), every gate of the reconstructed column holds, and the CPU oracle
 * restates it independently (oracle/trace.c).
 *   rows: 1208 for 2 inputs, 1209 for 3 (imt_hash_trace_rows); the hash itself is row rows - 4.
 *   trace layout: [rows][n][32] (row-major, coalesced on the device) or, with IMT_TRACE_ITEM_MAJOR, [n][rows][32]
 *   (one hash's rows contiguous).  With IMT_FMT_MONT256 a row is the in-memory [u64;4] of a halo2curves Fr:
 *   Witness(unsafe { transmute(row) }) needs no arithmetic on the host. */
#define IMT_TRACE_ITEM_MAJOR IMT_SIB_ITEM_MAJOR
size_t imt_hash_trace_rows(int arity);
int imt_hash_trace_batch(imt_ctx *ctx, const void *in /*[n][arity][32]*/, int arity, size_t n,
                         void *trace /*[rows][n][32]*/, unsigned flags);
/* The traces of ALL hashes of compute_merkle_root (src/indexed_merkle_tree.rs:78-96) for n paths: the leaf hash
 * (3 inputs; only when leaf3 is given instead of leaf) followed by the `depth` path hashes bottom-up, each with the
 * (left, right) inputs dual_mux selects.  trace = the blocks one after the other, [1209][n] (if leaf3) then depth x
 * [1208][n]; item-major: [n][1209 + depth * 1208] (IMT_TRACE_ITEM_MAJOR is the same bit as IMT_SIB_ITEM_MAJOR: the siblings
 * are then read item-major too, sib[item][level] -- the reference's per-proof Vec<F> -- exactly as in
 * imt_insert_trace_batch).  root_out (optional) = the recomputed roots. */
int imt_path_trace_batch(imt_ctx *ctx, const void *leaf /*[n][32] or NULL*/, const void *leaf3 /*[n][3][32] or NULL*/,
                         const uint64_t *index /*[n]*/, const void *sib, unsigned depth, size_t n, void *trace,
                         void *root_out /*[n][32] or NULL*/, unsigned flags);
/* The traces of ALL 3 + 4 * depth hashes of insert_leaf (src/indexed_merkle_tree.rs:231-314) for n insertions, in the
 * order the circuit reaches hash_fix_len_array: low leaf + its path (:193-204), rewritten low leaf {low.val, new.val,
 * new_index} + the same path (:271-284), the zero leaf's path at the new slot (:286-294; no leaf hash, the zero-leaf
 * hash is a constant), new leaf + its path (:299-312).  Inputs as imt_insert_witness_batch (what imt_itree_insert_batch
 * returned).  trace: the four blocks one after the other, each as imt_path_trace_batch lays it out; item-major
 * (IMT_TRACE_ITEM_MAJOR, which is the same bit as IMT_SIB_ITEM_MAJOR: siblings are then item-major too):
 * [n][imt_insert_trace_rows(depth)].  5.1 MB per insertion at depth 32: size the batch to the memory at hand. */
size_t imt_insert_trace_rows(unsigned depth);
int imt_insert_trace_batch(imt_ctx *ctx, const void *low_leaf /*[n][3][32]*/, const uint64_t *low_index,
                           const void *low_sib, const void *new_leaf /*[n][3][32]*/, const uint64_t *new_index,
                           const uint64_t *new_path_index /*[n] or NULL = new_index*/, const void *new_sib,
                           unsigned depth, size_t n, void *trace, unsigned flags);
/* The advice column of ONE hash, cell by cell, in assignment order: where each cell's value comes from and where
 * the vertical gates a + b*c = d start (gate = 1 on cell a).  Static per arity; host pointers only. */
#define IMT_CELL_CONST 0     /* constants[index] */
#define IMT_CELL_INPUT 1     /* copy (Existing) of hash input `index` */
#define IMT_CELL_INIT 2      /* copy of the hasher's initial-state cell `index`: 0 = 2^64, 1 and 2 = 0 */
#define IMT_CELL_WITNESS 3   /* NEW value: trace row `index` (rows appear in increasing order) */
#define IMT_CELL_COPY 4      /* copy (Existing) of trace row `index` */
typedef struct imt_trace_cell {
    uint8_t kind;            /* IMT_CELL_* */
    uint8_t gate;            /* 1: q_enable here, the gate covers this cell and the next three */
    uint16_t region;         /* 1: first cell of one ctx.assign_region call of the gadget (a gate.add / sum / mul /
                                mul_add / inner_product): copies inside a region only refer to EARLIER regions, so a
                                chip can assign region by region with Existing(..) handles it already holds */
    uint32_t index;
} imt_trace_cell;
/* cells / constants may be NULL (sizes only).  constants[n_constants][32] in the format of `flags`. */
int imt_hash_trace_layout(imt_ctx *ctx, int arity, imt_trace_cell *cells, size_t cells_cap, size_t *n_cells,
                          void *constants, size_t const_cap, size_t *n_constants, uint32_t *out_row, unsigned flags);

/* ---- a1 / f1 for any input length: hash_fix_len_array over 1 to 16 inputs ------------------------
 * The reference hands the CALLER's PoseidonHasher to hasher.hash_fix_len_array(ctx, gate, &inp), halo2-base's sponge over
 * a slice of any length; the tree itself calls it with 2 and 3 inputs (the calls above), a circuit that embeds the chip
 * hashes other things with the same hasher (a note commitment of 4-6 fields, a nullifier derived from a commitment and
 * a key).  These calls are the same hash -- T = 3, rate 2, the same permutation -- for `len` inputs, 1 <= len <=
 * IMT_HASH_MAX_INPUTS, with the same three faces: values, witness traces, the static cell map.
 *   The state starts as [2^64, 0, 0]; every full pair of inputs is added to lanes 1, 2 and permuted; then the leftover
 *   input (len odd) and the padding 1 are added to the next free lane(s) and the state is permuted once more; the
 *   result is lane 1: floor(len / 2) + 1 permutations.  len = 2 and 3 return what imt_hash2_batch / imt_hash3_batch and
 *   imt_hash_trace_batch / imt_hash_trace_layout return, bit for bit (those calls stay as they are and stay the ones to
 *   use for 2 and 3 inputs).
 *   rows: the NEW advice values in assignment order as in f1; a permutation that absorbs k inputs has 3 + k + 600 of
 *   them: imt_hash_n_trace_rows(len) = 605 floor(len / 2) + 603 + (len odd) = 604, 1208, 1209, 1813, ... 5443 at 16;
 *   the hash itself is row rows - 4.  The cell map has 2256 floor(len / 2) + 2250 + 3 (len odd) cells; IMT_CELL_INPUT
 *   indices run to len - 1.  Order and cell structure follow the published halo2-lib v0.4.x gadget
 *   (poseidon/hasher/state.rs over GateChip's vertical gate); halo2-base is not vendored in the reference, so this
 *   order is UNPINNED BY THE REFERENCE.  What pins it: the output row is the hash (reference KAT), every gate of the
 *   reconstructed column holds, and the CPU oracle restates it independently (oracle/trace.c).
 *   Formats, IMT_DEVICE_PTRS, errors reported at imt_ctx_sync, n == 0 and IMT_ERR_NONCANONICAL for an input >= p: as
 *   imt_hash2_batch / imt_hash_trace_batch.  len outside 1..16 -> IMT_ERR_ARG (imt_hash_n_trace_rows: 0).
 *   trace layout: [rows][n][32] or, with IMT_TRACE_ITEM_MAJOR, [n][rows][32]: 32 rows(len) bytes per hash. */
#define IMT_HASH_MAX_INPUTS 16
int imt_hash_n_batch(imt_ctx *ctx, const void *in /*[n][len][32]*/, unsigned len, void *out /*[n][32]*/, size_t n,
                     unsigned flags);
size_t imt_hash_n_trace_rows(unsigned len);
int imt_hash_n_trace_batch(imt_ctx *ctx, const void *in /*[n][len][32]*/, unsigned len, size_t n,
                           void *trace /*[rows][n][32]*/, unsigned flags);
/* cells / constants may be NULL (sizes only), as imt_hash_trace_layout; host pointers only */
int imt_hash_n_trace_layout(imt_ctx *ctx, unsigned len, imt_trace_cell *cells, size_t cells_cap, size_t *n_cells,
                            void *constants, size_t const_cap, size_t *n_constants, uint32_t *out_row, unsigned flags);

/* ---- f3: the rest of insert_leaf's advice column --------------------------------------------------
 * After f1 the only advice values of insert_leaf (src/indexed_merkle_tree.rs:231-314) a chip would still compute on the
 * CPU are those outside hash_fix_len_array: the two is_less_than calls of verify_non_inclusion (:180, :226 -> :98-125:
 * range.is_less_than(.,.,128) + gate.is_equal for the high and the low 128-bit limbs, then not x4, and x3, and, or),
 * is_equal(next_val, 0) with its inverse (:143), the limb loads and their mul_add checks (:169-178, :219-224), select
 * (:182-189 -> :33-45) and, per path, load_witness(leaf) + dual_mux's four values per level (:78-96 -> :47-63).  These
 * calls produce every such NEW advice value on the GPU, in assignment order.  Cell structure: the published halo2-lib
 * v0.4.x GateChip / RangeChip (sub [W a-b, b, 1, a]; mul [0, a, b, W]; mul_add [c, a, b, W]; or [W 1-b, 1, b, 1, b, a,
 * W 1-b, W out]; is_zero [W z, a, W 1/a, 1, 0, a, W z, 0]; range.is_less_than [W 2^p+a-b, b, 1, W 2^p+a, -2^p, 1, a] +
 * the limbs of the first cell as an inner product with 2^(lookup_bits i) + is_zero(top limb)).  UNPINNED BY THE
 * REFERENCE, exactly like f1 (halo2-base is not vendored): pinned by every gate of the column holding, by the results
 * equalling the reference's boolean formula, by the CPU oracle (oracle/gadget.c) and an independent big-integer model.
 * lookup_bits: the RangeChip's (the reference's tests: 18, :436); 1 .. 28.  Formats and layouts as for the f1 calls. */
size_t imt_less_than_trace_rows(unsigned lookup_bits);      /* 4 * (ceil(128 / lookup_bits) + 1) + 27; 63 for 18 */
/* rows of is_less_than(a_q, a_r, b_q, b_r) for the 256-bit values a[i], b[i] (a_q = a >> 128, ...: what
 * imt_split128_batch returns); trace [rows][n][32] or, with IMT_TRACE_ITEM_MAJOR, [n][rows][32]; lt_out[i] (optional)
 * = a[i] < b[i] */
int imt_less_than_trace_batch(imt_ctx *ctx, const void *a /*[n][32]*/, const void *b /*[n][32]*/, size_t n,
                              unsigned lookup_bits, void *trace, uint8_t *lt_out /*[n] or NULL*/, unsigned flags);
/* the column of one is_less_than, cell by cell, like imt_hash_trace_layout: IMT_CELL_INPUT index 0..3 = a_q, a_r, b_q,
 * b_r; *out_row = the row holding the result */
int imt_less_than_trace_layout(imt_ctx *ctx, unsigned lookup_bits, imt_trace_cell *cells, size_t cells_cap, size_t *n_cells,
                               void *constants, size_t const_cap, size_t *n_constants, uint32_t *out_row, unsigned flags);
/* Which of those rows the RangeChip ALSO constrains through its lookup table: range.is_less_than range-checks each
 * shifted difference by decomposing it into lookup_bits-wide limbs and adding every limb cell to the lookup
 * (add_cell_to_lookup); these are the 2 (ceil(128 / lookup_bits) + 1) limb rows, in column order.  A chip that assigns
 * the rows itself registers exactly these cells.  rows may be NULL (count only).  Arithmetic on sizes: no context. */
int imt_less_than_lookup_rows(unsigned lookup_bits, uint32_t *rows, size_t cap, size_t *n_rows);
/* ALL rows of insert_leaf outside its hashes ("glue rows"), in assignment order: is_equal(next_val, 0) [4 rows], the
 * limbs nl_q nl_r ll_q ll_r [4], their two mul_add [2], is_less_than(new, low.next_val) [K], select [3], then for the low
 * leaf's path load_witness [1] + dual_mux a-b, b-a, left, right per level [4 depth], the limbs of low.val + mul_add
 * [3], is_less_than(low.val, new) [K], and the same 1 + 4 depth rows for the rewritten low leaf's, the zero leaf's and
 * the new leaf's path: 20 + 2 K + 16 depth rows (658 at depth 32, lookup_bits 18).  Inputs as imt_insert_trace_batch
 * (what imt_itree_insert_batch returned) plus is_largest; depth >= 1.  Together with imt_insert_trace_batch this is
 * every new advice value of the call; imt_insert_column_segments tells how the two traces interleave. */
size_t imt_insert_gadget_rows(unsigned depth, unsigned lookup_bits);
/* the glue rows that are also lookup cells (imt_less_than_lookup_rows for both comparisons of the call, as glue-row
 * numbers): 4 (ceil(128 / lookup_bits) + 1) rows */
int imt_insert_gadget_lookup_rows(unsigned depth, unsigned lookup_bits, uint32_t *rows, size_t cap, size_t *n_rows);
int imt_insert_gadget_trace_batch(imt_ctx *ctx, const void *low_leaf /*[n][3][32]*/, const uint64_t *low_index,
                                  const void *low_sib, const void *new_leaf /*[n][3][32]*/, const uint64_t *new_index,
                                  const uint64_t *new_path_index /*[n] or NULL = new_index*/, const void *new_sib,
                                  const uint8_t *is_largest /*[n]*/, unsigned depth, unsigned lookup_bits, size_t n,
                                  void *trace, unsigned flags);
/* The same for ONE verify_non_inclusion call on its own (src/indexed_merkle_tree.rs:127-229 -- BASELINE config 3's
 * gadget): is_equal [4], limbs [4], mul_add [2], is_less_than(new, low.next_val) [K], select [3], the low leaf's path
 * [1 + 4 depth], the limbs of low.val + mul_add [3], is_less_than(low.val, new) [K] = 17 + 2 K + 4 depth rows per item
 * (the first rows of the insert_leaf call above, which begins with this gadget).  Inputs: what
 * imt_itree_non_membership_witness returned + the candidate values.  Its lookup cells: imt_insert_gadget_lookup_rows
 * (same row numbers).  Its hash blocks: imt_path_trace_batch(leaf3 = low_leaf, low_index, low_sib). */
size_t imt_non_inclusion_gadget_rows(unsigned depth, unsigned lookup_bits);
int imt_non_inclusion_gadget_trace_batch(imt_ctx *ctx, const void *low_leaf /*[n][3][32]*/, const uint64_t *low_index,
                                         const void *low_sib, const void *new_val /*[n][32]*/,
                                         const uint8_t *is_largest /*[n]*/, unsigned depth, unsigned lookup_bits, size_t n,
                                         void *trace, unsigned flags);
#define IMT_SEG_GLUE 0      /* n_rows rows of imt_insert_gadget_trace_batch starting at first_row */
#define IMT_SEG_HASH 1      /* one hash_fix_len_array call of `arity` inputs: rows [first_row, + n_rows) of imt_insert_trace_batch */
typedef struct imt_column_segment {
    uint32_t kind, arity;
    uint64_t first_row, n_rows;
} imt_column_segment;
/* the advice column of insert_leaf as alternating stretches of the two traces (3 + 4 depth hash segments); segs may be
 * NULL (count only) */
int imt_insert_column_segments(unsigned depth, unsigned lookup_bits, imt_column_segment *segs, size_t cap, size_t *n_segs);
/* ... and of verify_non_inclusion alone: 3 + 2 depth segments, 1 + depth of them hashes (rows of imt_path_trace_batch) */
int imt_non_inclusion_column_segments(unsigned depth, unsigned lookup_bits, imt_column_segment *segs, size_t cap,
                                      size_t *n_segs);

/* ---- a2 / a3 / a4: dense native tree ------------------------------------------- */
/* IndexedMerkleTree::new (src/utils.rs:20-57): level-by-level build on the device.
 * n_leaves == 0 -> IMT_ERR_NO_LEAVES; 1 -> root = leaf; odd -> IMT_ERR_ODD_LEAVES;
 * even but not a power of two -> IMT_ERR_NOT_POW2.  A leaf >= p -> IMT_ERR_NONCANONICAL and *out = NULL.
 * The call is synchronous with IMT_DEVICE_PTRS as well (the flag only says where `leaves` lies), so every
 * error is reported here and not by imt_ctx_sync().  The nodes are stored in the library's own format
 * whatever the flags' format: a tree built from one format reads back the same in any other. */
int imt_tree_new(imt_ctx *ctx, const void *leaves /*[n][32]*/, size_t n_leaves, unsigned flags,
                 imt_tree **out);
void imt_tree_free(imt_tree *t);
size_t imt_tree_num_levels(const imt_tree *t);           /* tree.len() */
int imt_tree_get_root(imt_tree *t, void *root /*[32]*/, unsigned flags);          /* utils.rs:59-61 */
/* get_proof (src/utils.rs:63-85): siblings and helpers (helper = 1 iff the node is a left
 * child, :79) for one index; helper elements are written as field elements like the reference
 * (1 and 0 in the flags' format).  Host pointers only: IMT_DEVICE_PTRS -> IMT_ERR_ARG.
 * index >= n_leaves -> IMT_ERR_RANGE, nothing written. */
int imt_tree_get_proof(imt_tree *t, size_t index, void *proof /*[levels-1][32]*/,
                       void *helper /*[levels-1][32] or NULL*/, unsigned flags);
/* The siblings of n indices (repeats allowed; n == 0 or a one-leaf tree: nothing written).  With host pointers
 * an index >= n_leaves anywhere in the batch -> IMT_ERR_RANGE before anything is enqueued or written.  With
 * IMT_DEVICE_PTRS the host cannot see the indices: such an item gets, at every level, the hash of the empty
 * subtree of that height (imt_zero_hashes) as its sibling, no error is reported and nothing outside the tree
 * is read -- range-check device-resident indices before relying on the proofs. */
int imt_tree_get_proof_batch(imt_tree *t, const uint64_t *index /*[n]*/, size_t n,
                             void *proof /*sib layout per flags*/, unsigned flags);
/* copy one level out (tree[level]); n_out receives its length */
int imt_tree_get_level(imt_tree *t, size_t level, void *out, size_t *n_out, unsigned flags);
/* one-shot: build and return root (+ all levels concatenated bottom-up if levels != NULL); root may be NULL
 * too.  Synchronous in both pointer modes, like imt_tree_new. */
int imt_tree_build(imt_ctx *ctx, const void *leaves, size_t n_leaves, void *levels /*[2n-1][32] or NULL*/,
                   void *root /*[32]*/, unsigned flags);

/* ---- a5 / a7 / a8 / a9: batched path recompute --------------------------------- */
/* WHEN A HOST CORE IS FASTER.  One call costs about 7 ms whatever it carries (a depth-32 path is 66 dependent
 * permutations; small calls use the latency form): one depth-32 verify_proof 7.0 ms here against 1.2 ms
 * on one host core, one insert_leaf witness check 8.5 against 2.6 ms (profiles/r05_latency_vs_cpu.txt).  The reference's
 * own call pattern -- one proof, one insertion per call (src/utils.rs:87, src/indexed_merkle_tree.rs:231) -- is therefore a
 * CPU job; these calls (and imt_non_membership_batch, imt_insert_witness_batch, imt_*_trace_batch below) win from about
 * 4 - 8 items per call and reach their throughput from a few thousand.
 *
 * root_out[i] = fold of hash2 over depth siblings, order from the parity of index>>level
 * (verify_proof, src/utils.rs:87-107; compute_merkle_root, indexed_merkle_tree.rs:78-96). */
int imt_path_root_batch(imt_ctx *ctx, const void *leaf /*[n][32]*/, const uint64_t *index /*[n]*/,
                        const void *sib, unsigned depth, size_t n, void *root_out /*[n][32]*/,
                        unsigned flags);
/* same with the circuit's helper bits: bit l of helper_mask[i] = proof_helper[l]
 * (1 = current node is the left input of the hash, dual_mux :47-63) */
int imt_compute_merkle_root_batch(imt_ctx *ctx, const void *leaf, const uint64_t *helper_mask,
                                  const void *sib, unsigned depth, size_t n, void *root_out,
                                  unsigned flags);
/* ok_out[i] = 1 iff the recomputed root equals root (verify_proof's bool, utils.rs:106) */
int imt_verify_proof_batch(imt_ctx *ctx, const void *leaf, const uint64_t *index, const void *root,
                           const void *sib, unsigned depth, size_t n, uint8_t *ok_out /*[n]*/,
                           unsigned flags);
/* Root of a depth-`depth` tree before and after n leaves are written at slots start .. start+n-1, given the proof of
 * slot `start` while it and everything right of it is empty.  Right-hand siblings (bit l of start == 0) are NOT read:
 * Z[l] is used, so a forged one cannot pass.  leaf_hash [n][32], or leaf3 [n][3][32] hashed first (exactly one non-NULL).
 * root_before = path of Z[0] at `start`.  start + n > 2^depth -> IMT_ERR_RANGE.
 * This is what a circuit computes for an append: every node of the range (start >> l) .. ((start+n-1) >> l) hashed once,
 * level by level, until one node is left, then that node's path -- n + depth hashes or so instead of n * depth.  It
 * checks the append of imt_itree_insert_bulk (sib = append_sib, start = the size before, leaf3 = new_leaf) and serves any
 * append-only tree, a note-commitment tree for one.  n == 0: IMT_OK, nothing written.  sib / the leaves / the roots are
 * host or device memory per IMT_DEVICE_PTRS, in the flags' format. */
int imt_frontier_append_root(imt_ctx *ctx, const void *sib /*[depth][32]*/, uint64_t start, const void *leaf_hash,
                             const void *leaf3, size_t n, unsigned depth, void *root_before /*[32] or NULL*/,
                             void *root_after /*[32]*/, unsigned flags);

/* ---- a11 / a12 / a13: batched non-membership ----------------------------------- */
/* verify_non_inclusion (indexed_merkle_tree.rs:127-229) on n items: fail_out[i] is a mask of
 * IMT_F_* (0 = every constraint holds); root_out (optional) is the recomputed root. */
int imt_non_membership_batch(imt_ctx *ctx, const void *root, const void *low_leaf /*[n][3][32]*/,
                             const uint64_t *low_index /*[n]*/, const void *low_sib, unsigned depth,
                             const void *new_val /*[n][32]*/, const uint8_t *is_largest /*[n]*/,
                             size_t n, uint8_t *fail_out /*[n]*/, void *root_out /*[n][32] or NULL*/,
                             unsigned flags);

/* The 128-bit limb witnesses verify_non_inclusion loads for its comparisons
 * (src/indexed_merkle_tree.rs:145-178, :206-224): q[i] = vals[i] >> 128, r[i] = vals[i] mod 2^128 as
 * integers, returned as field elements in the format of `flags` (vals[i] = q[i] * 2^128 + r[i]). */
int imt_split128_batch(imt_ctx *ctx, const void *vals /*[n][32]*/, void *q /*[n][32]*/, void *r /*[n][32]*/,
                       size_t n, unsigned flags);

/* ---- a14: batched insert_leaf witness ------------------------------------------ */
/* insert_leaf (indexed_merkle_tree.rs:231-314): recomputes the 3 leaf hashes and 4 paths per
 * item and checks every constraint.  trace_out (optional) receives, level-major
 * [7][n][32]: low_leaf_hash, root_from_low, new_low_leaf_hash, interim_root,
 * zero_slot_root, new_leaf_hash, new_root_recomputed.
 * new_index is the field element hashed into the rewritten low leaf (:265-269);
 * new_path_index positions the new slot's path (the circuit's new_leaf_proof_helper bits).
 * The reference never ties the two together; pass NULL to use new_index for both. */
int imt_insert_witness_batch(imt_ctx *ctx, const void *old_root /*[n][32]*/,
                             const void *low_leaf /*[n][3][32]*/, const uint64_t *low_index,
                             const void *low_sib, const void *new_root /*[n][32]*/,
                             const void *new_leaf /*[n][3][32]*/, const uint64_t *new_index,
                             const uint64_t *new_path_index /*[n] or NULL = new_index*/,
                             const void *new_sib, const uint8_t *is_largest, unsigned depth, size_t n,
                             uint8_t *fail_out /*[n]*/, void *trace_out /*[7][n][32] or NULL*/,
                             unsigned flags);

/* ---- a15 (+ a2 at depth 32): stateful indexed tree ----------------------------- */
/* A depth-`depth` tree whose leaf i is H(val,next_val,next_idx) of the i-th inserted value
 * (leaf 0 = the {0,0,0} sentinel, empty slot = H(0,0,0): indexed_merkle_tree.rs:373-376).
 * Only the filled prefix (up to `capacity` leaves, a power of two) is stored. */
int imt_itree_new(imt_ctx *ctx, unsigned depth, uint64_t capacity, imt_itree **out);
void imt_itree_free(imt_itree *t);
uint64_t imt_itree_size(const imt_itree *t);      /* leaves in use, sentinel included */
int imt_itree_root(imt_itree *t, void *root /*[32]*/, unsigned flags);
/* Root as it was after the batch inserted `lag` calls ago (0 = the latest batch, 1 = the one before;
 * lag <= 1).  Orders the context's stream behind THAT batch only, so with IMT_PIPELINE a root
 * exchange that lags one step does not stall the batches still in flight. */
int imt_itree_root_lagged(imt_itree *t, unsigned lag, void *root /*[32]*/, unsigned flags);

/* outputs of a batch insertion; every pointer may be NULL; host or device per flags */
typedef struct imt_insert_out {
    uint64_t *low_index;     /* [n]        low leaf of insertion i (update_idx_leaf's 2nd result) */
    void *low_leaf;          /* [n][3][32] the low leaf's preimage BEFORE insertion i */
    uint8_t *is_largest;     /* [n]        low_leaf.next_val == 0 (:737-742) */
    void *old_root;          /* [n][32]    root before insertion i */
    void *interim_root;      /* [n][32]    after the low leaf was rewritten */
    void *new_root;          /* [n][32]    after the new leaf was written */
    void *new_leaf;          /* [n][3][32] preimage written at the new slot */
    void *low_sib;           /* [depth][n][32] low-leaf proof against old_root (layout per flags) */
    void *new_sib;           /* [depth][n][32] new-slot proof against interim_root / new_root */
} imt_insert_out;
/* Every 32-byte row a device pointer refers to (values, preimages, roots, sibling rows) must be 16-byte
 * aligned: the kernels move field elements as two 16-byte words.  hipMalloc, imt_host_alloc and torch
 * allocations are; an offset into them must be a multiple of 16 bytes. */

/* n sequential insertions with the semantics of update_idx_leaf + rebuild (:632-660,
 * :715-735): insertion i finds the low leaf among everything inserted before it, rewrites
 * it, and writes the new leaf at index size+i.  All 2n path recomputes (2 + 2*depth hashes
 * per insertion) run on the device as a level sweep over time-versioned nodes.
 * vals[i] == 0, duplicates (within the batch or already present) -> IMT_ERR_VALUE, nothing
 * changes.  Exceeding capacity -> IMT_ERR_FULL.
 * HOW LONG THE CALL HOLDS THE CALLING THREAD.  IMT_ERR_VALUE must be the call's own return value with the tree
 * untouched, so the call returns when the batch's values have been checked on the GPU (the preparation: sort, low-leaf
 * search), and with IMT_PIPELINE that check is enqueued behind the hashing of the batches already in flight (at most four;
 * the back-pressure that keeps the queues short).  At 2^16 insertions per batch the thread is inside the call for 18.75 ms
 * of every 21.09 ms batch (BENCH_r05: host_call_ms_per_step), almost all of it waiting.  A host that needs its thread
 * calls from a thread of its own -- one caller at a time per tree is all the library asks.  Without IMT_DEVICE_PTRS the
 * call also copies the outputs back and returns when they are there. */
int imt_itree_insert_batch(imt_itree *t, const void *vals /*[n][32]*/, size_t n,
                           const imt_insert_out *out /*may be NULL*/, unsigned flags);
/* current siblings of leaf `index` for n indices (get_proof on the stored tree) */
int imt_itree_get_proof_batch(imt_itree *t, const uint64_t *index, size_t n, void *sib,
                              unsigned flags);
/* preimages {val, next_val, next_idx} of n leaves, all-zero for an empty slot.  index == NULL: the n leaves from the
 * tree's first one on (the whole tree: n = imt_itree_size).  Read from the device-resident index by one kernel (a leaf's
 * successor is the next value in value order); with IMT_DEVICE_PTRS `index` and `preimage` are device pointers and
 * nothing crosses PCIe.  An index outside the tree's capacity -> IMT_ERR_RANGE. */
int imt_itree_get_leaves(imt_itree *t, const uint64_t *index /*[n] or NULL*/, size_t n, void *preimage /*[n][3][32]*/,
                         unsigned flags);
/* Checkpoint / resume and bulk build.  The snapshot of a tree is its leaf preimages in index order
 * (imt_itree_get_leaves(t, NULL, size, ..)): the reference's serde leaf {val, next_val, next_idx}
 * (src/utils.rs:12-17).  imt_itree_load replaces the tree's contents with n such leaves (host memory, or device memory
 * with IMT_DEVICE_PTRS; any IMT_FMT_*).  ON THE GPU it checks that they form one sorted linked list starting at the
 * {0,..} sentinel -- leaves ordered by val (radix sort, 256-bit merge sort if top limbs tie), every leaf's next_val /
 * next_idx = its successor, the largest one's = {0, 0}, no duplicates, every element < p: IMT_ERR_VALUE /
 * IMT_ERR_NONCANONICAL otherwise, naming the first leaf with a broken link, and the tree is left as it was -- then
 * rebuilds every stored level (n leaf hashes + one pass of k_tree_level per level: about 2 hashes per leaf, the "final
 * root only" build of SURVEY.md 8d).  Host memory needed: none beyond the caller's own buffer. */
int imt_itree_load(imt_itree *t, const void *preimages /*[n][3][32]*/, uint64_t n, unsigned flags);
/* The same from the value log alone: a tree is a function of its values in leaf order.  imt_itree_load_values replaces
 * the tree's contents by what a fresh tree of the same depth, capacity, placement and value partition holds after
 * imt_itree_apply_batch(vals, n) -- every stored node, the index, the size n + 1 and every answer afterwards are the
 * same bytes.  vals: the inserted values in insertion order (leaves 1 .. n; the sentinel is not passed), host memory or
 * device memory with IMT_DEVICE_PTRS, any IMT_FMT_*.  32 bytes per leaf instead of imt_itree_load's 96, no links to
 * check, and the leaf hashes read each successor through the sorted order: the preimages are never written anywhere.
 * Refused like imt_itree_load where the values do not matter (IMT_ERR_FULL if n + 1 exceeds the capacity, IMT_ERR_ARG
 * for NULL / n == 0 / an unknown format / an open slice), and with imt_itree_apply_batch's code where they do:
 * IMT_ERR_NONCANONICAL, else IMT_ERR_VALUE for a 0, a repeated value or a foreign residue.  On those two *bad_pos (may be
 * NULL) is the smallest position of vals that is >= p, 0, foreign or equal to a value at a smaller position: where
 * inserting one by one would stop.  A refused call has written nothing of the tree.  Synchronous; afterwards as after
 * imt_itree_load (no lagged root, views rebuild on their next query). */
int imt_itree_load_values(imt_itree *t, const void *vals /*[n][32]*/, uint64_t n, uint64_t *bad_pos /*or NULL*/,
                          unsigned flags);
/* the values of leaves [first, first + n), global leaf indices as imt_itree_get_leaves counts them (leaf 0 gives 0): a
 * copy of the device index, any format, host or device memory.  IMT_ERR_RANGE unless all of them are below the size.
 * imt_itree_load_values(imt_itree_get_values(first leaf + 1, size - 1)) reproduces the tree. */
int imt_itree_get_values(imt_itree *t, uint64_t first, size_t n, void *vals /*[n][32]*/, unsigned flags);
/* low leaf (greatest val < v) for n candidate values: a binary search per value in the device-resident index
 * (k_find_low; with IMT_DEVICE_PTRS `vals` and `low_index` are device pointers); IMT_ERR_VALUE if some v is 0, present,
 * or (with a value partition set) of another subtree's residue */
int imt_itree_find_low_batch(imt_itree *t, const void *vals /*[n][32]*/, size_t n,
                             uint64_t *low_index /*[n]*/, unsigned flags);

/* Status of one value of imt_itree_insert_filtered / imt_itree_lookup_batch.  When several apply, the first in this
 * order wins: ZERO, FOREIGN, PRESENT, REPEATED, NEW (a value both stored and repeated in the batch is PRESENT at every
 * occurrence). */
#define IMT_VAL_NEW 0         /* insert_filtered: inserted; lookup: absent */
#define IMT_VAL_ZERO 1        /* 0, the sentinel (:373-376): refused */
#define IMT_VAL_PRESENT 2     /* already stored: skipped */
#define IMT_VAL_REPEATED 3    /* insert_filtered only: an earlier occurrence in the same batch was inserted; skipped */
#define IMT_VAL_FOREIGN 4     /* another subtree's residue (imt_itree_set_value_partition): skipped */
/* A sequencer's batch that may hold double spends: the reference's sequence of insert_leaf calls with the rejected
 * values skipped.  Let A be the values whose status is IMT_VAL_NEW, in input order: the call IS
 * imt_itree_insert_batch(t, A, |A|, out, flags) -- the same tree, byte for byte the same witness rows.  Row r of every
 * out array belongs to the r-th accepted value and rows [0, *n_inserted) are written; sibling arrays keep the caller's
 * dimensions (level-major [depth][n][32] with level stride n, not *n_inserted; or item-major [n][depth][32]).
 * leaf_index[i]: NEW -> the leaf it was written to; PRESENT -> the stored leaf that holds it; REPEATED -> the leaf its
 * first occurrence was written to; ZERO -> the sentinel; FOREIGN -> UINT64_MAX (global indices on a placed tree).
 * status / leaf_index are host or device memory per flags, *n_inserted is host memory; all three are complete when the
 * call returns (it waits for the classification on the GPU, as imt_itree_insert_batch waits for its value check).
 * Every flag means what it means to imt_itree_insert_batch.  Errors, the tree untouched: IMT_ERR_FULL if size +
 * *n_inserted exceeds the capacity, IMT_ERR_NONCANONICAL for a value >= p (malformed input, not a rejection), and the
 * calls imt_itree_insert_batch refuses.  Nothing accepted: IMT_OK, *n_inserted = 0, only status / leaf_index written.
 * NULL status or n_inserted -> IMT_ERR_ARG. */
int imt_itree_insert_filtered(imt_itree *t, const void *vals /*[n][32]*/, size_t n, uint8_t *status /*[n]*/,
                              uint64_t *leaf_index /*[n] or NULL*/, uint64_t *n_inserted /*host*/,
                              const imt_insert_out *out /*may be NULL*/, unsigned flags);
/* WITNESS-FREE INSERTION, for whoever keeps the tree current and proves nothing about the way there (a node following
 * the chain, a prover catching up on history, a sequencer that filters now and proves elsewhere, the non-membership
 * service).  The tree after imt_itree_insert_batch(t, vals, n, NULL, flags), and nothing else: same value checks, same
 * errors with the tree untouched, same index, same stored nodes byte for byte -- but every node the batch touches is
 * hashed ONCE, from its children's final values (imt_apply.hpp): 3 to 9 hashes per insertion where the witness sweep
 * spends 2 + 2*depth.  root_out: the root after the batch, [32] in the flags' format, host or device memory per
 * IMT_DEVICE_PTRS, may be NULL.  n == 0: IMT_OK, root_out = the current root.
 * IMT_FMT_*, IMT_DEVICE_PTRS, IMT_HOST_PREP and IMT_INPUTS_READY mean what they mean to imt_itree_insert_batch.  The call
 * runs on the context's stream behind every batch still in flight on the pipeline streams, later calls are ordered
 * behind it, and witness and apply calls may alternate freely on one tree; this call does not overlap with the one before:
 * IMT_PIPELINE -> IMT_ERR_ARG, imt_itree_apply_pipelined below is the call that does.  On a placed / partitioned tree the residue check and the global next_idx come
 * with the shared preparation; only local nodes are written. */
int imt_itree_apply_batch(imt_itree *t, const void *vals /*[n][32]*/, size_t n, void *root_out /*[32] or NULL*/,
                          unsigned flags);
/* WITNESS-FREE BATCHES THAT OVERLAP, for the follower that applies block after block and checks every block's root: the
 * tree after imt_itree_apply_batch(t, vals, n, ...) and nothing else -- same value checks, same error codes with the tree
 * untouched, same index, size and stored nodes byte for byte -- but the call returns when the batch's values have been
 * checked on the GPU, as imt_itree_insert_batch with IMT_PIPELINE does, and the hashing goes on running on one of the
 * tree's pipeline streams behind the batches before it.  An apply batch is some 34 dependent launches of one hash's
 * latency each; up to four consecutive batches now run them side by side, two launches apart (imt_apply_pipe.hpp has the
 * rule and the reason it is two), each chain to the root hashed beside the others and only its store ordered.  A fifth
 * call waits for the first (back-pressure, as for pipelined witness batches).
 * IMT_DEVICE_PTRS is required (otherwise IMT_ERR_ARG, nothing changed): vals and root_out are device-addressable memory,
 * 16-byte aligned -- a row of an imt_host_alloc buffer is fine -- and root_out ([32] in the flags' format, may be NULL)
 * is complete after imt_ctx_sync(), like the outputs of a pipelined witness batch.  Every batch delivers its own root.
 * IMT_FMT_*, IMT_INPUTS_READY and IMT_HOST_PREP mean what they mean to imt_itree_apply_batch; IMT_PIPELINE may be set and
 * means nothing more.  Placement and value partition work as there, and the refusals are that call's: a NULL tree, NULL
 * vals with n > 0, an unknown format, a misaligned row, sliced steps in flight, an open slice, an open sharded batch,
 * IMT_ERR_FULL.  n == 0: IMT_OK, root_out = the current root, ordered behind everything in flight.  A refused batch
 * (IMT_ERR_VALUE, IMT_ERR_NONCANONICAL, IMT_ERR_FULL) leaves alone the tree, the batches in flight and their roots.
 * Every other call on the tree orders itself behind pipelined apply batches exactly as behind pipelined witness batches
 * (queries, views, imt_itree_rewind, imt_itree_load*, imt_itree_root_lagged, un-pipelined batches of every kind, imt_sliced_*
 * entry), and pipelined batches of either kind may follow each other in any order.  imt_itree_apply_stats reports the last
 * apply call of either kind and waits for that call only.
 * Which call at which block size: profiles/apply_pipelined.txt, README "Witness-free insertion".
 * Blocks with READs overlap through imt_itree_apply_mixed_pipelined / imt_itree_mixed_pipelined below: the INSERT count and
 * the verdict they read back come with the waits for the value checks that every pipelined call makes anyway.
 * Not offered: pipelined forms of imt_itree_apply_filtered, imt_itree_mixed_filtered and imt_itree_apply_mixed_filtered --
 * they return a status per value or operation, complete at return, and (the mixed ones) make a third wait for the
 * classification: a call that has waited that long on the side stream has little left to overlap. */
int imt_itree_apply_pipelined(imt_itree *t, const void *vals /*[n][32]*/, size_t n, void *root_out /*[32] or NULL*/,
                              unsigned flags);
/* imt_itree_insert_filtered without witnesses: status / leaf_index / *n_inserted exactly as that call writes them, then
 * imt_itree_apply_batch of the accepted values.  Nothing accepted: IMT_OK, *n_inserted = 0, root_out = the current
 * root. */
int imt_itree_apply_filtered(imt_itree *t, const void *vals /*[n][32]*/, size_t n, uint8_t *status /*[n]*/,
                             uint64_t *leaf_index /*[n] or NULL*/, uint64_t *n_inserted /*host*/,
                             void *root_out /*[32] or NULL*/, unsigned flags);
/* What the last apply call that inserted something hashed (imt_itree_apply_batch, _apply_filtered, _apply_mixed or
 * _apply_mixed_filtered; a call that inserted nothing, a block of READs only included, hashed nothing and is not it):
 * hashes[0] = leaf hashes, hashes[l] = hash2 calls that produced level-l nodes, l = 1 .. depth -- the number of distinct
 * nodes the batch touched at every level.  Host memory; waits for that call.  IMT_ERR_ARG if there has been none. */
int imt_itree_apply_stats(imt_itree *t, uint64_t *hashes /*[depth + 1]*/);
/* BULK INSERTION: THE BATCH WITNESS ROLLUP CIRCUITS USE, one path per insertion plus one shared append.  The tree, the
 * value log and the index after this call are byte for byte those after imt_itree_insert_batch(t, vals, n, ...): value
 * v[i] becomes leaf M + i (M = imt_itree_size before the call), and no later call can tell the two apart.  The witness
 * is another one.  The values are taken in DESCENDING canonical-integer order, row k = the k-th largest, at the caller's
 * position order[k].  In that order the low leaf of every value is a leaf stored before the call (index < M), never one
 * of the batch, so row k rewrites one stored leaf -- low_leaf[k] is its preimage as of step k, which already points at
 * v[order[k-1]] when that larger value shares the low leaf; low_sib[k] proves it against root_before[k]; root_after[k]
 * is the root once it holds {low.val, v[order[k]], M + order[k]}; root_before[0] is the root before the call and
 * root_before[k+1] == root_after[k].  Between the rows the tree is deliberately no closed list: a low leaf points at a
 * slot that is still empty.  Then all new leaves are appended at once: new_leaf[i] (caller's order) is the FINAL preimage
 * of leaf M + i, what imt_itree_get_leaves returns afterwards; append_sib is the proof of the empty slot M against
 * root_after[n-1], with Z[l] (imt_zero_hashes) at every level where bit l of M is 0; root is the root after the call.
 * imt_frontier_append_root recomputes the append.  The sweep hashes n * (1 + depth) times and the append once per distinct
 * node of the range M .. M+n-1 at every level (imt_itree_apply_stats reports the latter), against n * (2 + 2 * depth).
 * This form is not in the reference: what pins it is the reference's verify_non_inclusion relation for every row and the
 * final tree being the reference's.  The witness-free twin is imt_itree_apply_batch.
 * Formats, IMT_DEVICE_PTRS, IMT_SIB_ITEM_MAJOR, alignment and refusals are those of imt_itree_insert_batch: 0, a value
 * >= p (IMT_ERR_NONCANONICAL), a stored value or a repeat -> IMT_ERR_VALUE with the tree and every output untouched;
 * IMT_ERR_FULL; n == 0 is a no-op.  IMT_PIPELINE, IMT_HOST_PREP, IMT_INPUTS_READY, a placed tree and a partitioned tree
 * -> IMT_ERR_ARG, as for imt_itree_mixed_batch.  The call runs on the context's stream behind every pipelined batch
 * still in flight, and afterwards it is a batch like any other (lagged roots, views, rewind into its middle). */
typedef struct imt_bulk_out {          /* every pointer may be NULL; host or device per flags */
    uint64_t *order;        /* [n]        caller's position of the k-th row's value (descending values) */
    uint64_t *low_index;    /* [n]        */
    void *low_leaf;         /* [n][3][32] preimage before row k's rewrite */
    uint8_t *is_largest;    /* [n]        */
    void *root_before;      /* [n][32]    */
    void *root_after;       /* [n][32]    */
    void *low_sib;          /* [depth][n][32], layout per flags as for imt_insert_out */
    void *new_leaf;         /* [n][3][32] caller's order: leaf M + i */
    void *append_sib;       /* [depth][32] */
    void *root;             /* [32]       */
} imt_bulk_out;
int imt_itree_insert_bulk(imt_itree *t, const void *vals /*[n][32]*/, size_t n,
                          const imt_bulk_out *out /*may be NULL*/, unsigned flags);
/* GOING BACK, for the same callers when the last blocks are dropped (a reorg, a failed proof, a batch the L1 did not
 * accept).  The tree as it was when it held new_size leaves (sentinel included; 1 = the empty tree): byte for byte --
 * index, leaf preimages, every stored node, root -- the tree a fresh imt_itree would be after inserting the first
 * new_size - 1 values this one received.  Nothing is needed from the caller but the size: the tree stores no preimage,
 * so the earlier one is a function of the values it still holds (imt_rewind.hpp).  With M = imt_itree_size(t) and
 * k = M - new_size: one pass over the 4-byte-per-leaf index, the stored nodes [ceil(new_size / 2^l), ceil(M / 2^l)) of
 * every level back to the empty subtree, and one hash per node of
 *     S_0 = { kept leaves whose successor in value order was removed } + { new_size },  S_(l+1) = { x >> 1 : x in S_l }
 * -- of the order of an apply batch of k values, where imt_itree_load of a snapshot hashes about 2 * new_size nodes.
 * Measured against the load of a snapshot already on the device (profiles/rewind.txt): 2.0 to 2.8 times faster for
 * k = 2^10 .. 2^16 at 2^20 leaves, 4.8 to 19 times for k = 2^10 .. 2^20 at 2^24; no measured k / M, up to 1 / 16, made the
 * load the better call.
 * new_size counts local leaves, as imt_itree_size does, on a placed tree too.  new_size == 0 or > M -> IMT_ERR_RANGE, the
 * tree untouched.  new_size == M: IMT_OK, nothing runs, root_out = the current root, hashes all zero.
 * root_out: the root afterwards, [32] in the flags' format (IMT_FMT_*), host or device memory per IMT_DEVICE_PTRS, may be
 * NULL.  hashes, if not NULL: host memory, hashes[l] = |S_l| for l < ceil(log2(M)), 1 for every level from there to depth
 * (the single chain to the root) -- what the call hashed, level by level.  imt_itree_apply_stats keeps reporting the last
 * apply call.
 * The call is rare and synchronous: it orders itself behind everything in flight on this tree (pipelined batches
 * included; the caller need not synchronise first), returns when the tree is the earlier one, and later calls of any kind
 * are ordered behind it.  IMT_PIPELINE -> IMT_ERR_ARG.  Refused with the tree untouched, like imt_itree_load: a replica of
 * a sliced world with steps in flight (imt_sliced_flush first; every replica may then be rewound to the same size), an
 * open slice, and a sharded batch between imt_itree_batch_begin and _end (IMT_ERR_ARG).
 * Placement and value partition stay as they are (the relinked leaves' next_idx is global).  Afterwards the host mirror
 * is rebuilt on demand, so an IMT_HOST_PREP batch works, and imt_itree_root_lagged behaves as after imt_itree_load: it has
 * no root to give until the next batch. */
int imt_itree_rewind(imt_itree *t, uint64_t new_size, void *root_out /*[32] or NULL*/,
                     uint64_t *hashes /*[depth + 1] host, or NULL*/, unsigned flags);
/* ANOTHER CAPACITY, for the same callers once the tree has outgrown the first guess (a batch answered IMT_ERR_FULL) or
 * should give memory back (after a deep imt_itree_rewind, after an over-generous guess).  After IMT_OK no call can tell
 * the tree from one made by imt_itree_new(ctx, depth, new_capacity, ..) with the same placement and value partition that
 * received the same values in the same order: size, root, every leaf preimage and proof at every index below
 * new_capacity (the empty slots included), get_values, lookup_batch, find_low_batch, non_membership_witness, and every
 * later batch of every kind byte for byte, prepared on the device or with IMT_HOST_PREP.
 * It costs a copy and hashes nothing: level l stores max(1, capacity >> l) nodes as a filled prefix and every node outside
 * the prefix reads as the empty subtree Z[l], so node i of level l of the new layout is the old node i where the old
 * layout has one and Z[l] where it has not (imt_resize.hpp; one launch for all levels), and of the values and the index
 * only the imt_itree_size(t) rows in use move.  A growing tree migrates one array at a time -- the nodes, the values,
 * each index buffer -- and allocates the new array before it frees the old one, so the extra memory at the peak is the
 * largest new array (the nodes, 64 bytes per leaf of new_capacity), not a second tree; a shrinking tree, whose new arrays
 * together are at most half the old ones, allocates all of them first.  IMT_ERR_ALLOC leaves the capacity as it was and
 * the tree usable (an array that has grown already stays grown).
 * new_capacity > capacity grows, imt_itree_size(t) <= new_capacity < capacity shrinks, == capacity: IMT_OK, nothing runs.
 * IMT_ERR_RANGE, the tree untouched: new_capacity not a power of two in [2, 2^31], above 2^depth, or below the size.
 * flags must be 0 (IMT_PIPELINE or any other bit: IMT_ERR_ARG).  Synchronous and ordered like imt_itree_rewind: behind
 * everything in flight on the tree, pipelined batches of every kind and the caller's stream included, and refused where
 * a rewind is refused (steps of a sliced world in flight -- after imt_sliced_flush every replica may be reserved alike --
 * an open slice, a sharded batch between _batch_begin and _end: IMT_ERR_ARG), the tree and its capacity untouched.
 * The contents do not change: a view made before the call answers afterwards without rebuilding its side table
 * (imt_itree_view_stats), and imt_itree_root_lagged keeps answering.  The batch calls do not grow the tree themselves:
 * the caller knows the size, n and the capacity, and reserves between calls. */
uint64_t imt_itree_capacity(const imt_itree *t);   /* leaves the tree can hold, sentinel included; 0 for NULL */
int imt_itree_reserve(imt_itree *t, uint64_t new_capacity, unsigned flags);
/* Where the last imt_itree_reserve that changed the capacity spent its time, in milliseconds: ms[0] the whole call (host
 * clock), ms[1] the kernel that moved the nodes (device time), ms[2] hipMalloc + hipFree (host clock).  All zero before
 * the first such call.  Host memory.  IMT_ERR_ARG for NULL. */
int imt_itree_reserve_stats(const imt_itree *t, double *ms /*[3]*/);
/* READING AT AN EARLIER SIZE, for whoever answers against a root that lags the head: the non-membership service bound to
 * the finalized root, a prover catching up on a block that has since been built upon, a node asking whether a value would
 * have been a double spend at block B.  A view is the tree as it was when it held `size` leaves (sentinel included),
 * read-only, while the tree stays where it is.  It is neither a second tree nor a rewind: the earlier tree differs from
 * the stored one only in the nodes imt_itree_rewind would hash (S_l above), which a view keeps in a side table of its own,
 * and in the nodes at or beyond the cut, which are empty subtrees; every other node is read from the tree (imt_view.hpp).
 * DEFINED BY THE SIZE ALONE.  Every query answers byte for byte what the imt_itree_* call of the same name answers on a
 * fresh tree that received the first size - 1 values this tree holds: root, status, leaf indices, preimages, sibling
 * rows, errors -- IMT_ERR_VALUE for a candidate that is 0, stored as of `size` or foreign, IMT_ERR_RANGE for an index
 * outside the capacity.  A value inserted after `size` is NEW, its low leaf among the kept leaves.  Placement, value
 * partition, global indices, IMT_FMT_*, IMT_SIB_ITEM_MAJOR and IMT_DEVICE_PTRS mean what they mean to the tree's calls.
 * A VIEW NEVER CHANGES THE TREE: no stored node, no index buffer of the tree (not the spare one a rewind uses either), no
 * plan set.  The tree's own calls answer and behave as before, whether views exist or not.
 * A VIEW FOLLOWS THE TREE.  The side table is a cache for (size, state of the tree); the tree counts every call that
 * changes its contents (an insertion of any kind that accepted something, imt_itree_load, a rewind below the current size,
 * imt_itree_batch_end, a slice), and a query that finds another count rebuilds first: on the context's stream, behind
 * everything in flight on the tree, pipelined batches included (the caller need not synchronise), and synchronously -- it
 * reads the number of relinked leaves back.  While the tree is smaller than the view a query returns IMT_ERR_RANGE; the
 * view stays valid and answers again once the tree has grown, for the prefix of whatever history the tree then has.
 * imt_itree_view_stats: *builds = rebuilds so far, hashes[l] = what the last one hashed at level l -- what
 * imt_itree_rewind(t, size) reports for the same pair of sizes; host memory, either may be NULL.
 * A view at the current size (size == imt_itree_size(t)) hashes nothing and answers as the tree does.
 * REFUSALS.  size == 0 or above the tree's size at creation: IMT_ERR_RANGE.  IMT_PIPELINE in a query's flags: IMT_ERR_ARG.
 * Creation and queries are refused like imt_itree_rewind, with IMT_ERR_ARG and everything untouched: a replica of a sliced
 * world with steps in flight, an open slice, between imt_itree_batch_begin and _end.
 * Several views of one tree may exist; each owns its memory: 4 * size bytes for the earlier index, and per rebuild 32
 * bytes per listed node (a level's row is as long as S_0) + 96 bytes per relinked leaf.  A rebuild borrows 8 bytes per
 * leaf of the tree from the context for the time of the call, as a rewind does.  Free every view before its tree.
 * A handle that is not a live view (NULL, one already freed, another kind of handle) is IMT_ERR_ARG to every call here,
 * size 0 to imt_itree_view_size and nothing to imt_itree_view_free: it is looked up before anything is read through it. */
typedef struct imt_itree_view imt_itree_view;
int imt_itree_view_create(imt_itree *t, uint64_t size, imt_itree_view **out);
void imt_itree_view_free(imt_itree_view *v); /* NULL is fine; before imt_itree_free of its tree */
uint64_t imt_itree_view_size(const imt_itree_view *v);
int imt_itree_view_root(imt_itree_view *v, void *root /*[32]*/, unsigned flags);
int imt_itree_view_lookup_batch(imt_itree_view *v, const void *vals /*[n][32]*/, size_t n, uint8_t *status /*[n]*/,
                                uint64_t *leaf_index /*[n] or NULL*/, unsigned flags);
int imt_itree_view_get_leaves(imt_itree_view *v, const uint64_t *index /*[n] or NULL*/, size_t n,
                              void *preimage /*[n][3][32]*/, unsigned flags);
/* imt_itree_get_values below the view's size: reads stored values only, so it never builds the view */
int imt_itree_view_get_values(imt_itree_view *v, uint64_t first, size_t n, void *vals /*[n][32]*/, unsigned flags);
int imt_itree_view_get_proof_batch(imt_itree_view *v, const uint64_t *index /*[n]*/, size_t n,
                                   void *sib /*[depth][n][32]*/, unsigned flags);
int imt_itree_view_non_membership_witness(imt_itree_view *v, const void *vals /*[n][32]*/, size_t n,
                                          uint64_t *low_index /*[n]*/, void *low_leaf /*[n][3][32]*/,
                                          uint8_t *is_largest /*[n]*/, void *low_sib /*[depth][n][32]*/,
                                          unsigned flags);
int imt_itree_view_stats(imt_itree_view *v, uint64_t *hashes /*[depth + 1] or NULL*/, uint64_t *builds /*or NULL*/);
/* APPLY NOW, PROVE LATER: the insert_leaf witnesses of the n insertions that followed the view's size -- the values the
 * tree holds at leaves [size, size + n), in that order, inserted into the tree as of `size`.  There is no `vals`: the tree
 * has the values, however they went in (apply, witness, filtered, sliced, loaded).
 * DEFINED BY THE SIZES ALONE.  Take a fresh tree fed the first size - 1 values and call imt_itree_insert_batch on it with
 * the next n values and the same flags: this call writes into `out` what that call would write, byte for byte -- all nine
 * fields, NULL fields skipped, placement, global indices and value partition, IMT_FMT_*, IMT_SIB_ITEM_MAJOR and
 * IMT_DEVICE_PTRS, level-major stride n, rows [depth, global_depth) of a placed tree's sibling arrays left to the caller
 * (imt_itree_lift_batch).  IMT_INPUTS_READY and IMT_HOST_PREP change nothing here: the call runs on the context's stream
 * and prepares on the GPU.
 * It is a view query otherwise: it never changes the tree (stored nodes, index buffers, plan sets, size, rows of the value
 * array), it rebuilds a stale side table first, behind everything in flight, and it is refused where the other queries
 * are.  Synchronous for host pointers; with IMT_DEVICE_PTRS it is enqueued on the context's stream.
 * size + n above the tree's current size (so any n > 0 on a view at the current size, and any n while the tree is
 * smaller than the view): IMT_ERR_RANGE.  out == NULL: IMT_ERR_ARG.  A misaligned device buffer: IMT_ERR_ARG, as for
 * imt_itree_insert_batch.  n == 0: IMT_OK.  Nothing is written in any of these cases.  Never IMT_ERR_VALUE: stored values
 * were valid when they went in.
 * Memory: the view owns a plan set for 2n events (what one of the tree's own plan sets holds for a batch of n), grow-only
 * and freed with the view; the merged index of size + n entries, 4 bytes each, is borrowed from the context for the time
 * of the call, as a rebuild borrows its scratch. */
int imt_itree_view_insert_witness(imt_itree_view *v, size_t n, const imt_insert_out *out, unsigned flags);
/* Its twin for a block that also held READs, imt_itree_view_mixed_witness, takes an imt_read_out and is declared with
 * the mixed batches below, behind imt_itree_mixed_filtered. */
/* ... AND IN THE BULK FORM: the imt_bulk_out of the n insertions that followed the view's size (imt_itree_insert_bulk
 * above: one low-leaf path per value in descending value order, one shared append).
 * DEFINED BY THE SIZES ALONE.  Let S = imt_itree_view_size(v).  Take a fresh tree fed the first S - 1 values and call
 * imt_itree_insert_bulk on it with the values of leaves [S, S + n), in leaf order, and the same flags: this call writes
 * into `out` what that call would write, byte for byte, in all ten fields; NULL fields are skipped.  order[k] is a position
 * 0 .. n - 1 of the block (leaf S + order[k]); new_leaf[i] is the preimage of leaf S + i AS OF SIZE S + n, not as the tree
 * holds it now; root is the root as of S + n.  IMT_FMT_*, IMT_SIB_ITEM_MAJOR, IMT_DEVICE_PTRS and the alignment rules mean
 * what they mean to imt_itree_insert_bulk.  There is no `vals`: the tree has the values, however they went in (apply,
 * pipelined, witness, bulk, filtered, load_values).  IMT_HOST_PREP and IMT_INPUTS_READY change nothing.
 * A view query otherwise, like imt_itree_view_insert_witness: on the context's stream behind everything in flight, a stale
 * side table rebuilt first, the tree never changed (stored nodes, index buffers, plan sets, apply stats, size, rows of
 * the value array), nothing rotated or committed; synchronous for host pointers, only enqueued with IMT_DEVICE_PTRS, and
 * with no host wait of its own -- stored values were accepted when they went in, there is no verdict to read back.
 * out == NULL: IMT_ERR_ARG.  n == 0: IMT_OK.  S + n above the tree's size (any n > 0 on a view at the current size, any n
 * while the tree is smaller than the view): IMT_ERR_RANGE.  A placed or value-partitioned tree, IMT_PIPELINE, a misaligned
 * device buffer: IMT_ERR_ARG, as for imt_itree_insert_bulk.  A dead handle: IMT_ERR_ARG.  Nothing is written in any of
 * these cases.  Never IMT_ERR_VALUE.
 * Memory: the view's plan set grows to 2n events; the merged index of S + n entries and the append's rows (about 2n nodes
 * of 32 bytes) are borrowed from the context for the time of the call. */
int imt_itree_view_bulk_witness(imt_itree_view *v, size_t n, const imt_bulk_out *out, unsigned flags);
/* Read-only query of the device-resident index for any mix of values (one kernel, k_lookup): status ZERO / FOREIGN /
 * PRESENT / NEW and leaf_index = the sentinel / UINT64_MAX / the stored leaf / the low leaf (what find_low returns).
 * Fails only for its arguments, a value >= p (IMT_ERR_NONCANONICAL) or a HIP error, never for a value's class.  With
 * imt_itree_get_leaves and imt_itree_get_proof_batch a PRESENT index gives the membership witness verify_proof takes
 * (src/utils.rs:87). */
int imt_itree_lookup_batch(imt_itree *t, const void *vals /*[n][32]*/, size_t n, uint8_t *status /*[n]*/,
                           uint64_t *leaf_index /*[n] or NULL*/, unsigned flags);

/* Witness of verify_non_inclusion for n candidate values against the current tree, produced on the
 * GPU from the device-resident index: the low leaf (greatest stored value below the candidate), its
 * preimage, the is_largest flag and its `depth` siblings.  Outputs feed imt_non_membership_batch
 * unchanged.  Any output pointer may be NULL.  IMT_ERR_VALUE if a candidate is 0, already stored, or -- with a value
 * partition set (imt_itree_set_value_partition) -- of another subtree's residue: this subtree's list says nothing about it.
 * On a placed tree low_sib holds the subtree's `depth` rows; imt_itree_lift_batch with out = {low_sib} and
 * roots_before = roots_after = the subtrees' current roots appends the rows above (a depth-global_depth witness). */
int imt_itree_non_membership_witness(imt_itree *t, const void *vals /*[n][32]*/, size_t n,
                                     uint64_t *low_index /*[n]*/, void *low_leaf /*[n][3][32]*/,
                                     uint8_t *is_largest /*[n]*/, void *low_sib /*[depth][n][32]*/,
                                     unsigned flags);

/* A BLOCK AS IT IS: insertions and non-inclusion checks in one ordered list, for the prover of a block whose transactions
 * either insert a nullifier (insert_leaf) or only assert that a value is absent (verify_non_inclusion) against the tree as
 * it stands at that point of the block.
 * DEFINED BY THE SEQUENCE ALONE.  Walk the n operations in order on the tree: op[p] == IMT_OP_INSERT is
 * imt_itree_insert_batch of the one value vals[p]; op[p] == IMT_OP_READ is imt_itree_non_membership_witness of that one
 * value against the tree at that moment, plus imt_itree_root.  The call writes, byte for byte, what that walk writes, and
 * leaves the tree the walk leaves.  Row r of every `ins` array belongs to the r-th INSERT, row q of every `rd` array to the
 * q-th READ; sibling arrays of both keep the caller's dimensions (level-major [depth][n][32] with level stride n, the
 * number of operations; or item-major), imt_itree_insert_filtered's convention.  *n_inserted = the number of INSERTs.
 * What follows from the definition:
 *  - a batch of INSERTs only is imt_itree_insert_batch(t, vals, n, ins, flags);
 *  - a batch of READs only is imt_itree_non_membership_witness plus the current root in every row: it changes nothing,
 *    it is not counted as a change of the tree (views stay fresh) and imt_itree_root_lagged does not see it;
 *  - a READ of a value that a LATER operation of the batch inserts is legal, and so are two READs of one value -- their
 *    rows differ if an insertion between them changed the low leaf;
 *  - the root of a READ is new_root of the last INSERT before it, the tree's root before the call if there is none.
 * One level sweep serves both kinds: an INSERT costs 2 + 2*depth hashes, a READ 1 + depth.
 * REFUSALS, the tree untouched and no output written in every one of them.  IMT_ERR_VALUE: an INSERT
 * imt_itree_insert_batch would refuse at that point of the walk (0, stored, inserted earlier in the batch), or a READ of
 * 0, of a stored value or of a value an EARLIER operation of the batch inserts; *bad_op is then the smallest offending
 * position (written in this case only; *n_inserted with IMT_OK only).  IMT_ERR_NONCANONICAL and IMT_ERR_FULL as for
 * imt_itree_insert_batch, the latter counting INSERTs only.  IMT_ERR_ARG: an op byte above 1 (above 2 under
 * IMT_MEMBER_OPS, which adds IMT_OP_MEMBER: "PRESENCE READS" below); NULL vals or op with
 * n > 0; a misaligned device buffer; IMT_PIPELINE, IMT_HOST_PREP or IMT_INPUTS_READY in flags; a placed or partitioned
 * tree (so a value of another subtree's residue cannot occur); a replica of a sliced world with steps in flight; an open
 * slice; a call between imt_itree_batch_begin and _end.  n == 0: IMT_OK.
 * NOT IN THIS CALL: placed / partitioned trees, and overlap with the batches around it -- imt_itree_mixed_pipelined below.
 * IMT_FMT_*, IMT_SIB_ITEM_MAJOR and IMT_DEVICE_PTRS mean what they mean to imt_itree_insert_batch; with IMT_DEVICE_PTRS
 * `op` is a device pointer too, n_inserted and bad_op are host memory always.  The call orders itself behind batches in
 * flight (pipelined ones included), later calls are ordered behind it, and like imt_itree_insert_batch it returns once the
 * values have been checked on the GPU: n_inserted and bad_op are complete at return. */
#define IMT_OP_INSERT 0
#define IMT_OP_READ 1
/* PRESENCE READS (IMT_MEMBER_OPS in flags; the third kind of operation, for a transaction that asserts a value IS in the
 * tree as of its place in the block: "this nullifier has been emitted").  Accepted by the seven mixed-block calls --
 * imt_itree_mixed_batch, _mixed_filtered, _apply_mixed, _apply_mixed_filtered, _mixed_pipelined, _apply_mixed_pipelined and
 * imt_itree_view_mixed_witness.  WITHOUT THE FLAG every one of them is what its comment says and nothing more: op byte 2
 * is "an op byte above 1".  WITH IT op bytes 0, 1 and 2 are legal and anything above is IMT_ERR_ARG.
 * DEFINED BY THE WALK, like the other two kinds: op[p] == IMT_OP_MEMBER with value v asks imt_itree_lookup_batch of v on
 * the tree at that moment; the answer must be IMT_VAL_PRESENT at some leaf L, and the row the call writes holds
 *     low_index = L,  low_leaf = imt_itree_get_leaves(L) then = {v, next_val, next_idx},  is_largest = (next_val == 0),
 *     root = imt_itree_root then,  low_sib = imt_itree_get_proof_batch(L) then.
 * A consumer checks low_leaf.val == v and imt_verify_proof_batch(hash3(low_leaf), low_index, root, low_sib).
 * THE ROWS go to the `rd` arrays: row q of `rd` belongs to the q-th operation that is NOT AN INSERT, so READs and MEMBERs
 * share one numbering in block order and the caller tells them apart by `op`; without MEMBERs that is the numbering of
 * the READs.  Level stride, IMT_FMT_*, IMT_SIB_ITEM_MAJOR and IMT_DEVICE_PTRS as for a READ.
 * REFUSED (IMT_ERR_VALUE, tree and outputs untouched, *bad_op the smallest offending position over all kinds): a MEMBER
 * of 0, or of a value that is neither stored before the call nor put in by an INSERT at a SMALLER position -- a later
 * INSERT does not help.  The rules of INSERT and READ do not change; IMT_ERR_FULL counts INSERTs only.
 * COST: 1 + depth hashes in the witness forms, as a READ.  In the apply forms no hash and no event: imt_itree_apply_stats
 * is that of the INSERTs alone.  A block with no INSERT is no change of the tree (views stay fresh, imt_itree_root_lagged
 * does not see it).
 * THE FILTERED TWINS: status[p] keeps its meaning for every kind -- it says what the VALUE is at that place.  What is
 * carried out depends on the kind: an INSERT or a READ iff IMT_VAL_NEW, a MEMBER iff IMT_VAL_PRESENT or IMT_VAL_REPEATED.
 * With A the carried-out positions the call IS the strict call on vals[A], op[A] with the same flags; *n_read counts the
 * carried-out READs plus MEMBERs.  leaf_index[p] of a MEMBER: PRESENT -> the stored leaf; REPEATED -> the leaf the INSERT
 * at f(v) wrote; ZERO -> the sentinel; NEW (skipped: the value is not there) -> UINT64_MAX.
 * THE REPLAY (imt_itree_view_mixed_witness) judges a MEMBER on the fresh tree of the view's size plus the list's INSERTs
 * before it: values the tree received after size + n_ins do not count.
 * Placed and partitioned trees stay refused either way. */
#define IMT_OP_MEMBER 2
typedef struct imt_read_out {   /* rows of the q-th READ (under IMT_MEMBER_OPS: of the q-th operation that is no INSERT; for a
                                   MEMBER read "the leaf that holds the value" for "the low leaf"); every pointer may be NULL;
                                   host or device per flags */
    uint64_t *low_index;     /* [n]        the low leaf of the value as of the READ */
    void *low_leaf;          /* [n][3][32] its preimage then */
    uint8_t *is_largest;     /* [n]        low_leaf.next_val == 0 */
    void *root;              /* [n][32]    the root the witness verifies against */
    void *low_sib;           /* [depth][n][32] the low leaf's proof against it (layout per flags) */
} imt_read_out;
int imt_itree_mixed_batch(imt_itree *t, const void *vals /*[n][32]*/, const uint8_t *op /*[n]*/, size_t n,
                          const imt_insert_out *ins /*may be NULL*/, const imt_read_out *rd /*may be NULL*/,
                          uint64_t *n_inserted /*host, may be NULL*/, uint64_t *bad_op /*host, may be NULL*/,
                          unsigned flags);
/* THE SAME BLOCK WHEN IT MAY HOLD INVALID TRANSACTIONS (a sequencer's): imt_itree_mixed_batch with the operations it
 * would refuse skipped, each with a status, in one call.
 * DEFINED BY THE SEQUENCE ALONE.  Walk the n operations in order as imt_itree_mixed_batch does; an operation the walk
 * would refuse at that point is skipped, every other one is carried out.  status[p] of the operation at position p with
 * value v is the first that applies of (whether the operation is an INSERT or a READ makes no difference):
 *   IMT_VAL_ZERO      v == 0;
 *   IMT_VAL_PRESENT   v was stored before the call;
 *   IMT_VAL_REPEATED  p > f(v), with f(v) the smallest position whose operation is an INSERT of v: an earlier INSERT of
 *                     this block put v in -- a double spend inside the block, or a READ of a value present by then;
 *   IMT_VAL_NEW       otherwise (p <= f(v), or no INSERT of v at all): carried out.  A READ of a value a later operation
 *                     inserts is NEW, as in imt_itree_mixed_batch; two READs of one value before its INSERT are both NEW.
 * IMT_VAL_FOREIGN does not occur: placed and partitioned trees are refused as there.
 * Let A be the positions with status NEW, in order: the call IS imt_itree_mixed_batch(t, vals[A], op[A], |A|, ins, rd, ..)
 * -- the same tree, byte for byte the same rows, row r of the `ins` arrays the r-th accepted INSERT, row q of the `rd`
 * arrays the q-th accepted READ -- except that sibling arrays keep the caller's dimensions: level-major [depth][n][32]
 * with level stride n, the operations passed in, not |A| (item-major arrays are unchanged); imt_itree_insert_filtered's
 * convention.  *n_inserted / *n_read = the accepted INSERTs / READs; rows at or beyond them are not written.
 * leaf_index[p]: INSERT, NEW -> the leaf it was written to; READ, NEW -> the low leaf as of the READ (its rd->low_index
 * row, what imt_itree_lookup_batch would report there); PRESENT -> the stored leaf; REPEATED -> the leaf the INSERT at
 * f(v) was written to; ZERO -> the sentinel.
 * status, leaf_index, *n_inserted and *n_read are complete when the call returns; status / leaf_index are host or device
 * memory per IMT_DEVICE_PTRS (then `op` is a device pointer too), the two counts host memory always.
 * What follows from the definition:
 *  - a block in which nothing is refused is imt_itree_mixed_batch of it;
 *  - a block of INSERTs only is imt_itree_insert_filtered of its values: the same status, leaf_index, *n_inserted and
 *    `ins` rows;
 *  - a block in which nothing is accepted, or only READs are, returns IMT_OK and changes nothing: it is not counted as a
 *    change of the tree (views stay fresh) and imt_itree_root_lagged does not see it.
 * ERRORS, the tree and every ins / rd buffer untouched, both counts 0.  IMT_ERR_ARG, nothing else written at all: NULL
 * status, n_inserted or n_read; NULL vals or op with n > 0; an op byte above 1 (above 2 under IMT_MEMBER_OPS, which also
 * says what is carried out of a MEMBER and what its leaf_index is: "PRESENCE READS" above); a misaligned device buffer;
 * IMT_PIPELINE, IMT_HOST_PREP or IMT_INPUTS_READY; a placed or partitioned tree; a replica of a sliced world with steps
 * in flight; an open slice; a call between imt_itree_batch_begin and _end.  IMT_ERR_NONCANONICAL for a value >= p
 * (malformed input, not a rejection); IMT_ERR_FULL if size + the accepted INSERTs exceeds the capacity (skipped INSERTs
 * do not count): on these two status holds the classification and leaf_index is unspecified.  Never IMT_ERR_VALUE; should
 * the checks of imt_itree_mixed_batch refuse what the filter accepted, that is a bug and IMT_ERR_INTERNAL.
 * n == 0: IMT_OK, both counts 0.
 * IMT_FMT_*, IMT_SIB_ITEM_MAJOR and IMT_DEVICE_PTRS mean what they mean to imt_itree_mixed_batch, and the call is ordered
 * as that one: behind batches in flight, later calls behind it.  The classification costs one more host
 * wait, a sort of the positions, two scans and four short kernels. */
int imt_itree_mixed_filtered(imt_itree *t, const void *vals /*[n][32]*/, const uint8_t *op /*[n]*/, size_t n,
                             uint8_t *status /*[n]*/, uint64_t *leaf_index /*[n] or NULL*/,
                             const imt_insert_out *ins /*may be NULL*/, const imt_read_out *rd /*may be NULL*/,
                             uint64_t *n_inserted /*host*/, uint64_t *n_read /*host*/, unsigned flags);
/* THE SAME TWO BLOCKS WITHOUT WITNESSES, for whoever applies a block now and proves it elsewhere or later (the sequencer
 * and the chain follower of INTEGRATION.md 4): the ordered walk decides what each READ may see, and nothing is proved.
 * DEFINED BY THE CALLS ABOVE.  imt_itree_apply_mixed IS
 *     imt_itree_mixed_batch(t, vals, op, n, NULL, NULL, n_inserted, bad_op, flags)
 * -- the same result, *n_inserted with IMT_OK only and *bad_op with IMT_ERR_VALUE only, every refusal of that call with
 * the tree untouched (IMT_ERR_VALUE, IMT_ERR_NONCANONICAL, IMT_ERR_FULL counting INSERTs only, and IMT_ERR_ARG: an op byte
 * above 1, above 2 under IMT_MEMBER_OPS -- a MEMBER is judged like a READ and like a READ costs no hash and no event,
 * "PRESENCE READS" above; NULL vals or op with n > 0; a misaligned device buffer; IMT_PIPELINE, IMT_HOST_PREP or IMT_INPUTS_READY; a
 * placed or partitioned tree; a replica of a sliced world with steps in flight; an open slice; a call between
 * imt_itree_batch_begin and _end), and afterwards the same tree byte for byte: stored nodes, value rows, index, size.  A
 * block without an INSERT changes nothing, is not counted as a change (views stay fresh) and imt_itree_root_lagged does not
 * see it.  imt_itree_apply_mixed_filtered IS
 *     imt_itree_mixed_filtered(t, vals, op, n, status, leaf_index, NULL, NULL, n_inserted, n_read, flags)
 * in the same sense: status, leaf_index (the low leaf of an accepted READ as of its place in the block included), both
 * counts and every error case as that call writes them, and the same tree afterwards.
 * ON TOP OF THAT both write root_out, as imt_itree_apply_batch does: the root after the block, [32] in the flags' format,
 * host or device memory per IMT_DEVICE_PTRS, may be NULL; the current root when n == 0 or the block inserts nothing;
 * not written on any refusal.
 * THE COST IS imt_itree_apply_batch's, exactly: the call hashes what imt_itree_apply_batch of the carried-out INSERT values,
 * in their order, hashes -- every touched node once, 3 to 9 hashes per INSERT where the calls above spend 2 + 2*depth per
 * INSERT and 1 + depth per READ -- and imt_itree_apply_stats reports the same depth + 1 counts afterwards.  A READ adds no
 * hash: it is judged by the checks and reaches no hash kernel.  A block that inserts nothing hashes nothing, and
 * imt_itree_apply_stats keeps reporting the earlier apply call.
 * Ordered as imt_itree_apply_batch: on the context's stream, behind every batch in flight (pipelined ones included),
 * later calls of any kind behind it; witness, apply, mixed and apply-mixed calls alternate freely on one tree.  status,
 * leaf_index and the counts are complete at return, as for the calls above.
 * NOT IN THESE CALLS: placed and partitioned trees, overlap between consecutive blocks (imt_itree_apply_mixed_pipelined
 * below has it; the filtered twin does not, see imt_itree_apply_pipelined), and witness rows of any kind -- a view at the
 * size before the block gives them later: imt_itree_view_mixed_witness below, over the operations that were carried out. */
int imt_itree_apply_mixed(imt_itree *t, const void *vals /*[n][32]*/, const uint8_t *op /*[n]*/, size_t n,
                          void *root_out /*[32] or NULL*/, uint64_t *n_inserted /*host, may be NULL*/,
                          uint64_t *bad_op /*host, may be NULL*/, unsigned flags);
int imt_itree_apply_mixed_filtered(imt_itree *t, const void *vals /*[n][32]*/, const uint8_t *op /*[n]*/, size_t n,
                                   uint8_t *status /*[n]*/, uint64_t *leaf_index /*[n] or NULL*/,
                                   uint64_t *n_inserted /*host*/, uint64_t *n_read /*host*/,
                                   void *root_out /*[32] or NULL*/, unsigned flags);
/* CONSECUTIVE MIXED BLOCKS THAT OVERLAP, for the prover and the follower of a chain whose blocks hold
 * verify_non_inclusion transactions: imt_itree_mixed_batch and imt_itree_apply_mixed on the tree's pipeline streams.
 * DEFINED BY THE CALLS ABOVE.  Play the same blocks on a twin tree through imt_itree_mixed_batch (imt_itree_apply_mixed for
 * the apply form), one at a time with imt_ctx_sync() after each.  AT RETURN this call has given the same return code, the
 * same *n_inserted (with IMT_OK only) and *bad_op (with IMT_ERR_VALUE only) -- host memory, complete at return -- and the
 * same imt_itree_size.  AFTER imt_ctx_sync() every array of `ins` and `rd` holds the same rows byte for byte (NULL fields
 * skipped, level stride n, IMT_FMT_* and IMT_SIB_ITEM_MAJOR as there, nothing written at or beyond row n_inserted of `ins`
 * or row n - n_inserted of `rd`), root_out holds the same root, and the tree is the same tree: index, leaf preimages,
 * every stored node, root -- so every later call answers the same, imt_itree_root_lagged, imt_itree_apply_stats and whether
 * a view rebuilds included.
 * WHAT DIFFERS.  The call returns once the block has passed the mixed checks on the GPU (the two host waits of the calls
 * above: the INSERT count, then the verdict); its hashing runs on one of the tree's pipeline streams behind the blocks
 * before it -- a witness block one level behind the block in front, an apply block two launches behind
 * (imt_apply_pipe.hpp: by the levels it reads and writes a mixed witness block is a witness batch of its events, a READ's
 * write-back putting back the bytes it read, and a mixed apply block is the apply batch of its INSERTs).  Up to four
 * consecutive blocks hash at once; a fifth call waits for the first.
 * IMT_DEVICE_PTRS is required (otherwise IMT_ERR_ARG, nothing changed): vals, op, every output array and root_out are
 * device-addressable memory -- a row of an imt_host_alloc buffer is fine -- aligned as the device-pointer path of the calls
 * above demands; n_inserted and bad_op stay host pointers.  IMT_PIPELINE may be set and means nothing more; IMT_HOST_PREP
 * and IMT_INPUTS_READY are IMT_ERR_ARG, and so is every other refusal of the calls above (placed and partitioned trees, an
 * open slice, ...).  IMT_MEMBER_OPS means what it means to the calls above ("PRESENCE READS"): the rows of MEMBERs are rows
 * of `rd`, and a block of READs and MEMBERs only is "a block of READs only" below.
 * vals AND op MAY BE REUSED WHEN THE CALL RETURNS, whatever it returns: nothing enqueued after the checks reads them (the
 * INSERT values are in the tree's value rows by then, the op bytes in the block's own tables).  The output arrays and
 * root_out belong to the block until imt_ctx_sync() or any later call on the tree has ordered the context's stream
 * behind it.
 * A REFUSED BLOCK (IMT_ERR_VALUE with *bad_op, IMT_ERR_NONCANONICAL, IMT_ERR_FULL, a bad op byte as IMT_ERR_ARG) leaves
 * alone the tree, the blocks in flight and their outputs, and writes nothing of the caller's but *bad_op.
 * A BLOCK OF READS ONLY goes through imt_itree_mixed_pipelined like any other block: it runs behind the block before it,
 * so its rows carry that block's effects, and the block behind it waits for it level by level; as in the calls above it
 * is no change of the tree (views stay fresh, imt_itree_root_lagged does not see it, the size stays).  Through
 * imt_itree_apply_mixed_pipelined it hashes nothing: root_out = the current root, ordered behind everything in flight, and
 * imt_itree_apply_stats keeps reporting the earlier apply call.  n == 0: IMT_OK, *n_inserted = 0, root_out likewise.
 * imt_itree_apply_stats treats imt_itree_apply_mixed_pipelined as it treats imt_itree_apply_pipelined: the counts are
 * those of imt_itree_apply_batch of the carried-out INSERT values, and it waits for that call only.
 * Every other call on the tree orders itself behind these blocks exactly as behind pipelined batches (queries, views and
 * their replays, imt_itree_rewind, imt_itree_load*, un-pipelined batches of every kind, imt_sliced_* entry), and the four
 * pipelined kinds -- imt_itree_insert_batch with IMT_PIPELINE, imt_itree_apply_pipelined and these two -- may follow each
 * other in any order with no synchronisation between them.
 * Measured against the calls above: profiles/mixed_pipelined.txt, README "Mixed blocks that overlap". */
int imt_itree_mixed_pipelined(imt_itree *t, const void *vals /*[n][32]*/, const uint8_t *op /*[n]*/, size_t n,
                              const imt_insert_out *ins /*may be NULL*/, const imt_read_out *rd /*may be NULL*/,
                              uint64_t *n_inserted /*host, may be NULL*/, uint64_t *bad_op /*host, may be NULL*/,
                              unsigned flags);
int imt_itree_apply_mixed_pipelined(imt_itree *t, const void *vals /*[n][32]*/, const uint8_t *op /*[n]*/, size_t n,
                                    void *root_out /*[32] or NULL*/, uint64_t *n_inserted /*host, may be NULL*/,
                                    uint64_t *bad_op /*host, may be NULL*/, unsigned flags);
/* APPLY A MIXED BLOCK NOW, PROVE IT LATER (beside imt_itree_view_insert_witness; declared here for imt_read_out): the
 * witnesses of a block of INSERTs and READs whose insertions the tree has already made, witness-free or otherwise, and may
 * since have built upon -- every READ's witness against the tree as it stood at that point of the block.
 * DEFINED BY THE SIZE AND THE LIST ALONE.  Take a fresh tree fed the first size - 1 values this tree holds and call
 * imt_itree_mixed_batch(fresh, vals, op, n, ins, rd, n_inserted, bad_op, flags) on it: this call writes what that call
 * writes, byte for byte -- every `ins` and `rd` field, NULL fields skipped, row r of `ins` the r-th INSERT, row q of `rd` the
 * q-th READ, sibling arrays level-major with level stride n or item-major, IMT_FMT_*, IMT_SIB_ITEM_MAJOR and
 * IMT_DEVICE_PTRS as there (`op` a device pointer too), *n_inserted = the number of INSERTs.
 * ONE CONDITION MAKES IT A REPLAY: the INSERTs of the list must be the values the tree holds at leaves
 * [size, size + n_ins), in that order.  The caller passes the block as it was, and the call checks that it was this block.
 * What follows from the definition:
 *  - a list of INSERTs only is imt_itree_view_insert_witness(v, n, ins, flags);
 *  - a list of READs only is imt_itree_view_non_membership_witness of those values with imt_itree_view_root in every
 *    rd->root row (on a view at the tree's current size too);
 *  - the root of a READ with no INSERT before it, and old_root of the first INSERT, are the VIEW's root, not the tree's;
 *  - a READ of a value that a later operation of the list inserts is legal, so is a READ of a value the tree received
 *    after size + n_ins, and so are two READs of one value.
 * It is a view query otherwise: it never changes the tree (stored nodes, index buffers, plan sets, size, lagged roots,
 * rows of the value array -- an INSERT's value is compared with its row, never written there), it rebuilds a stale side
 * table first, behind everything in flight, pipelined batches included, and it is refused where the other view queries
 * are.  Synchronous for host pointers; with IMT_DEVICE_PTRS it is enqueued on the context's stream.  n_inserted and
 * bad_op are host memory and complete at return.
 * REFUSALS, nothing written to `ins` or `rd`, tree and view untouched.  IMT_ERR_VALUE with *bad_op = the smallest position
 * p at which either the walk on the fresh tree refuses the operation (a READ of 0, of a value stored as of the view's
 * size, or of a value an earlier INSERT of the list put in) or the operation is an INSERT of rank r whose value is not the
 * one the tree holds at leaf size + r.  IMT_ERR_RANGE: more INSERTs in the list than imt_itree_size(t) - size, or a tree
 * smaller than the view.  IMT_ERR_NONCANONICAL for a value >= p.  IMT_ERR_ARG: a handle that is not a live view; NULL
 * vals or op with n > 0; an op byte above 1 (above 2 under IMT_MEMBER_OPS: a MEMBER is judged on that fresh tree plus
 * the list's INSERTs before it, "PRESENCE READS" above -- a value the tree received after size + n_ins is not there);
 * a misaligned device buffer; IMT_PIPELINE, IMT_HOST_PREP or
 * IMT_INPUTS_READY in flags; a placed or partitioned tree; a replica of a sliced world with steps in flight; an open
 * slice; a call between imt_itree_batch_begin and _end.  n == 0: IMT_OK, *n_inserted = 0.  Never IMT_ERR_FULL.
 * NOT IN THIS CALL: a filtered form (the caller kept the statuses from when the block went in and passes the accepted
 * operations), placed and partitioned trees.
 * Memory as for imt_itree_view_insert_witness: the view's plan set grows to 2n events, the merged index of size + n_ins
 * entries is borrowed from the context for the time of the call. */
int imt_itree_view_mixed_witness(imt_itree_view *v, const void *vals /*[n][32]*/, const uint8_t *op /*[n]*/, size_t n,
                                 const imt_insert_out *ins /*may be NULL*/, const imt_read_out *rd /*may be NULL*/,
                                 uint64_t *n_inserted /*host, may be NULL*/, uint64_t *bad_op /*host, may be NULL*/,
                                 unsigned flags);

/* ---- e: the tree as ONE SUBTREE of a deeper tree (sharding by leaf-index range) -----------------
 * north_star's multi-GPU layout: GPU g owns leaf indices [g << depth, (g + 1) << depth) of a tree of depth
 * global_depth as an indexed tree of its own (own {0,0,0} sentinel at its first leaf, own sorted list; the
 * value space is partitioned between the subtrees by the caller).
 * After imt_itree_set_placement (on an empty tree) every LEAF INDEX that crosses the API is global,
 * (subtree_index << depth) + local: low_index outputs, index arguments, and the next_idx field of leaf
 * preimages -- hence what is hashed into the leaves (new_val_idx, src/indexed_merkle_tree.rs:655,:715).
 * Sibling arrays passed to imt_itree_insert_batch are dimensioned for global_depth levels ([global_depth][n]
 * or, item-major, [n][global_depth]); the batch writes levels [0, depth). */
int imt_itree_set_placement(imt_itree *t, unsigned global_depth, uint64_t subtree_index);
/* The value partition between subtrees: from now on imt_itree_insert_batch / imt_itree_batch_begin accept only
 * values with v mod modulus == residue (checked for every value, on the GPU with the default prepare) and
 * fail with IMT_ERR_VALUE otherwise, the tree unchanged.  modulus 0 or 1 = accept everything. */
int imt_itree_set_value_partition(imt_itree *t, uint32_t modulus, uint32_t residue);
/* Lifts the outputs of ONE imt_itree_insert_batch on a placed tree to witnesses of the enclosing tree, so
 * that they are what insert_leaf takes (src/indexed_merkle_tree.rs:231-245: depth-d proofs, depth-d roots):
 * old_root / interim_root / new_root (given as subtree roots, replaced in place) climb the global_depth - depth
 * upper levels, and rows [depth, global_depth) of low_sib / new_sib receive the siblings of that climb.
 * Order of a step across subtrees: subtree 0's insertions, then subtree 1's, ...; so the siblings left of
 * this subtree are taken from roots_after (every subtree's root after the step) and those right of it from
 * roots_before.  Both are [n_subtrees][32] in the format of `flags` (what an all-gather of imt_itree_root /
 * imt_itree_root_lagged returns); levels above depth + log2(n_subtrees) meet empty subtrees.
 * 2 * (global_depth - depth) hashes per insertion: with the batch's 2 + 2 * depth that is the 2 + 2 * 32 of an
 * unsharded depth-32 insertion.  Host or device pointers per flags; enqueued on the context's stream, which
 * the caller must have ordered behind the batch (imt_itree_root_lagged for that batch, or imt_ctx_sync). */
int imt_itree_lift_batch(imt_itree *t, const void *roots_before /*[n_subtrees][32]*/,
                         const void *roots_after /*[n_subtrees][32]*/, size_t n_subtrees, size_t n,
                         const imt_insert_out *out, unsigned flags);

/* ---- e: one tree on several GPUs, sequential semantics (single sorted list) ------------------
 * Every rank holds a replica of the tree and calls the same sequence with the same values; the hashing
 * of each step is split by slot range between the ranks, and the caller all-gathers the value arrays in
 * between (RCCL).  A batch of n insertions has E = 2n events; level l has E slots for l = 0..l0 (l0 =
 * ceil(log2(size + n))), val[l] is [E][32] in the library's device format.  All data pointers are
 * device pointers; work is enqueued on the context's stream.
 *   begin   : values (host or device per flags; identical on all ranks) -> plan; E and l0 returned.
 *             IMT_ERR_VALUE / IMT_ERR_NONCANONICAL / IMT_ERR_FULL exactly as imt_itree_insert_batch.
 *   leaves  : val0[k] for slots [k_begin, k_begin + k_count)
 *   level   : val_out[k] (level l+1) for a slot range, from the COMPLETE val_in (level l)
 *   top     : from the complete val[l0]: root after every event of [e_begin, +e_count) -> roots[e][32]
 *             (device format); the rank whose range contains the last event also fills top_path
 *             ([depth - l0 + 1][32], the stored nodes above l0), which the caller broadcasts.
 *   extract : witnesses of insertions [ins_begin, +ins_count) (any subset, any rank) from the complete
 *             val[0..l0] and roots: every field of imt_insert_out, rows indexed from ins_begin;
 *             formats / sibling layout per flags (level stride = ins_count).
 *   end     : write the batch into the replica (needs the complete val[0..l0] and top_path). */
int imt_itree_batch_begin(imt_itree *t, const void *vals /*[n][32]*/, size_t n, unsigned flags,
                          uint32_t *events_out, uint32_t *l0_out);
int imt_itree_batch_leaves(imt_itree *t, void *val0, uint32_t k_begin, uint32_t k_count);
int imt_itree_batch_level(imt_itree *t, unsigned level, const void *val_in, void *val_out, uint32_t k_begin,
                          uint32_t k_count);
int imt_itree_batch_top(imt_itree *t, const void *val_l0, uint32_t e_begin, uint32_t e_count, void *roots,
                        void *top_path);
int imt_itree_batch_extract(imt_itree *t, const void *const *val_levels /*host array of l0+1 device ptrs*/,
                            const void *roots, uint32_t ins_begin, uint32_t ins_count,
                            const imt_insert_out *out, unsigned flags);
int imt_itree_batch_end(imt_itree *t, const void *const *val_levels, const void *top_path);
/* gives up an open batch (after a failed collective, say): the tree is as it was before imt_itree_batch_begin */
int imt_itree_batch_abort(imt_itree *t);

/* ---- e: ONE tree on several GPUs, sequential semantics, TIME-SLICED ------------------------------
 * The reference's single sorted list (update_idx_leaf, src/indexed_merkle_tree.rs:632-660; insertion i at leaf
 * size + i, :715) at any number of GPUs, bit-exact with one GPU.  A step's world x n insertions are cut into `world`
 * consecutive slices in insertion order: GPU g hashes slice g -- low-leaf rewrites, new leaves, every node version up to
 * the root, 2 + 2 * depth hashes per insertion -- and writes the witnesses of its own insertions directly; every GPU
 * keeps a replica of the stored tree and of the sorted index (all ranks see all values of a step; the index work is
 * hash-free).  What crosses GPUs is what a slice WRITES BACK to the stored tree, level by level, as packed (node,
 * value) pairs: the ranks form a systolic chain `lag` levels apart, the pairs of a tick are all-gathered
 * asynchronously and applied `lag` ticks later, and up to IMT_SLICED_ROUNDS steps overlap.
 *
 * THE SCHEDULE, ITS STREAMS AND EVENTS AND THE COLLECTIVE LIVE IN THE LIBRARY: a host calls imt_sliced_step once per
 * step and imt_sliced_wait / imt_sliced_flush to read results.  Correctness (a slice's level l sees the level-l
 * write-backs of every earlier slice and of no later one) does not depend on anything the caller orders.
 *
 * One imt_sliced drives the ranks of THIS process: one (a distributed world, one process per GPU: the production form,
 * transport = RCCL) or all of them (all replicas in one process: tests and the one-GPU rehearsal, transport = local).
 * Every rank of a world must make the same sequence of imt_sliced_step / imt_sliced_wait / imt_sliced_flush calls, with
 * the same values and the same `round` arguments (imt_sliced_wait included: a wait may issue what is left of its round,
 * and the order in which the collectives of overlapping rounds are issued must be the same on every rank -- with it,
 * no placement of the library's streams on hardware queues can make two ranks wait for each other: tests/hwq_model.py). */
#define IMT_SLICED_ROUNDS 4
typedef struct imt_sliced imt_sliced;
typedef struct imt_transport imt_transport;    /* how the payloads of one tick meet: an all-gather */

/* A caller-supplied collective (MPI, a test double, ...).  all_gather is enqueued on hip_stream and must be complete, in
 * stream order, when the stream gets past it (NCCL semantics): recv[r * bytes, (r + 1) * bytes) = rank r's send[0, bytes)
 * for every rank r of the world.  Calls with different `channel` (0 .. IMT_SLICED_ROUNDS - 1) come from different streams
 * and may overlap; calls on one channel are issued in the same order on every rank.  `buffer` (0 .. lag) tells which of
 * the channel's buffer pairs is in use: the (send, recv) pointers of a (channel, buffer) never change. */
typedef struct imt_transport_ops {
    void *self;
    int (*all_gather)(void *self, int channel, int buffer, const void *send, void *recv, size_t bytes, void *hip_stream);
    void (*destroy)(void *self);       /* may be NULL */
} imt_transport_ops;
int imt_transport_custom_create(const imt_transport_ops *ops, imt_transport **out);
/* all ranks in this process (any devices that can copy to each other): device-to-device copies ordered by events */
int imt_transport_local_create(imt_transport **out);
/* RCCL over xGMI: ncclAllGather on communicators of this library's own (n_comms of them, 1 .. IMT_SLICED_ROUNDS: the
 * rounds in flight use different communicators, so their gathers do not queue behind each other).  Bootstrap like any
 * NCCL program: rank 0 calls imt_rccl_get_unique_id n_comms times, the host broadcasts the ids by whatever means it has,
 * every rank calls imt_transport_rccl_create (collective: it returns when all ranks have joined). */
#define IMT_RCCL_UNIQUE_ID_BYTES 128
int imt_rccl_get_unique_id(void *id /*[IMT_RCCL_UNIQUE_ID_BYTES]*/);
int imt_transport_rccl_create(imt_ctx *ctx, const void *unique_ids /*[n_comms][IMT_RCCL_UNIQUE_ID_BYTES]*/, int n_comms,
                              int world, int rank, imt_transport **out);
/* the same over communicators the host owns (ncclComm_t handles of this device; not destroyed by the library) */
int imt_transport_rccl_adopt(void *const *nccl_comms, int n_comms, imt_transport **out);
/* RCCL is bound at run time: the copy the process already holds (a host that has loaded one), else librccl.so.1 from
 * the library's RUNPATH.  Returns the path of the bound library (or why none was found); *version_out = its
 * NCCL_VERSION_CODE.  IMT_ERR_NO_DEVICE from the calls above when there is none. */
const char *imt_rccl_library(int *version_out);
/* Direct peer copies between processes of one node (HIP IPC memory + event handles; xGMI point-to-point reads when the
 * ranks sit on different GPUs, plain device copies when they share one: the one-GPU rehearsal of a multi-process run).
 * create writes this rank's handle blob (imt_transport_ipc_blob_bytes() bytes); the host all-gathers the blobs by
 * whatever means it has and every rank passes all of them, in rank order, to connect.  depth / max_slice / lag as given
 * to imt_sliced_create. */
size_t imt_transport_ipc_blob_bytes(void);
int imt_transport_ipc_create(imt_ctx *ctx, int world, int rank, unsigned depth, size_t max_slice, int lag,
                             imt_transport **out, void *blob_out);
int imt_transport_ipc_connect(imt_transport *tp, const void *all_blobs /*[world][blob_bytes]*/);
/* after every imt_sliced that uses it (IMT_ERR_ARG and nothing destroyed while one still does), and before the imt_ctx it
 * was created on */
int imt_transport_destroy(imt_transport *tp);
const char *imt_transport_last_error(const imt_transport *tp);
/* IMT_TRANSPORT_OPT_TIMEOUT_MS: how long a wait for a peer inside the IPC transport may last (GPU-side and host-side;
 * default 60 000, at least 10) before it gives up -- the transport's error word then turns non-zero and STAYS so: the
 * copies, acknowledgements and applies behind the wait are skipped on the device, the next imt_sliced_step / _wait /
 * _flush returns IMT_ERR_INTERNAL and the world refuses to go on.  IMT_TRANSPORT_OPT_HOST_POLL (before
 * imt_transport_ipc_connect): -1 decide from the PCI bus ids (ranks that share a GPU wait on the host), 0 / 1 forced. */
#define IMT_TRANSPORT_OPT_TIMEOUT_MS 1
#define IMT_TRANSPORT_OPT_HOST_POLL 2
int imt_transport_set_option(imt_transport *tp, int option, long value);
/* One small all-gather on the transport's own channel 0, enqueued on hip_stream (NULL = the stream of the context the
 * transport was created on): recv[r * bytes, (r + 1) * bytes) = rank r's send[0, bytes), device pointers, bytes a
 * multiple of 16 and at most 4096.  This is the ONE collective of the subtree layout (the all-gather of the per-GPU
 * subtree roots, 32 bytes per rank and step: examples/subtree_procs_demo.c, sharded.py), offered so that a host without a
 * collective library of its own can use the communicators this library already has (RCCL: ncclAllGather on communicator
 * 0; IPC: peer reads behind stream-ordered flags; custom: the vtable's all_gather with channel 0, buffer 0).  Every rank
 * calls it the same number of times in the same order; not while an imt_sliced uses the transport.  With the IPC
 * transport between ranks that share a GPU the call waits ON THE HOST for the peers (as that transport's fence does). */
int imt_transport_all_gather(imt_transport *tp, const void *send, void *recv, size_t bytes, void *hip_stream);
/* Has a GPU-side wait of the transport given up on a peer (IMT_TRANSPORT_OPT_TIMEOUT_MS)?  IMT_OK, or IMT_ERR_INTERNAL
 * (text in imt_transport_last_error): the error is STICKY -- every copy behind the wait was skipped on the device, `recv`
 * of that gather and of every later one holds whatever it held before, and later imt_transport_all_gather calls return
 * IMT_ERR_INTERNAL themselves.  The wait runs on the device: a caller of imt_transport_all_gather synchronises the stream
 * it named and then asks here BEFORE it reads `recv` (sharded.py does; an imt_sliced asks by itself in every
 * imt_sliced_step / _wait / _flush).  Transports without a GPU-side wait (RCCL, local, custom) always answer IMT_OK. */
int imt_transport_poll_error(imt_transport *tp);

/* trees[k] = the replica of rank first_rank + k (each on its own context; empty or with the same contents on every rank;
 * not placed, not partitioned); n_local = 1, or = world with the local transport.  max_slice = the largest n of a step.
 * lag = 0: the default max(2, ceil((depth + 1) / (3 * world))) (6, 3, 2 at 2, 4, 8 GPUs for depth 32).
 * IMT_ERR_RANGE if (world, depth, lag) would keep more than IMT_SLICED_ROUNDS steps in flight. */
int imt_sliced_create(imt_itree *const *trees, int n_local, int world, int first_rank, imt_transport *tp,
                      size_t max_slice, int lag, imt_sliced **out);
/* Options.  w == NULL: the defaults that imt_sliced_create calls made LATER in this process start from (every option);
 * w != NULL: an existing world (PREP_STREAM, WATCHDOG_MS, TIMING only -- the others decide which streams exist).
 * IMT_ERR_RANGE for a value outside the option's range, IMT_ERR_ARG for an unknown option or one that cannot be changed
 * any more.  (tools/ may override the defaults through environment variables of the same names, IMT_SLICED_COMM_STREAMS
 * ...; they are read once per imt_sliced_create.) */
#define IMT_SLICED_OPT_COMM_STREAMS 1      /* 0 .. 4 streams for the collectives (0: on the round's own stream); default 4 */
#define IMT_SLICED_OPT_COMM_PRIORITY 2     /* their HIP stream priority; default 0 = the pool of hardware queues the rounds use */
#define IMT_SLICED_OPT_ROUND_PRIORITIES 3  /* the four round streams: 0 (default) all at normal priority; 1 one normal + three high
                                              (not verified); 2 all LOW; 3 all HIGH -- a pool of hardware queues per priority */
#define IMT_SLICED_OPT_APPLY_STREAMS 4     /* 1: other ranks' write-backs are applied on a stream of their own per round slot; default 0 */
#define IMT_SLICED_OPT_PREP_STREAM 5       /* a step's preparation runs on 0 (default) the new round slot's collective stream, 1 its round stream, 2 the tree's side stream */
#define IMT_SLICED_OPT_VERIFY_QUEUES 6     /* 1 (default): imt_sliced_create measures which of its streams share a hardware queue
                                              and re-creates streams until the placement below holds; 0: take what the runtime gives.
                                              The measurement (a few milliseconds: a wave spinning 200 us on one stream, GPU-clock
                                              stamps on the others) wants the process's OTHER streams idle -- work queued elsewhere
                                              on a shared hardware queue delays a stamp and reads as "shares a queue"; the result is
                                              then a more cautious placement (imt_sliced_info.placement), never a wrong tree */
#define IMT_SLICED_OPT_WATCHDOG_MS 7       /* a host wait inside imt_sliced_step / _wait / _flush gives up after this long
                                              (default 120 000; 0 = never): IMT_ERR_TIMEOUT, the world's state on stderr and in
                                              imt_sliced_last_error, the world refuses to go on */
#define IMT_SLICED_OPT_TIMING 8            /* 1: host time per phase on stderr at imt_sliced_destroy */
#define IMT_SLICED_OPT_COMM_PLACEMENT 9    /* which hardware queues the collectives' streams are put on (by creating streams until one
                                              lands there): 0 (default) queues of their OWN -- none a round stream is on, none shared --
                                              if the runtime has any to give, else the queue of their round's stream; 1 their round's
                                              queue; 2 their own or IMT_SLICED_PLACEMENT_DEGRADED.  On its round's queue a collective
                                              holds up the round's next unit until the slowest rank has packed (every tick a barrier
                                              across ranks); on its own it overlaps the next `lag` units.  The runtime has four queues
                                              per priority level unless the host's environment says GPU_MAX_HW_QUEUES=8 (or more)
                                              BEFORE the first HIP call; queues in ANOTHER priority pool are what
                                              IMT_SLICED_OPT_POOLS (below, the default for one process per GPU) arranges */
#define IMT_SLICED_OPT_POOLS 10            /* 1: three priority pools -- round streams HIGH, collectives' streams LOW, the preparation
                                              on the round's stream (sets ROUND_PRIORITIES 3, COMM_PRIORITY lowest, PREP_STREAM 1); 2:
                                              round AND collectives' streams HIGH, the collectives' on their rounds' queues (4 % more per
                                              rank on one GPU, but every tick a barrier across ranks: COMM_PLACEMENT); 0: everything in
                                              the normal pool, as the options above say; -1 (default): 1 for a world of more than one
                                              rank with one rank in this process, else 0.
                                              Options the caller has set explicitly (imt_sliced_set_option(NULL, ...)) are NOT
                                              overwritten by a preset: the caller's value stands and imt_sliced_last_error of the new
                                              world says which preset was left out.  The runtime keeps a set of
                                              hardware queues per priority, and everybody else's streams are in the normal one -- the
                                              host's, and RCCL's: a communicator creates three of its own and brackets every
                                              collective with one (the user's stream waits for it, it waits for the kernel).  Sharing
                                              a round's queue, such a stream puts the round behind every collective and the collective
                                              behind the round's backlog, and this library can neither see nor move it; in the HIGH
                                              pool the rounds are alone.  Needs no GPU_MAX_HW_QUEUES.  One rank of 2 / 4 / 8 alone on
                                              a GPU: within 1 % of one pool */
#define IMT_SLICED_OPT_RESET 11            /* w == NULL, value 0: every default back to the library's own, and no option counts as
                                              "set explicitly by the caller" any more (see IMT_SLICED_OPT_POOLS) */
int imt_sliced_set_option(imt_sliced *w, int option, long value);
/* One step: vals = ALL world x n values of the step in insertion order (device pointer, identical contents on every
 * rank; format per flags), outs[k] = where local rank k's witnesses of ITS slice (insertions [rank * n, (rank + 1) * n)
 * of the step, n rows; sibling arrays [depth][n] or item-major per flags) are written; both stay untouched by the caller
 * until imt_sliced_wait for that round.  Enqueues the step's preparation and advances the schedule by one round
 * period; returns without waiting for the GPU (except for the values check: IMT_ERR_VALUE / IMT_ERR_NONCANONICAL /
 * IMT_ERR_FULL exactly as imt_itree_insert_batch, the same verdict on every rank, nothing changed).  *round_out = the
 * step's number.  flags: IMT_FMT_*, IMT_SIB_ITEM_MAJOR, IMT_INPUTS_READY. */
int imt_sliced_step(imt_sliced *w, const void *vals /*[world * n][32]*/, size_t n, const imt_insert_out *outs /*[n_local]*/,
                    unsigned flags, uint64_t *round_out);
/* HOW LONG imt_sliced_step BLOCKS, and why.  The call returns when the step's values have been checked on the GPU (the
 * preparation: sort, low-leaf search, merge into the index), because IMT_ERR_VALUE must be the call's own return value
 * and must leave every rank's tree untouched.  The preparation is short (1.5 - 2 ms at 2^16 values per rank) but is
 * enqueued behind the hashing already in flight, and one period of ticks (a whole step's worth of hashing per rank) is
 * issued per call and no more -- the back-pressure that keeps the hardware queues from filling up with a backlog other
 * streams would stand behind.  At 2^16 insertions per rank and step the calling thread is therefore inside the call for
 * about 16 - 17 ms of every 21.6 ms step: 1.4 - 3.8 ms issuing (imt_sliced_info.host_issue_ms), the rest waiting
 * (host_wait_ms).  A host that needs its thread runs the world from a thread of its own: the calls of one world need one
 * caller at a time, nothing else.  (Splitting the call into issue + verdict was measured and is slower at 8 ranks:
 * docs/LAB_NOTES.md.)
 *
 * host waits until local rank k's witnesses of `round` are complete (issues what is left of that ROUND first -- up to the
 * tick at which every rank's last unit of the round has been issued: the same tick on every rank) */
int imt_sliced_wait(imt_sliced *w, int local_rank, uint64_t round);
/* issues everything that is left of the steps in flight and waits for it: all replicas then hold the same tree, and the
 * trees may be used through the ordinary imt_itree_* calls again (roots, proofs, non-membership witnesses: every replica
 * holds the whole list, so such queries need no exchange).  Between imt_sliced_step and imt_sliced_flush only
 * imt_sliced_* calls may touch the trees. */
int imt_sliced_flush(imt_sliced *w);
typedef struct imt_sliced_info {
    int world, n_local, lag, period, gathers_per_round, round_ticks, rounds_in_flight;
    size_t payload_bytes;            /* size of one send buffer */
    uint64_t rounds, collectives, bytes_gathered;    /* since creation; collectives / bytes per local rank summed */
    double host_issue_ms, host_wait_ms;              /* wall time inside imt_sliced_step since creation: issuing work (every
                                                        launch, event and collective of the step) / waiting (for the GPU: the
                                                        values check of the step, back-pressure when the host runs ahead; for
                                                        peers: the host-polled IPC transport) */
    /* Where the world's streams sit (local rank 0's; measured at creation, IMT_SLICED_OPT_VERIFY_QUEUES).  The HIP runtime
     * multiplexes streams onto a few in-order hardware queues per priority level; wanted: the four round streams on four
     * different queues, slot i's collective stream on a queue of its own (IMT_SLICED_OPT_COMM_PLACEMENT; else on round stream
     * i's), its apply stream on round stream i's queue.  queue_map[k][slot] = hardware
     * queue class (0 .. hw_queues - 1, numbered by first use) of slot's round (k = 0), collective (1) and apply (2)
     * stream; 4 + slot = a queue of its own in the rounds' pool (shared with no round stream and no other helper), -2 = a
     * queue of its own in another priority pool, -1 = no such stream or not measured. */
    int placement;                   /* IMT_SLICED_PLACEMENT_* */
    int hw_queues;                   /* distinct hardware queues under the four round streams (4 wanted) */
    int comm_streams;                /* streams carrying collectives after placement (0: the round streams do) */
    int streams_recreated;           /* streams that had to be created again to get the placement */
    int queue_map[3][IMT_SLICED_ROUNDS];
    int pools;                       /* IMT_SLICED_OPT_POOLS as resolved: 1 = rounds HIGH / collectives LOW / RCCL and the host normal */
} imt_sliced_info;
#define IMT_SLICED_PLACEMENT_UNVERIFIED 0  /* not measured (option off, or unequal round priorities) */
#define IMT_SLICED_PLACEMENT_AS_CREATED 1  /* measured: as wanted, first try */
#define IMT_SLICED_PLACEMENT_REPAIRED 2    /* measured: as wanted after re-creating streams_recreated streams */
#define IMT_SLICED_PLACEMENT_DEGRADED 3    /* could not be had: collectives (applies) run on the round streams and / or the
                                              round streams share queues; imt_sliced_last_error says which */
int imt_sliced_get_info(const imt_sliced *w, imt_sliced_info *out);
/* Where the world stands, as text (what IMT_ERR_TIMEOUT writes to stderr): the global tick issued, per rank and round
 * slot the first tick whose unit / apply has not completed on the device, the collectives still pending with their
 * channel.  Writes at most cap - 1 characters + NUL; returns the length of the full text.  For a host's own watchdog. */
int imt_sliced_dump(imt_sliced *w, char *out, size_t cap);
const char *imt_sliced_last_error(const imt_sliced *w);
/* flushes first.  A world that failed (IMT_ERR_TIMEOUT, IMT_ERR_INTERNAL) is not flushed; if its streams do not drain
 * within the watchdog's limit the call returns anyway and leaves the world's device memory and streams allocated -- see
 * IMT_ERR_TIMEOUT above for what the process should do next. */
void imt_sliced_destroy(imt_sliced *w);

/* The building blocks imt_sliced_* is made of (kept exported for hosts that bring their own scheduler; a host that calls
 * them owns the ordering rule above).  A slice is hashed unit by unit (unit 0 = its leaf hashes, unit 1 + l = level
 * l -> l + 1) on a stream the caller names; each unit leaves a PAYLOAD -- the nodes it wrote back to level l of the
 * stored tree as packed (node, value) pairs.  Device pointers only.
 *   prepare : vals = the step's values for the slices before this GPU's, its own, and those after, in step order
 *             (identical on every GPU).  Index work for all of them on the tree's side stream (sort, low-leaf
 *             search, merge into the sorted index), events + level tables for the own slice only; the hash-free
 *             outputs (low_index, is_largest, low_leaf, new_leaf) are written now.  Blocks until the values are
 *             checked: IMT_ERR_VALUE / IMT_ERR_NONCANONICAL / IMT_ERR_FULL as imt_itree_insert_batch, the same
 *             verdict on every GPU, tree and index unchanged.  On success the index holds the whole step and
 *             *slice_out names the slice (up to 4 may be open).  `out` pointers are kept until the last unit.  The
 *             slice's units are ordered behind every ordinary batch (imt_itree_insert_batch, pipelined or not) issued
 *             on the tree before.
 *   unit    : enqueue unit `unit` (0 .. depth, in order) of an open slice on hip_stream; payload (NULL = none
 *             wanted) receives imt_itree_slice_payload_bytes(n_own) bytes, stream-ordered.
 *   apply   : enqueue another GPU's payload for (slice of n insertions into a tree of size_before leaves, unit) on
 *             hip_stream: writes that unit's nodes into this replica.
 * After the last apply the caller synchronises the streams it passed before any other call on the tree.
 * imt_itree_root_lagged does not see slices (a slice's own last root is a mid-step root on every rank but the last). */
size_t imt_itree_slice_payload_bytes(size_t n);   /* the largest payload of a slice of n insertions (buffer size) */
/* bytes the payload of `unit` of a slice of n insertions into a tree of size_before leaves actually uses (<= the above):
 * 128 B of header + one (node, value) pair per node the level can hold under the leaves in use, at most one per
 * event -- what an all-gather of that unit has to move.  The same on every GPU (it depends on sizes only). */
size_t imt_itree_slice_unit_bytes(const imt_itree *t, uint64_t size_before, size_t n, unsigned unit);
int imt_itree_slice_prepare(imt_itree *t, const void *vals /*[n_before + n_own + n_after][32]*/, size_t n_before,
                            size_t n_own, size_t n_after, const imt_insert_out *out, unsigned flags, int *slice_out,
                            uint32_t *l0_out);
int imt_itree_slice_unit(imt_itree *t, int slice, unsigned unit, void *payload, void *hip_stream);
int imt_itree_slice_apply(imt_itree *t, uint64_t size_before, size_t n, unsigned unit, const void *payload,
                          void *hip_stream);
/* the same for the `count` payloads of one all-gather (payload r at gathered + r * stride, stride >= the bytes
 * imt_itree_slice_unit_bytes gives for every r that is not skipped); unit[r] < 0 = skip */
int imt_itree_slice_apply_gathered(imt_itree *t, const void *gathered, size_t stride, size_t count,
                                   const uint64_t *size_before /*[count]*/, const uint64_t *n /*[count]*/,
                                   const int32_t *unit /*[count]*/, void *hip_stream);

/* ---- e: multi-GPU helpers ------------------------------------------------------ */
/* Root of a depth-`depth` tree whose 2^k subtrees of height `sub_height` have the given
 * roots (k = log2(n_roots)); the levels above sub_height + k are extended with the
 * all-empty subtree hashes.  Used after the all-gather of per-GPU subtree roots. */
int imt_combine_subtree_roots(imt_ctx *ctx, const void *sub_roots /*[n_roots][32]*/, size_t n_roots,
                              unsigned sub_height, unsigned depth, void *root /*[32]*/,
                              unsigned flags);
/* Z[0..depth]: hash of the empty subtree of each height, Z[0] = H(0,0,0) */
int imt_zero_hashes(imt_ctx *ctx, unsigned depth, void *out /*[depth+1][32]*/, unsigned flags);

#ifdef __cplusplus
}
#endif
#endif /* IMT_H */
