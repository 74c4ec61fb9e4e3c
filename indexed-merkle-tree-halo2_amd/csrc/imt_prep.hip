// imt_prep.hip -- device kernels of the GPU batch preparation (see imt_prep.hpp).  Index and byte
// work only (no field arithmetic): bound by HBM latency, a few hundred microseconds per 2^16 batch.
// Sorting and merging use rocPRIM (AMD's device primitives) with a 256-bit comparator.
#include <algorithm>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "imt_prep.hpp"
#include "imt_prep_logic.hpp"
#include "imt_filter_logic.hpp"
#include "imt_rewind.hpp"

namespace imt {
namespace prep {
namespace {

constexpr int BLOCK = 256;
inline unsigned nblk(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

struct ValLess {                       // order leaf indices by the value they index
    const uint8_t* val;
    __device__ bool operator()(uint32_t a, uint32_t b) const {
        return lt256(val + (uint64_t)a * 32, val + (uint64_t)b * 32);
    }
};

struct alignas(16) W4 { uint32_t x, y, z, w; };
__device__ __forceinline__ void copy32(uint8_t* dst, const uint8_t* src) {
    const W4* s = reinterpret_cast<const W4*>(src);
    W4* d = reinterpret_cast<W4*>(dst);
    d[0] = s[0];
    d[1] = s[1];
}
__device__ __forceinline__ void zero32(uint8_t* dst) {
    W4* d = reinterpret_cast<W4*>(dst);
    d[0] = W4{0, 0, 0, 0};
    d[1] = W4{0, 0, 0, 0};
}
__device__ __forceinline__ void put_u64(uint8_t* dst, uint64_t v) {
    W4* d = reinterpret_cast<W4*>(dst);
    d[0] = W4{(uint32_t)v, (uint32_t)(v >> 32), 0, 0};
    d[1] = W4{0, 0, 0, 0};
}

// p, little-endian 64-bit limbs
__device__ __forceinline__ bool geq_p(const uint8_t* v) {
    const uint64_t P[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
    const uint64_t* x = reinterpret_cast<const uint64_t*>(v);
    for (int i = 3; i >= 0; i--)
        if (x[i] != P[i]) return x[i] > P[i];
    return true;
}

__global__ void __launch_bounds__(BLOCK) k_scatter(const uint8_t* __restrict__ vals, uint8_t* __restrict__ d_val,
                                                   uint32_t M, uint32_t n, uint32_t part_mod, uint32_t part_res,
                                                   uint32_t* __restrict__ iota, int* err) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* v = vals + (uint64_t)i * 32;
    const uint64_t* x = reinterpret_cast<const uint64_t*>(v);
    if (geq_p(v)) atomicOr(err, ERR_NONCANONICAL);
    if ((x[0] | x[1] | x[2] | x[3]) == 0) atomicOr(err, ERR_ZERO);
    if (part_mod > 1 && mod_small(v, part_mod) != part_res) atomicOr(err, ERR_FOREIGN);
    copy32(d_val + (uint64_t)(M + i) * 32, v);
    iota[i] = M + i;
}

// k_scatter for values that are rows [M, M + n) of d_val already (run() with vals == NULL): nothing of d_val is written
__global__ void __launch_bounds__(BLOCK) k_iota(uint32_t M, uint32_t n, uint32_t* __restrict__ iota) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) iota[i] = M + i;
}

__global__ void __launch_bounds__(BLOCK) k_gap(const uint8_t* __restrict__ d_val, const uint32_t* __restrict__ sorted_old,
                                               uint32_t M, const uint32_t* __restrict__ bsorted, uint32_t n,
                                               uint32_t* __restrict__ gap, uint32_t* __restrict__ st0, int* err) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t* x = d_val + (uint64_t)bsorted[j] * 32;
    const uint32_t g = count_below(d_val, sorted_old, M, x);
    gap[j] = g;
    st0[j] = bsorted[j] - M;                                  // insertion time of the j-th smallest new value
    if (g < M && eq256(d_val + (uint64_t)sorted_old[g] * 32, x)) atomicOr(err, ERR_DUPLICATE);
    if (j + 1 < n && eq256(d_val + (uint64_t)bsorted[j + 1] * 32, x)) atomicOr(err, ERR_DUPLICATE);
}

__global__ void __launch_bounds__(BLOCK) k_sparse_level(uint32_t* __restrict__ st, uint32_t n, int k) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t w = 1u << k, h = w >> 1;
    if (j >= n || j + w > n) return;
    const uint32_t* prev = st + (uint64_t)(k - 1) * n;
    const uint32_t a = prev[j], b = prev[j + h];
    st[(uint64_t)k * n + j] = a < b ? a : b;
}

// low leaf and successor of every insertion, at the time it is inserted
__global__ void __launch_bounds__(BLOCK) k_neighbours(const uint32_t* __restrict__ st, int levels,
                                                      const uint32_t* __restrict__ bsorted,
                                                      const uint32_t* __restrict__ gap,
                                                      const uint32_t* __restrict__ sorted_old, uint32_t M, uint32_t n,
                                                      uint32_t* __restrict__ low, uint32_t* __restrict__ succ) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t g = gap[j], t = st[j];
    const uint32_t jl = nearest_smaller_left(st, n, levels, j);
    const uint32_t jr = nearest_smaller_right(st, n, levels, j);
    // a new neighbour counts only if no stored value lies between (same gap).  g >= 1 because the sentinel 0
    // is stored; g == 0 only for the rejected value 0 (ERR_ZERO is already set), keep the read in bounds.
    low[t] = (jl < n && gap[jl] == g) ? bsorted[jl] : sorted_old[g > 0 ? g - 1 : 0];
    succ[t] = (jr < n && gap[jr] == g) ? bsorted[jr] : (g < M ? sorted_old[g] : NONE);
}

// preimages at every time step (:650-656), event keys, and the hash-free outputs
__global__ void __launch_bounds__(BLOCK)
k_events(const uint8_t* __restrict__ d_val, uint32_t M, uint32_t n, uint64_t base, const uint32_t* __restrict__ low,
         const uint32_t* __restrict__ succ, uint8_t* __restrict__ pre, uint64_t* __restrict__ keys,
         uint64_t* __restrict__ o_low_index, uint8_t* __restrict__ o_is_largest, uint8_t* __restrict__ o_low_leaf,
         uint8_t* __restrict__ o_new_leaf) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t lo = low[i], su = succ[i];
    const uint8_t* v = d_val + (uint64_t)(M + i) * 32;
    const uint8_t* lv = d_val + (uint64_t)lo * 32;
    uint8_t* e0 = pre + (uint64_t)(2 * i) * 96;
    uint8_t* e1 = e0 + 96;
    copy32(e0, lv);                      // low leaf rewritten: {low.val, v, base+M+i}
    copy32(e0 + 32, v);
    put_u64(e0 + 64, base + M + i);      // `base`: the tree is a subtree of a deeper one (imt_itree_set_placement)
    copy32(e1, v);                       // new leaf inherits the low leaf's old pointers
    if (su != NONE) { copy32(e1 + 32, d_val + (uint64_t)su * 32); put_u64(e1 + 64, base + su); }
    else { zero32(e1 + 32); zero32(e1 + 64); }
    keys[2 * i] = ((uint64_t)lo << 32) | (uint64_t)(2 * i);
    keys[2 * i + 1] = ((uint64_t)(M + i) << 32) | (uint64_t)(2 * i + 1);
    if (o_low_index) o_low_index[i] = base + lo;
    if (o_is_largest) o_is_largest[i] = su == NONE ? 1 : 0;
    if (o_low_leaf) {                    // the low leaf BEFORE this insertion: {low.val, succ.val, succ.idx}
        uint8_t* o = o_low_leaf + (uint64_t)i * 96;
        copy32(o, lv);
        copy32(o + 32, e1 + 32);
        copy32(o + 64, e1 + 64);
    }
    if (o_new_leaf) {
        uint8_t* o = o_new_leaf + (uint64_t)i * 96;
        copy32(o, e1);
        copy32(o + 32, e1 + 32);
        copy32(o + 64, e1 + 64);
    }
}

// level-0 tables from the sorted keys: node, time and the run [rs, re) of equal positions
__global__ void __launch_bounds__(BLOCK) k_runs(const uint64_t* __restrict__ keys, uint32_t E, uint32_t* __restrict__ node,
                                                uint32_t* __restrict__ time, uint32_t* __restrict__ rs,
                                                uint32_t* __restrict__ re) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= E) return;
    const uint64_t key = keys[k];
    const uint32_t pos = (uint32_t)(key >> 32);
    node[k] = pos;
    time[k] = (uint32_t)key;
    const uint64_t lo_key = (uint64_t)pos << 32, hi_key = ((uint64_t)pos + 1) << 32;
    uint32_t lo = 0, hi = k;                        // first index with key >= lo_key
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (keys[mid] < lo_key) lo = mid + 1; else hi = mid; }
    rs[k] = lo;
    lo = k + 1; hi = E;                             // first index with key >= hi_key
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (keys[mid] < hi_key) lo = mid + 1; else hi = mid; }
    re[k] = lo;
}

// ---- bulk insertion (imt_itree_insert_bulk; the rule is bulk_row, imt_prep_logic.hpp) ----
// One event per value: row k rewrites its low leaf.  The new leaves' final preimages go to rows [n, 2n) of `pre` by the
// caller's position, where the append stage hashes them from.
__global__ void __launch_bounds__(BLOCK)
k_bulk_events(const uint8_t* __restrict__ d_val, const uint32_t* __restrict__ sorted_old, uint32_t M,
              const uint32_t* __restrict__ bsorted, const uint32_t* __restrict__ gap, uint32_t n, uint8_t* __restrict__ pre,
              uint64_t* __restrict__ keys, uint32_t* __restrict__ erow, BulkOut o) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const BulkRow r = bulk_row(sorted_old, M, bsorted, gap, n, j);
    const uint8_t* v = d_val + (uint64_t)bsorted[j] * 32;
    const uint8_t* lv = d_val + (uint64_t)r.low * 32;
    uint8_t* e0 = pre + (uint64_t)r.k * 96;                    // low leaf rewritten: {low.val, v, M + pos}
    copy32(e0, lv);
    copy32(e0 + 32, v);
    put_u64(e0 + 64, (uint64_t)M + r.pos);
    uint8_t* e1 = pre + ((uint64_t)n + r.pos) * 96;            // the new leaf as the batch leaves it: {v, succ.val, succ.idx}
    copy32(e1, v);
    if (r.succ != OP_NONE) { copy32(e1 + 32, d_val + (uint64_t)r.succ * 32); put_u64(e1 + 64, r.succ); }
    else { zero32(e1 + 32); zero32(e1 + 64); }
    keys[r.k] = ((uint64_t)r.low << 32) | (uint64_t)r.k;
    erow[r.k] = (r.k << 2) | ROW_LOW;
    if (o.order) o.order[r.k] = r.pos;
    if (o.low_index) o.low_index[r.k] = r.low;
    if (o.is_largest) o.is_largest[r.k] = r.succ == OP_NONE ? 1 : 0;
    if (o.low_leaf) {                                          // before the rewrite: {low.val, succ.val, succ.idx}
        uint8_t* q = o.low_leaf + (uint64_t)r.k * 96;
        copy32(q, lv);
        copy32(q + 32, e1 + 32);
        copy32(q + 64, e1 + 64);
    }
    if (o.new_leaf) {
        uint8_t* q = o.new_leaf + (uint64_t)r.pos * 96;
        copy32(q, e1);
        copy32(q + 32, e1 + 32);
        copy32(q + 64, e1 + 64);
    }
}
// the level-0 table of the append: leaf M + i alone in its run, its preimage row n + i of `pre`
__global__ void __launch_bounds__(BLOCK) k_append_table(uint32_t M, uint32_t n, uint32_t* __restrict__ node,
                                                        uint32_t* __restrict__ time, uint32_t* __restrict__ rs,
                                                        uint32_t* __restrict__ re) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    node[i] = M + i;
    time[i] = n + i;
    rs[i] = i;
    re[i] = i + 1;
}

// ---- mixed batches (imt_itree_mixed_batch; the rules are in imt_prep_logic.hpp) ----
static_assert(OP_ZERO == ERR_ZERO && OP_DUPLICATE == ERR_DUPLICATE && OP_FOREIGN == ERR_FOREIGN && OP_ABSENT == ERR_ABSENT,
              "one set of error bits");
struct ValRankLess {                   // ValLess with equal values ordered by leaf index, i.e. by rank
    const uint8_t* val;
    __device__ bool operator()(uint32_t a, uint32_t b) const {
        const uint8_t *x = val + (uint64_t)a * 32, *y = val + (uint64_t)b * 32;
        return lt256(x, y) || (a < b && !lt256(y, x));
    }
};

// max_op: the greatest op byte the call takes -- OP_READ, OP_MEMBER under IMT_MEMBER_OPS
__global__ void __launch_bounds__(BLOCK) k_mixed_flag(const uint8_t* __restrict__ op, uint32_t n, uint8_t max_op,
                                                      uint32_t* __restrict__ flag, int* err) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint8_t o = op[p];
    if (o > max_op) atomicOr(err, ERR_OP);
    flag[p] = o == 0 ? 1u : 0u;
}
__global__ void k_mixed_count(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank, uint32_t n,
                              uint32_t* __restrict__ word) {
    word[0] = rank[n - 1] + flag[n - 1];
    word[1] = OP_NONE;
}
// every operation's value on its own; an INSERT's value goes to its row of d_val
__global__ void __launch_bounds__(BLOCK)
k_mixed_scatter(const uint8_t* __restrict__ vals, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                uint8_t* __restrict__ d_val, uint32_t M, uint32_t n, uint32_t part_mod, uint32_t part_res,
                uint32_t* __restrict__ iota, uint32_t* __restrict__ ipos, int* err, uint32_t* bad) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint8_t* v = vals + (uint64_t)p * 32;
    if (geq_p(v)) atomicOr(err, ERR_NONCANONICAL);
    const int e = op_value_class(v, part_mod, part_res);
    if (e) { atomicOr(err, e); atomicMin(bad, p); }
    if (!flag[p]) return;
    const uint32_t r = rank[p];
    copy32(d_val + (uint64_t)(M + r) * 32, v);
    iota[r] = M + r;
    ipos[r] = p;
}
// k_mixed_scatter for a list replayed against the tree (imt_itree_view_mixed_witness): no row of d_val is written, not
// even with the bytes it holds -- an INSERT's value is compared with the row it went to instead (replay_op_class)
__global__ void __launch_bounds__(BLOCK)
k_mixed_match(const uint8_t* __restrict__ vals, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
              const uint8_t* __restrict__ d_val, uint32_t S, uint32_t n, uint32_t part_mod, uint32_t part_res,
              uint32_t* __restrict__ iota, uint32_t* __restrict__ ipos, int* err, uint32_t* bad) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint8_t* v = vals + (uint64_t)p * 32;
    if (geq_p(v)) atomicOr(err, ERR_NONCANONICAL);
    const bool ins = flag[p];
    const uint32_t r = rank[p];
    const int e = replay_op_class(v, ins, r, d_val, S, part_mod, part_res);
    if (e) { atomicOr(err, e); atomicMin(bad, p); }
    if (!ins) return;
    iota[r] = S + r;
    ipos[r] = p;
}
// k_gap for the INSERTs of a mixed batch: the duplicate is named
__global__ void __launch_bounds__(BLOCK)
k_mixed_gap(const uint8_t* __restrict__ d_val, const uint32_t* __restrict__ sorted_old, uint32_t M,
            const uint32_t* __restrict__ bsorted, uint32_t n_ins, const uint32_t* __restrict__ ipos,
            uint32_t* __restrict__ gap, uint32_t* __restrict__ st0, int* err, uint32_t* bad) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_ins) return;
    const uint32_t g = count_below(d_val, sorted_old, M, d_val + (uint64_t)bsorted[j] * 32);
    gap[j] = g;
    st0[j] = bsorted[j] - M;
    if (insert_is_duplicate(d_val, sorted_old, M, bsorted, j, g)) { atomicOr(err, ERR_DUPLICATE); atomicMin(bad, ipos[bsorted[j] - M]); }
}
// low leaf and successor of every READ, as of its place in the batch: behind the INSERTs' in low / succ.  A MEMBER's are
// the leaf that holds its value and that leaf's successor (member_neighbours): the same two words, the verdict inverted.
__global__ void __launch_bounds__(BLOCK)
k_mixed_reads(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ op, const uint32_t* __restrict__ flag,
              const uint32_t* __restrict__ rank, const uint8_t* __restrict__ d_val, const uint32_t* __restrict__ sorted_old, uint32_t M,
              const uint32_t* __restrict__ bsorted, const uint32_t* __restrict__ gap, const uint32_t* __restrict__ st,
              uint32_t n, uint32_t n_ins, int levels, uint32_t part_mod, uint32_t part_res, uint32_t* __restrict__ low,
              uint32_t* __restrict__ succ, int* err, uint32_t* bad) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n || flag[p]) return;
    const uint32_t R = rank[p], q = p - R;
    const uint8_t* x = vals + (uint64_t)p * 32;
    const ReadAnswer a = op[p] == OP_MEMBER
                             ? member_neighbours(x, R, d_val, sorted_old, M, bsorted, gap, st, n_ins, levels, part_mod, part_res)
                             : read_neighbours(x, R, d_val, sorted_old, M, bsorted, gap, st, n_ins, levels, part_mod, part_res);
    if (a.err) { atomicOr(err, a.err); atomicMin(bad, p); }
    low[n_ins + q] = a.low;
    succ[n_ins + q] = a.succ;
}
// k_events over the operations: an INSERT's two events as there, a READ's one -- the low leaf's preimage as of the READ,
// which is what that leaf holds then, so hashing it rewrites the leaf with its own bytes
__global__ void __launch_bounds__(BLOCK)
k_mixed_events(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank, const uint8_t* __restrict__ d_val,
               uint32_t M, uint32_t n, uint32_t n_ins, uint64_t base, const uint32_t* __restrict__ low,
               const uint32_t* __restrict__ succ, uint8_t* __restrict__ pre, uint64_t* __restrict__ keys,
               uint32_t* __restrict__ erow, uint64_t* __restrict__ o_low_index, uint8_t* __restrict__ o_is_largest,
               uint8_t* __restrict__ o_low_leaf, uint8_t* __restrict__ o_new_leaf, ReadOut rd) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = rank[p], e = p + r;
    const bool ins = flag[p];
    const uint32_t row = ins ? r : p - r, at = ins ? r : n_ins + row;
    const uint32_t lo = low[at], su = succ[at];
    const uint8_t* lv = d_val + (uint64_t)lo * 32;
    uint8_t* e0 = pre + (uint64_t)e * 96;
    copy32(e0, lv);
    keys[e] = ((uint64_t)lo << 32) | (uint64_t)e;
    // {succ.val, succ.idx}, what the low leaf points at before the operation: a READ's event keeps it, an INSERT's new leaf
    // inherits it
    uint8_t* nxt = ins ? e0 + 96 + 32 : e0 + 32;
    if (su != NONE) { copy32(nxt, d_val + (uint64_t)su * 32); put_u64(nxt + 32, base + su); }
    else { zero32(nxt); zero32(nxt + 32); }
    if (ins) {
        const uint8_t* v = d_val + (uint64_t)(M + r) * 32;
        uint8_t* e1 = e0 + 96;
        copy32(e0 + 32, v);
        put_u64(e0 + 64, base + M + r);
        copy32(e1, v);
        keys[e + 1] = ((uint64_t)(M + r) << 32) | (uint64_t)(e + 1);
        erow[e] = (r << 2) | ROW_LOW;
        erow[e + 1] = (r << 2) | ROW_NEW;
        if (o_new_leaf) {
            uint8_t* o = o_new_leaf + (uint64_t)r * 96;
            copy32(o, e1);
            copy32(o + 32, e1 + 32);
            copy32(o + 64, e1 + 64);
        }
    } else {
        erow[e] = (row << 2) | ROW_READ;
    }
    uint64_t* oi = ins ? o_low_index : rd.low_index;
    uint8_t* og = ins ? o_is_largest : rd.is_largest;
    uint8_t* ol = ins ? o_low_leaf : rd.low_leaf;
    if (oi) oi[row] = base + lo;
    if (og) og[row] = su == NONE ? 1 : 0;
    if (ol) {                            // the low leaf before the operation: {low.val, succ.val, succ.idx}
        uint8_t* o = ol + (uint64_t)row * 96;
        copy32(o, lv);
        copy32(o + 32, nxt);
        copy32(o + 64, nxt + 32);
    }
}

// the events of the INSERTs alone (imt_itree_apply_mixed): what k_events writes for an insertion-only batch of the same
// values, from the neighbours the mixed checks left by rank.  A READ has no event here.
__global__ void __launch_bounds__(BLOCK)
k_insert_events(const uint8_t* __restrict__ d_val, uint32_t M, uint32_t n_ins, uint64_t base, const uint32_t* __restrict__ low,
                const uint32_t* __restrict__ succ, uint8_t* __restrict__ pre, uint64_t* __restrict__ keys) {
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_ins) return;
    const InsertEvent e = insert_event(r, M, low, succ);
    insert_event_preimages(e, d_val, base, pre + (uint64_t)(2 * r) * 96);
    keys[2 * r] = e.key_low;
    keys[2 * r + 1] = e.key_new;
}

__global__ void __launch_bounds__(BLOCK) k_find_low(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ d_val,
                                                    const uint32_t* __restrict__ sorted, uint32_t M, uint32_t n,
                                                    uint64_t base, uint32_t part_mod, uint32_t part_res,
                                                    uint64_t* __restrict__ low_index, int* err) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* x = vals + (uint64_t)i * 32;
    if (geq_p(x)) atomicOr(err, ERR_NONCANONICAL);
    if (part_mod > 1 && mod_small(x, part_mod) != part_res) atomicOr(err, ERR_FOREIGN);
    const uint32_t g = count_below(d_val, sorted, M, x);
    if (g == 0) { atomicOr(err, ERR_ZERO); low_index[i] = base; return; }
    if (g < M && eq256(d_val + (uint64_t)sorted[g] * 32, x)) atomicOr(err, ERR_DUPLICATE);
    low_index[i] = base + sorted[g - 1];
}

__global__ void __launch_bounds__(BLOCK)
k_nm_witness(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ d_val, const uint32_t* __restrict__ sorted,
             uint32_t M, uint32_t n, uint64_t base, uint32_t part_mod, uint32_t part_res, uint64_t* __restrict__ low_index,
             uint8_t* __restrict__ low_leaf, uint8_t* __restrict__ is_largest, int* err) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* x = vals + (uint64_t)i * 32;
    if (geq_p(x)) atomicOr(err, ERR_NONCANONICAL);
    // a value of another subtree's residue is absent from THIS list whether or not the tree holds it
    if (part_mod > 1 && mod_small(x, part_mod) != part_res) atomicOr(err, ERR_FOREIGN);
    uint32_t g = count_below(d_val, sorted, M, x);
    if (g == 0) { atomicOr(err, ERR_ZERO); g = 1; }
    if (g < M && eq256(d_val + (uint64_t)sorted[g] * 32, x)) atomicOr(err, ERR_DUPLICATE);
    const uint32_t lo = sorted[g - 1];
    if (low_index) low_index[i] = base + lo;
    if (is_largest) is_largest[i] = g == M ? 1 : 0;
    if (low_leaf) {        // the stored list: a leaf points at its successor in value order
        uint8_t* o = low_leaf + (uint64_t)i * 96;
        copy32(o, d_val + (uint64_t)lo * 32);
        if (g < M) { copy32(o + 32, d_val + (uint64_t)sorted[g] * 32); put_u64(o + 64, base + sorted[g]); }
        else { zero32(o + 32); zero32(o + 64); }
    }
}

// ---- filtered insertion and lookup (imt_filter_logic.hpp) ----
struct PosLess {                       // order input positions by value, then position
    const uint8_t* vals;
    __device__ bool operator()(uint32_t a, uint32_t b) const { return pos_less(vals, a, b); }
};

__global__ void __launch_bounds__(BLOCK) k_filter_class(const uint8_t* __restrict__ vals, uint32_t n, uint32_t part_mod,
                                                        uint32_t part_res, uint32_t* __restrict__ idx,
                                                        uint8_t* __restrict__ st, int* err) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* v = vals + (uint64_t)i * 32;
    if (geq_p(v)) atomicOr(err, ERR_NONCANONICAL);
    st[i] = filter_class(v, part_mod, part_res);
    idx[i] = i;
}

// over the batch order: PRESENT against the stored index, REPEATED against the head of the run
__global__ void __launch_bounds__(BLOCK) k_filter_rank(const uint8_t* __restrict__ vals, const uint32_t* __restrict__ ord,
                                                       uint32_t n, const uint8_t* __restrict__ d_val,
                                                       const uint32_t* __restrict__ sorted, uint32_t M,
                                                       uint8_t* __restrict__ st, uint32_t* __restrict__ aux,
                                                       uint32_t* __restrict__ flag) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = ord[j];
    uint32_t a = 0;
    const uint8_t s = filter_rank(vals, ord, j, st[i], d_val, sorted, M, &a);
    st[i] = s;
    aux[i] = a;
    flag[i] = s == VAL_NEW ? 1u : 0u;
}

__global__ void __launch_bounds__(BLOCK) k_filter_compact(const uint8_t* __restrict__ vals, uint32_t n,
                                                          const uint8_t* __restrict__ st, const uint32_t* __restrict__ aux,
                                                          const uint32_t* __restrict__ flag,
                                                          const uint32_t* __restrict__ rank, uint64_t base, uint32_t M,
                                                          uint8_t* __restrict__ acc, uint8_t* __restrict__ status,
                                                          uint64_t* __restrict__ leaf, uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t s = st[i];
    if (s == VAL_NEW) copy32(acc + (uint64_t)rank[i] * 32, vals + (uint64_t)i * 32);
    status[i] = s;
    if (leaf) leaf[i] = filter_leaf(s, aux[i], rank, i, base, M);
    if (i + 1 == n) *count = rank[i] + flag[i];
}

// ---- filtered mixed batches (imt_itree_mixed_filtered; the rule is in imt_filter_logic.hpp) ----
struct MixedPosLess {                  // order positions by value, INSERT before READ, then position
    const uint8_t* vals;
    const uint8_t* op;
    __device__ bool operator()(uint32_t a, uint32_t b) const { return mixed_pos_less(vals, op, a, b); }
};

__global__ void __launch_bounds__(BLOCK) k_mixed_filter_class(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ op,
                                                              uint32_t n, uint8_t max_op, uint32_t* __restrict__ idx,
                                                              uint8_t* __restrict__ st, int* err) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* v = vals + (uint64_t)i * 32;
    if (geq_p(v)) atomicOr(err, ERR_NONCANONICAL);
    if (op[i] > max_op) atomicOr(err, ERR_OP);
    st[i] = filter_class(v, 0, 0);
    idx[i] = i;
}

// over the batch order: PRESENT against the stored index, REPEATED against the head of the run; the accepted flags by kind
// (flag_rd: the READs and the MEMBERs, which share the rows of rd)
__global__ void __launch_bounds__(BLOCK)
k_mixed_filter_rank(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ op, const uint32_t* __restrict__ ord, uint32_t n,
                    const uint8_t* __restrict__ d_val, const uint32_t* __restrict__ sorted, uint32_t M, uint8_t* __restrict__ st,
                    uint32_t* __restrict__ aux, uint32_t* __restrict__ flag_ins, uint32_t* __restrict__ flag_rd) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = ord[j];
    uint32_t a = 0;
    const uint8_t s = mixed_filter_rank(vals, op, ord, j, st[i], d_val, sorted, M, &a);
    const uint8_t o = op[i];
    st[i] = s;
    aux[i] = a;
    flag_ins[i] = (o == OP_INSERT && mixed_carried(o, s)) ? 1u : 0u;
    flag_rd[i] = (o != OP_INSERT && mixed_carried(o, s)) ? 1u : 0u;
}

// input order: status, the leaf of everything but an accepted READ (a MEMBER's is known here: the leaf that holds its
// value), the accepted operations side by side, the counts
__global__ void __launch_bounds__(BLOCK)
k_mixed_filter_compact(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ op, uint32_t n, const uint8_t* __restrict__ st,
                       const uint32_t* __restrict__ aux, const uint32_t* __restrict__ flag_ins,
                       const uint32_t* __restrict__ rank_ins, const uint32_t* __restrict__ flag_rd,
                       const uint32_t* __restrict__ rank_rd, uint64_t base, uint32_t M, uint8_t* __restrict__ acc,
                       uint8_t* __restrict__ aop, uint32_t* __restrict__ apos, uint8_t* __restrict__ status,
                       uint64_t* __restrict__ leaf, uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t s = st[i], o = op[i];
    const bool carried = mixed_carried(o, s);
    if (carried) {
        const uint32_t k = rank_ins[i] + rank_rd[i];
        copy32(acc + (uint64_t)k * 32, vals + (uint64_t)i * 32);
        aop[k] = o;
        apos[k] = i;
    }
    status[i] = s;
    if (leaf && !(carried && o == OP_READ)) leaf[i] = mixed_filter_op_leaf(o, s, aux[i], rank_ins, i, base, M);
    if (i + 1 == n) {
        count[0] = rank_ins[i] + flag_ins[i];
        count[1] = rank_rd[i] + flag_rd[i];
    }
}

// behind mixed_check of the accepted operations: an accepted READ reports its low leaf (rank: INSERTs before operation k)
__global__ void __launch_bounds__(BLOCK)
k_mixed_filter_reads(const uint8_t* __restrict__ aop, const uint32_t* __restrict__ apos, const uint32_t* __restrict__ rank,
                     const uint32_t* __restrict__ low, uint32_t n_acc, uint32_t n_ins, uint64_t base, uint64_t* __restrict__ leaf) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n_acc || aop[k] != OP_READ) return;
    leaf[apos[k]] = base + low[n_ins + (k - rank[k])];
}

__global__ void __launch_bounds__(BLOCK) k_lookup(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ d_val,
                                                  const uint32_t* __restrict__ sorted, uint32_t M, uint32_t n, uint64_t base,
                                                  uint32_t part_mod, uint32_t part_res, uint8_t* __restrict__ status,
                                                  uint64_t* __restrict__ leaf, int* err) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* x = vals + (uint64_t)i * 32;
    if (geq_p(x)) atomicOr(err, ERR_NONCANONICAL);
    uint64_t l = 0;
    status[i] = lookup_one(x, d_val, sorted, M, base, part_mod, part_res, &l);
    if (leaf) leaf[i] = l;
}

// ---- snapshot: imt_itree_load's list check and imt_itree_get_leaves, on the device ----
struct PreLess {                       // order leaf indices by the val field of their [3][32] preimage
    const uint8_t* pre;
    __device__ bool operator()(uint32_t a, uint32_t b) const {
        return lt256(pre + (uint64_t)a * 96, pre + (uint64_t)b * 96);
    }
};

__global__ void __launch_bounds__(BLOCK) k_load_keys(const uint8_t* __restrict__ pre, uint32_t n, uint32_t part_mod,
                                                     uint32_t part_res, uint64_t* __restrict__ keys,
                                                     uint32_t* __restrict__ idx, int* err) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = pre + (uint64_t)i * 96;
    if (geq_p(p) || geq_p(p + 32) || geq_p(p + 64)) atomicOr(err, ERR_NONCANONICAL);
    if (part_mod > 1 && i > 0 && mod_small(p, part_mod) != part_res) atomicOr(err, ERR_FOREIGN);
    keys[i] = reinterpret_cast<const uint64_t*>(p)[3];
    idx[i] = i;
}

__global__ void __launch_bounds__(BLOCK) k_load_check(const uint8_t* __restrict__ pre, uint32_t n, uint64_t base,
                                                      const uint32_t* __restrict__ idx, int* err, uint32_t* bad) {
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    const int e = load_check_rank(pre, n, base, idx, r);
    if (e) {
        atomicOr(err, e);
        if (e & LOAD_LINK) atomicMin(bad, idx[r]);
    }
}

__global__ void __launch_bounds__(BLOCK) k_load_commit(const uint8_t* __restrict__ pre, uint32_t n,
                                                       uint8_t* __restrict__ d_val) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    copy32(d_val + (uint64_t)i * 32, pre + (uint64_t)i * 96);
}

// preimage {val, next_val, next_idx} of leaves: the successor of a stored value is the next one in value order
__global__ void __launch_bounds__(BLOCK) k_leaves(const uint64_t* __restrict__ index, uint64_t first, uint32_t n,
                                                  const uint8_t* __restrict__ d_val, const uint32_t* __restrict__ sorted,
                                                  uint32_t M, uint64_t cap, uint64_t base, uint8_t* __restrict__ out,
                                                  int* err) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t li = (index ? index[i] : first + i) - base;     // wraps below the base: out of range
    uint8_t* o = out + (uint64_t)i * 96;
    if (li >= cap) atomicOr(err, ERR_RANGE);
    if (li >= M) { zero32(o); zero32(o + 32); zero32(o + 64); return; }
    const uint8_t* x = d_val + li * 32;
    const uint32_t r = count_below(d_val, sorted, M, x);            // its rank: sorted[r] == li
    copy32(o, x);
    if (r + 1 < M) { const uint32_t su = sorted[r + 1]; copy32(o + 32, d_val + (uint64_t)su * 32); put_u64(o + 64, base + su); }
    else { zero32(o + 32); zero32(o + 64); }
}

// ---- value log: imt_itree_load_values' check and commit (the rule is in imt_prep_logic.hpp) ----
struct LvPosLess {                     // order positions by value, then position
    const uint8_t* vals;
    __device__ bool operator()(uint32_t a, uint32_t b) const { return lv_pos_less(vals, a, b); }
};

__global__ void __launch_bounds__(BLOCK) k_lv_keys(const uint8_t* __restrict__ vals, uint32_t n, uint64_t* __restrict__ keys,
                                                   uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    keys[i] = reinterpret_cast<const uint64_t*>(vals + (uint64_t)i * 32)[3];
    idx[i] = i;
}

__global__ void __launch_bounds__(BLOCK) k_lv_check(const uint8_t* __restrict__ vals, uint32_t n, uint32_t part_mod,
                                                    uint32_t part_res, const uint32_t* __restrict__ ord, int* err,
                                                    uint32_t* bad) {
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    const int e = load_values_rank(vals, ord, r, part_mod, part_res);
    if (e) {
        atomicOr(err, e);
        if (e & ~LOAD_TIE) atomicMin(bad, ord[r]);
    }
}

__global__ void __launch_bounds__(BLOCK) k_first_noncanonical(const uint8_t* __restrict__ raw, uint32_t n, int* err,
                                                              uint32_t* bad) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (geq_p(raw + (uint64_t)i * 32)) {
        atomicOr(err, ERR_NONCANONICAL);
        atomicMin(bad, i);
    }
}

// thread i writes row i of d_val and entry i of the index, i = 0 .. n: both have n + 1 entries
__global__ void __launch_bounds__(BLOCK) k_lv_commit(const uint8_t* __restrict__ vals, const uint32_t* __restrict__ ord,
                                                     uint32_t n, uint8_t* __restrict__ d_val, uint32_t* __restrict__ sorted) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    if (i == 0) { zero32(d_val); sorted[0] = 0; return; }
    copy32(d_val + (uint64_t)i * 32, vals + (uint64_t)(i - 1) * 32);
    sorted[i] = ord[i - 1] + 1;
}

int levels_for(uint32_t n) {
    int k = 1;
    while ((1u << k) <= n) k++;
    return k;   // table rows 0 .. k-1, 2^(k-1) <= n
}

// ---- the lists of imt_itree_apply_batch (imt_apply.hpp) ----
struct HeadFlag {
    const uint32_t* node;
    unsigned l;
    __device__ uint32_t operator()(uint32_t x) const { return apply::head(node, x, l); }
};
typedef rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, HeadFlag, uint32_t> HeadIter;
inline HeadIter head_iter(const uint32_t* node, unsigned l) {
    return HeadIter(rocprim::counting_iterator<uint32_t>(0), HeadFlag{node, l});
}
size_t apply_scan_bytes(size_t total) {
    size_t a = 0;
    (void)rocprim::exclusive_scan(nullptr, a, head_iter(nullptr, 0), (uint32_t*)nullptr, 0u, total, rocprim::plus<uint32_t>(),
                                  nullptr);
    return a;
}
// blockIdx.y = level: every slot of every level in one launch
__global__ void __launch_bounds__(BLOCK) k_apply_scatter(const uint32_t* __restrict__ node, const uint32_t* __restrict__ time,
                                                         const uint32_t* __restrict__ re, uint32_t total, unsigned l0,
                                                         unsigned depth, const uint32_t* __restrict__ pos, apply::Lists o) {
    const uint32_t x = blockIdx.x * BLOCK + threadIdx.x;
    if (x >= total) return;
    const unsigned l = blockIdx.y;
    apply::scatter_element(node, time, re, total, x, l, pos[(size_t)l * o.stride + x], l0, depth, o);
}


// ---- going back (imt_itree_rewind, imt_rewind.hpp): 4 .. 36 bytes per index entry, no field arithmetic ----
struct RewindFlag {
    const uint32_t* sorted;
    uint32_t M, s;
    __device__ uint64_t operator()(uint32_t j) const { return rewind::scan_flag(sorted, M, j, s); }
};
typedef rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, RewindFlag, uint64_t> RewindIter;
inline RewindIter rewind_iter(const uint32_t* sorted, uint32_t M, uint32_t s) {
    return RewindIter(rocprim::counting_iterator<uint32_t>(0), RewindFlag{sorted, M, s});
}
size_t rewind_tmp_bytes(size_t M, size_t rows) {
    size_t a = 0, b = 0;
    (void)rocprim::exclusive_scan(nullptr, a, rewind_iter(nullptr, 0, 0), (uint64_t*)nullptr, (uint64_t)0, M,
                                  rocprim::plus<uint64_t>(), nullptr);
    (void)rocprim::radix_sort_pairs(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                    (uint32_t*)nullptr, rows, 0, 32, nullptr);
    return (a > b ? a : b) + 256;
}

__global__ void __launch_bounds__(BLOCK) k_rewind_compact(const uint32_t* __restrict__ sorted, uint32_t M, uint32_t s,
                                                          const uint64_t* __restrict__ pos, uint32_t* __restrict__ out,
                                                          uint32_t* __restrict__ n_relinked) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= M) return;
    rewind::compact_element(sorted, M, j, s, pos[j], out, n_relinked);
}

__global__ void __launch_bounds__(BLOCK) k_rewind_relink(const uint8_t* __restrict__ d_val, const uint32_t* __restrict__ sorted,
                                                         const uint32_t* __restrict__ compact, uint32_t M, uint32_t s,
                                                         const uint64_t* __restrict__ pos, uint64_t base, rewind::Table t) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= M) return;
    rewind::relink_element(d_val, sorted, compact, M, j, s, pos[j], base, t);
}

// blockIdx.y = level: the nodes the earlier tree does not fill are the empty subtree of their height again
__global__ void __launch_bounds__(BLOCK) k_rewind_refill(uint8_t* __restrict__ nodes, const uint64_t* __restrict__ off,
                                                         const uint64_t* __restrict__ len, const uint8_t* __restrict__ zero,
                                                         uint64_t s, uint64_t M) {
    const unsigned l = blockIdx.y;
    uint64_t lo, hi;
    rewind::refill_range(s, M, l, &lo, &hi);
    const uint64_t x = lo + (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= hi || x >= len[l]) return;
    copy32(nodes + (off[l] + x) * 32, zero + (size_t)l * 32);
}

}  // namespace

size_t rewind_ws_bytes(size_t M, size_t rows) { return (M * 8 + 255) / 256 * 256 + 256 + rewind_tmp_bytes(M, rows); }

namespace {
struct RewindLayout {
    uint64_t* pos;
    uint32_t* count;
    void* tmp;
    size_t tmp_bytes;
};
inline RewindLayout rewind_layout(void* ws, size_t ws_bytes, size_t M) {
    uint8_t* w = (uint8_t*)ws;
    const size_t p = (M * 8 + 255) / 256 * 256;
    return {(uint64_t*)w, (uint32_t*)(w + p), w + p + 256, ws_bytes - p - 256};
}
}  // namespace

hipError_t rewind_compact(hipStream_t st, void* ws, size_t ws_bytes, const uint32_t* sorted_old, uint32_t* sorted_new,
                          uint32_t M, uint32_t s, const uint32_t** n_relinked) {
    if (s == 0 || s >= M || rewind_ws_bytes(M, 1) > ws_bytes) return hipErrorInvalidValue;
    const RewindLayout w = rewind_layout(ws, ws_bytes, M);
    hipError_t e;
    (void)hipGetLastError();
    size_t tb = w.tmp_bytes;
    if ((e = rocprim::exclusive_scan(w.tmp, tb, rewind_iter(sorted_old, M, s), w.pos, (uint64_t)0, (size_t)M,
                                     rocprim::plus<uint64_t>(), st)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_rewind_compact, dim3(nblk(M)), dim3(BLOCK), 0, st, sorted_old, M, s, w.pos, sorted_new, w.count);
    *n_relinked = w.count;
    return hipGetLastError();
}

hipError_t rewind_table(hipStream_t st, void* ws, size_t ws_bytes, const uint8_t* d_val, const uint32_t* sorted_old,
                        const uint32_t* sorted_new, uint32_t M, uint32_t s, uint64_t base, uint32_t rows, uint32_t* key,
                        uint32_t* row, uint8_t* pre, uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re) {
    if (s == 0 || s >= M || rows == 0 || rows > s + 1 || rewind_ws_bytes(M, rows) > ws_bytes) return hipErrorInvalidValue;
    const RewindLayout w = rewind_layout(ws, ws_bytes, M);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_rewind_relink, dim3(nblk(M)), dim3(BLOCK), 0, st, d_val, sorted_old, sorted_new, M, s, w.pos, base,
                       rewind::Table{key, row, rs, re, pre, rows});
    size_t tb = w.tmp_bytes;
    hipError_t e;
    if ((e = rocprim::radix_sort_pairs(w.tmp, tb, key, node, row, time, (size_t)rows, 0, 32, st)) != hipSuccess) return e;
    return hipGetLastError();
}

void rewind_refill(hipStream_t st, uint8_t* nodes, const uint64_t* off, const uint64_t* len, const uint8_t* zero, uint64_t s,
                   uint64_t M, unsigned l0) {
    if (s >= M || l0 == 0) return;
    hipLaunchKernelGGL(k_rewind_refill, dim3(nblk(M - s), l0), dim3(BLOCK), 0, st, nodes, off, len, zero, s, M);
}

size_t apply_lists_tmp_bytes(size_t total) { return apply_scan_bytes(total) + 256; }

hipError_t apply_lists(hipStream_t s, void* tmp, size_t tmp_bytes, const uint32_t* node, const uint32_t* time,
                       const uint32_t* re, uint32_t total, unsigned l0, unsigned depth, uint32_t* pos,
                       const apply::Lists& lists) {
    hipError_t e;
    if (total == 0 || l0 == 0 || l0 > 31 || l0 > depth || total > lists.stride || apply_scan_bytes(total) > tmp_bytes)
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    for (unsigned l = 0; l < l0; l++) {
        size_t tb = tmp_bytes;
        if ((e = rocprim::exclusive_scan(tmp, tb, head_iter(node, l), pos + (size_t)l * lists.stride, 0u, (size_t)total,
                                         rocprim::plus<uint32_t>(), s)) != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(k_apply_scatter, dim3(nblk(total), l0), dim3(BLOCK), 0, s, node, time, re, total, l0, depth, pos, lists);
    return hipGetLastError();
}

size_t temp_bytes_needed(size_t n, size_t max_size) {
    size_t a = 0, b = 0, c = 0;
    (void)rocprim::merge_sort(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, n, ValLess{nullptr}, nullptr);
    (void)rocprim::merge(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, max_size, n,
                         ValLess{nullptr}, nullptr);
    (void)rocprim::radix_sort_keys(nullptr, c, (uint64_t*)nullptr, (uint64_t*)nullptr, 2 * n, 0, 64, nullptr);
    const size_t d = apply_scan_bytes(2 * n);       // the scans of apply_lists run over the 2n events
    size_t m = a > b ? a : b;
    m = m > c ? m : c;
    return (m > d ? m : d) + 256;
}

hipError_t run(hipStream_t s, Workspace& ws, const uint8_t* vals, uint8_t* d_val, const uint32_t* sorted_old,
               uint32_t* sorted_new, uint32_t M, uint32_t n, uint64_t base, uint8_t* pre, uint32_t* node, uint32_t* time,
               uint32_t* rs, uint32_t* re, uint64_t* o_low_index, uint8_t* o_is_largest, uint8_t* o_low_leaf,
               uint8_t* o_new_leaf) {
    const int levels = levels_for(n);
    hipError_t e;
    // the workspace was sized for (cap_n, tree capacity); a larger request must not run into it
    if (n > ws.cap_n || temp_bytes_needed(n, (size_t)M) > ws.tmp_bytes) return hipErrorInvalidValue;
    (void)hipGetLastError();       // the thread's sticky error may be a stale one from an unrelated earlier call
    if (vals)
        hipLaunchKernelGGL(k_scatter, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, d_val, M, n, ws.part_mod, ws.part_res, ws.iota,
                           ws.err);
    else
        hipLaunchKernelGGL(k_iota, dim3(nblk(n)), dim3(BLOCK), 0, s, M, n, ws.iota);
    size_t tb = ws.tmp_bytes;
    if ((e = rocprim::merge_sort(ws.tmp, tb, ws.iota, ws.bsorted, (size_t)n, ValLess{d_val}, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_gap, dim3(nblk(n)), dim3(BLOCK), 0, s, d_val, sorted_old, M, ws.bsorted, n, ws.gap, ws.st,
                       ws.err);
    for (int k = 1; k < levels; k++)
        hipLaunchKernelGGL(k_sparse_level, dim3(nblk(n)), dim3(BLOCK), 0, s, ws.st, n, k);
    hipLaunchKernelGGL(k_neighbours, dim3(nblk(n)), dim3(BLOCK), 0, s, ws.st, levels, ws.bsorted, ws.gap, sorted_old, M,
                       n, ws.low, ws.succ);
    hipLaunchKernelGGL(k_events, dim3(nblk(n)), dim3(BLOCK), 0, s, d_val, M, n, base, ws.low, ws.succ, pre, ws.keys,
                       o_low_index, o_is_largest, o_low_leaf, o_new_leaf);
    tb = ws.tmp_bytes;
    if ((e = rocprim::radix_sort_keys(ws.tmp, tb, ws.keys, ws.keys_sorted, (size_t)2 * n, 0, 64, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_runs, dim3(nblk(2 * (size_t)n)), dim3(BLOCK), 0, s, ws.keys_sorted, 2 * n, node, time, rs, re);
    tb = ws.tmp_bytes;
    if ((e = rocprim::merge(ws.tmp, tb, sorted_old, ws.bsorted, sorted_new, (size_t)M, (size_t)n, ValLess{d_val}, s)) !=
        hipSuccess)
        return e;
    return hipGetLastError();      // a failed launch anywhere in the sequence
}

hipError_t index_only(hipStream_t s, Workspace& ws, const uint8_t* vals, uint8_t* d_val, const uint32_t* sorted_old,
                      uint32_t* sorted_new, uint32_t M, uint32_t n) {
    hipError_t e;
    if (n > ws.cap_n || temp_bytes_needed(n, (size_t)M) > ws.tmp_bytes) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_scatter, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, d_val, M, n, ws.part_mod, ws.part_res, ws.iota,
                       ws.err);
    size_t tb = ws.tmp_bytes;
    if ((e = rocprim::merge_sort(ws.tmp, tb, ws.iota, ws.bsorted, (size_t)n, ValLess{d_val}, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_gap, dim3(nblk(n)), dim3(BLOCK), 0, s, d_val, sorted_old, M, ws.bsorted, n, ws.gap, ws.st,
                       ws.err);
    tb = ws.tmp_bytes;
    if ((e = rocprim::merge(ws.tmp, tb, sorted_old, ws.bsorted, sorted_new, (size_t)M, (size_t)n, ValLess{d_val}, s)) !=
        hipSuccess)
        return e;
    return hipGetLastError();
}

hipError_t bulk_check(hipStream_t s, Workspace& ws, const uint8_t* vals, uint8_t* d_val, const uint32_t* sorted_old, uint32_t M,
                      uint32_t n) {
    hipError_t e;
    if (n > ws.cap_n || temp_bytes_needed(n, (size_t)M) > ws.tmp_bytes) return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (vals)
        hipLaunchKernelGGL(k_scatter, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, d_val, M, n, ws.part_mod, ws.part_res, ws.iota,
                           ws.err);
    else
        hipLaunchKernelGGL(k_iota, dim3(nblk(n)), dim3(BLOCK), 0, s, M, n, ws.iota);
    size_t tb = ws.tmp_bytes;
    if ((e = rocprim::merge_sort(ws.tmp, tb, ws.iota, ws.bsorted, (size_t)n, ValLess{d_val}, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_gap, dim3(nblk(n)), dim3(BLOCK), 0, s, d_val, sorted_old, M, ws.bsorted, n, ws.gap, ws.st,
                       ws.err);
    return hipGetLastError();
}

hipError_t bulk_events(hipStream_t s, Workspace& ws, const uint8_t* d_val, const uint32_t* sorted_old, uint32_t* sorted_new,
                       uint32_t M, uint32_t n, uint8_t* pre, uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re,
                       uint32_t* erow, const BulkOut& o) {
    hipError_t e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_bulk_events, dim3(nblk(n)), dim3(BLOCK), 0, s, d_val, sorted_old, M, ws.bsorted, ws.gap, n, pre,
                       ws.keys, erow, o);
    size_t tb = ws.tmp_bytes;
    if ((e = rocprim::radix_sort_keys(ws.tmp, tb, ws.keys, ws.keys_sorted, (size_t)n, 0, 64, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_runs, dim3(nblk(n)), dim3(BLOCK), 0, s, ws.keys_sorted, n, node, time, rs, re);
    tb = ws.tmp_bytes;
    if ((e = rocprim::merge(ws.tmp, tb, sorted_old, ws.bsorted, sorted_new, (size_t)M, (size_t)n, ValLess{d_val}, s)) !=
        hipSuccess)
        return e;
    return hipGetLastError();
}

hipError_t append_table(hipStream_t s, uint32_t M, uint32_t n, uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re) {
    hipLaunchKernelGGL(k_append_table, dim3(nblk(n)), dim3(BLOCK), 0, s, M, n, node, time, rs, re);
    return hipGetLastError();
}

hipError_t mixed_ranks(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* op, uint32_t n, uint8_t max_op) {
    hipError_t e;
    size_t need = 0;
    (void)rocprim::exclusive_scan(nullptr, need, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(),
                                  nullptr);
    if (n == 0 || n > ws.cap_n || need > ws.tmp_bytes) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_mixed_flag, dim3(nblk(n)), dim3(BLOCK), 0, s, op, n, max_op, mx.flag, ws.err);
    size_t tb = ws.tmp_bytes;
    if ((e = rocprim::exclusive_scan(ws.tmp, tb, mx.flag, mx.rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_mixed_count, dim3(1), dim3(1), 0, s, mx.flag, mx.rank, n, mx.word);
    return hipGetLastError();
}

// the checks behind the first kernel of mixed_check / mixed_check_view: the INSERT values are rows [M, M + n_ins) of d_val
static hipError_t mixed_neighbours(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* vals, const uint8_t* op,
                                   const uint8_t* d_val, const uint32_t* sorted_old, uint32_t M, uint32_t n, uint32_t n_ins);

hipError_t mixed_check(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* vals, const uint8_t* op, uint8_t* d_val,
                       const uint32_t* sorted_old, uint32_t M, uint32_t n, uint32_t n_ins) {
    if (n == 0 || n > ws.cap_n || n_ins > n || temp_bytes_needed(n_ins, (size_t)M) > ws.tmp_bytes) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_mixed_scatter, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, mx.flag, mx.rank, d_val, M, n, ws.part_mod,
                       ws.part_res, ws.iota, mx.ipos, ws.err, mx.word + 1);
    return mixed_neighbours(s, ws, mx, vals, op, d_val, sorted_old, M, n, n_ins);
}

hipError_t mixed_check_view(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* vals, const uint8_t* op,
                            const uint8_t* d_val, const uint32_t* sorted_view, uint32_t S, uint32_t n, uint32_t n_ins) {
    static_assert(OP_MISMATCH == ERR_MISMATCH, "one set of error bits");
    if (n == 0 || n > ws.cap_n || n_ins > n || temp_bytes_needed(n_ins, (size_t)S) > ws.tmp_bytes) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_mixed_match, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, mx.flag, mx.rank, d_val, S, n, ws.part_mod,
                       ws.part_res, ws.iota, mx.ipos, ws.err, mx.word + 1);
    return mixed_neighbours(s, ws, mx, vals, op, d_val, sorted_view, S, n, n_ins);
}

static hipError_t mixed_neighbours(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* vals, const uint8_t* op,
                                   const uint8_t* d_val, const uint32_t* sorted_old, uint32_t M, uint32_t n, uint32_t n_ins) {
    const int levels = levels_for(n_ins);
    hipError_t e;
    if (n_ins) {
        size_t tb = ws.tmp_bytes;
        if ((e = rocprim::merge_sort(ws.tmp, tb, ws.iota, ws.bsorted, (size_t)n_ins, ValRankLess{d_val}, s)) != hipSuccess)
            return e;
        hipLaunchKernelGGL(k_mixed_gap, dim3(nblk(n_ins)), dim3(BLOCK), 0, s, d_val, sorted_old, M, ws.bsorted, n_ins, mx.ipos,
                           ws.gap, ws.st, ws.err, mx.word + 1);
        for (int k = 1; k < levels; k++)
            hipLaunchKernelGGL(k_sparse_level, dim3(nblk(n_ins)), dim3(BLOCK), 0, s, ws.st, n_ins, k);
        hipLaunchKernelGGL(k_neighbours, dim3(nblk(n_ins)), dim3(BLOCK), 0, s, ws.st, levels, ws.bsorted, ws.gap, sorted_old, M,
                           n_ins, ws.low, ws.succ);
    }
    if (n_ins < n)
        hipLaunchKernelGGL(k_mixed_reads, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, op, mx.flag, mx.rank, d_val, sorted_old, M,
                           ws.bsorted, ws.gap, ws.st, n, n_ins, levels, ws.part_mod, ws.part_res, ws.low, ws.succ, ws.err,
                           mx.word + 1);
    return hipGetLastError();
}

static hipError_t mixed_tables(hipStream_t s, Workspace& ws, const uint8_t* d_val, const uint32_t* sorted_old, uint32_t* sorted_new,
                               uint32_t M, uint32_t E, uint32_t n_ins, uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re);

hipError_t mixed_events(hipStream_t s, Workspace& ws, const MixedWs& mx, const uint8_t* d_val, const uint32_t* sorted_old,
                        uint32_t* sorted_new, uint32_t M, uint32_t n, uint32_t n_ins, uint64_t base, uint8_t* pre,
                        uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re, uint64_t* o_low_index,
                        uint8_t* o_is_largest, uint8_t* o_low_leaf, uint8_t* o_new_leaf, const ReadOut& rd) {
    if (n == 0 || n > ws.cap_n || n_ins > n) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_mixed_events, dim3(nblk(n)), dim3(BLOCK), 0, s, mx.flag, mx.rank, d_val, M, n, n_ins, base, ws.low,
                       ws.succ, pre, ws.keys, mx.erow, o_low_index, o_is_largest, o_low_leaf, o_new_leaf, rd);
    return mixed_tables(s, ws, d_val, sorted_old, sorted_new, M, n + n_ins, n_ins, node, time, rs, re);
}

hipError_t mixed_insert_events(hipStream_t s, Workspace& ws, const uint8_t* d_val, const uint32_t* sorted_old, uint32_t* sorted_new,
                               uint32_t M, uint32_t n_ins, uint64_t base, uint8_t* pre, uint32_t* node, uint32_t* time,
                               uint32_t* rs, uint32_t* re) {
    if (n_ins == 0 || n_ins > ws.cap_n) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_insert_events, dim3(nblk(n_ins)), dim3(BLOCK), 0, s, d_val, M, n_ins, base, ws.low, ws.succ, pre, ws.keys);
    return mixed_tables(s, ws, d_val, sorted_old, sorted_new, M, 2 * n_ins, n_ins, node, time, rs, re);
}

// behind the event kernel of either: the keys sorted, the level-0 tables from them, the INSERTs merged into the index
static hipError_t mixed_tables(hipStream_t s, Workspace& ws, const uint8_t* d_val, const uint32_t* sorted_old, uint32_t* sorted_new,
                               uint32_t M, uint32_t E, uint32_t n_ins, uint32_t* node, uint32_t* time, uint32_t* rs, uint32_t* re) {
    hipError_t e;
    size_t tb = ws.tmp_bytes;
    if ((e = rocprim::radix_sort_keys(ws.tmp, tb, ws.keys, ws.keys_sorted, (size_t)E, 0, 64, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_runs, dim3(nblk(E)), dim3(BLOCK), 0, s, ws.keys_sorted, E, node, time, rs, re);
    if (n_ins) {
        tb = ws.tmp_bytes;
        if ((e = rocprim::merge(ws.tmp, tb, sorted_old, ws.bsorted, sorted_new, (size_t)M, (size_t)n_ins, ValLess{d_val}, s)) !=
            hipSuccess)
            return e;
    }
    return hipGetLastError();
}

static size_t mixed_filter_temp_bytes(size_t n);
size_t filter_temp_bytes(size_t n) {
    size_t a = 0, b = 0;
    (void)rocprim::merge_sort(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, n, PosLess{nullptr}, nullptr);
    (void)rocprim::exclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(),
                                  nullptr);
    return std::max(std::max(a, b) + 256, mixed_filter_temp_bytes(n));      // one allocation serves both filters
}

hipError_t filter(hipStream_t s, FilterWs& ws, const uint8_t* vals, uint32_t n, const uint8_t* d_val,
                  const uint32_t* sorted, uint32_t M, uint64_t base, uint32_t part_mod, uint32_t part_res,
                  uint8_t* status, uint64_t* leaf, int* err) {
    hipError_t e;
    if (n == 0 || n > ws.cap_n || filter_temp_bytes(n) > ws.tmp_bytes) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_filter_class, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, n, part_mod, part_res, ws.idx, ws.st, err);
    size_t tb = ws.tmp_bytes;
    if ((e = rocprim::merge_sort(ws.tmp, tb, ws.idx, ws.ord, (size_t)n, PosLess{vals}, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_filter_rank, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, ws.ord, n, d_val, sorted, M, ws.st, ws.aux,
                       ws.flag);
    tb = ws.tmp_bytes;
    if ((e = rocprim::exclusive_scan(ws.tmp, tb, ws.flag, ws.rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), s)) !=
        hipSuccess)
        return e;
    hipLaunchKernelGGL(k_filter_compact, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, n, ws.st, ws.aux, ws.flag, ws.rank, base,
                       M, ws.acc, status, leaf, ws.count);
    return hipGetLastError();
}

static size_t mixed_filter_temp_bytes(size_t n) {
    size_t a = 0;
    (void)rocprim::merge_sort(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, n, MixedPosLess{nullptr, nullptr}, nullptr);
    return a + 256;
}

hipError_t mixed_filter(hipStream_t s, FilterWs& ws, const uint8_t* vals, const uint8_t* op, uint32_t n, uint8_t max_op,
                        const uint8_t* d_val, const uint32_t* sorted, uint32_t M, uint64_t base, uint8_t* status, uint64_t* leaf,
                        int* err) {
    hipError_t e;
    if (n == 0 || n > ws.cap_n || filter_temp_bytes(n) > ws.tmp_bytes || mixed_filter_temp_bytes(n) > ws.tmp_bytes)
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_mixed_filter_class, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, op, n, max_op, ws.idx, ws.st, err);
    size_t tb = ws.tmp_bytes;
    if ((e = rocprim::merge_sort(ws.tmp, tb, ws.idx, ws.ord, (size_t)n, MixedPosLess{vals, op}, s)) != hipSuccess) return e;
    // ws.idx has been sorted from and is free: it holds the accepted-READ flags, and ws.ord, read for the last time by the
    // rank kernel, their scan
    uint32_t *flag_rd = ws.idx, *rank_rd = ws.ord;
    hipLaunchKernelGGL(k_mixed_filter_rank, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, op, ws.ord, n, d_val, sorted, M, ws.st, ws.aux,
                       ws.flag, flag_rd);
    tb = ws.tmp_bytes;
    if ((e = rocprim::exclusive_scan(ws.tmp, tb, ws.flag, ws.rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), s)) != hipSuccess)
        return e;
    tb = ws.tmp_bytes;
    if ((e = rocprim::exclusive_scan(ws.tmp, tb, flag_rd, rank_rd, 0u, (size_t)n, rocprim::plus<uint32_t>(), s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_mixed_filter_compact, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, op, n, ws.st, ws.aux, ws.flag, ws.rank,
                       flag_rd, rank_rd, base, M, ws.acc, ws.aop, ws.apos, status, leaf, ws.count);
    return hipGetLastError();
}

hipError_t mixed_filter_reads(hipStream_t s, const FilterWs& ws, const Workspace& prep_ws, const MixedWs& mx, uint32_t n_acc,
                              uint32_t n_ins, uint64_t base, uint64_t* leaf) {
    if (n_acc == 0 || n_acc > ws.cap_n || n_ins > n_acc || !leaf) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_mixed_filter_reads, dim3(nblk(n_acc)), dim3(BLOCK), 0, s, ws.aop, ws.apos, mx.rank, prep_ws.low, n_acc,
                       n_ins, base, leaf);
    return hipGetLastError();
}

void lookup(hipStream_t s, const uint8_t* vals, const uint8_t* d_val, const uint32_t* sorted, uint32_t M, uint32_t n,
            uint64_t base, uint32_t part_mod, uint32_t part_res, uint8_t* status, uint64_t* leaf, int* err) {
    if (!n) return;
    hipLaunchKernelGGL(k_lookup, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, d_val, sorted, M, n, base, part_mod, part_res,
                       status, leaf, err);
}

void nm_witness(hipStream_t s, const uint8_t* vals, const uint8_t* d_val, const uint32_t* sorted, uint32_t M, uint32_t n,
                uint64_t base, uint32_t part_mod, uint32_t part_res, uint64_t* low_index, uint8_t* low_leaf,
                uint8_t* is_largest, int* err) {
    if (!n) return;
    hipLaunchKernelGGL(k_nm_witness, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, d_val, sorted, M, n, base, part_mod, part_res,
                       low_index, low_leaf, is_largest, err);
}

void find_low(hipStream_t s, const uint8_t* vals, const uint8_t* d_val, const uint32_t* sorted, uint32_t M, uint32_t n,
              uint64_t base, uint32_t part_mod, uint32_t part_res, uint64_t* low_index, int* err) {
    if (!n) return;
    hipLaunchKernelGGL(k_find_low, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, d_val, sorted, M, n, base, part_mod, part_res,
                       low_index, err);
}

size_t load_ws_bytes(size_t n) {
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                    (uint32_t*)nullptr, n, 0, 64, nullptr);
    (void)rocprim::merge_sort(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, n, PreLess{nullptr}, nullptr);
    const size_t r = (n + 63) / 64 * 64;
    return 2 * r * 8 + 2 * r * 4 + 256 + (a > b ? a : b) + 256;
}

hipError_t load_check(hipStream_t s, const uint8_t* pre, uint32_t n, uint64_t base, uint32_t part_mod, uint32_t part_res,
                      void* ws, size_t ws_bytes, bool full_sort, int* err, uint32_t** bad, const uint32_t** sorted) {
    if (load_ws_bytes(n) > ws_bytes) return hipErrorInvalidValue;
    const size_t r = ((size_t)n + 63) / 64 * 64;
    uint8_t* w = (uint8_t*)ws;
    uint64_t* keys = (uint64_t*)w;
    uint64_t* keys2 = keys + r;
    uint32_t* idx = (uint32_t*)(keys2 + r);
    uint32_t* idx2 = idx + r;
    *bad = idx2 + r;
    void* tmp = (uint8_t*)(*bad) + 256;
    size_t tb = ws_bytes - (size_t)((uint8_t*)tmp - w);
    hipError_t e;
    (void)hipGetLastError();
    if ((e = hipMemsetAsync(*bad, 0xff, 4, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_load_keys, dim3(nblk(n)), dim3(BLOCK), 0, s, pre, n, part_mod, part_res, keys, idx, err);
    if (full_sort) e = rocprim::merge_sort(tmp, tb, idx, idx2, (size_t)n, PreLess{pre}, s);
    else e = rocprim::radix_sort_pairs(tmp, tb, keys, keys2, idx, idx2, (size_t)n, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_load_check, dim3(nblk(n)), dim3(BLOCK), 0, s, pre, n, base, idx2, err, *bad);
    *sorted = idx2;
    return hipGetLastError();
}

void load_commit(hipStream_t s, const uint8_t* pre, uint32_t n, uint8_t* d_val) {
    if (!n) return;
    hipLaunchKernelGGL(k_load_commit, dim3(nblk(n)), dim3(BLOCK), 0, s, pre, n, d_val);
}

void leaves(hipStream_t s, const uint64_t* index, uint64_t first, uint32_t n, const uint8_t* d_val, const uint32_t* sorted,
            uint32_t M, uint64_t cap, uint64_t base, uint8_t* out, int* err) {
    if (!n) return;
    hipLaunchKernelGGL(k_leaves, dim3(nblk(n)), dim3(BLOCK), 0, s, index, first, n, d_val, sorted, M, cap, base, out, err);
}

size_t load_values_ws_bytes(size_t n) {
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                    (uint32_t*)nullptr, n, 0, 64, nullptr);
    (void)rocprim::merge_sort(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, n, LvPosLess{nullptr}, nullptr);
    const size_t r = (n + 63) / 64 * 64;
    return 2 * r * 8 + 2 * r * 4 + (a > b ? a : b) + 256;
}

hipError_t load_values_check(hipStream_t s, const uint8_t* vals, uint32_t n, uint32_t part_mod, uint32_t part_res, void* ws,
                             size_t ws_bytes, bool full_sort, int* err, uint32_t* bad, const uint32_t** order) {
    if (!n || load_values_ws_bytes(n) > ws_bytes) return hipErrorInvalidValue;
    const size_t r = ((size_t)n + 63) / 64 * 64;
    uint8_t* w = (uint8_t*)ws;
    uint64_t* keys = (uint64_t*)w;
    uint64_t* keys2 = keys + r;
    uint32_t* idx = (uint32_t*)(keys2 + r);
    uint32_t* idx2 = idx + r;
    void* tmp = idx2 + r;
    size_t tb = ws_bytes - (size_t)((uint8_t*)tmp - w);
    hipError_t e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_lv_keys, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, n, keys, idx);
    if (full_sort) e = rocprim::merge_sort(tmp, tb, idx, idx2, (size_t)n, LvPosLess{vals}, s);
    else e = rocprim::radix_sort_pairs(tmp, tb, keys, keys2, idx, idx2, (size_t)n, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lv_check, dim3(nblk(n)), dim3(BLOCK), 0, s, vals, n, part_mod, part_res, idx2, err, bad);
    *order = idx2;
    return hipGetLastError();
}

void first_noncanonical(hipStream_t s, const uint8_t* raw, uint32_t n, int* err, uint32_t* bad) {
    if (!n) return;
    hipLaunchKernelGGL(k_first_noncanonical, dim3(nblk(n)), dim3(BLOCK), 0, s, raw, n, err, bad);
}

void load_values_commit(hipStream_t s, const uint8_t* vals, const uint32_t* order, uint32_t n, uint8_t* d_val, uint32_t* sorted) {
    hipLaunchKernelGGL(k_lv_commit, dim3(nblk((size_t)n + 1)), dim3(BLOCK), 0, s, vals, order, n, d_val, sorted);
}

}  // namespace prep
}  // namespace imt
