// imt_itree.cpp -- the stateful depth-d indexed tree behind imt_itree_* (include/imt.h).
//
// A batch insertion has a hash-free part -- the low-leaf search of update_idx_leaf
// (/root/reference/src/indexed_merkle_tree.rs:632-660), the leaf preimages at every time
// step and the (position, time) order of the 2N leaf events -- and the hashing, which is the
// level sweep of imt_sweep.hpp on the GPU.  The hash-free part runs on the GPU too by default
// (imt_prep.hip, over a device-resident sorted index); IMT_HOST_PREP selects the equivalent host
// code in this file.  Plan buffers exist three times and are filled on a side stream, so with
// IMT_DEVICE_PTRS | IMT_PIPELINE consecutive batches overlap on two compute streams.
#include "imt_ctx.hpp"
#include "imt_prep.hpp"
#include "imt_prep_logic.hpp"
#include "imt_filter_logic.hpp"
#include "imt_apply_pipe.hpp"
#include "imt_resize.hpp"
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <numeric>
#include <thread>
#include <unordered_set>

using namespace imt;

namespace {

typedef std::array<uint64_t, 4> U256;   // little-endian limbs of a canonical integer

inline bool lt256(const U256& a, const U256& b) {
    for (int i = 3; i >= 0; i--)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}
inline bool is_zero256(const U256& a) { return (a[0] | a[1] | a[2] | a[3]) == 0; }

struct Pre {            // {val, next_val, next_idx}: src/utils.rs:12-17
    U256 val, next_val;
    uint64_t next_idx;
};
struct SortedEnt {      // 16 bytes: the value's top limb (ties resolved through pre[idx].val) + leaf index
    uint64_t top;
    uint64_t idx;
};

inline void put_pre(uint8_t* dst, const U256& val, const U256& next_val, uint64_t next_idx) {
    std::memcpy(dst, val.data(), 32);
    std::memcpy(dst + 32, next_val.data(), 32);
    std::memset(dst + 64, 0, 32);
    std::memcpy(dst + 64, &next_idx, 8);
}

// include/imt.h: every field-element row a DEVICE pointer refers to must be 16-byte aligned (the kernels move an
// element as two 16-byte words).  A misaligned one is refused here as an argument error instead of faulting there.
int check_fe_ptrs(imt_ctx* c, bool dev, std::initializer_list<const void*> ps) {
    if (!dev) return IMT_OK;
    for (const void* p : ps)
        if (p && ((uintptr_t)p & 15u)) return c->fail(IMT_ERR_ARG, "device pointer %p to field elements is not 16-byte aligned", p);
    return IMT_OK;
}
int check_out_ptrs(imt_ctx* c, bool dev, const imt_insert_out* o) {
    if (!o) return IMT_OK;
    return check_fe_ptrs(c, dev, {o->low_leaf, o->old_root, o->interim_root, o->new_root, o->new_leaf, o->low_sib, o->new_sib});
}

unsigned ceil_log2(uint64_t x) {
    unsigned l = 0;
    while (l < 63 && ((uint64_t)1 << l) < x) l++;
    return l;
}

// one set of plan buffers (device + pinned host staging)
// Batches in flight on the GPU under IMT_PIPELINE, each on its own stream, one tree level apart.  At 2^16
// insertions per batch two already saturate the SIMDs (2, 4: 3.03 M insertions/s; 8: 2.97).  Four is for smaller
// batches, whose 33 dependent launches cost 0.39 ms each whatever their size: 2^15 goes from 2.73 to 3.01 M/s,
// 2^10..2^13 double (profiles/r02_small_batch_rates.txt).  More needs GPU_MAX_HW_QUEUES > 4 in the environment.
#ifndef IMT_NPIPE
#define IMT_NPIPE 4
#endif

struct PlanSet {
    size_t cap_events = 0;       // capacity in events
    unsigned cap_levels = 0;
    uint8_t* h_pin = nullptr;    // pinned: [pre 96*E][node,time,rs,re 4*E each]
    uint8_t* d_pre = nullptr;
    uint32_t* d_tab[2][4] = {{nullptr}};   // ping-pong {node,time,rs,re}
    uint32_t* d_from = nullptr;  // [levels][E]
    int32_t* d_sibsrc = nullptr;
    uint32_t* d_nodeb = nullptr;
    uint32_t* d_timen = nullptr; // [levels][E] time table of level l+1
    uint8_t* d_val[2] = {nullptr, nullptr};
    prep::Workspace ws;                  // GPU-prepare scratch
    prep::FilterWs fw;                   // classification scratch of imt_itree_insert_filtered
    uint32_t* d_slot = nullptr;          // [levels + 1][E] slot of every event per level (sharded mode)
    const uint8_t** d_valptr = nullptr;  // [levels + 1] device array of level value pointers (sharded mode)
    uint8_t* d_root = nullptr;           // [2][32] stored root right after this batch (device format); row 1: see reads_only
    bool has_root = false;
    // A pipelined mixed block of READs only (imt_itree_mixed_pipelined) takes a turn in the rotation without being a batch:
    // row 0 of d_root is then the root it found, row 1 (has_root2) the root one batch before that, carried along so that
    // imt_itree_root_lagged answers as if the block had not rotated.  sliced1 / sliced2: the set the row stands for was a slice's.
    bool reads_only = false, has_root2 = false, sliced1 = false, sliced2 = false;
    hipEvent_t done = nullptr;           // recorded after the batch's last kernel
    // [l]: stored level l is final and this batch no longer reads it (imt_apply_pipe.hpp) -- after k_writeback of the
    // level for a witness batch, after the launch that reads the level for a pipelined apply batch
    hipEvent_t wb_done[IMT_MAX_DEPTH + 1] = {nullptr};
    bool in_flight = false;
    bool pipelined = false;              // ran on a pipeline stream (IMT_PIPELINE, imt_itree_*_pipelined)
    bool applied = false;                // ... as an apply batch: which events it recorded, and when
    // a tree's plan sets only (imt_itree_new), kept when the set grows: what a pipelined apply batch must not share
    uint64_t* d_count = nullptr;         // [IMT_MAX_DEPTH + 1] its hashes per level, sizing its launches on the device
    uint8_t* d_chain = nullptr;          // [IMT_MAX_DEPTH + 1][32] node 0 of the levels from its L0 up, before they are stored
    unsigned l0 = 0;                     // its L0
    uint8_t* d_canon = nullptr;          // [E/2][32] canonical copy of the batch's values when they arrive in another format
    // a time slice of a multi-GPU step (imt_itree_slice_*): prepared here, hashed unit by unit on the caller's streams
    hipEvent_t prep_done = nullptr;      // recorded on the side stream behind the slice's preparation and index phase
    bool open = false;                   // prepared, last unit not yet issued
    bool sliced = false;                 // the set's last user was a slice (imt_itree_slice_prepare), not an ordinary batch
    size_t slice_n = 0;
    imt_insert_out slice_out = {};
    unsigned slice_fmt = 0;
    unsigned slice_next_unit = 0;
    uint64_t slice_size_before = 0;      // leaves in the tree before this slice (its own first new leaf)
    launch::SibLayout slice_lay = {0, 0};
    // row l of the per-level tables: written by the index phase, read by the sweep and the write-back of level l
    struct Level {
        uint32_t* from;
        int32_t* sibsrc;
        uint32_t *nodeb, *timen;
    };
    Level level(unsigned l) const {
        const size_t o = (size_t)l * cap_events;
        return {d_from + o, d_sibsrc + o, d_nodeb + o, d_timen + o};
    }
};

}  // namespace

struct imt_itree {
    imt_ctx* ctx = nullptr;
    unsigned depth = 0;
    uint64_t cap = 0, size = 0;
    // placement as a subtree of a deeper tree (imt_itree_set_placement); the defaults are "not placed"
    unsigned global_depth = 0;       // = depth when not placed
    uint64_t sub_index = 0;          // which subtree of height `depth`
    uint64_t index_base = 0;         // sub_index << depth: added to every leaf index that crosses the API
    uint32_t part_mod = 0, part_res = 0;   // value partition between the subtrees (imt_itree_set_value_partition)
    hipEvent_t in_mark = nullptr;    // position of the context's stream when a device-pointer call starts
    std::vector<uint64_t> h_off, h_len;
    uint8_t* d_nodes = nullptr;
    uint64_t* d_off = nullptr;
    uint64_t* d_len = nullptr;
    uint8_t* nodes(unsigned l) const { return d_nodes + h_off[l] * 32; }   // stored level l (h_len[l] nodes, device format)
    std::vector<Pre> pre;            // host mirror of the leaf preimages
    std::vector<SortedEnt> sorted;   // leaves ordered by val
    // device-resident index (default prepare path): values in leaf order + leaf indices in value order.
    // The host mirror and the device index are each refreshed from the other on demand.
    uint8_t* d_val = nullptr;        // [cap][32] canonical
    uint32_t* d_sorted[2] = {nullptr, nullptr};
    int sorted_cur = 0;
    bool mirror_valid = true, dev_index_valid = true;
    int* h_err_pin = nullptr;        // pinned word for the prepare kernels' error bits
    uint32_t* h_cnt_pin = nullptr;   // two pinned words: the accepted count of imt_itree_insert_filtered, the two of _mixed_filtered
    // a sharded batch between imt_itree_batch_begin and _end
    struct Pending { bool active = false; size_t n = 0; unsigned l0 = 0; int set = 0; } pending;
    static constexpr int NPIPE = IMT_NPIPE;     // batches in flight on the GPU under IMT_PIPELINE
    static constexpr int NSETS = NPIPE + 1;     // host work may run one batch further ahead
    PlanSet plan[NSETS];
    int cur = 0;
    uint64_t batch_no = 0;
    hipStream_t up_stream = nullptr;
    hipEvent_t up_done = nullptr;
    // IMT_PIPELINE: consecutive batches rotate over NPIPE internal streams and run one level
    // apart (batch k+1 sweeps level l once batch k has written level l back), so up to NPIPE hash
    // kernels share the GPU and the SIMDs see several times the waves of a single 2^16 batch.
    // imt_itree_apply_pipelined rotates over the same streams, two launches apart (imt_apply_pipe.hpp).
    hipStream_t pipe_stream[NPIPE] = {};
    hipEvent_t user_mark = nullptr;  // position of the context's stream when a pipelined call starts
    uint64_t pipe_turn = 0;          // pipelined blocks so far: whose turn among the pipeline streams it is
    bool pipe_pending = false;       // pipelined work the context's stream has not been ordered behind
    // reusable host work arrays of insert_batch
    std::vector<uint32_t> w_ord, w_rank;
    std::vector<std::pair<uint64_t, uint32_t>> w_sortkey;
    std::vector<int64_t> w_prv, w_nxt, w_pred, w_succ;
    std::vector<uint64_t> w_keys, w_keys2, w_low;
    std::vector<uint8_t> w_largest;
    std::vector<uint32_t> w_hist;
    std::vector<SortedEnt> w_merged;
    // imt_itree_slice_prepare: index workspace for the values other GPUs hash, canonical copy of a step's values
    prep::Workspace fws;
    uint8_t* d_canon_all = nullptr;
    size_t canon_all_cap = 0;
    uint32_t* d_sorted_extra = nullptr;      // third index buffer: a step's up to three merges never write the committed one
    hipStream_t slice_prep_stream = nullptr; // where the next imt_itree_slice_prepare runs (nullptr: the side stream)
    const uint32_t* slice_poison = nullptr;  // device-visible word of the world's transport: non-zero = skip applies
    double slice_wait_limit_ms = 0;          // > 0: host waits inside imt_itree_slice_prepare give up after this long
    hipEvent_t slice_tail_event = nullptr;   // one shot (imt_itree_set_slice_tail_event)
    bool slice_tail_attached = false;
    double slice_wait_ms = 0;                // host time spent waiting for the GPU inside imt_itree_slice_prepare
    double slice_backpressure_ms = 0;        // ... the part of it spent waiting for the plan set's previous slice (all-time total)
    bool sliced_busy = false;                // an imt_sliced world has steps in flight on this replica (until its flush)
    size_t reserved_events = 0;              // every plan set holds at least this many events (reserve_all_plans)
    // imt_itree_apply_batch: hashes per level of the last apply call, written by its kernels (imt_itree_apply_stats)
    uint64_t* d_apply_stats = nullptr;       // [IMT_MAX_DEPTH + 1]
    bool apply_seen = false;
    // imt_itree_apply_pipelined keeps them in its plan set: the set of the last apply call if that was a pipelined one
    const PlanSet* apply_stats_set = nullptr;
    uint64_t* d_rewind_stats = nullptr;      // [IMT_MAX_DEPTH + 1]: the same of the last imt_itree_rewind
    double reserve_ms[3] = {0, 0, 0};        // the last imt_itree_reserve: the call, its node kernel, its hipMalloc + hipFree
    uint64_t gen = 0;                        // bumped by every call that changes the contents: what a view's side table is for
};

// A read-only view of a tree at an earlier size (imt_view.hpp).  The compacted index and the side table are a cache for
// (size, t->gen); everything is the view's own memory, so building one writes nothing the tree or another view reads.
struct imt_itree_view {
    imt_itree* t = nullptr;
    uint64_t size = 0;
    uint64_t gen = ~(uint64_t)0;             // the tree's generation the cache was built for (none yet)
    bool current = false;                    // size == the tree's size at that generation: nothing cached, the tree answers
    uint64_t builds = 0;
    uint64_t h_hashes[IMT_MAX_DEPTH + 1] = {0};
    uint32_t* d_sorted = nullptr;            // [size] the index as of `size`
    uint64_t* d_count = nullptr;             // [IMT_MAX_DEPTH + 1] listed nodes per level
    uint8_t* d_chain = nullptr;              // [IMT_MAX_DEPTH + 1][32] node 0 of the levels from `top` up
    // per build, for `rows` = relinked leaves + 1 table rows (grow-only)
    size_t rows_cap = 0;
    unsigned levels_cap = 0;
    uint32_t* d_tab[4] = {nullptr};          // node, time, rs, re [rows]
    uint32_t* d_src = nullptr;               // [rows]
    uint8_t* d_pre = nullptr;                // [rows][96]
    uint32_t* d_list = nullptr;              // [levels][rows]
    uint8_t* d_side = nullptr;               // [levels][rows][32]
    unsigned top = 0;                        // of the last build
    PlanSet plan;                            // imt_itree_view_insert_witness: tables and versions of a replay (grow-only)
    view::Side side() const { return {d_list, d_count, rows_cap, top, size, d_side, d_chain}; }
};

static void plan_free(PlanSet& p) {
    if (p.h_pin) hipHostFree(p.h_pin);
    if (p.d_pre) hipFree(p.d_pre);
    for (auto& pp : p.d_tab)
        for (auto& q : pp)
            if (q) hipFree(q);
    if (p.d_from) hipFree(p.d_from);
    if (p.d_sibsrc) hipFree(p.d_sibsrc);
    if (p.d_nodeb) hipFree(p.d_nodeb);
    if (p.d_timen) hipFree(p.d_timen);
    for (auto& q : p.d_val)
        if (q) hipFree(q);
    if (p.d_root) hipFree(p.d_root);
    if (p.d_slot) hipFree(p.d_slot);
    if (p.d_valptr) hipFree(p.d_valptr);
    if (p.d_canon) hipFree(p.d_canon);
    for (void* q : {(void*)p.ws.o_low, (void*)p.ws.o_largest, (void*)p.ws.o_lowleaf, (void*)p.ws.o_newleaf})
        if (q) hipFree(q);
    for (void* q : {(void*)p.ws.iota, (void*)p.ws.bsorted, (void*)p.ws.gap, (void*)p.ws.st, (void*)p.ws.low,
                    (void*)p.ws.succ, (void*)p.ws.keys, (void*)p.ws.keys_sorted, p.ws.tmp, (void*)p.ws.err})
        if (q) hipFree(q);
    for (void* q : {(void*)p.fw.idx, (void*)p.fw.ord, (void*)p.fw.st, (void*)p.fw.aux, (void*)p.fw.flag, (void*)p.fw.rank,
                    (void*)p.fw.count, (void*)p.fw.acc, (void*)p.fw.aop, (void*)p.fw.apos, (void*)p.fw.status, (void*)p.fw.leaf,
                    p.fw.tmp})
        if (q) hipFree(q);
    PlanSet keep;
    keep.done = p.done;
    keep.prep_done = p.prep_done;
    for (int l = 0; l <= IMT_MAX_DEPTH; l++) keep.wb_done[l] = p.wb_done[l];
    keep.d_count = p.d_count;
    keep.d_chain = p.d_chain;
    p = keep;
}

static int plan_reserve(imt_ctx* c, PlanSet& p, size_t events, unsigned levels, size_t tree_cap) {
    if (p.cap_events >= events && p.cap_levels >= levels) return IMT_OK;
    plan_free(p);
    const size_t E = std::max(events + events / 4, (size_t)1024);
    const unsigned L = std::max(levels, 1u);
    hipError_t e = hipSuccess;
    auto A = [&](void** ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(ptr, bytes);
    };
    if (hipHostMalloc((void**)&p.h_pin, E * (96 + 16), hipHostMallocDefault) != hipSuccess)
        return c->fail(IMT_ERR_ALLOC, "hipHostMalloc(plan staging) failed");
    A((void**)&p.d_pre, E * 96);
    for (int s = 0; s < 2; s++)
        for (int j = 0; j < 4; j++) A((void**)&p.d_tab[s][j], E * 4);
    A((void**)&p.d_from, (size_t)L * E * 4);
    A((void**)&p.d_sibsrc, (size_t)L * E * 4);
    A((void**)&p.d_nodeb, (size_t)L * E * 4);
    A((void**)&p.d_timen, (size_t)L * E * 4);
    A((void**)&p.d_val[0], E * 32);
    A((void**)&p.d_val[1], E * 32);
    A((void**)&p.d_root, 64);
    {   // GPU-prepare workspace for E/2 insertions
        const size_t N = E / 2;
        int lv = 1;
        while (((size_t)1 << lv) <= N) lv++;
        p.ws.cap_n = N;
        A((void**)&p.ws.iota, N * 4);
        A((void**)&p.ws.bsorted, N * 4);
        A((void**)&p.ws.gap, N * 4);
        A((void**)&p.ws.st, (size_t)lv * N * 4);
        A((void**)&p.ws.low, N * 4);
        A((void**)&p.ws.succ, N * 4);
        A((void**)&p.ws.keys, E * 8);
        A((void**)&p.ws.keys_sorted, E * 8);
        p.ws.tmp_bytes = prep::temp_bytes_needed(N, tree_cap);
        A((void**)&p.ws.tmp, p.ws.tmp_bytes);
        A((void**)&p.ws.err, sizeof(int));
        A((void**)&p.ws.o_low, N * 8);
        A((void**)&p.ws.o_largest, N);
        A((void**)&p.ws.o_lowleaf, N * 96);
        A((void**)&p.ws.o_newleaf, N * 96);
        p.fw.cap_n = N;
        A((void**)&p.fw.idx, N * 4);
        A((void**)&p.fw.ord, N * 4);
        A((void**)&p.fw.st, N);
        A((void**)&p.fw.aux, N * 4);
        A((void**)&p.fw.flag, N * 4);
        A((void**)&p.fw.rank, N * 4);
        A((void**)&p.fw.count, 2 * sizeof(uint32_t));
        A((void**)&p.fw.acc, N * 32);
        A((void**)&p.fw.aop, N);
        A((void**)&p.fw.apos, N * 4);
        A((void**)&p.fw.status, N);
        A((void**)&p.fw.leaf, N * 8);
        p.fw.tmp_bytes = prep::filter_temp_bytes(N);
        A((void**)&p.fw.tmp, p.fw.tmp_bytes);
    }
    A((void**)&p.d_slot, (size_t)(L + 1) * E * 4);
    A((void**)&p.d_valptr, (size_t)(L + 1) * sizeof(void*));
    A((void**)&p.d_canon, (E / 2) * 32);
    if (e != hipSuccess) {
        plan_free(p);
        return c->hip_fail(e, "hipMalloc(plan)");
    }
    p.cap_events = E;
    p.cap_levels = L;
    return IMT_OK;
}

// All plan sets at once: a pipelined caller (IMT_PIPELINE, imt_sliced_*) rotates through every set within its first
// NSETS batches, and each first use is a dozen hipMalloc calls in the middle of somebody's pipeline.
static int reserve_all_plans(imt_itree* t, size_t events) {
    if (t->reserved_events >= events) return IMT_OK;
    for (auto& p : t->plan) {
        if (p.in_flight || p.open) continue;              // its buffers are in use: it grows when its turn comes
        int rc = plan_reserve(t->ctx, p, events, t->depth, t->cap);
        if (rc) return rc;
    }
    t->reserved_events = events;
    return IMT_OK;
}

extern "C" void imt_itree_free(imt_itree* t) {
    if (!t) return;
    hipSetDevice(t->ctx->device);
    hipStreamSynchronize(t->ctx->stream);
    if (t->up_stream) hipStreamSynchronize(t->up_stream);
    for (auto& p : t->plan) {
        plan_free(p);
        if (p.done) hipEventDestroy(p.done);
        if (p.prep_done) hipEventDestroy(p.prep_done);
        for (auto& e : p.wb_done)
            if (e) hipEventDestroy(e);
        if (p.d_count) hipFree(p.d_count);
        if (p.d_chain) hipFree(p.d_chain);
    }
    if (t->up_done) hipEventDestroy(t->up_done);
    if (t->up_stream) hipStreamDestroy(t->up_stream);
    for (auto& ps : t->pipe_stream) {
        if (!ps) continue;
        hipStreamSynchronize(ps);
        auto& ss = t->ctx->side_streams;
        ss.erase(std::remove(ss.begin(), ss.end(), ps), ss.end());
        hipStreamDestroy(ps);
    }
    if (t->user_mark) hipEventDestroy(t->user_mark);
    if (t->in_mark) hipEventDestroy(t->in_mark);
    if (t->d_nodes) hipFree(t->d_nodes);
    if (t->d_off) hipFree(t->d_off);
    if (t->d_len) hipFree(t->d_len);
    if (t->d_val) hipFree(t->d_val);
    if (t->d_apply_stats) hipFree(t->d_apply_stats);
    if (t->d_rewind_stats) hipFree(t->d_rewind_stats);
    for (auto q : t->d_sorted)
        if (q) hipFree(q);
    if (t->h_err_pin) hipHostFree(t->h_err_pin);
    if (t->h_cnt_pin) hipHostFree(t->h_cnt_pin);
    for (void* q : {(void*)t->fws.iota, (void*)t->fws.bsorted, (void*)t->fws.gap, (void*)t->fws.st, t->fws.tmp,
                    (void*)t->d_canon_all, (void*)t->d_sorted_extra})
        if (q) hipFree(q);
    delete t;
}

extern "C" int imt_itree_new(imt_ctx* c, unsigned depth, uint64_t capacity, imt_itree** out) {
    if (!c || !out) return IMT_ERR_ARG;
    *out = nullptr;
    if (depth == 0 || depth > IMT_MAX_DEPTH) return c->fail(IMT_ERR_RANGE, "depth %u out of range", depth);
    if (capacity < 2 || (capacity & (capacity - 1)) || capacity > ((uint64_t)1 << 31))
        return c->fail(IMT_ERR_RANGE, "capacity must be a power of two in [2, 2^31]");
    if (depth < 63 && capacity > ((uint64_t)1 << depth)) return c->fail(IMT_ERR_RANGE, "capacity exceeds 2^depth");
    int rc = c->set_device();
    if (rc) return rc;
    imt_itree* t = new (std::nothrow) imt_itree();
    if (!t) return c->fail(IMT_ERR_ALLOC, "out of host memory");
    t->ctx = c;
    t->depth = depth;
    t->global_depth = depth;
    t->cap = capacity;
    uint64_t off = 0;
    for (unsigned l = 0; l <= depth; l++) {
        const uint64_t n = resize::level_len(capacity, l);
        t->h_off.push_back(off);
        t->h_len.push_back(n);
        off += n;
    }
    hipError_t e;
    if ((e = hipMalloc((void**)&t->d_val, capacity * 32)) != hipSuccess ||
        (e = hipMalloc((void**)&t->d_sorted[0], capacity * 4)) != hipSuccess ||
        (e = hipMalloc((void**)&t->d_sorted[1], capacity * 4)) != hipSuccess ||
        (e = hipHostMalloc((void**)&t->h_err_pin, sizeof(int), hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&t->h_cnt_pin, 2 * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess ||
        (e = hipMalloc((void**)&t->d_nodes, off * 32)) != hipSuccess ||
        (e = hipMalloc((void**)&t->d_off, (depth + 1) * 8)) != hipSuccess ||
        (e = hipMalloc((void**)&t->d_len, (depth + 1) * 8)) != hipSuccess ||
        (e = hipMalloc((void**)&t->d_apply_stats, (IMT_MAX_DEPTH + 1) * 8)) != hipSuccess ||
        (e = hipMalloc((void**)&t->d_rewind_stats, (IMT_MAX_DEPTH + 1) * 8)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&t->up_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&t->up_done, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&t->in_mark, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&t->user_mark, hipEventDisableTiming)) != hipSuccess) {
        imt_itree_free(t);
        return c->hip_fail(e, "imt_itree_new allocation");
    }
    {
        // different priorities: the runtime may otherwise map the streams to one hardware queue, which
        // serialises them (seen with rocprofv3: same Queue_Id, zero overlap)
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;   // numerically: least >= greatest
        for (int i = 0; i < imt_itree::NPIPE; i++) {
            const int prio = std::max(greatest, std::min(least, 0 - i));
            if ((e = hipStreamCreateWithPriority(&t->pipe_stream[i], hipStreamNonBlocking, prio)) != hipSuccess) {
                imt_itree_free(t);
                return c->hip_fail(e, "hipStreamCreateWithPriority");
            }
        }
        for (auto& pl : t->plan)
            if ((e = hipEventCreateWithFlags(&pl.done, hipEventDisableTiming)) != hipSuccess ||
                (e = hipEventCreateWithFlags(&pl.prep_done, hipEventDisableTiming)) != hipSuccess) {
                imt_itree_free(t);
                return c->hip_fail(e, "hipEventCreate");
            }
    }
    for (auto& pl : t->plan) {
        for (unsigned l = 0; l <= depth; l++)
            if ((e = hipEventCreateWithFlags(&pl.wb_done[l], hipEventDisableTiming)) != hipSuccess) {
                imt_itree_free(t);
                return c->hip_fail(e, "hipEventCreate");
            }
        if ((e = hipMalloc((void**)&pl.d_count, (IMT_MAX_DEPTH + 1) * 8)) != hipSuccess ||
            (e = hipMalloc((void**)&pl.d_chain, (IMT_MAX_DEPTH + 1) * 32)) != hipSuccess) {
            imt_itree_free(t);
            return c->hip_fail(e, "imt_itree_new allocation");
        }
    }
    if ((e = hipMemsetAsync(t->d_val, 0, 32, c->stream)) != hipSuccess ||          // leaf 0: the sentinel value 0
        (e = hipMemsetAsync(t->d_sorted[0], 0, 4, c->stream)) != hipSuccess ||     // sorted index = [leaf 0]
        (e = hipMemcpyAsync(t->d_off, t->h_off.data(), (depth + 1) * 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(t->d_len, t->h_len.data(), (depth + 1) * 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess) {
        imt_itree_free(t);
        return c->hip_fail(e, "imt_itree_new init copies");
    }
    for (unsigned l = 0; l <= depth; l++)   // every stored node starts as the empty subtree of its height
        launch::fill_level(c->stream, t->nodes(l), t->h_len[l], c->d_zero + (size_t)l * 32);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        imt_itree_free(t);
        return c->hip_fail(e, "imt_itree_new init");
    }
    // leaf 0 is the {0,0,0} sentinel; its hash equals the empty-slot hash
    t->pre.push_back(Pre{{0, 0, 0, 0}, {0, 0, 0, 0}, 0});
    t->sorted.push_back(SortedEnt{0, 0});
    t->size = 1;
    for (auto ps : t->pipe_stream) c->side_streams.push_back(ps);
    *out = t;
    return IMT_OK;
}

// a slice between imt_itree_slice_prepare and its last unit owns its plan set and has moved the index ahead of the
// stored tree: the batch calls wait until it is finished
static bool slice_open(const imt_itree* t) {
    for (const auto& pl : t->plan)
        if (pl.open) return true;
    return false;
}

// Between imt_sliced_step and imt_sliced_flush the replica is mid-step: other ranks' write-backs are still arriving on
// the world's own streams, which nothing here is ordered behind.  The ordinary entry points refuse instead of reading
// or writing a half-applied tree (include/imt.h: "only imt_sliced_* calls may touch the trees").
#define IMT_NOT_SLICED(t)                                                                                              \
    do {                                                                                                               \
        if ((t)->sliced_busy) return (t)->ctx->fail(IMT_ERR_ARG, "the tree has sliced steps in flight: imt_sliced_flush first"); \
    } while (0)

// order the context's stream behind every pipelined batch still in flight
static int join_top(imt_itree* t) {
    if (!t->pipe_pending) return IMT_OK;
    for (auto& pl : t->plan)
        if (pl.in_flight && pl.pipelined) IMT_HIP(t->ctx, hipStreamWaitEvent(t->ctx->stream, pl.done, 0));
    t->pipe_pending = false;
    return IMT_OK;
}

// host mirror <- device index (after GPU-prepared batches)
static int ensure_mirror(imt_itree* t) {
    if (t->mirror_valid) return IMT_OK;
    imt_ctx* c = t->ctx;
    const size_t M = t->size;
    std::vector<U256> vals(M);
    std::vector<uint32_t> order(M);
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    IMT_HIP(c, hipMemcpy(vals.data(), t->d_val, M * 32, hipMemcpyDeviceToHost));
    IMT_HIP(c, hipMemcpy(order.data(), t->d_sorted[t->sorted_cur], M * 4, hipMemcpyDeviceToHost));
    static const U256 ZERO = {0, 0, 0, 0};
    t->pre.resize(M);
    t->sorted.resize(M);
    for (size_t r = 0; r < M; r++) {
        const uint32_t i = order[r];
        t->sorted[r] = SortedEnt{vals[i][3], i};
        t->pre[i].val = vals[i];
        t->pre[i].next_val = r + 1 < M ? vals[order[r + 1]] : ZERO;
        t->pre[i].next_idx = r + 1 < M ? order[r + 1] : 0;
    }
    t->mirror_valid = true;
    return IMT_OK;
}
// device index <- host mirror (after host-prepared batches or a snapshot load)
static int ensure_device_index(imt_itree* t) {
    if (t->dev_index_valid) return IMT_OK;
    imt_ctx* c = t->ctx;
    int rc = ensure_mirror(t);
    if (rc) return rc;
    const size_t M = t->size;
    std::vector<U256> vals(M);
    std::vector<uint32_t> order(M);
    for (size_t i = 0; i < M; i++) vals[i] = t->pre[i].val;
    for (size_t r = 0; r < M; r++) order[r] = (uint32_t)t->sorted[r].idx;
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    IMT_HIP(c, hipMemcpy(t->d_val, vals.data(), M * 32, hipMemcpyHostToDevice));
    IMT_HIP(c, hipMemcpy(t->d_sorted[t->sorted_cur], order.data(), M * 4, hipMemcpyHostToDevice));
    t->dev_index_valid = true;
    return IMT_OK;
}

// ------------------------------------------------------------------------------------
// The stages the ways into the tree are built from.  A batch enters through imt_itree_insert_batch / _apply_batch,
// through _insert_filtered / _apply_filtered, through _mixed_batch / _apply_mixed and their filtered twins, through
// _batch_begin (sharded) or through _slice_prepare + _slice_unit (sliced), and a view replays what went in
// (_view_insert_witness, _view_mixed_witness); each of those is a sequence of the stages below -- of the two schedules
// witness_sweep and apply_hashes above all -- and of what is its own.  None of the stages asks who calls.
// ------------------------------------------------------------------------------------
struct HostTimer {      // host milliseconds since it was made
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Context scratch slots [first, last] borrowed for one bulk call -- a copy or a workspace as large as the tree: given back
// when the call returns if they have grown beyond 64 MiB (the callers wait for the stream before they return).
struct ScratchTrim {
    imt_ctx* c;
    size_t first, last;
    ~ScratchTrim() {
        for (size_t slot = first; slot <= last; slot++) c->trim_scratch(slot, (size_t)64 << 20);
    }
};

// A host wait with a time limit (limit_ms <= 0: wait as long as it takes): the sliced mode's waits stand behind work
// that stands behind collectives, i.e. behind other ranks -- a peer that died would otherwise hang the caller for good.
// IMT_ERR_TIMEOUT leaves the stream as it is (still busy); the caller gives the world up.
template <class Query, class Sync>
static int bounded_wait(imt_ctx* c, double limit_ms, Query query, Sync sync, const char* what) {
    if (limit_ms <= 0) {
        const hipError_t e = sync();
        return e == hipSuccess ? IMT_OK : c->hip_fail(e, what);
    }
    const HostTimer waited;
    for (unsigned spins = 0;; spins++) {
        const hipError_t e = query();
        if (e == hipSuccess) return IMT_OK;
        if (e != hipErrorNotReady) return c->hip_fail(e, what);
        if (spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50));     // ~0.1 ms of pure polling first
        if ((spins & 63) == 63 && waited.ms() > limit_ms)
            return c->fail(IMT_ERR_TIMEOUT, "gave up after %.0f ms waiting for %s", limit_ms, what);
    }
}

// The refusals the batch entries share, in the order imt_itree_insert_batch has always made them, then the device.
// What one entry alone refuses, or refuses in other words or at another point of its own order, stays with that entry.
static int check_batch_call(imt_itree* t, size_t n, unsigned flags) {
    imt_ctx* c = t->ctx;
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (n > ((size_t)1 << 30)) return c->fail(IMT_ERR_RANGE, "batch too large");
    if (t->pending.active) return c->fail(IMT_ERR_ARG, "a sharded batch is open (imt_itree_batch_end first)");
    if (slice_open(t)) return c->fail(IMT_ERR_ARG, "a slice is open (issue its remaining units first)");
    return c->set_device();
}
static int check_room(imt_itree* t, size_t n) {
    if (t->size + n > t->cap) return t->ctx->fail(IMT_ERR_FULL, "tree capacity %llu exceeded (imt_itree_reserve)", (unsigned long long)t->cap);
    return IMT_OK;
}

// The plan set of the next batch (t->plan[t->cur]): wait until the batch that used it last has left the GPU --
// back-pressure, at most NSETS batches in flight; limit_ms as in bounded_wait -- then make it large enough, all levels
// up front: growing later would stall the pipeline.  The time waited is added to waited_ms, also when the wait fails;
// which counters it belongs in is the caller's business.
static int acquire_plan(imt_itree* t, size_t events, double limit_ms, double& waited_ms) {
    imt_ctx* c = t->ctx;
    PlanSet& P = t->plan[t->cur];
    if (P.in_flight) {
        const HostTimer w;
        const int rc = bounded_wait(c, limit_ms, [&] { return hipEventQuery(P.done); }, [&] { return hipEventSynchronize(P.done); },
                                    "the plan set's previous batch or slice");
        waited_ms += w.ms();
        if (rc) return rc;
        P.in_flight = false;
    }
    return plan_reserve(c, P, events, t->depth, t->cap);
}

// The hash-free part of a batch runs on a side stream, reads the caller's `vals` and writes the caller's hash-free
// outputs (low_index, is_largest, low_leaf, new_leaf), so with device pointers that stream is first ordered behind
// everything the caller has enqueued on the context's stream (imt.h: "work is enqueued on the context's stream").
// IMT_INPUTS_READY waives that: the caller guarantees those buffers are idle.
// (Host-pointer calls are ordered too: their staging scratch may still be read by an asynchronous
// device-pointer call, e.g. imt_itree_lift_batch, enqueued earlier on the context's stream.)
static int order_behind_caller(imt_itree* t, hipStream_t side, unsigned flags) {
    imt_ctx* c = t->ctx;
    if ((flags & IMT_DEVICE_PTRS) && (flags & IMT_INPUTS_READY)) return IMT_OK;
    IMT_HIP(c, hipEventRecord(t->in_mark, c->stream));
    IMT_HIP(c, hipStreamWaitEvent(side, t->in_mark, 0));
    return IMT_OK;
}

// n values, wherever `flags` says they are and in whatever format, to canonical device memory on stream s: the error
// word cleared, host values copied to `up`, any other format converted into `canon` (a value >= p sets bit 0 of the
// error word; `up` and `canon` may be one buffer, the conversion works in place).  *d_vals is where they end up -- `vals`
// itself when they were canonical device values all along.  The buffers are the caller's choice and encode on which
// stream they are safe: a buffer that is not needed may be NULL, a NULL that is needed is a scratch slot that could not
// be had.
static int stage_canonical(imt_ctx* c, hipStream_t s, const void* vals, size_t n, unsigned flags, uint8_t* up, uint8_t* canon,
                           int* d_err, const uint8_t** d_vals) {
    const unsigned fmt = flags & IMT_FMT_MASK;
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((!dev && !up) || (fmt != IMT_FMT_CANONICAL && !canon)) return IMT_ERR_HIP;
    const uint8_t* d = (const uint8_t*)vals;
    IMT_HIP(c, hipMemsetAsync(d_err, 0, sizeof(int), s));
    if (!dev) {
        IMT_HIP(c, hipMemcpyAsync(up, vals, n * 32, hipMemcpyHostToDevice, s));
        d = up;
    }
    if (fmt != IMT_FMT_CANONICAL) {
        launch::convert(s, d, canon, n, fmt, IMT_FMT_CANONICAL, d_err);
        d = canon;
    }
    *d_vals = d;
    return IMT_OK;
}

// What the prepare kernels (prep::run) found wrong with the values, as the call's result; `noun`: a batch or a step
static int insertion_verdict(imt_itree* t, int perr, const char* noun) {
    imt_ctx* c = t->ctx;
    if (perr & prep::ERR_NONCANONICAL) return c->fail(IMT_ERR_NONCANONICAL, "a value is not reduced (>= p)");
    if (perr & prep::ERR_ZERO) return c->fail(IMT_ERR_VALUE, "value 0 cannot be inserted");
    if (perr & prep::ERR_FOREIGN)
        return c->fail(IMT_ERR_VALUE, "a value belongs to another subtree (v %% %u != %u)", t->part_mod, t->part_res);
    if (perr & prep::ERR_DUPLICATE)
        return c->fail(IMT_ERR_VALUE, "duplicate value (inside the %s or already in the tree)", noun);
    return IMT_OK;
}

// The index phase (no hashing): from the prepared level-0 table in P.d_tab[0] the tables of every level below L0, the
// two table sets taking turns.  slots: NULL, or [levels + 1][cap_events] for the slot of every event per level.
static void index_phase(const PlanSet& P, hipStream_t s, size_t E, unsigned L0, uint32_t* slots) {
    for (unsigned l = 0; l < L0; l++) {
        const int a = l & 1, b = a ^ 1;
        const PlanSet::Level row = P.level(l);
        // time table of level l: the prepared one for l = 0, otherwise row l - 1 of d_timen
        const uint32_t* time_in = l == 0 ? P.d_tab[0][1] : P.level(l - 1).timen;
        sweep::LevelTable in{P.d_tab[a][0], time_in, P.d_tab[a][2], P.d_tab[a][3]};
        sweep::LevelOut o{P.d_tab[b][0], row.timen, P.d_tab[b][2], P.d_tab[b][3], row.from, row.sibsrc, row.nodeb,
                          slots ? slots + (size_t)(l + 1) * P.cap_events : nullptr};
        launch::merge_level(s, in, o, (uint32_t)E);
    }
}

extern "C" uint64_t imt_itree_size(const imt_itree* t) { return t ? t->size : 0; }
// internal (imt_itree_internal.hpp): what imt_sliced.cpp needs to know about a tree
imt_ctx* imt_itree_ctx(const imt_itree* t) { return t ? t->ctx : nullptr; }
unsigned imt_itree_depth(const imt_itree* t) { return t ? t->depth : 0; }
void imt_itree_mark_sliced(imt_itree* t, bool busy) {
    if (t) t->sliced_busy = busy;
}
double imt_itree_slice_backpressure_ms(const imt_itree* t) { return t ? t->slice_backpressure_ms : 0; }
void imt_itree_set_slice_tail_event(imt_itree* t, void* hip_event) {
    if (t) {
        t->slice_tail_event = (hipEvent_t)hip_event;
        t->slice_tail_attached = false;
    }
}
bool imt_itree_take_slice_tail_attached(imt_itree* t) {
    if (!t) return false;
    const bool a = t->slice_tail_attached;
    t->slice_tail_attached = false;
    t->slice_tail_event = nullptr;
    return a;
}
void imt_itree_set_slice_poison(imt_itree* t, const uint32_t* device_word) {
    if (t) t->slice_poison = device_word;
}
void imt_itree_set_slice_wait_limit(imt_itree* t, double ms) {
    if (t) t->slice_wait_limit_ms = ms;
}
void imt_itree_set_slice_prep_stream(imt_itree* t, void* hip_stream) {
    if (t) t->slice_prep_stream = (hipStream_t)hip_stream;
}
double imt_itree_take_wait_ms(imt_itree* t) {
    const double w = t ? t->slice_wait_ms : 0;
    if (t) t->slice_wait_ms = 0;
    return w;
}
bool imt_itree_is_plain(const imt_itree* t) { return t && !t->index_base && t->part_mod <= 1 && !t->pending.active; }

extern "C" int imt_itree_root(imt_itree* t, void* root, unsigned flags) {
    if (!t || !root) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    int rc = c->set_device();
    if (rc) return rc;
    if ((rc = check_fe_ptrs(c, flags & IMT_DEVICE_PTRS, {root}))) return rc;
    if ((rc = join_top(t))) return rc;
    const unsigned fmt = flags & IMT_FMT_MASK;
    const uint8_t* src = t->nodes(t->depth);
    if (flags & IMT_DEVICE_PTRS) {
        launch::convert(c->stream, src, (uint8_t*)root, 1, IMT_FMT_DEVICE, fmt, c->d_err);
        return IMT_OK;
    }
    uint8_t* d = (uint8_t*)c->dev_scratch(0, 32);
    if (!d) return IMT_ERR_HIP;
    launch::convert(c->stream, src, d, 1, IMT_FMT_DEVICE, fmt, c->d_err);
    IMT_HIP(c, hipMemcpyAsync(root, d, 32, hipMemcpyDeviceToHost, c->stream));
    IMT_HIP(c, hipStreamSynchronize(c->stream));
    return IMT_OK;
}

extern "C" int imt_itree_root_lagged(imt_itree* t, unsigned lag, void* root, unsigned flags) {
    if (!t || !root) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (lag > 1) return c->fail(IMT_ERR_RANGE, "lag must be 0 or 1");
    int rc = c->set_device();
    if (rc) return rc;
    if (t->batch_no <= lag) return c->fail(IMT_ERR_RANGE, "no batch %u calls ago", lag);
    if ((rc = check_fe_ptrs(c, flags & IMT_DEVICE_PTRS, {root}))) return rc;
    // The newest turn of the rotation is a pipelined block of READs only: not a batch, so it answers for the batches
    // in front of it from the two roots it carries.  (One further back holds the root it found, which is the root of
    // the batch before it: the right answer for lag 1 as it stands.)
    const PlanSet& newest = t->plan[(t->cur + imt_itree::NSETS - 1) % imt_itree::NSETS];
    const bool carried = newest.reads_only;
    const PlanSet& P = carried ? newest : t->plan[(t->cur + 2 * imt_itree::NSETS - 1 - (int)lag) % imt_itree::NSETS];
    const bool row1 = carried && lag == 1;
    const bool have = row1 ? P.has_root2 : P.has_root, sliced = row1 ? P.sliced2 : P.reads_only ? P.sliced1 : P.sliced;
    if (!have)
        return c->fail(sliced ? IMT_ERR_ARG : IMT_ERR_INTERNAL,
                       sliced ? "imt_itree_root_lagged does not see slices: imt_sliced_flush, then imt_itree_root" : "batch root not recorded");
    IMT_HIP(c, hipStreamWaitEvent(c->stream, P.done, 0));
    const unsigned fmt = flags & IMT_FMT_MASK;
    const uint8_t* src = P.d_root + (row1 ? 32 : 0);
    if (flags & IMT_DEVICE_PTRS) {
        launch::convert(c->stream, src, (uint8_t*)root, 1, IMT_FMT_DEVICE, fmt, c->d_err);
        return IMT_OK;
    }
    uint8_t* d = (uint8_t*)c->dev_scratch(0, 32);
    if (!d) return IMT_ERR_HIP;
    launch::convert(c->stream, src, d, 1, IMT_FMT_DEVICE, fmt, c->d_err);
    IMT_HIP(c, hipMemcpyAsync(root, d, 32, hipMemcpyDeviceToHost, c->stream));
    IMT_HIP(c, hipStreamSynchronize(c->stream));
    return IMT_OK;
}

// canonical host copy of n field elements given in any format / location
static int fetch_canonical(imt_ctx* c, hipStream_t st, const void* vals, size_t n, unsigned flags, std::vector<U256>& out) {
    out.resize(n);
    const unsigned fmt = flags & IMT_FMT_MASK;
    const bool dev = flags & IMT_DEVICE_PTRS;
    if (!dev && fmt == IMT_FMT_CANONICAL) {
        std::memcpy(out.data(), vals, n * 32);
    } else if (dev && fmt == IMT_FMT_CANONICAL) {
        IMT_HIP(c, hipMemcpyAsync(out.data(), vals, n * 32, hipMemcpyDeviceToHost, st));
        IMT_HIP(c, hipStreamSynchronize(st));
    } else {
        // convert on the device, then read back
        uint8_t* d_in = (uint8_t*)vals;
        if (!dev) {
            d_in = (uint8_t*)c->dev_scratch(0, n * 32);
            if (!d_in) return IMT_ERR_HIP;
            IMT_HIP(c, hipMemcpyAsync(d_in, vals, n * 32, hipMemcpyHostToDevice, st));
        }
        uint8_t* d_out = (uint8_t*)c->dev_scratch(1, n * 32);
        if (!d_out) return IMT_ERR_HIP;
        launch::convert(st, d_in, d_out, n, fmt, IMT_FMT_CANONICAL, c->d_err);
        IMT_HIP(c, hipMemcpyAsync(out.data(), d_out, n * 32, hipMemcpyDeviceToHost, st));
        IMT_HIP(c, hipStreamSynchronize(st));
    }
    for (size_t i = 0; i < n; i++)
        if (HField::geq_p(out[i].data())) return c->fail(IMT_ERR_NONCANONICAL, "value %zu is not reduced (>= p)", i);
    return IMT_OK;
}

// stored entry e compared with value v: -1 / 0 / +1
static inline int cmp_ent(const imt_itree* t, const SortedEnt& e, const U256& v) {
    if (e.top != v[3]) return e.top < v[3] ? -1 : 1;
    const U256& x = t->pre[e.idx].val;
    for (int i = 2; i >= 0; i--)
        if (x[i] != v[i]) return x[i] < v[i] ? -1 : 1;
    return 0;
}

// position in t->sorted of the greatest val < v; IMT_ERR_VALUE if v == 0 or present
static int find_pred(const imt_itree* t, const U256& v, size_t& pos) {
    size_t lo = 0, hi = t->sorted.size();   // first entry with val >= v
    while (lo < hi) {
        size_t mid = (lo + hi) / 2;
        if (cmp_ent(t, t->sorted[mid], v) < 0) lo = mid + 1; else hi = mid;
    }
    if (lo < t->sorted.size() && cmp_ent(t, t->sorted[lo], v) == 0) return IMT_ERR_VALUE;
    if (lo == 0) return IMT_ERR_VALUE;
    pos = lo - 1;
    return IMT_OK;
}

// What the read calls below answer from: the tree itself (v == NULL), or a view of it at an earlier size (imt_view.hpp),
// whose index is its own and whose nodes are (side table | stored node | empty subtree).  The same code serves both, so a
// view's answers and refusals are the tree's by construction.
static const uint32_t* read_index(const imt_itree* t, const imt_itree_view* v) { return v ? v->d_sorted : t->d_sorted[t->sorted_cur]; }
static uint64_t read_size(const imt_itree* t, const imt_itree_view* v) { return v ? v->size : t->size; }
static void read_proofs(imt_itree* t, const imt_itree_view* v, hipStream_t s, const uint64_t* d_idx, size_t n, uint8_t* d_out,
                        launch::SibLayout lay, unsigned fmt) {
    const launch::TreeView tv{t->d_nodes, t->d_off, t->d_len, t->ctx->d_zero, t->index_base};
    if (v) launch::view_gather_proof(s, v->side(), tv, d_idx, n, t->depth, d_out, lay, fmt);
    else launch::gather_proof(s, tv, d_idx, n, t->depth, d_out, lay, fmt);
}

extern "C" int imt_itree_find_low_batch(imt_itree* t, const void* vals, size_t n, uint64_t* low_index, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (n == 0) return IMT_OK;
    if (!vals || !low_index) return c->fail(IMT_ERR_ARG, "null buffer");
    int rc = c->set_device();
    if (rc) return rc;
    if ((rc = check_fe_ptrs(c, flags & IMT_DEVICE_PTRS, {vals}))) return rc;
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if ((flags & IMT_DEVICE_PTRS) || !t->mirror_valid) {
        // predecessor search in the device-resident index (k_find_low); the host mirror is not built for it
        const bool dev = flags & IMT_DEVICE_PTRS;
        const unsigned fmt = flags & IMT_FMT_MASK;
        if (n > ((size_t)1 << 31)) return c->fail(IMT_ERR_RANGE, "batch too large");
        if (dev && ((uintptr_t)low_index & 7u)) return c->fail(IMT_ERR_ARG, "device low_index array is not 8-byte aligned");
        if ((rc = ensure_device_index(t))) return rc;
        if ((rc = join_top(t))) return rc;
        hipStream_t s = c->stream;
        IMT_HIP(c, hipStreamSynchronize(t->up_stream));
        const uint8_t* d_vals = nullptr;
        int* d_perr = (int*)c->dev_scratch(2, sizeof(int));
        if (!d_perr) return IMT_ERR_HIP;
        uint8_t* buf = (!dev || fmt != IMT_FMT_CANONICAL) ? (uint8_t*)c->dev_scratch(0, n * 32) : nullptr;
        if ((rc = stage_canonical(c, s, vals, n, flags, buf, buf, d_perr, &d_vals))) return rc;
        uint64_t* d_low = dev ? low_index : (uint64_t*)c->dev_scratch(1, n * 8);
        if (!d_low) return IMT_ERR_HIP;
        prep::find_low(s, d_vals, t->d_val, t->d_sorted[t->sorted_cur], (uint32_t)t->size, (uint32_t)n, t->index_base,
                       t->part_mod, t->part_res, d_low, d_perr);
        int perr = 0;
        IMT_HIP(c, hipMemcpyAsync(&perr, d_perr, sizeof(int), hipMemcpyDeviceToHost, s));
        if (!dev) IMT_HIP(c, hipMemcpyAsync(low_index, d_low, n * 8, hipMemcpyDeviceToHost, s));
        IMT_HIP(c, hipStreamSynchronize(s));
        if (perr & prep::ERR_NONCANONICAL) return c->fail(IMT_ERR_NONCANONICAL, "a value is not reduced (>= p)");
        if (perr & prep::ERR_FOREIGN)
            return c->fail(IMT_ERR_VALUE, "a value belongs to another subtree (v %% %u != %u)", t->part_mod, t->part_res);
        if (perr & (prep::ERR_ZERO | prep::ERR_DUPLICATE)) return c->fail(IMT_ERR_VALUE, "a value is zero or already in the tree");
        return IMT_OK;
    }
    std::vector<U256> v;
    rc = fetch_canonical(c, c->stream, vals, n, flags, v);
    if (rc) return rc;
    std::vector<uint64_t> res(n);
    for (size_t i = 0; i < n; i++) {
        size_t pos;
        if (t->part_mod > 1 && prep::mod_small(reinterpret_cast<const uint8_t*>(v[i].data()), t->part_mod) != t->part_res)
            return c->fail(IMT_ERR_VALUE, "value %zu belongs to another subtree (v %% %u != %u)", i, t->part_mod, t->part_res);
        if (find_pred(t, v[i], pos)) return c->fail(IMT_ERR_VALUE, "value %zu is zero or already in the tree", i);
        res[i] = t->index_base + t->sorted[pos].idx;
    }
    if (flags & IMT_DEVICE_PTRS) {
        IMT_HIP(c, hipMemcpy(low_index, res.data(), n * 8, hipMemcpyHostToDevice));
    } else {
        std::memcpy(low_index, res.data(), n * 8);
    }
    return IMT_OK;
}

static int get_leaves(imt_itree* t, const imt_itree_view* v, const uint64_t* index, size_t n, void* preimage, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (n == 0) return IMT_OK;
    if (!preimage) return c->fail(IMT_ERR_ARG, "null buffer");
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (n > ((size_t)1 << 32) - 1) return c->fail(IMT_ERR_RANGE, "too many leaves in one call");
    int rc = c->set_device();
    if (rc) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    if ((rc = check_fe_ptrs(c, dev, {preimage}))) return rc;
    if (dev && index && ((uintptr_t)index & 7u)) return c->fail(IMT_ERR_ARG, "device index array is not 8-byte aligned");
    if (!dev && t->mirror_valid && !v) {
        // the host mirror is current (host-prepared batches): answer from it
        std::vector<uint8_t> buf(n * 96);
        for (size_t i = 0; i < n; i++) {
            const uint64_t li = (index ? index[i] : t->index_base + i) - t->index_base;   // wraps below the base: caught below
            if (li >= t->cap) return c->fail(IMT_ERR_RANGE, "leaf index out of range");
            if (li < t->size) {
                const Pre& p = t->pre[li];                      // the mirror holds local indices; 0 = "no successor"
                put_pre(&buf[i * 96], p.val, p.next_val, is_zero256(p.next_val) ? 0 : t->index_base + p.next_idx);
            } else {
                std::memset(&buf[i * 96], 0, 96);
            }
        }
        if (fmt == IMT_FMT_CANONICAL) {
            std::memcpy(preimage, buf.data(), n * 96);
            return IMT_OK;
        }
        uint8_t* d_in = (uint8_t*)c->dev_scratch(0, n * 96);
        uint8_t* d_out = (uint8_t*)c->dev_scratch(1, n * 96);
        if (!d_in || !d_out) return IMT_ERR_HIP;
        IMT_HIP(c, hipMemcpyAsync(d_in, buf.data(), n * 96, hipMemcpyHostToDevice, c->stream));
        launch::convert(c->stream, d_in, d_out, n * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
        IMT_HIP(c, hipMemcpyAsync(preimage, d_out, n * 96, hipMemcpyDeviceToHost, c->stream));
        IMT_HIP(c, hipStreamSynchronize(c->stream));
        return IMT_OK;
    }
    // from the device index: a leaf's successor is the next value in value order (k_leaves)
    if ((rc = ensure_device_index(t))) return rc;
    if ((rc = join_top(t))) return rc;
    hipStream_t s = c->stream;
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));     // the index may have been written on the side stream
    const uint64_t* d_idx = index;
    if (index && !dev) {
        uint64_t* up = (uint64_t*)c->dev_scratch(0, n * 8);
        if (!up) return IMT_ERR_HIP;
        IMT_HIP(c, hipMemcpyAsync(up, index, n * 8, hipMemcpyHostToDevice, s));
        d_idx = up;
    }
    uint8_t* d_out = dev ? (uint8_t*)preimage : (uint8_t*)c->dev_scratch(1, n * 96);
    int* d_perr = (int*)c->dev_scratch(2, sizeof(int));
    if (!d_out || !d_perr) return IMT_ERR_HIP;
    IMT_HIP(c, hipMemsetAsync(d_perr, 0, sizeof(int), s));
    prep::leaves(s, d_idx, t->index_base, (uint32_t)n, t->d_val, read_index(t, v), (uint32_t)read_size(t, v), t->cap,
                 t->index_base, d_out, d_perr);
    if (fmt != IMT_FMT_CANONICAL) launch::convert(s, d_out, d_out, n * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
    int perr = 0;
    IMT_HIP(c, hipMemcpyAsync(&perr, d_perr, sizeof(int), hipMemcpyDeviceToHost, s));
    if (!dev) IMT_HIP(c, hipMemcpyAsync(preimage, d_out, n * 96, hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipStreamSynchronize(s));
    c->trim_scratch(0, (size_t)64 << 20);               // a whole-tree snapshot to the host staged 104 bytes per leaf here
    c->trim_scratch(1, (size_t)64 << 20);
    if (perr & prep::ERR_RANGE) return c->fail(IMT_ERR_RANGE, "leaf index out of range");
    return IMT_OK;
}
extern "C" int imt_itree_get_leaves(imt_itree* t, const uint64_t* index, size_t n, void* preimage, unsigned flags) {
    return get_leaves(t, nullptr, index, n, preimage, flags);
}

static int get_proof_batch(imt_itree* t, const imt_itree_view* v, const uint64_t* index, size_t n, void* sib, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (n == 0) return IMT_OK;
    if (!index || !sib) return c->fail(IMT_ERR_ARG, "null buffer");
    int rc = c->set_device();
    if (rc) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((rc = check_fe_ptrs(c, dev, {sib}))) return rc;
    if (!dev)
        for (size_t i = 0; i < n; i++)
            if (index[i] - t->index_base >= t->cap) return c->fail(IMT_ERR_RANGE, "leaf index out of range");
    if ((rc = join_top(t))) return rc;
    const unsigned depth = t->depth;
    const uint64_t* d_idx = index;
    uint8_t* d_out = (uint8_t*)sib;
    if (!dev) {
        d_idx = (const uint64_t*)c->dev_scratch(0, n * 8);
        d_out = (uint8_t*)c->dev_scratch(1, (size_t)depth * n * 32);
        if (!d_idx || !d_out) return IMT_ERR_HIP;
        IMT_HIP(c, hipMemcpyAsync((void*)d_idx, index, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    launch::SibLayout lay = (flags & IMT_SIB_ITEM_MAJOR) ? launch::SibLayout{1, depth} : launch::SibLayout{n, 1};
    read_proofs(t, v, c->stream, d_idx, n, d_out, lay, flags & IMT_FMT_MASK);
    if (!dev) {
        IMT_HIP(c, hipMemcpyAsync(sib, d_out, (size_t)depth * n * 32, hipMemcpyDeviceToHost, c->stream));
        IMT_HIP(c, hipStreamSynchronize(c->stream));
    }
    return IMT_OK;
}
extern "C" int imt_itree_get_proof_batch(imt_itree* t, const uint64_t* index, size_t n, void* sib, unsigned flags) {
    return get_proof_batch(t, nullptr, index, n, sib, flags);
}

// ------------------------------------------------------------------------------------
// non-membership witness on the GPU
// ------------------------------------------------------------------------------------
static int non_membership_witness(imt_itree* t, const imt_itree_view* v, const void* vals, size_t n, uint64_t* low_index,
                                  void* low_leaf, uint8_t* is_largest, void* low_sib, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (n == 0) return IMT_OK;
    if (!vals) return c->fail(IMT_ERR_ARG, "null vals");
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (n > ((size_t)1 << 31)) return c->fail(IMT_ERR_RANGE, "batch too large");
    int rc = c->set_device();
    if (rc) return rc;
    if ((rc = check_fe_ptrs(c, flags & IMT_DEVICE_PTRS, {vals, low_leaf, low_sib}))) return rc;
    if ((rc = ensure_device_index(t))) return rc;
    if ((rc = join_top(t))) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    hipStream_t s = c->stream;
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));     // the index may have been written on the side stream
    size_t slot = 0;
    auto scratch = [&](size_t bytes) { return (uint8_t*)c->dev_scratch(slot++, bytes); };
    const uint8_t* d_vals = nullptr;
    uint8_t* up = dev ? nullptr : scratch(n * 32);
    int* d_perr = (int*)scratch(sizeof(int));
    if (!d_perr) return IMT_ERR_HIP;
    uint8_t* can = fmt == IMT_FMT_CANONICAL ? nullptr : scratch(n * 32);
    if ((rc = stage_canonical(c, s, vals, n, flags, up, can, d_perr, &d_vals))) return rc;
    auto outbuf = [&](void* user, size_t bytes) -> uint8_t* {
        if (!user) return nullptr;
        return dev ? (uint8_t*)user : scratch(bytes);
    };
    // the low index is needed on the device for the proof gather even if the caller does not want it
    uint64_t* g_low = (uint64_t*)(low_index && dev ? (uint8_t*)low_index : scratch(n * 8));
    uint8_t* g_leaf = outbuf(low_leaf, n * 96);
    uint8_t* g_lg = outbuf(is_largest, n);
    const size_t sib_bytes = (size_t)t->depth * n * 32;
    uint8_t* g_sib = outbuf(low_sib, sib_bytes);
    if (!g_low || (low_leaf && !g_leaf) || (is_largest && !g_lg) || (low_sib && !g_sib)) return IMT_ERR_HIP;
    prep::nm_witness(s, d_vals, t->d_val, read_index(t, v), (uint32_t)read_size(t, v), (uint32_t)n, t->index_base,
                     t->part_mod, t->part_res, g_low, g_leaf, g_lg, d_perr);
    if (g_leaf && fmt != IMT_FMT_CANONICAL) launch::convert(s, g_leaf, g_leaf, n * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
    if (g_sib) {
        launch::SibLayout lay = (flags & IMT_SIB_ITEM_MAJOR) ? launch::SibLayout{1, t->depth} : launch::SibLayout{n, 1};
        read_proofs(t, v, s, g_low, n, g_sib, lay, fmt);
    }
    int perr = 0;
    IMT_HIP(c, hipMemcpyAsync(&perr, d_perr, sizeof(int), hipMemcpyDeviceToHost, s));
    if (!dev) {
        if (low_index) IMT_HIP(c, hipMemcpyAsync(low_index, g_low, n * 8, hipMemcpyDeviceToHost, s));
        if (low_leaf) IMT_HIP(c, hipMemcpyAsync(low_leaf, g_leaf, n * 96, hipMemcpyDeviceToHost, s));
        if (is_largest) IMT_HIP(c, hipMemcpyAsync(is_largest, g_lg, n, hipMemcpyDeviceToHost, s));
        if (low_sib) IMT_HIP(c, hipMemcpyAsync(low_sib, g_sib, sib_bytes, hipMemcpyDeviceToHost, s));
    }
    IMT_HIP(c, hipStreamSynchronize(s));
    if (perr & prep::ERR_NONCANONICAL) return c->fail(IMT_ERR_NONCANONICAL, "a candidate is not reduced (>= p)");
    if (perr & prep::ERR_FOREIGN)
        return c->fail(IMT_ERR_VALUE, "a candidate belongs to another subtree (v %% %u != %u): this list says nothing about it",
                       t->part_mod, t->part_res);
    if (perr & (prep::ERR_ZERO | prep::ERR_DUPLICATE))
        return c->fail(IMT_ERR_VALUE, "a candidate is 0 or already in the tree (it has no non-membership witness)");
    return IMT_OK;
}
extern "C" int imt_itree_non_membership_witness(imt_itree* t, const void* vals, size_t n, uint64_t* low_index,
                                                void* low_leaf, uint8_t* is_largest, void* low_sib, unsigned flags) {
    return non_membership_witness(t, nullptr, vals, n, low_index, low_leaf, is_largest, low_sib, flags);
}

// ------------------------------------------------------------------------------------
// snapshot load / bulk build
// ------------------------------------------------------------------------------------
extern "C" int imt_itree_load(imt_itree* t, const void* preimages, uint64_t n, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (!preimages || n == 0) return c->fail(IMT_ERR_ARG, "null / empty snapshot");
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (n > t->cap) return c->fail(IMT_ERR_FULL, "snapshot has %llu leaves, capacity is %llu", (unsigned long long)n,
                                   (unsigned long long)t->cap);
    if (slice_open(t)) return c->fail(IMT_ERR_ARG, "a slice is open (issue its remaining units first)");
    int rc = c->set_device();
    if (rc) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    if ((rc = check_fe_ptrs(c, dev, {preimages}))) return rc;
    if ((rc = join_top(t))) return rc;
    for (auto& pl : t->plan)
        if (pl.in_flight) { IMT_HIP(c, hipEventSynchronize(pl.done)); pl.in_flight = false; pl.pipelined = false; }
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    hipStream_t s = c->stream;
    // the snapshot copy and the sort workspace are as large as the tree: not something a context keeps after the call
    const ScratchTrim trim{c, 2, 3};
    // ---- the canonical preimages on the device (what is hashed; next_idx fields are global indices) ----
    const uint8_t* d_pre = (const uint8_t*)preimages;
    if (!dev || fmt != IMT_FMT_CANONICAL) {
        uint8_t* buf = (uint8_t*)c->dev_scratch(2, (size_t)n * 96);
        if (!buf) return IMT_ERR_HIP;
        if (!dev) IMT_HIP(c, hipMemcpyAsync(buf, preimages, (size_t)n * 96, hipMemcpyHostToDevice, s));
        if (fmt != IMT_FMT_CANONICAL) {
            if ((rc = c->clear_err())) return rc;
            launch::convert(s, dev ? d_pre : buf, buf, (size_t)n * 3, fmt, IMT_FMT_CANONICAL, c->d_err);
            if ((rc = c->sync_and_check())) return rc;
        }
        d_pre = buf;
    }
    // ---- list check on the device: ordered by val, every leaf points to its successor, the last one to {0, 0} ----
    const size_t ws_bytes = prep::load_ws_bytes((size_t)n);
    uint8_t* ws = (uint8_t*)c->dev_scratch(3, ws_bytes + 256);      // [error word | 256-byte aligned workspace]
    if (!ws) return IMT_ERR_HIP;
    int* d_perr = (int*)ws;
    const uint32_t* d_order = nullptr;
    int perr = 0;
    uint32_t bad = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        uint32_t* d_bad = nullptr;
        IMT_HIP(c, hipMemsetAsync(d_perr, 0, sizeof(int), s));
        IMT_HIP(c, prep::load_check(s, d_pre, (uint32_t)n, t->index_base, t->part_mod, t->part_res, ws + 256, ws_bytes,
                                    attempt == 1, d_perr, &d_bad, &d_order));
        IMT_HIP(c, hipMemcpyAsync(&perr, d_perr, sizeof(int), hipMemcpyDeviceToHost, s));
        IMT_HIP(c, hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, s));
        IMT_HIP(c, hipStreamSynchronize(s));
        // values that agree in their top 64 bits and came out of the radix sort in the wrong order: sort with the
        // 256-bit comparator and check again (the other bits of a first attempt that tied mean nothing)
        if (!(perr & prep::LOAD_TIE)) break;
    }
    if (perr & prep::ERR_NONCANONICAL) return c->fail(IMT_ERR_NONCANONICAL, "a field element in the snapshot is not reduced (>= p)");
    if (perr & prep::LOAD_SENTINEL) return c->fail(IMT_ERR_VALUE, "leaf 0 must be the {0,..} sentinel");
    if (perr & prep::LOAD_DUP) return c->fail(IMT_ERR_VALUE, "duplicate value in snapshot");
    if (perr & prep::LOAD_LINK)
        return c->fail(IMT_ERR_VALUE, "leaf %llu does not point to its successor", (unsigned long long)(t->index_base + bad));
    if (perr & prep::LOAD_LAST) return c->fail(IMT_ERR_VALUE, "the largest leaf must have next_val = next_idx = 0");
    if (perr & prep::ERR_FOREIGN)
        return c->fail(IMT_ERR_VALUE, "a value belongs to another subtree (v %% %u != %u)", t->part_mod, t->part_res);
    if (perr) return c->fail(IMT_ERR_INTERNAL, "snapshot check: unexpected error bits %d", perr);
    // ---- device rebuild: nothing of the tree has been written up to here ----
    if ((rc = c->clear_err())) return rc;
    prep::load_commit(s, d_pre, (uint32_t)n, t->d_val);
    IMT_HIP(c, hipMemcpyAsync(t->d_sorted[t->sorted_cur], d_order, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    for (unsigned l = 0; l <= t->depth; l++)
        launch::fill_level(s, t->nodes(l), t->h_len[l], c->d_zero + (size_t)l * 32);
    launch::hash_batch(s, d_pre, t->d_nodes, (size_t)n, 3, IMT_FMT_CANONICAL, IMT_FMT_DEVICE, c->d_err);
    uint64_t filled = n;
    for (unsigned l = 0; l < t->depth; l++) {
        const uint64_t parents = (filled + 1) / 2;
        if (t->h_len[l] >= 2) {
            launch::tree_level(s, t->nodes(l), t->nodes(l + 1), parents);
        } else {   // a single stored node: its sibling is the empty subtree of this height
            IMT_HIP(c, hipMemcpyAsync(t->nodes(l + 1), t->nodes(l), 32, hipMemcpyDeviceToDevice, s));
            launch::extend_root(s, t->nodes(l + 1), c->d_zero, l, l + 1);
        }
        filled = parents;
    }
    rc = c->sync_and_check();
    if (rc) return rc;
    // the device index is the tree's list now; the host mirror is rebuilt from it if a host-side call asks (ensure_mirror)
    t->pre.clear();
    t->pre.shrink_to_fit();
    t->sorted.clear();
    t->sorted.shrink_to_fit();
    t->size = n;
    t->mirror_valid = false;
    t->dev_index_valid = true;
    t->pending.active = false;
    t->gen++;
    for (auto& pl : t->plan) pl.has_root = pl.has_root2 = false;
    return IMT_OK;
}

// The tree of a value log: what a fresh tree holds after imt_itree_apply_batch(vals, n).  imt_itree_load's sequence with
// the values in the preimages' place: the same sort, a check that asks what the walk would refuse instead of whether the
// links close, and leaf hashes that read the successor through the order (launch::index_leaves) instead of from a
// [n][3][32] array nobody has.
extern "C" int imt_itree_load_values(imt_itree* t, const void* vals, uint64_t n, uint64_t* bad_pos, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (!vals || n == 0) return c->fail(IMT_ERR_ARG, "null / empty value log");
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (n >= t->cap) return c->fail(IMT_ERR_FULL, "%llu values and the sentinel make %llu leaves, capacity is %llu",
                                    (unsigned long long)n, (unsigned long long)n + 1, (unsigned long long)t->cap);
    if (slice_open(t)) return c->fail(IMT_ERR_ARG, "a slice is open (issue its remaining units first)");
    int rc = c->set_device();
    if (rc) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    if ((rc = check_fe_ptrs(c, dev, {vals}))) return rc;
    if ((rc = join_top(t))) return rc;
    for (auto& pl : t->plan)
        if (pl.in_flight) { IMT_HIP(c, hipEventSynchronize(pl.done)); pl.in_flight = false; pl.pipelined = false; }
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    hipStream_t s = c->stream;
    const ScratchTrim trim{c, 2, 3};
    const size_t ws_bytes = prep::load_values_ws_bytes((size_t)n);
    uint8_t* ws = (uint8_t*)c->dev_scratch(3, ws_bytes + 256);      // [error word, offending position | 256-byte aligned workspace]
    if (!ws) return IMT_ERR_HIP;
    int* d_perr = (int*)ws;
    uint32_t* d_bad = (uint32_t*)(ws + 4);
    // ---- the canonical values on the device: the caller's own memory if that is what it holds ----
    const uint8_t* d_can = (const uint8_t*)vals;
    int raw_err = 0;
    uint32_t raw_bad = 0xffffffffu;
    if (!dev || fmt != IMT_FMT_CANONICAL) {
        uint8_t* buf = (uint8_t*)c->dev_scratch(2, (size_t)n * 32);
        if (!buf) return IMT_ERR_HIP;
        if (!dev) IMT_HIP(c, hipMemcpyAsync(buf, vals, (size_t)n * 32, hipMemcpyHostToDevice, s));
        if (fmt != IMT_FMT_CANONICAL) {
            // every format refuses an encoding >= p, and the conversion reduces it: found here, on the bytes as they came
            IMT_HIP(c, hipMemsetAsync(d_perr, 0, sizeof(int), s));
            IMT_HIP(c, hipMemsetAsync(d_bad, 0xff, sizeof(uint32_t), s));
            prep::first_noncanonical(s, dev ? d_can : buf, (uint32_t)n, d_perr, d_bad);
            IMT_HIP(c, hipMemcpyAsync(&raw_err, d_perr, sizeof(int), hipMemcpyDeviceToHost, s));
            IMT_HIP(c, hipMemcpyAsync(&raw_bad, d_bad, sizeof(raw_bad), hipMemcpyDeviceToHost, s));
            if ((rc = c->clear_err())) return rc;
            launch::convert(s, dev ? d_can : buf, buf, (size_t)n, fmt, IMT_FMT_CANONICAL, c->d_err);
        }
        d_can = buf;
    }
    // ---- the check: ordered by (value, position), every rank against its predecessor ----
    const uint32_t* d_order = nullptr;
    int perr = 0;
    uint32_t bad = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        IMT_HIP(c, hipMemsetAsync(d_perr, 0, sizeof(int), s));
        IMT_HIP(c, hipMemsetAsync(d_bad, 0xff, sizeof(uint32_t), s));
        IMT_HIP(c, prep::load_values_check(s, d_can, (uint32_t)n, t->part_mod, t->part_res, ws + 256, ws_bytes, attempt == 1,
                                           d_perr, d_bad, &d_order));
        IMT_HIP(c, hipMemcpyAsync(&perr, d_perr, sizeof(int), hipMemcpyDeviceToHost, s));
        IMT_HIP(c, hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, s));
        IMT_HIP(c, hipStreamSynchronize(s));
        // values that agree in their top 64 bits and came out of the radix sort in the wrong order: sort with the full
        // comparator and check again (the other bits of a first attempt that tied mean nothing)
        if (!(perr & prep::LOAD_TIE)) break;
    }
    perr |= raw_err;
    bad = std::min(bad, raw_bad);
    if (perr & (prep::ERR_NONCANONICAL | prep::ERR_ZERO | prep::ERR_FOREIGN | prep::ERR_DUPLICATE)) {
        if (bad_pos && bad < n) *bad_pos = bad;
        return insertion_verdict(t, perr, "log");
    }
    if (perr) return c->fail(IMT_ERR_INTERNAL, "value log check: unexpected error bits %d", perr);
    // ---- device rebuild: nothing of the tree has been written up to here ----
    if ((rc = c->clear_err())) return rc;
    const uint64_t M = n + 1;
    prep::load_values_commit(s, d_can, d_order, (uint32_t)n, t->d_val, t->d_sorted[t->sorted_cur]);
    for (unsigned l = 0; l <= t->depth; l++)
        launch::fill_level(s, t->nodes(l), t->h_len[l], c->d_zero + (size_t)l * 32);
    launch::index_leaves(s, t->d_val, t->d_sorted[t->sorted_cur], (uint32_t)M, t->index_base, t->d_nodes, c->d_err);
    uint64_t filled = M;
    for (unsigned l = 0; l < t->depth; l++) {
        const uint64_t parents = (filled + 1) / 2;
        if (t->h_len[l] >= 2) {
            launch::tree_level(s, t->nodes(l), t->nodes(l + 1), parents);
        } else {   // a single stored node: its sibling is the empty subtree of this height
            IMT_HIP(c, hipMemcpyAsync(t->nodes(l + 1), t->nodes(l), 32, hipMemcpyDeviceToDevice, s));
            launch::extend_root(s, t->nodes(l + 1), c->d_zero, l, l + 1);
        }
        filled = parents;
    }
    rc = c->sync_and_check();
    if (rc) return rc;
    t->pre.clear();
    t->pre.shrink_to_fit();
    t->sorted.clear();
    t->sorted.shrink_to_fit();
    t->size = M;
    t->mirror_valid = false;
    t->dev_index_valid = true;
    t->pending.active = false;
    t->gen++;
    for (auto& pl : t->plan) pl.has_root = pl.has_root2 = false;
    return IMT_OK;
}

// values of leaves [first, first + n) (global indices) of the tree, or of the tree as of a view's size: rows of d_val
static int get_values(imt_itree* t, uint64_t size, uint64_t first, size_t n, void* vals, unsigned flags) {
    imt_ctx* c = t->ctx;
    if (n == 0) return IMT_OK;
    if (!vals) return c->fail(IMT_ERR_ARG, "null buffer");
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    int rc;
    if ((rc = check_fe_ptrs(c, dev, {vals}))) return rc;
    const uint64_t lo = first - t->index_base;                    // wraps below the base: out of range
    if (lo >= size || n > size - lo)
        return c->fail(IMT_ERR_RANGE, "leaves [%llu, %llu) are not all below the size %llu", (unsigned long long)first,
                       (unsigned long long)(first + n), (unsigned long long)(t->index_base + size));
    if ((rc = ensure_device_index(t))) return rc;
    if ((rc = join_top(t))) return rc;
    hipStream_t s = c->stream;
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));     // the index may have been written on the side stream
    const uint8_t* src = t->d_val + lo * 32;
    if (dev) {
        if (fmt == IMT_FMT_CANONICAL) IMT_HIP(c, hipMemcpyAsync(vals, src, n * 32, hipMemcpyDeviceToDevice, s));
        else launch::convert(s, src, (uint8_t*)vals, n, IMT_FMT_CANONICAL, fmt, c->d_err);
        return IMT_OK;
    }
    if (fmt != IMT_FMT_CANONICAL) {
        uint8_t* d_out = (uint8_t*)c->dev_scratch(1, n * 32);
        if (!d_out) return IMT_ERR_HIP;
        launch::convert(s, src, d_out, n, IMT_FMT_CANONICAL, fmt, c->d_err);
        src = d_out;
    }
    IMT_HIP(c, hipMemcpyAsync(vals, src, n * 32, hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipStreamSynchronize(s));
    c->trim_scratch(1, (size_t)64 << 20);
    return IMT_OK;
}
extern "C" int imt_itree_get_values(imt_itree* t, uint64_t first, size_t n, void* vals, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    int rc = c->set_device();
    return rc ? rc : get_values(t, t->size, first, n, vals, flags);
}

// ------------------------------------------------------------------------------------
// batch insertion
// ------------------------------------------------------------------------------------
namespace {

const int64_t REF_NONE = INT64_MIN;   // "no successor" in the host path's neighbour references
const U256 U256_ZERO = {0, 0, 0, 0};

// Host prepare (IMT_HOST_PREP).  Neighbour references: >= 0 -> rank of a batch element in value order;
// < 0 -> ~(leaf index of a stored leaf); REF_NONE.
struct HostPlan {
    std::vector<U256> v;                      // batch values in insertion order, canonical
    std::vector<uint8_t> lowleaf, newleaf;    // hash-free outputs, if requested
    uint64_t M = 0;
};

inline uint64_t ref_leaf(const imt_itree* t, const HostPlan& hp, int64_t ref) {
    return ref >= 0 ? hp.M + t->w_ord[(size_t)ref] : (uint64_t)~ref;
}
inline const U256& ref_val(const imt_itree* t, const HostPlan& hp, int64_t ref) {
    return ref >= 0 ? hp.v[t->w_ord[(size_t)ref]] : t->pre[(size_t)~ref].val;
}

// Sections of the host path: (1) values to the host, (2) low leaf of every insertion
// (update_idx_leaf :639-658 as a predecessor search: sort the batch, locate each value between two
// stored leaves, then unlink the batch from that list in reverse insertion order -- what is adjacent at
// unlink time is exactly what had been inserted earlier), (4) event preimages and their (position,
// time) order into the pinned staging of P, (5) upload on the side stream.
int host_prepare(imt_itree* t, PlanSet& P, const void* vals, size_t n, unsigned flags, bool want_lowleaf,
                 bool want_newleaf, HostPlan& hp) {
    imt_ctx* c = t->ctx;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const uint64_t M = hp.M = t->size;
    const size_t E = 2 * n;
    int rc = ensure_mirror(t);
    if (rc) return rc;
    // With device pointers the values are read on the side stream, so the call does not wait for an
    // earlier batch that is still running.
    std::vector<U256>& v = hp.v;
    if ((rc = fetch_canonical(c, dev ? t->up_stream : c->stream, vals, n, flags, v))) return rc;

    std::vector<uint32_t>& ord = t->w_ord;
    {
        std::vector<std::pair<uint64_t, uint32_t>>& sk = t->w_sortkey;   // (top limb, index): cheap compares
        sk.resize(n);
        for (size_t i = 0; i < n; i++) sk[i] = {v[i][3], (uint32_t)i};
        std::sort(sk.begin(), sk.end(),
                  [&](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) {
                      if (a.first != b.first) return a.first < b.first;
                      return lt256(v[a.second], v[b.second]);
                  });
        ord.resize(n);
        for (size_t i = 0; i < n; i++) ord[i] = sk[i].second;
    }
    if (is_zero256(v[ord[0]])) return c->fail(IMT_ERR_VALUE, "value 0 cannot be inserted");
    if (t->part_mod > 1)
        for (size_t i = 0; i < n; i++)
            if (prep::mod_small(reinterpret_cast<const uint8_t*>(v[i].data()), t->part_mod) != t->part_res)
                return c->fail(IMT_ERR_VALUE, "a value belongs to another subtree (v %% %u != %u)", t->part_mod, t->part_res);
    for (size_t r = 1; r < n; r++)
        if (v[ord[r]] == v[ord[r - 1]]) return c->fail(IMT_ERR_VALUE, "duplicate value inside the batch");
    std::vector<int64_t>&prv = t->w_prv, &nxt = t->w_nxt;
    prv.resize(n);
    nxt.resize(n);
    {
        size_t q = 0;   // first stored entry with val >= current
        const size_t S = t->sorted.size();
        for (size_t r = 0; r < n; r++) {
            const U256& x = v[ord[r]];
            while (q < S && cmp_ent(t, t->sorted[q], x) < 0) q++;
            if (q < S && cmp_ent(t, t->sorted[q], x) == 0) return c->fail(IMT_ERR_VALUE, "value already in the tree");
            // q >= 1 because the sentinel 0 is stored and x > 0
            const bool same_gap_prev = r > 0 && cmp_ent(t, t->sorted[q - 1], v[ord[r - 1]]) < 0;
            prv[r] = same_gap_prev ? (int64_t)(r - 1) : ~(int64_t)t->sorted[q - 1].idx;
            const bool next_in_gap = r + 1 < n && (q >= S || cmp_ent(t, t->sorted[q], v[ord[r + 1]]) > 0);
            nxt[r] = next_in_gap ? (int64_t)(r + 1) : (q < S ? ~(int64_t)t->sorted[q].idx : REF_NONE);
        }
    }
    std::vector<uint32_t>& rank_of = t->w_rank;
    rank_of.resize(n);
    for (size_t r = 0; r < n; r++) rank_of[ord[r]] = (uint32_t)r;
    std::vector<int64_t>&pred = t->w_pred, &succ = t->w_succ;   // by insertion time
    pred.resize(n);
    succ.resize(n);
    for (size_t ii = n; ii-- > 0;) {
        const uint32_t r = rank_of[ii];
        pred[ii] = prv[r];
        succ[ii] = nxt[r];
        if (prv[r] >= 0) nxt[prv[r]] = nxt[r];
        if (nxt[r] >= 0) prv[nxt[r]] = prv[r];
    }

    // events: preimages at every time step + the hash-free outputs
    uint8_t* h_pre = P.h_pin;
    uint32_t* h_tab = reinterpret_cast<uint32_t*>(P.h_pin + P.cap_events * 96);
    uint32_t *h_node = h_tab, *h_time = h_tab + P.cap_events, *h_rs = h_tab + 2 * P.cap_events,
             *h_re = h_tab + 3 * P.cap_events;
    std::vector<uint64_t>& o_low = t->w_low;
    std::vector<uint8_t>& o_largest = t->w_largest;
    o_low.resize(n);
    o_largest.resize(n);
    hp.lowleaf.assign(want_lowleaf ? n * 96 : 0, 0);
    hp.newleaf.assign(want_newleaf ? n * 96 : 0, 0);
    std::vector<uint64_t>& keys = t->w_keys;   // (pos << 32) | event
    keys.resize(E);
    for (size_t i = 0; i < n; i++) {
        const uint64_t low = ref_leaf(t, hp, pred[i]);
        const U256& lowval = ref_val(t, hp, pred[i]);
        const bool has_succ = succ[i] != REF_NONE;
        const U256& sval = has_succ ? ref_val(t, hp, succ[i]) : U256_ZERO;
        const uint64_t sidx = has_succ ? t->index_base + ref_leaf(t, hp, succ[i]) : 0;
        o_low[i] = low;
        o_largest[i] = has_succ ? 0 : 1;                               // :737-742
        if (want_lowleaf) put_pre(&hp.lowleaf[i * 96], lowval, sval, sidx);
        put_pre(h_pre + (2 * i) * 96, lowval, v[i], t->index_base + M + i);   // low leaf rewritten :655-656
        put_pre(h_pre + (2 * i + 1) * 96, v[i], sval, sidx);           // new leaf inherits :650-654
        if (want_newleaf) std::memcpy(&hp.newleaf[i * 96], h_pre + (2 * i + 1) * 96, 96);
        keys[2 * i] = (low << 32) | (uint64_t)(2 * i);
        keys[2 * i + 1] = ((M + i) << 32) | (uint64_t)(2 * i + 1);
    }
    {   // stable LSD radix sort on the 32-bit position (two 16-bit passes); events are already in time order
        std::vector<uint64_t>& tmp = t->w_keys2;
        std::vector<uint32_t>& hist = t->w_hist;
        tmp.resize(E);
        hist.resize(1u << 16);
        for (int pass = 0; pass < 2; pass++) {
            const int sh = 32 + 16 * pass;
            std::vector<uint64_t>& src = pass ? tmp : keys;
            std::vector<uint64_t>& dst = pass ? keys : tmp;
            std::fill(hist.begin(), hist.end(), 0u);
            for (size_t x = 0; x < E; x++) hist[(src[x] >> sh) & 0xffff]++;
            uint32_t run = 0;
            for (auto& hcount : hist) { const uint32_t cnt = hcount; hcount = run; run += cnt; }
            for (size_t x = 0; x < E; x++) dst[hist[(src[x] >> sh) & 0xffff]++] = src[x];
        }
    }
    for (size_t k = 0; k < E;) {
        size_t j = k;
        const uint32_t pos = (uint32_t)(keys[k] >> 32);
        while (j < E && (uint32_t)(keys[j] >> 32) == pos) j++;
        for (size_t x = k; x < j; x++) {
            h_node[x] = pos;
            h_time[x] = (uint32_t)keys[x];
            h_rs[x] = (uint32_t)k;
            h_re[x] = (uint32_t)j;
        }
        k = j;
    }
    IMT_HIP(c, hipMemcpyAsync(P.d_pre, h_pre, E * 96, hipMemcpyHostToDevice, t->up_stream));
    IMT_HIP(c, hipMemcpyAsync(P.d_tab[0][0], h_node, E * 4, hipMemcpyHostToDevice, t->up_stream));
    IMT_HIP(c, hipMemcpyAsync(P.d_tab[0][1], h_time, E * 4, hipMemcpyHostToDevice, t->up_stream));
    IMT_HIP(c, hipMemcpyAsync(P.d_tab[0][2], h_rs, E * 4, hipMemcpyHostToDevice, t->up_stream));
    IMT_HIP(c, hipMemcpyAsync(P.d_tab[0][3], h_re, E * 4, hipMemcpyHostToDevice, t->up_stream));
    return IMT_OK;
}

// host mirror after a host-prepared batch: new preimages, rewritten low leaves, merged sorted index
void host_commit(imt_itree* t, const HostPlan& hp, size_t n) {
    const uint64_t M = hp.M;
    const std::vector<U256>& v = hp.v;
    t->dev_index_valid = false;
    t->pre.resize(M + n);
    for (size_t i = 0; i < n; i++) {
        const bool has_succ = t->w_succ[i] != REF_NONE;
        Pre& lowp = t->pre[t->w_low[i]];
        Pre& np = t->pre[M + i];
        np.val = v[i];
        np.next_val = has_succ ? ref_val(t, hp, t->w_succ[i]) : U256_ZERO;
        np.next_idx = has_succ ? ref_leaf(t, hp, t->w_succ[i]) : 0;
        lowp.next_val = v[i];
        lowp.next_idx = M + i;
    }
    std::vector<SortedEnt>& merged = t->w_merged;
    merged.clear();
    merged.reserve(t->sorted.size() + n);
    size_t q = 0;
    for (size_t r = 0; r < n; r++) {
        const U256& x = v[t->w_ord[r]];
        while (q < t->sorted.size() && cmp_ent(t, t->sorted[q], x) < 0) merged.push_back(t->sorted[q++]);
        merged.push_back(SortedEnt{x[3], M + t->w_ord[r]});
    }
    while (q < t->sorted.size()) merged.push_back(t->sorted[q++]);
    t->sorted.swap(merged);
    t->size = M + n;
}

// Where the kernels write an output the caller asked for: the caller's own array with device pointers, otherwise the
// context's next scratch slot, copied back at the end of the call.  False: that scratch could not be had.
template <class T>
bool stage_out(imt_ctx* c, bool dev, size_t& slot, T* user, size_t bytes, T*& d) {
    d = !user ? nullptr : dev ? user : (T*)c->dev_scratch(slot++, bytes);
    return !user || d;
}

// GPU prepare (default): the same on the device (imt_prep.hip), on the side stream.  `val_flags` say where the values
// are and in which format, `dev` where the outputs go.  The hash-free outputs go straight to device buffers (the user's,
// or scratch in host-pointer mode), noted in `d`.  The batch is committed to the device index only if its values are
// acceptable.
int gpu_prepare(imt_itree* t, PlanSet& P, const void* vals, unsigned val_flags, size_t n, const imt_insert_out* out, bool dev,
                size_t& slot, imt_insert_out& d, double& wait_ms) {
    imt_ctx* c = t->ctx;
    int rc = ensure_device_index(t);
    if (rc) return rc;
    hipStream_t ps = t->up_stream;
    const uint8_t* d_vals = nullptr;
    uint8_t* up = (val_flags & IMT_DEVICE_PTRS) ? nullptr : (uint8_t*)c->dev_scratch(slot++, n * 32);
    // converted into the plan's own buffer, not context scratch: this runs on the side stream, which IMT_INPUTS_READY
    // leaves unordered behind the context's stream, where an earlier asynchronous call (imt_itree_lift_batch,
    // imt_insert_trace_batch) may still be using the context's scratch slots
    if ((rc = stage_canonical(c, ps, vals, n, val_flags, up, P.d_canon, P.ws.err, &d_vals))) return rc;
    if (out && (!stage_out(c, dev, slot, out->low_index, n * 8, d.low_index) ||
                !stage_out(c, dev, slot, out->is_largest, n, d.is_largest) ||
                !stage_out(c, dev, slot, out->low_leaf, n * 96, d.low_leaf) ||
                !stage_out(c, dev, slot, out->new_leaf, n * 96, d.new_leaf)))
        return IMT_ERR_HIP;
    P.ws.part_mod = t->part_mod;
    P.ws.part_res = t->part_res;
    IMT_HIP(c, prep::run(ps, P.ws, d_vals, t->d_val, t->d_sorted[t->sorted_cur], t->d_sorted[t->sorted_cur ^ 1],
                         (uint32_t)t->size, (uint32_t)n, t->index_base, P.d_pre, P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][2],
                         P.d_tab[0][3], d.low_index, d.is_largest, (uint8_t*)d.low_leaf, (uint8_t*)d.new_leaf));
    IMT_HIP(c, hipMemcpyAsync(t->h_err_pin, P.ws.err, sizeof(int), hipMemcpyDeviceToHost, ps));
    const HostTimer w;
    IMT_HIP(c, hipStreamSynchronize(ps));
    wait_ms += w.ms();
    // accepted: the merged index sits in d_sorted[sorted_cur ^ 1]; the caller flips when it commits
    return insertion_verdict(t, *t->h_err_pin, "batch");
}

// The pipeline context of a batch's hashing (imt_apply_pipe.hpp); the defaults are "on the context's stream, alone"
struct PipeCtx {
    const PlanSet* prev = nullptr;        // the batch in front, if it is still on a pipeline stream: whose events are waited for
    bool pipelined = false;               // this batch is on a pipeline stream and records its own per-level events
};
// What a witness sweep is run for: an insertion batch into the live tree (all defaults), a mixed batch (route), a replay
// through a view (side, the view's root, nothing stored), or both.  Plain data, read by the steps below.
struct WitnessSweep {
    const launch::MixedRoute* route = nullptr;    // NULL: event e fills the rows of insertion e / 2; else erow says whose
    size_t n_ins = 0;                             // with a route: the INSERTs among the operations,
    uint8_t* read_root = nullptr;                 // and the READs' roots (NULL: not wanted)
    bool bulk = false;                            // every event is a row's ROW_LOW (imt_itree_insert_bulk): d.old_root / d.interim_root
                                                  // are its root_before / root_after, chained by the roots kernel
    const view::Side* side = nullptr;             // NULL: base siblings below L0 are read from the stored tree as it is
    bool store = true;                            // levels written back, the nodes from L0 up and the root stored
    const uint8_t* view_root = nullptr;           // NULL: old_root[0] is the stored root; else the root in a view's chain
    uint8_t* frontier = nullptr;                  // a bulk replay (imt_itree_view_bulk_witness): [depth][32] device format, where
    uint64_t frontier_size = 0;                   // the final versions of the frontier of slot frontier_size are picked up
    PipeCtx pipe;                                 // imt_itree_insert_batch under IMT_PIPELINE, imt_itree_mixed_pipelined
};

// ---- one step each of the witness schedule on stream s, with its profile brackets.  `d` holds the device pointers of
// the outputs (NULL: not wanted), `lay` the layout of its sibling arrays, `fmt` the format of both; `w` picks the launch. ----
void sweep_leaf_hashes(imt_itree* t, const PlanSet& P, hipStream_t s, size_t E) {
    imt_ctx* c = t->ctx;
    const int pf = c->prof_begin(IMT_PROF_LEAVES, s);
    launch::sweep_leaves(s, P.d_pre, P.d_tab[0][1], P.d_val[0], 0, (uint32_t)E, IMT_FMT_CANONICAL, c->d_err, c->coop_max_events);
    c->prof_end(pf, s);
}
// level l < L0 -> l + 1: reads the stored level l, which the caller has made sure holds what came before this batch --
// or, through a view's side table, what it held at the view's size
void sweep_one_level(imt_itree* t, const PlanSet& P, hipStream_t s, unsigned l, size_t E, const imt_insert_out& d,
                     launch::SibLayout lay, unsigned fmt, const WitnessSweep& w = {}) {
    imt_ctx* c = t->ctx;
    const PlanSet::Level row = P.level(l);
    const uint8_t *in = P.d_val[l & 1], *zero = c->d_zero + (size_t)l * 32;
    uint8_t *out = P.d_val[(l & 1) ^ 1], *low_sib = (uint8_t*)d.low_sib, *new_sib = (uint8_t*)d.new_sib;
    const uint32_t coop = c->coop_max_events;
    const int pf = c->prof_begin(IMT_PROF_LEVEL, s);
    if (w.route && w.side)
        launch::sweep_view_level_mixed(s, *w.side, *w.route, in, out, row.from, row.sibsrc, row.nodeb, row.timen, t->nodes(l),
                                       t->h_len[l], zero, (uint32_t)E, low_sib, new_sib, lay, l, fmt, coop);
    else if (w.route)
        launch::sweep_level_mixed(s, *w.route, in, out, row.from, row.sibsrc, row.nodeb, row.timen, t->nodes(l), t->h_len[l], zero,
                                  (uint32_t)E, low_sib, new_sib, lay, l, fmt, coop);
    else if (w.side)
        launch::sweep_view_level(s, *w.side, in, out, row.from, row.sibsrc, row.nodeb, row.timen, t->nodes(l), t->h_len[l], zero,
                                 (uint32_t)E, low_sib, new_sib, lay, l, fmt, coop);
    else
        launch::sweep_level(s, in, out, row.from, row.sibsrc, row.nodeb, row.timen, t->nodes(l), t->h_len[l], zero, 0, (uint32_t)E,
                            low_sib, new_sib, lay, l, fmt, coop);
    c->prof_end(pf, s);
}
// old_root[0] is the root the batch before left -- read right before the launch that overwrites the stored root -- or the
// root of the view a replay starts from
void read_old_root(imt_itree* t, hipStream_t s, const imt_insert_out& d, unsigned fmt, const WitnessSweep& w = {}) {
    const uint8_t* src = w.view_root ? w.view_root : t->nodes(t->depth);
    if (d.old_root) launch::convert(s, src, (uint8_t*)d.old_root, 1, IMT_FMT_DEVICE, fmt, t->ctx->d_err);
}
// level l >= L0 -> l + 1: every event alone in node 0 against the empty subtree of that height.  Ordinary launches of
// the same kernel, so consecutive batches overlap here level by level as well; unless nothing is stored, the last event's
// node of every level goes back to the stored tree.
void sweep_one_upper(imt_itree* t, const PlanSet& P, hipStream_t s, unsigned l, size_t E, unsigned L0, const imt_insert_out& d,
                     launch::SibLayout lay, unsigned fmt, const WitnessSweep& w = {}) {
    imt_ctx* c = t->ctx;
    const uint8_t *in = P.d_val[l & 1], *zero = c->d_zero + (size_t)l * 32;
    uint8_t *out = P.d_val[(l & 1) ^ 1], *low_sib = (uint8_t*)d.low_sib, *new_sib = (uint8_t*)d.new_sib;
    uint8_t *node_in = w.store && l == L0 ? t->nodes(l) : nullptr, *node_out = w.store ? t->nodes(l + 1) : nullptr;
    const int pf = c->prof_begin(IMT_PROF_TOP, s);
    if (w.route)
        launch::sweep_upper_mixed(s, *w.route, in, out, zero, (uint32_t)E, node_in, node_out, low_sib, new_sib, lay, l, fmt,
                                  c->coop_max_events);
    else
        launch::sweep_upper(s, in, out, zero, 0, (uint32_t)E, w.store ? (uint32_t)E - 1 : 0xffffffffu, node_in, node_out, low_sib,
                            new_sib, lay, l, fmt, c->coop_max_events);
    c->prof_end(pf, s);
}
// the roots of every event from the top values; a batch that fills the tree to its full depth stores its root here
void finish_roots(imt_itree* t, const PlanSet& P, hipStream_t s, size_t E, unsigned L0, const imt_insert_out& d, unsigned fmt,
                  const WitnessSweep& w = {}) {
    const uint8_t* top = P.d_val[t->depth & 1];
    uint8_t* node_store = w.store && L0 == t->depth ? t->nodes(t->depth) : nullptr;
    if (w.bulk)
        launch::emit_roots_bulk(s, top, (uint32_t)E, (uint8_t*)d.old_root, (uint8_t*)d.interim_root, fmt, node_store);
    else if (w.route)
        launch::emit_roots_mixed(s, *w.route, top, (uint32_t)E, (uint32_t)w.n_ins, (uint8_t*)d.old_root, (uint8_t*)d.interim_root,
                                 (uint8_t*)d.new_root, w.read_root, fmt, node_store);
    else
        launch::emit_roots(s, top, 0, (uint32_t)E, (uint32_t)E, (uint8_t*)d.old_root, (uint8_t*)d.interim_root,
                           (uint8_t*)d.new_root, fmt, nullptr, node_store);
}

}  // namespace

// apply != NULL: imt_itree_apply_batch / _apply_filtered -- same preparation, same commit, but the hashing is the
// witness-free schedule (apply_hashes) and the only output is the root.
struct ApplyReq {
    void* root_out;
};
// The order between consecutive batches on the pipeline streams (imt_apply_pipe.hpp): launch x of a batch of `kind`
// waits for the event of the batch in front that the rule names, and records the event the rule names.  A batch that is
// not on a pipeline stream has nobody in front and records nothing.
static int pipe_wait(imt_itree* t, hipStream_t s, const PipeCtx& pipe, apipe::Kind kind, unsigned L0, apipe::Launch x) {
    const PlanSet* prev = pipe.prev;
    if (!prev) return IMT_OK;
    const apipe::Event e = apipe::waits(prev->applied ? apipe::APPLY : apipe::WITNESS, prev->l0, kind, L0, t->depth, x);
    if (e.type == apipe::EV_NONE) return IMT_OK;
    IMT_HIP(t->ctx, hipStreamWaitEvent(s, e.type == apipe::EV_LEVEL ? prev->wb_done[e.l] : prev->done, 0));
    return IMT_OK;
}
static int pipe_record(imt_itree* t, hipStream_t s, PlanSet& P, const PipeCtx& pipe, apipe::Kind kind, unsigned L0, apipe::Launch x) {
    if (!pipe.pipelined) return IMT_OK;
    const apipe::Event e = apipe::records(kind, L0, t->depth, x);
    if (e.type == apipe::EV_LEVEL) IMT_HIP(t->ctx, hipEventRecord(P.wb_done[e.l], s));
    return IMT_OK;
}

// The witness schedule on stream s, behind the preparation: leaf hashes, index phase (no hashing), then the hash sweep
// level by level -- with each level's write-back unless nothing is stored -- and the roots.  Every witness there is comes
// through here; `w` says which: imt_itree_insert_batch, a mixed batch (of either: w.pipe.prev is the batch before this one
// if it is still on a pipeline stream -- this batch then runs one level behind it), or a replay of either through a view.
static int witness_sweep(imt_itree* t, PlanSet& P, hipStream_t s, size_t E, unsigned L0, const imt_insert_out& d,
                         launch::SibLayout lay, unsigned fmt, const WitnessSweep& w) {
    imt_ctx* c = t->ctx;
    sweep_leaf_hashes(t, P, s, E);
    int pf = c->prof_begin(IMT_PROF_INDEX, s);
    index_phase(P, s, E, L0, nullptr);
    c->prof_end(pf, s);
    int rc;
    for (unsigned l = 0; l < L0; l++) {
        // stored level l must hold the previous batch's final versions: its write-back of that level,
        // or (at and above its L0) its top kernel
        if ((rc = pipe_wait(t, s, w.pipe, apipe::WITNESS, L0, {apipe::WI_LEVEL, l}))) return rc;
        sweep_one_level(t, P, s, l, E, d, lay, fmt, w);
        // the versions of level l live until the launch after next: what the write-back would store of the frontier's node
        if (w.frontier)
            launch::bulk_frontier_level(s, w.frontier_size, l, P.d_val[l & 1], P.level(l).from, P.level(l).nodeb, (uint32_t)E,
                                        w.frontier + (size_t)l * 32);
        if (!w.store) continue;
        pf = c->prof_begin(IMT_PROF_WRITEBACK, s);
        launch::writeback(s, P.d_val[l & 1], P.level(l).from, P.level(l).nodeb, t->nodes(l), (uint32_t)E);
        c->prof_end(pf, s);
        if ((rc = pipe_record(t, s, P, w.pipe, apipe::WITNESS, L0, {apipe::WI_LEVEL, l}))) return rc;
    }
    // right before the first launch that writes the stored root; a sweep that stores nothing reads it before the roots
    auto old_root = [&]() -> int {
        const int r = pipe_wait(t, s, w.pipe, apipe::WITNESS, L0, {apipe::WI_OLD_ROOT, 0});
        if (r) return r;
        read_old_root(t, s, d, fmt, w);
        return IMT_OK;
    };
    for (unsigned l = L0; l < t->depth; l++) {
        if (w.store && l + 1 == t->depth && (rc = old_root())) return rc;
        // the previous batch stored node l + 1 (and node l, at its own L0) from its launch of this level
        if ((rc = pipe_wait(t, s, w.pipe, apipe::WITNESS, L0, {apipe::WI_UPPER, l}))) return rc;
        uint32_t last;      // node 0 of level L0 after the last event: what the live sweep stores through node_in
        if (w.frontier && l == L0 && replay::frontier_top_version(w.frontier_size, L0, (uint32_t)E, last))
            IMT_HIP(c, hipMemcpyAsync(w.frontier + (size_t)l * 32, P.d_val[l & 1] + (size_t)last * 32, 32, hipMemcpyDeviceToDevice, s));
        sweep_one_upper(t, P, s, l, E, L0, d, lay, fmt, w);
        if ((rc = pipe_record(t, s, P, w.pipe, apipe::WITNESS, L0, {apipe::WI_UPPER, l}))) return rc;
    }
    if ((!w.store || L0 == t->depth) && (rc = old_root())) return rc;
    if ((rc = pipe_wait(t, s, w.pipe, apipe::WITNESS, L0, {apipe::WI_ROOTS, 0}))) return rc;
    finish_roots(t, P, s, E, L0, d, fmt, w);
    return IMT_OK;
}

// The witness-free schedule (imt_apply.hpp) on stream s, behind the preparation: the lists of every level (index work),
// the touched leaves from their final preimages, then level by level every touched parent from the stored level below --
// which the launch before has just made final -- and from level L0 - 1 up the single chain to the root.  The launches
// are sized by host-side bounds; the counts stay on the device (`count`, [depth + 1]), so nothing here waits for the GPU.
// imt_itree_rewind hashes through here too: its table has one event per touched leaf, its L0 is that of the size it finds
// and its counts are its own.
// On a pipeline stream (imt_itree_apply_pipelined, imt_itree_apply_mixed_pipelined; `count` is then the plan set's) the
// batch in front may be two launches ahead: every launch that writes a stored level first waits for the event imt_apply_pipe.hpp names -- an apply batch in
// front reads level l in the launch AFTER the one that wrote it -- and records its own; and the chain to the root is
// hashed into the plan set's rows (k_apply_chain), beside the chains of the batches in front, with only the store of those
// rows into the tree and into P.d_root ordered behind them.
static int apply_hashes(imt_itree* t, PlanSet& P, hipStream_t s, size_t E, unsigned L0, uint64_t* count, const PipeCtx& pipe = {}) {
    imt_ctx* c = t->ctx;
    const apply::Lists lists{P.d_nodeb, P.d_timen, count, P.cap_events};
    int rc, pf = c->prof_begin(IMT_PROF_APPLY_LISTS, s);
    IMT_HIP(c, prep::apply_lists(s, P.ws.tmp, P.ws.tmp_bytes, P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][3], (uint32_t)E, L0,
                                 t->depth, P.d_from, lists));
    c->prof_end(pf, s);
    if ((rc = pipe_wait(t, s, pipe, apipe::APPLY, L0, {apipe::AP_LEVEL, 0}))) return rc;
    pf = c->prof_begin(IMT_PROF_APPLY_LEAVES, s);
    launch::apply_leaves(s, lists.count, apply::bound((uint32_t)E, L0, 0), lists.node, lists.src, P.d_pre, IMT_FMT_CANONICAL,
                         c->d_err, t->nodes(0), t->h_len[0], c->coop_max_events);
    c->prof_end(pf, s);
    for (unsigned l = 0; l + 1 < L0; l++) {
        if ((rc = pipe_wait(t, s, pipe, apipe::APPLY, L0, {apipe::AP_LEVEL, l + 1}))) return rc;
        pf = c->prof_begin(IMT_PROF_APPLY_LEVEL, s);
        launch::apply_level(s, lists.count + l + 1, apply::bound((uint32_t)E, L0, l + 1), P.level(l + 1).nodeb,
                            t->nodes(l), t->h_len[l], c->d_zero + (size_t)l * 32, t->nodes(l + 1), t->h_len[l + 1],
                            c->coop_max_events);
        c->prof_end(pf, s);
        if ((rc = pipe_record(t, s, P, pipe, apipe::APPLY, L0, {apipe::AP_LEVEL, l + 1}))) return rc;
    }
    if ((rc = pipe_wait(t, s, pipe, apipe::APPLY, L0, {apipe::AP_CHAIN, 0}))) return rc;
    pf = c->prof_begin(IMT_PROF_APPLY_TOP, s);
    if (pipe.pipelined) launch::apply_chain(s, t->d_nodes, t->d_off, t->d_len, c->d_zero, P.d_chain, L0 - 1, t->depth);
    else launch::apply_top(s, t->d_nodes, t->d_off, t->d_len, c->d_zero, L0 - 1, t->depth);
    c->prof_end(pf, s);
    if (!pipe.pipelined) return IMT_OK;
    if ((rc = pipe_record(t, s, P, pipe, apipe::APPLY, L0, {apipe::AP_CHAIN, 0}))) return rc;
    if ((rc = pipe_wait(t, s, pipe, apipe::APPLY, L0, {apipe::AP_STORE, 0}))) return rc;
    launch::apply_chain_store(s, P.d_chain, t->d_nodes, t->d_off, L0, t->depth, P.d_root);
    return IMT_OK;
}

// The hash-free outputs of a batch to the caller, behind the hashing on stream s.  Prepared on the GPU they are in
// d.low_index .. d.new_leaf already (gpu_prepare); prepared on the host they are in the tree's work arrays and in hp.
static int deliver_hashfree_outputs(imt_itree* t, hipStream_t s, size_t n, const imt_insert_out* out, const imt_insert_out& d,
                                    const HostPlan& hp, unsigned flags, size_t& slot) {
    imt_ctx* c = t->ctx;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    if (!(flags & IMT_HOST_PREP)) {
        // written by k_events in canonical form; other formats are converted in place behind up_done
        if (fmt != IMT_FMT_CANONICAL) {
            if (d.low_leaf) launch::convert(s, (uint8_t*)d.low_leaf, (uint8_t*)d.low_leaf, n * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
            if (d.new_leaf) launch::convert(s, (uint8_t*)d.new_leaf, (uint8_t*)d.new_leaf, n * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
        }
        if (!dev) {
            if (d.low_index) IMT_HIP(c, hipMemcpyAsync(out->low_index, d.low_index, n * 8, hipMemcpyDeviceToHost, s));
            if (d.is_largest) IMT_HIP(c, hipMemcpyAsync(out->is_largest, d.is_largest, n, hipMemcpyDeviceToHost, s));
            if (d.low_leaf) IMT_HIP(c, hipMemcpyAsync(out->low_leaf, d.low_leaf, n * 96, hipMemcpyDeviceToHost, s));
            if (d.new_leaf) IMT_HIP(c, hipMemcpyAsync(out->new_leaf, d.new_leaf, n * 96, hipMemcpyDeviceToHost, s));
        }
        return IMT_OK;
    }
    int rc;
    auto host_out = [&](void* user, const void* src, size_t bytes) -> int {
        if (!user) return IMT_OK;
        if (dev) {   // side stream: does not wait for the sweep; src is host memory of this call
            IMT_HIP(c, hipMemcpyAsync(user, src, bytes, hipMemcpyHostToDevice, t->up_stream));
            IMT_HIP(c, hipStreamSynchronize(t->up_stream));
        } else {
            std::memcpy(user, src, bytes);
        }
        return IMT_OK;
    };
    if (t->index_base && out->low_index) {
        std::vector<uint64_t> glob(t->w_low);
        for (auto& x : glob) x += t->index_base;
        if ((rc = host_out(out->low_index, glob.data(), n * 8))) return rc;
    } else if ((rc = host_out(out->low_index, t->w_low.data(), n * 8))) return rc;
    if ((rc = host_out(out->is_largest, t->w_largest.data(), n))) return rc;
    if (fmt == IMT_FMT_CANONICAL) {
        if ((rc = host_out(out->low_leaf, hp.lowleaf.data(), n * 96))) return rc;
        return host_out(out->new_leaf, hp.newleaf.data(), n * 96);
    }
    for (int w = 0; w < 2; w++) {
        void* user = w ? out->new_leaf : out->low_leaf;
        if (!user) continue;
        const std::vector<uint8_t>& src = w ? hp.newleaf : hp.lowleaf;
        uint8_t* d_in = (uint8_t*)c->dev_scratch(slot++, n * 96);
        if (!d_in) return IMT_ERR_HIP;
        IMT_HIP(c, hipMemcpyAsync(d_in, src.data(), n * 96, hipMemcpyHostToDevice, s));
        uint8_t* d_o = dev ? (uint8_t*)user : (uint8_t*)c->dev_scratch(slot++, n * 96);
        if (!d_o) return IMT_ERR_HIP;
        launch::convert(s, d_in, d_o, n * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
        if (!dev) IMT_HIP(c, hipMemcpyAsync(user, d_o, n * 96, hipMemcpyDeviceToHost, s));
        IMT_HIP(c, hipStreamSynchronize(s));
    }
    return IMT_OK;
}

// The roots and sibling paths of a host-pointer call from their staging in `d` to the caller's arrays.
static int deliver_witness_outputs(imt_itree* t, hipStream_t s, size_t n, const imt_insert_out* out, const imt_insert_out& d,
                                   bool item_major, size_t sib_stride) {
    imt_ctx* c = t->ctx;
    if (out->old_root) IMT_HIP(c, hipMemcpyAsync(out->old_root, d.old_root, n * 32, hipMemcpyDeviceToHost, s));
    if (out->interim_root) IMT_HIP(c, hipMemcpyAsync(out->interim_root, d.interim_root, n * 32, hipMemcpyDeviceToHost, s));
    if (out->new_root) IMT_HIP(c, hipMemcpyAsync(out->new_root, d.new_root, n * 32, hipMemcpyDeviceToHost, s));
    // only rows [0, depth) were written: a placed tree's rows [depth, global_depth) stay the caller's until
    // imt_itree_lift_batch, so they are not copied over with the scratch behind them
    if (item_major ? t->global_depth == t->depth : sib_stride == n) {
        const size_t sib_copy = (size_t)t->depth * n * 32;
        if (out->low_sib) IMT_HIP(c, hipMemcpyAsync(out->low_sib, d.low_sib, sib_copy, hipMemcpyDeviceToHost, s));
        if (out->new_sib) IMT_HIP(c, hipMemcpyAsync(out->new_sib, d.new_sib, sib_copy, hipMemcpyDeviceToHost, s));
    } else if (item_major) {    // the first depth rows of every item's global_depth
        const size_t pitch = (size_t)t->global_depth * 32, width = (size_t)t->depth * 32;
        if (out->low_sib)
            IMT_HIP(c, hipMemcpy2DAsync(out->low_sib, pitch, d.low_sib, pitch, width, n, hipMemcpyDeviceToHost, s));
        if (out->new_sib)
            IMT_HIP(c, hipMemcpy2DAsync(out->new_sib, pitch, d.new_sib, pitch, width, n, hipMemcpyDeviceToHost, s));
    } else {    // rows [0, n) of every level, level stride sib_stride
        const size_t pitch = sib_stride * 32;
        if (out->low_sib)
            IMT_HIP(c, hipMemcpy2DAsync(out->low_sib, pitch, d.low_sib, pitch, n * 32, t->depth, hipMemcpyDeviceToHost, s));
        if (out->new_sib)
            IMT_HIP(c, hipMemcpy2DAsync(out->new_sib, pitch, d.new_sib, pitch, n * 32, t->depth, hipMemcpyDeviceToHost, s));
    }
    return IMT_OK;
}

// Nothing was inserted: a call that reports the root (root_out != NULL) reports the one the tree has
static int report_unchanged_root(imt_itree* t, void* root_out, unsigned flags) {
    return root_out ? imt_itree_root(t, root_out, flags & (IMT_FMT_MASK | IMT_DEVICE_PTRS)) : IMT_OK;
}

// The root a batch left (src, device format) to the caller on stream s, in the caller's format: straight into a device
// pointer, through the context's next scratch slot to a host pointer -- which holds it once the caller has waited for s.
static int deliver_root(imt_ctx* c, hipStream_t s, const uint8_t* src, void* root_out, unsigned flags, size_t& slot) {
    if (!root_out) return IMT_OK;
    const bool dev = flags & IMT_DEVICE_PTRS;
    uint8_t* r = dev ? (uint8_t*)root_out : (uint8_t*)c->dev_scratch(slot++, 32);
    if (!r) return IMT_ERR_HIP;
    launch::convert(s, src, r, 1, IMT_FMT_DEVICE, flags & IMT_FMT_MASK, c->d_err);
    if (!dev) IMT_HIP(c, hipMemcpyAsync(root_out, r, 32, hipMemcpyDeviceToHost, s));
    return IMT_OK;
}

// The two halves of a batch's commit.  Its plan set launched: the hashing is enqueued on s and P.d_root filled behind it,
// so the set holds a root, is in flight until `done`, and the next batch takes the next set.
static int plan_launched(imt_itree* t, PlanSet& P, hipStream_t s, unsigned L0, bool pipelined, bool applied) {
    P.has_root = true;
    P.reads_only = false;
    IMT_HIP(t->ctx, hipEventRecord(P.done, s));
    P.pipelined = pipelined;
    P.applied = applied;
    P.sliced = false;
    P.l0 = L0;
    P.in_flight = true;
    t->cur = (t->cur + 1) % imt_itree::NSETS;
    t->batch_no++;
    return IMT_OK;
}
// The stream a batch hashes on and its pipeline context: the context's stream behind every batch in flight, or -- a
// pipelined block -- the next of the NPIPE pipeline streams, behind what the caller has enqueued on the context's stream
// (the buffers were last used there) and with the block in front, if that is still on a pipeline stream, to take its waits
// from.  Called with t->cur the block's own plan set.
static int hashing_stream(imt_itree* t, bool pipelined, hipStream_t& s, PipeCtx& pipe) {
    imt_ctx* c = t->ctx;
    s = c->stream;
    pipe = PipeCtx{nullptr, pipelined};
    if (!pipelined) return join_top(t);
    s = t->pipe_stream[t->pipe_turn++ % imt_itree::NPIPE];
    IMT_HIP(c, hipEventRecord(t->user_mark, c->stream));
    IMT_HIP(c, hipStreamWaitEvent(s, t->user_mark, 0));
    const PlanSet& o = t->plan[(t->cur + imt_itree::NSETS - 1) % imt_itree::NSETS];
    if (o.in_flight && o.pipelined) pipe.prev = &o;
    t->pipe_pending = true;
    return IMT_OK;
}
// The device index committed: the merged index the preparation left in the other buffer becomes current together with
// the size; the host mirror is rebuilt from it when a host-side call needs it.
static void index_committed(imt_itree* t, uint64_t size) {
    t->sorted_cur ^= 1;
    t->size = size;
    t->mirror_valid = false;
    t->gen++;
}

// A batch behind its validation: n values (val_flags: where they are and in which format) into the tree, the outputs as
// `flags` say.  Level-major sibling arrays have level stride sib_stride (>= n).  The sequence: plan set, side stream
// behind the caller, hash-free part, compute stream, hashing, record, commit, outputs.
static int insert_core(imt_itree* t, const void* vals, unsigned val_flags, size_t n, const imt_insert_out* out, unsigned flags,
                       size_t sib_stride, const ApplyReq* apply) {
    imt_ctx* c = t->ctx;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const bool gpu_prep = (flags & IMT_HOST_PREP) == 0;
    const bool pipelined = dev && (flags & IMT_PIPELINE);
    const unsigned fmt = flags & IMT_FMT_MASK;
    const uint64_t M = t->size;
    const size_t E = 2 * n;
    const unsigned L0 = std::min(ceil_log2(M + n), t->depth);
    const HostTimer host;
    double host_wait_ms = 0;

    // ---- plan buffers ----
    PlanSet& P = t->plan[t->cur];
    int rc = acquire_plan(t, E, 0, host_wait_ms);
    if (rc) return rc;
    if (pipelined && (rc = reserve_all_plans(t, E))) return rc;

    // ---- hash-free part: low leaves, event preimages, event order (side stream) ----
    if ((rc = order_behind_caller(t, t->up_stream, flags))) return rc;
    size_t slot = 2;                 // context scratch slots, handed out in one order from here to the last output
    HostPlan hp;
    imt_insert_out d = {};           // where on the device each requested output is written
    if (gpu_prep)
        rc = gpu_prepare(t, P, vals, val_flags, n, out, dev, slot, d, host_wait_ms);
    else
        rc = host_prepare(t, P, vals, n, val_flags, out && out->low_leaf, out && out->new_leaf, hp);
    if (rc) return rc;
    IMT_HIP(c, hipEventRecord(t->up_done, t->up_stream));

    // ---- compute stream: the context's, or one of the NPIPE pipeline streams ----
    hipStream_t s;
    PipeCtx pipe;
    if ((rc = hashing_stream(t, pipelined, s, pipe))) return rc;
    IMT_HIP(c, hipStreamWaitEvent(s, t->up_done, 0));

    // ---- hashing: one hash per touched node straight into the stored tree (imt_apply.hpp), or the witness sweep ----
    const bool item_major = flags & IMT_SIB_ITEM_MAJOR;
    const size_t sib_bytes = (size_t)t->global_depth * (item_major ? n : sib_stride) * 32;
    if (out && (!stage_out(c, dev, slot, out->old_root, n * 32, d.old_root) ||
                !stage_out(c, dev, slot, out->interim_root, n * 32, d.interim_root) ||
                !stage_out(c, dev, slot, out->new_root, n * 32, d.new_root) ||
                !stage_out(c, dev, slot, out->low_sib, sib_bytes, d.low_sib) ||
                !stage_out(c, dev, slot, out->new_sib, sib_bytes, d.new_sib)))
        return IMT_ERR_HIP;
    // a placed tree writes rows [0, depth) of sibling arrays dimensioned for global_depth levels
    const launch::SibLayout lay = item_major ? launch::SibLayout{1, t->global_depth} : launch::SibLayout{sib_stride, 1};
    if (!apply) {
        WitnessSweep w;
        w.pipe = pipe;
        rc = witness_sweep(t, P, s, E, L0, d, lay, fmt, w);
    } else {    // a pipelined apply batch keeps its counts in its plan set, and its store of the chain fills P.d_root as well
        rc = apply_hashes(t, P, s, E, L0, pipelined ? P.d_count : t->d_apply_stats, pipe);
    }
    if (rc) return rc;
    if (apply) {
        t->apply_seen = true;
        t->apply_stats_set = pipelined ? &P : nullptr;
    }
    if (!(apply && pipelined)) IMT_HIP(c, hipMemcpyAsync(P.d_root, t->nodes(t->depth), 32, hipMemcpyDeviceToDevice, s));
    if ((rc = plan_launched(t, P, s, L0, pipelined, apply && pipelined))) return rc;

    // ---- commit the hash-free state ----
    if (gpu_prep) {
        index_committed(t, M + n);
    } else {
        host_commit(t, hp, n);
        t->gen++;
    }

    // ---- outputs ----
    if (out && (rc = deliver_hashfree_outputs(t, s, n, out, d, hp, flags, slot))) return rc;
    if (apply && (rc = deliver_root(c, s, P.d_root, apply->root_out, flags, slot))) return rc;
    if (out && !dev && (rc = deliver_witness_outputs(t, s, n, out, d, item_major, sib_stride))) return rc;
    if (c->profiling) {
        c->prof_ms[IMT_PROF_HOST] += host.ms() - host_wait_ms;
        c->prof_n[IMT_PROF_HOST] += 1;
    }
    if (!dev) IMT_HIP(c, hipStreamSynchronize(s));
    return IMT_OK;
}

// imt_itree_insert_batch and imt_itree_apply_batch: the refusals, then the batch
static int insert_call(imt_itree* t, const void* vals, size_t n, const imt_insert_out* out, unsigned flags,
                       const ApplyReq* apply) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (n == 0) return IMT_OK;
    if (!vals) return c->fail(IMT_ERR_ARG, "null vals");
    int rc = check_batch_call(t, n, flags);
    if (rc) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((rc = check_fe_ptrs(c, dev, {vals})) || (rc = check_out_ptrs(c, dev, out))) return rc;
    if (apply && (rc = check_fe_ptrs(c, dev, {apply->root_out}))) return rc;
    if ((rc = check_room(t, n))) return rc;
    return insert_core(t, vals, flags, n, out, flags, n, apply);
}

extern "C" int imt_itree_insert_batch(imt_itree* t, const void* vals, size_t n, const imt_insert_out* out,
                                      unsigned flags) {
    return insert_call(t, vals, n, out, flags, nullptr);
}

extern "C" int imt_itree_apply_batch(imt_itree* t, const void* vals, size_t n, void* root_out, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    if (flags & IMT_PIPELINE) return t->ctx->fail(IMT_ERR_ARG, "apply batches are not pipelined (IMT_PIPELINE)");
    if (n == 0) {
        IMT_NOT_SLICED(t);
        return report_unchanged_root(t, root_out, flags);
    }
    const ApplyReq req{root_out};
    return insert_call(t, vals, n, nullptr, flags, &req);
}

// Witness-free batches that overlap (imt.h): imt_itree_apply_batch's checks, preparation and commit, the hashing on one
// of the tree's pipeline streams behind the batches in front (apply_hashes with a pipeline context).
extern "C" int imt_itree_apply_pipelined(imt_itree* t, const void* vals, size_t n, void* root_out, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    if (!(flags & IMT_DEVICE_PTRS)) return t->ctx->fail(IMT_ERR_ARG, "imt_itree_apply_pipelined needs device pointers (IMT_DEVICE_PTRS)");
    if (n == 0) {
        IMT_NOT_SLICED(t);
        return report_unchanged_root(t, root_out, flags);
    }
    const ApplyReq req{root_out};
    return insert_call(t, vals, n, nullptr, flags | IMT_PIPELINE, &req);
}

extern "C" int imt_itree_apply_stats(imt_itree* t, uint64_t* hashes) {
    if (!t || !hashes) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (!t->apply_seen) return c->fail(IMT_ERR_ARG, "no apply call has inserted anything into this tree");
    int rc = c->set_device();
    if (rc) return rc;
    // the apply call ran on the context's stream, which is therefore behind its last kernel -- or on a pipeline stream
    // with its counts in its plan set, and then this waits for that batch and for none of those behind it
    const uint64_t* src = t->d_apply_stats;
    if (t->apply_stats_set) {
        src = t->apply_stats_set->d_count;
        IMT_HIP(c, hipStreamWaitEvent(c->stream, t->apply_stats_set->done, 0));
    }
    IMT_HIP(c, hipMemcpyAsync(hashes, src, (t->depth + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    IMT_HIP(c, hipStreamSynchronize(c->stream));
    return IMT_OK;
}

// ------------------------------------------------------------------------------------
// mixed batches: non-inclusion READs between the INSERTs of one call and, under IMT_MEMBER_OPS, presence
// reads (IMT_OP_MEMBER) -- to everything below the checks a MEMBER is a READ: one event, one row of `rd`
// ------------------------------------------------------------------------------------
// rows [0, rows) of a staged sibling array to the caller's: item-major they are one block, level-major they are the
// first `rows` of every level's n
static int copy_sib_rows(imt_itree* t, hipStream_t s, void* user, const void* dev_buf, size_t rows, size_t n, bool item_major) {
    imt_ctx* c = t->ctx;
    if (!user || !rows) return IMT_OK;
    if (item_major || rows == n)
        IMT_HIP(c, hipMemcpyAsync(user, dev_buf, (size_t)t->depth * rows * 32, hipMemcpyDeviceToHost, s));
    else
        IMT_HIP(c, hipMemcpy2DAsync(user, n * 32, dev_buf, n * 32, rows * 32, t->depth, hipMemcpyDeviceToHost, s));
    return IMT_OK;
}

// Where the kernels write the nine outputs of n insertions the caller asked for (stage_out; sib_bytes: a sibling array of
// the caller's dimensions), in the one order the scratch slots are handed out in.  False: scratch could not be had.
static bool stage_insert_outputs(imt_ctx* c, bool dev, size_t& slot, const imt_insert_out* ins, size_t n, size_t sib_bytes,
                                 imt_insert_out& d) {
    return stage_out(c, dev, slot, ins->low_index, n * 8, d.low_index) && stage_out(c, dev, slot, ins->is_largest, n, d.is_largest) &&
           stage_out(c, dev, slot, ins->low_leaf, n * 96, d.low_leaf) && stage_out(c, dev, slot, ins->new_leaf, n * 96, d.new_leaf) &&
           stage_out(c, dev, slot, ins->old_root, n * 32, d.old_root) &&
           stage_out(c, dev, slot, ins->interim_root, n * 32, d.interim_root) &&
           stage_out(c, dev, slot, ins->new_root, n * 32, d.new_root) && stage_out(c, dev, slot, ins->low_sib, sib_bytes, d.low_sib) &&
           stage_out(c, dev, slot, ins->new_sib, sib_bytes, d.new_sib);
}
// The same for a mixed batch: row r of `ins` the r-th INSERT, row q of `rd` the q-th READ.
static bool mixed_stage_outputs(imt_ctx* c, bool dev, size_t& slot, const imt_insert_out* ins, const imt_read_out* rd, size_t n_ins,
                                size_t n_rd, size_t sib_bytes, imt_insert_out& d, imt_read_out& r) {
    if (ins && n_ins && !stage_insert_outputs(c, dev, slot, ins, n_ins, sib_bytes, d)) return false;
    if (rd && n_rd &&
        (!stage_out(c, dev, slot, rd->low_index, n_rd * 8, r.low_index) ||
         !stage_out(c, dev, slot, rd->is_largest, n_rd, r.is_largest) ||
         !stage_out(c, dev, slot, rd->low_leaf, n_rd * 96, r.low_leaf) || !stage_out(c, dev, slot, rd->root, n_rd * 32, r.root) ||
         !stage_out(c, dev, slot, rd->low_sib, sib_bytes, r.low_sib)))
        return false;
    return true;
}

// The end of a mixed call on stream s, behind its hashing: the preimages into the caller's format, and for a host-pointer
// caller every staged array copied to the caller's and the stream waited for.  stride: the level stride of the sibling
// arrays.
static int mixed_deliver_outputs(imt_itree* t, hipStream_t s, const imt_insert_out* ins, const imt_read_out* rd,
                                 const imt_insert_out& d, const imt_read_out& r, size_t n_ins, size_t n_rd, size_t stride,
                                 unsigned flags) {
    imt_ctx* c = t->ctx;
    int rc;
    const bool dev = flags & IMT_DEVICE_PTRS, item_major = flags & IMT_SIB_ITEM_MAJOR;
    const unsigned fmt = flags & IMT_FMT_MASK;
    if (fmt != IMT_FMT_CANONICAL) {
        if (d.low_leaf) launch::convert(s, (uint8_t*)d.low_leaf, (uint8_t*)d.low_leaf, n_ins * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
        if (d.new_leaf) launch::convert(s, (uint8_t*)d.new_leaf, (uint8_t*)d.new_leaf, n_ins * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
        if (r.low_leaf) launch::convert(s, (uint8_t*)r.low_leaf, (uint8_t*)r.low_leaf, n_rd * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
    }
    if (dev) return IMT_OK;
    auto back = [&](void* user, const void* from, size_t bytes) -> int {
        if (user && from) IMT_HIP(c, hipMemcpyAsync(user, from, bytes, hipMemcpyDeviceToHost, s));
        return IMT_OK;
    };
    if (ins && n_ins &&
        ((rc = back(ins->low_index, d.low_index, n_ins * 8)) || (rc = back(ins->is_largest, d.is_largest, n_ins)) ||
         (rc = back(ins->low_leaf, d.low_leaf, n_ins * 96)) || (rc = back(ins->new_leaf, d.new_leaf, n_ins * 96)) ||
         (rc = back(ins->old_root, d.old_root, n_ins * 32)) || (rc = back(ins->interim_root, d.interim_root, n_ins * 32)) ||
         (rc = back(ins->new_root, d.new_root, n_ins * 32)) ||
         (rc = copy_sib_rows(t, s, ins->low_sib, d.low_sib, n_ins, stride, item_major)) ||
         (rc = copy_sib_rows(t, s, ins->new_sib, d.new_sib, n_ins, stride, item_major))))
        return rc;
    if (rd && n_rd &&
        ((rc = back(rd->low_index, r.low_index, n_rd * 8)) || (rc = back(rd->is_largest, r.is_largest, n_rd)) ||
         (rc = back(rd->low_leaf, r.low_leaf, n_rd * 96)) || (rc = back(rd->root, r.root, n_rd * 32)) ||
         (rc = copy_sib_rows(t, s, rd->low_sib, r.low_sib, n_rd, stride, item_major))))
        return rc;
    IMT_HIP(c, hipStreamSynchronize(s));
    return IMT_OK;
}

// What imt_itree_mixed_filtered asks of the body below on top of a mixed batch: the low leaves of the accepted READs
// into its leaf_index once mixed_check has found them, and a refusal of what the filter accepted reported as a bug.
struct MixedFiltered {
    uint64_t* d_leaf;       // leaf_index on the device (the caller's array or its staging), NULL: not asked for
    uint64_t* h_leaf;       // a host-pointer caller's array, d_leaf is copied to; NULL otherwise
    size_t n_all;           // its length: the operations passed in
};

// The per-operation scratch of a mixed batch on plan set P: the filter's and the slot table's, idle by then.
static prep::MixedWs mixed_scratch(const PlanSet& P) { return prep::MixedWs{P.fw.flag, P.fw.rank, P.fw.idx, P.fw.aux, P.d_slot}; }

// ---- the front the mixed entry points share (batch, filtered, replay): each makes these refusals at its own point of
// its own order, in its own words where the words differ ----
struct MixedNoun {
    const char *takes, *plural;
};
static const MixedNoun MIXED_BATCH{"mixed batches take", "mixed batches"}, MIXED_REPLAY{"a mixed replay takes", "mixed replays"};
static int check_mixed_mode(imt_itree* t, unsigned flags, const MixedNoun& noun) {
    imt_ctx* c = t->ctx;
    if (flags & (IMT_PIPELINE | IMT_HOST_PREP | IMT_INPUTS_READY))
        return c->fail(IMT_ERR_ARG, "%s neither IMT_PIPELINE, IMT_HOST_PREP nor IMT_INPUTS_READY", noun.takes);
    if (t->index_base || t->global_depth != t->depth || t->part_mod > 1)
        return c->fail(IMT_ERR_ARG, "%s are not available on a placed or partitioned tree", noun.plural);
    return IMT_OK;
}
static int check_mixed_ptrs(imt_ctx* c, bool dev, const void* vals, const imt_insert_out* ins, const imt_read_out* rd) {
    int rc;
    if ((rc = check_fe_ptrs(c, dev, {vals})) || (rc = check_out_ptrs(c, dev, ins))) return rc;
    if (rd && (rc = check_fe_ptrs(c, dev, {rd->low_leaf, rd->root, rd->low_sib}))) return rc;
    if (dev && ((ins && ((uintptr_t)ins->low_index & 7u)) || (rd && ((uintptr_t)rd->low_index & 7u))))
        return c->fail(IMT_ERR_ARG, "device low_index array is not 8-byte aligned");
    return IMT_OK;
}
// The op bytes a call takes: IMT_OP_MEMBER only under IMT_MEMBER_OPS, so that a caller who never asked for presence reads
// has byte 2 refused as it always was, in the words it always was.
static uint8_t mixed_max_op(unsigned flags) { return (flags & IMT_MEMBER_OPS) ? IMT_OP_MEMBER : IMT_OP_READ; }
static const char* mixed_op_kinds(unsigned flags) {
    return (flags & IMT_MEMBER_OPS) ? "neither IMT_OP_INSERT, IMT_OP_READ nor IMT_OP_MEMBER"
                                    : "neither IMT_OP_INSERT nor IMT_OP_READ";
}
// a host-pointer caller's op bytes, before anything is enqueued; a device-pointer caller's are checked by the rank kernel
static int check_host_ops(imt_ctx* c, bool dev, const uint8_t* op, size_t n, unsigned flags) {
    if (!dev)
        for (size_t p = 0; p < n; p++)
            if (op[p] > mixed_max_op(flags)) return c->fail(IMT_ERR_ARG, "op[%zu] = %u is %s", p, op[p], mixed_op_kinds(flags));
    return IMT_OK;
}
// the op bytes where stream s may read them: a host-pointer caller's through the context's next scratch slot
static int stage_ops(imt_ctx* c, hipStream_t s, bool dev, const uint8_t* op, size_t n, size_t& slot, const uint8_t** d_op) {
    *d_op = op;
    if (dev) return IMT_OK;
    uint8_t* o = (uint8_t*)c->dev_scratch(slot++, n);
    if (!o) return IMT_ERR_HIP;
    IMT_HIP(c, hipMemcpyAsync(o, op, n, hipMemcpyHostToDevice, s));
    *d_op = o;
    return IMT_OK;
}
// The rank stage on stream s, the error word clear: every operation's rank among its kind, and -- one host wait -- a bad
// op byte refused and the number of INSERTs.
static int mixed_rank_stage(imt_itree* t, PlanSet& P, const prep::MixedWs& mx, hipStream_t s, const uint8_t* d_op, size_t n,
                            unsigned flags, size_t& n_ins) {
    imt_ctx* c = t->ctx;
    IMT_HIP(c, prep::mixed_ranks(s, P.ws, mx, d_op, (uint32_t)n, mixed_max_op(flags)));
    IMT_HIP(c, hipMemcpyAsync(t->h_cnt_pin, mx.word, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipMemcpyAsync(t->h_err_pin, P.ws.err, sizeof(int), hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipStreamSynchronize(s));
    if (*t->h_err_pin & prep::ERR_OP) return c->fail(IMT_ERR_ARG, "an op byte is %s", mixed_op_kinds(flags));
    n_ins = *t->h_cnt_pin;
    return IMT_OK;
}
// The end of the check stage on stream s -- the second host wait: the checks' error bits in *t->h_err_pin, the first
// position they refuse in *t->h_cnt_pin.
static int mixed_check_verdict(imt_itree* t, PlanSet& P, const prep::MixedWs& mx, hipStream_t s) {
    imt_ctx* c = t->ctx;
    IMT_HIP(c, hipMemcpyAsync(t->h_cnt_pin, mx.word + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipMemcpyAsync(t->h_err_pin, P.ws.err, sizeof(int), hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipStreamSynchronize(s));
    return IMT_OK;
}

// The front of every mixed batch behind the staging of its inputs: n operations (d_vals canonical, d_op, both device
// memory that stream t->up_stream may read), on plan set P, acquired for >= 2n events, with the error word clear.  Ranks,
// room for the n_ins INSERTs, their values into rows [M, M + n_ins) of the value array, every check and the neighbours of
// every operation (P.ws.low / succ) -- two host waits, after which either the batch is refused with nothing of the tree
// or the caller's changed, or it is accepted and the side stream is idle.
static int mixed_checks(imt_itree* t, PlanSet& P, const prep::MixedWs& mx, const uint8_t* d_vals, const uint8_t* d_op, size_t n,
                        unsigned flags, uint64_t* bad_op, const MixedFiltered* filtered, size_t& n_ins) {
    imt_ctx* c = t->ctx;
    int rc;
    const uint64_t M = t->size;
    hipStream_t ps = t->up_stream;
    if ((rc = mixed_rank_stage(t, P, mx, ps, d_op, n, flags, n_ins))) return rc;
    if ((rc = check_room(t, n_ins))) return rc;
    P.ws.part_mod = t->part_mod;
    P.ws.part_res = t->part_res;
    IMT_HIP(c, prep::mixed_check(ps, P.ws, mx, d_vals, d_op, t->d_val, t->d_sorted[t->sorted_cur], (uint32_t)M, (uint32_t)n,
                                 (uint32_t)n_ins));
    if (filtered && filtered->d_leaf && n_ins < n) {
        IMT_HIP(c, prep::mixed_filter_reads(ps, P.fw, P.ws, mx, (uint32_t)n, (uint32_t)n_ins, t->index_base, filtered->d_leaf));
    }
    if (filtered && filtered->h_leaf)
        IMT_HIP(c, hipMemcpyAsync(filtered->h_leaf, filtered->d_leaf, filtered->n_all * 8, hipMemcpyDeviceToHost, ps));
    if ((rc = mixed_check_verdict(t, P, mx, ps))) return rc;
    rc = insertion_verdict(t, *t->h_err_pin, "batch");
    // a MEMBER of a value that is not there; among several refusals of one block the others keep their words
    if (!rc && (*t->h_err_pin & prep::ERR_ABSENT)) rc = c->fail(IMT_ERR_VALUE, "the value of a MEMBER is not in the tree");
    if (rc) {
        if (filtered) {
            std::string why = c->last_error;
            return c->fail(IMT_ERR_INTERNAL, "the mixed checks refuse operation %u of those the filter accepted: %s", *t->h_cnt_pin,
                           why.c_str());
        }
        if (rc == IMT_ERR_VALUE) {
            if (bad_op) *bad_op = *t->h_cnt_pin;
            std::string why = c->last_error;
            if (flags & IMT_MEMBER_OPS)
                return c->fail(rc, "operation %u: %s (a READ: 0, stored, or inserted earlier in the batch; a MEMBER: 0, or neither "
                               "stored nor inserted earlier in the batch)", *t->h_cnt_pin, why.c_str());
            return c->fail(rc, "operation %u: %s (a READ: 0, stored, or inserted earlier in the batch)", *t->h_cnt_pin, why.c_str());
        }
        return rc;
    }
    return IMT_OK;
}

// The end of every mixed batch, its hashing enqueued on stream s.  Only READs: the plan set is in flight and that is all
// -- the rotation, the batch count, the size and the generation stay.  Otherwise the commit of a batch like any other.
// On a pipeline stream (pipe.pipelined; `applied`: as an apply batch, whose store of the chain has filled P.d_root) a block
// of READs only takes its turn in the rotation all the same: the block behind it takes its waits from this set's events,
// and this set stays the block's own until its `done`.  It is still no batch -- the batch count, the size and the
// generation stay -- so it carries the roots imt_itree_root_lagged would have found without it (PlanSet::reads_only).
static int mixed_commit(imt_itree* t, PlanSet& P, hipStream_t s, size_t n_ins, unsigned L0, const PipeCtx& pipe = {},
                        bool applied = false) {
    imt_ctx* c = t->ctx;
    if (!n_ins && !pipe.pipelined) {
        P.pipelined = false;
        IMT_HIP(c, hipEventRecord(P.done, s));
        P.in_flight = true;
        return IMT_OK;
    }
    if (!n_ins) {
        // the turn before this one, and the one before that: both behind `s` already -- a pipelined one through the waits
        // of the sweep (WI_OLD_ROOT waits for DONE, as every pipelined kind does before it ends), any other through the
        // context's stream -- the explicit wait says so where the copy is
        const PlanSet& o1 = t->plan[(t->cur + imt_itree::NSETS - 1) % imt_itree::NSETS];
        const PlanSet& o2 = t->plan[(t->cur + imt_itree::NSETS - 2) % imt_itree::NSETS];
        const bool chained = o1.reads_only;
        const PlanSet& from = chained ? o1 : o2;
        const bool have2 = chained ? o1.has_root2 : o2.has_root;
        if (have2) {
            IMT_HIP(c, hipStreamWaitEvent(s, from.done, 0));
            IMT_HIP(c, hipMemcpyAsync(P.d_root + 32, from.d_root + (chained ? 32 : 0), 32, hipMemcpyDeviceToDevice, s));
        }
        IMT_HIP(c, hipMemcpyAsync(P.d_root, t->nodes(t->depth), 32, hipMemcpyDeviceToDevice, s));
        P.has_root = o1.has_root;        // a turn without a root in front (a slice's, or none since a rewind) stays one
        P.reads_only = true;
        P.has_root2 = have2;
        P.sliced1 = chained ? o1.sliced1 : o1.sliced;
        P.sliced2 = chained ? o1.sliced2 : o2.sliced;
        IMT_HIP(c, hipEventRecord(P.done, s));
        P.pipelined = true;
        P.applied = false;
        P.sliced = false;
        P.l0 = L0;
        P.in_flight = true;
        t->cur = (t->cur + 1) % imt_itree::NSETS;
        return IMT_OK;
    }
    if (!applied) IMT_HIP(c, hipMemcpyAsync(P.d_root, t->nodes(t->depth), 32, hipMemcpyDeviceToDevice, s));
    int rc = plan_launched(t, P, s, L0, pipe.pipelined, applied);
    if (rc) return rc;
    index_committed(t, t->size + n_ins);
    return IMT_OK;
}

// The body of imt_itree_mixed_batch behind the staging of its inputs (mixed_checks says how they are passed).
// stride >= n is the level stride of level-major sibling arrays -- the caller's dimensions, imt_itree_insert_filtered's
// convention; slot: the first context scratch slot the staged outputs may take.
static int mixed_core(imt_itree* t, PlanSet& P, const uint8_t* d_vals, const uint8_t* d_op, size_t n, size_t stride, size_t slot,
                      const imt_insert_out* ins, const imt_read_out* rd, uint64_t* n_inserted, uint64_t* bad_op, unsigned flags,
                      const MixedFiltered* filtered, bool pipelined = false) {
    imt_ctx* c = t->ctx;
    int rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    const uint64_t M = t->size;
    hipStream_t ps = t->up_stream;
    const prep::MixedWs mx = mixed_scratch(P);
    size_t n_ins = 0;
    if ((rc = mixed_checks(t, P, mx, d_vals, d_op, n, flags, bad_op, filtered, n_ins))) return rc;
    const size_t n_rd = n - n_ins;

    // ---- accepted: events, tables, merged index, hash-free outputs (side stream) ----
    const size_t E = n + n_ins;
    const unsigned L0 = std::min(ceil_log2(M + n_ins), t->depth);
    const bool item_major = flags & IMT_SIB_ITEM_MAJOR;
    const size_t sib_bytes = (size_t)t->depth * stride * 32;      // the caller's dimensions, whichever kind the rows are
    imt_insert_out d = {};
    imt_read_out r = {};
    if (!mixed_stage_outputs(c, dev, slot, ins, rd, n_ins, n_rd, sib_bytes, d, r)) return IMT_ERR_HIP;
    IMT_HIP(c, prep::mixed_events(ps, P.ws, mx, t->d_val, t->d_sorted[t->sorted_cur], t->d_sorted[t->sorted_cur ^ 1], (uint32_t)M,
                                  (uint32_t)n, (uint32_t)n_ins, t->index_base, P.d_pre, P.d_tab[0][0], P.d_tab[0][1],
                                  P.d_tab[0][2], P.d_tab[0][3], d.low_index, d.is_largest, (uint8_t*)d.low_leaf,
                                  (uint8_t*)d.new_leaf, prep::ReadOut{r.low_index, r.is_largest, (uint8_t*)r.low_leaf}));
    IMT_HIP(c, hipEventRecord(t->up_done, ps));

    // ---- hashing on the context's stream, behind every batch in flight -- or on a pipeline stream, one level behind the
    // block in front: by its footprint on the stored levels a mixed block is a witness batch of its E events, a READ's
    // write-back putting back the bytes it read (imt_apply_pipe.hpp) ----
    hipStream_t s;
    WitnessSweep w;
    if ((rc = hashing_stream(t, pipelined, s, w.pipe))) return rc;
    if (w.pipe.prev && L0 == 0) {    // READs of a tree that holds the sentinel alone: below the heights the rule is checked for,
        IMT_HIP(c, hipStreamWaitEvent(s, w.pipe.prev->done, 0));      // and nothing to overlap -- behind all of the block in front
        w.pipe.prev = nullptr;
    }
    IMT_HIP(c, hipStreamWaitEvent(s, t->up_done, 0));
    const launch::SibLayout lay = item_major ? launch::SibLayout{1, t->depth} : launch::SibLayout{stride, 1};
    const launch::MixedRoute route{mx.erow, (uint8_t*)r.low_sib};
    w.route = &route;
    w.n_ins = n_ins;
    w.read_root = (uint8_t*)r.root;
    if ((rc = witness_sweep(t, P, s, E, L0, d, lay, fmt, w))) return rc;
    if ((rc = mixed_commit(t, P, s, n_ins, L0, w.pipe))) return rc;

    // ---- outputs ----
    if (n_inserted) *n_inserted = n_ins;
    return mixed_deliver_outputs(t, s, ins, rd, d, r, n_ins, n_rd, stride, flags);
}

// The body of imt_itree_apply_mixed behind the same staging: the same checks, then the events of the
// INSERTs alone and imt_itree_apply_batch's hashing and commit.  A READ is judged by the checks and is heard of no more;
// a batch without an INSERT ends behind them -- nothing was enqueued outside the side stream, which has been waited for,
// so the plan set stays idle, nothing is hashed and the only thing read of the tree is its root.
static int apply_mixed_core(imt_itree* t, PlanSet& P, const uint8_t* d_vals, const uint8_t* d_op, size_t n, size_t slot,
                            uint64_t* n_inserted, uint64_t* bad_op, unsigned flags, const MixedFiltered* filtered,
                            const ApplyReq& apply, bool pipelined = false) {
    imt_ctx* c = t->ctx;
    int rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const uint64_t M = t->size;
    hipStream_t ps = t->up_stream;
    size_t n_ins = 0;
    if ((rc = mixed_checks(t, P, mixed_scratch(P), d_vals, d_op, n, flags, bad_op, filtered, n_ins))) return rc;
    if (!n_ins) {
        if ((rc = report_unchanged_root(t, apply.root_out, flags))) return rc;
        if (n_inserted) *n_inserted = 0;
        return IMT_OK;
    }

    // ---- accepted: the 2 n_ins events an insertion-only batch of the INSERT values has, tables, merged index ----
    const size_t E = 2 * n_ins;
    const unsigned L0 = std::min(ceil_log2(M + n_ins), t->depth);
    IMT_HIP(c, prep::mixed_insert_events(ps, P.ws, t->d_val, t->d_sorted[t->sorted_cur], t->d_sorted[t->sorted_cur ^ 1], (uint32_t)M,
                                         (uint32_t)n_ins, t->index_base, P.d_pre, P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][2],
                                         P.d_tab[0][3]));
    IMT_HIP(c, hipEventRecord(t->up_done, ps));

    // ---- hashing on the context's stream, behind every batch in flight: every touched node once -- or on a pipeline
    // stream two launches behind the block in front, as the apply batch of its INSERTs that it is, with its counts in its
    // plan set and its store of the chain filling P.d_root ----
    hipStream_t s;
    PipeCtx pipe;
    if ((rc = hashing_stream(t, pipelined, s, pipe))) return rc;
    IMT_HIP(c, hipStreamWaitEvent(s, t->up_done, 0));
    if ((rc = apply_hashes(t, P, s, E, L0, pipelined ? P.d_count : t->d_apply_stats, pipe))) return rc;
    t->apply_seen = true;
    t->apply_stats_set = pipelined ? &P : nullptr;
    if ((rc = mixed_commit(t, P, s, n_ins, L0, pipe, pipelined))) return rc;

    // ---- outputs ----
    if (n_inserted) *n_inserted = n_ins;
    if ((rc = deliver_root(c, s, P.d_root, apply.root_out, flags, slot))) return rc;
    if (!dev) IMT_HIP(c, hipStreamSynchronize(s));
    return IMT_OK;
}

// imt_itree_mixed_batch and (apply != NULL) imt_itree_apply_mixed: the refusals, the staging of the inputs, then the body
// pipelined: imt_itree_mixed_pipelined / imt_itree_apply_mixed_pipelined -- the same call with its hashing on a pipeline
// stream; device pointers only, IMT_PIPELINE allowed and without a meaning of its own.
static int mixed_call(imt_itree* t, const void* vals, const uint8_t* op, size_t n, const imt_insert_out* ins,
                      const imt_read_out* rd, uint64_t* n_inserted, uint64_t* bad_op, unsigned flags, const ApplyReq* apply,
                      bool pipelined = false) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    int rc;
    if (pipelined) {
        if (!(flags & IMT_DEVICE_PTRS)) return c->fail(IMT_ERR_ARG, "pipelined mixed blocks need device pointers (IMT_DEVICE_PTRS)");
        flags &= ~(unsigned)IMT_PIPELINE;
    }
    if (n == 0) {
        if (apply && (rc = report_unchanged_root(t, apply->root_out, flags))) return rc;
        if (n_inserted) *n_inserted = 0;
        return IMT_OK;
    }
    if (!vals || !op) return c->fail(IMT_ERR_ARG, "null vals / op");
    if ((rc = check_mixed_mode(t, flags, MIXED_BATCH)) || (rc = check_batch_call(t, n, flags))) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((rc = check_mixed_ptrs(c, dev, vals, ins, rd))) return rc;
    if (apply && (rc = check_fe_ptrs(c, dev, {apply->root_out}))) return rc;
    if ((rc = check_host_ops(c, dev, op, n, flags))) return rc;
    if ((rc = ensure_device_index(t))) return rc;
    double waited_ms = 0;

    // ---- plan buffers: 2n events hold any mix ----
    PlanSet& P = t->plan[t->cur];
    if ((rc = acquire_plan(t, 2 * n, 0, waited_ms))) return rc;
    if (pipelined && (rc = reserve_all_plans(t, 2 * n))) return rc;

    // ---- ranks, then the checks: nothing of the caller's is written before the batch is accepted ----
    hipStream_t ps = t->up_stream;
    if ((rc = order_behind_caller(t, ps, flags))) return rc;
    size_t slot = 2;
    const uint8_t* d_vals = nullptr;
    uint8_t* up = dev ? nullptr : (uint8_t*)c->dev_scratch(slot++, n * 32);
    if ((rc = stage_canonical(c, ps, vals, n, flags, up, P.d_canon, P.ws.err, &d_vals))) return rc;
    const uint8_t* d_op = nullptr;
    if ((rc = stage_ops(c, ps, dev, op, n, slot, &d_op))) return rc;
    if (apply) return apply_mixed_core(t, P, d_vals, d_op, n, slot, n_inserted, bad_op, flags, nullptr, *apply, pipelined);
    return mixed_core(t, P, d_vals, d_op, n, n, slot, ins, rd, n_inserted, bad_op, flags, nullptr, pipelined);
}

extern "C" int imt_itree_mixed_batch(imt_itree* t, const void* vals, const uint8_t* op, size_t n, const imt_insert_out* ins,
                                     const imt_read_out* rd, uint64_t* n_inserted, uint64_t* bad_op, unsigned flags) {
    return mixed_call(t, vals, op, n, ins, rd, n_inserted, bad_op, flags, nullptr);
}

extern "C" int imt_itree_apply_mixed(imt_itree* t, const void* vals, const uint8_t* op, size_t n, void* root_out,
                                     uint64_t* n_inserted, uint64_t* bad_op, unsigned flags) {
    const ApplyReq req{root_out};
    return mixed_call(t, vals, op, n, nullptr, nullptr, n_inserted, bad_op, flags, &req);
}

// Mixed blocks that overlap (imt.h): the calls above with their hashing on the tree's pipeline streams.
extern "C" int imt_itree_mixed_pipelined(imt_itree* t, const void* vals, const uint8_t* op, size_t n, const imt_insert_out* ins,
                                         const imt_read_out* rd, uint64_t* n_inserted, uint64_t* bad_op, unsigned flags) {
    return mixed_call(t, vals, op, n, ins, rd, n_inserted, bad_op, flags, nullptr, true);
}

extern "C" int imt_itree_apply_mixed_pipelined(imt_itree* t, const void* vals, const uint8_t* op, size_t n, void* root_out,
                                               uint64_t* n_inserted, uint64_t* bad_op, unsigned flags) {
    const ApplyReq req{root_out};
    return mixed_call(t, vals, op, n, nullptr, nullptr, n_inserted, bad_op, flags, &req, true);
}

// ------------------------------------------------------------------------------------
// bulk insertion: the batch in descending value order -- one rewrite of a stored low leaf per value, swept
// with witnesses as a mixed batch of ROW_LOW events -- then the frontier of the first free slot and all new leaves at once
// through the witness-free schedule.  The entry is the stages above plus the three below.
// ------------------------------------------------------------------------------------
static const MixedNoun BULK_BATCH{"bulk batches take", "bulk batches"};
// The device pointers of a bulk call's outputs (the caller's, or staging for a host-pointer caller)
struct BulkDev {
    prep::BulkOut hashfree = {};
    imt_insert_out sweep = {};       // low_sib; old_root = root_before, interim_root = root_after
    uint8_t *append_sib = nullptr, *root = nullptr;
};
static bool bulk_stage_outputs(imt_ctx* c, bool dev, size_t& slot, const imt_bulk_out* o, size_t n, unsigned depth, BulkDev& d) {
    uint8_t *low_leaf = nullptr, *new_leaf = nullptr;
    const bool ok = stage_out(c, dev, slot, o->order, n * 8, d.hashfree.order) &&
                    stage_out(c, dev, slot, o->low_index, n * 8, d.hashfree.low_index) &&
                    stage_out(c, dev, slot, o->is_largest, n, d.hashfree.is_largest) &&
                    stage_out(c, dev, slot, (uint8_t*)o->low_leaf, n * 96, low_leaf) &&
                    stage_out(c, dev, slot, (uint8_t*)o->new_leaf, n * 96, new_leaf) &&
                    stage_out(c, dev, slot, o->root_before, n * 32, d.sweep.old_root) &&
                    stage_out(c, dev, slot, o->root_after, n * 32, d.sweep.interim_root) &&
                    stage_out(c, dev, slot, o->low_sib, (size_t)depth * n * 32, d.sweep.low_sib) &&
                    stage_out(c, dev, slot, (uint8_t*)o->append_sib, (size_t)depth * 32, d.append_sib) &&
                    stage_out(c, dev, slot, (uint8_t*)o->root, 32, d.root);
    d.hashfree.low_leaf = low_leaf;
    d.hashfree.new_leaf = new_leaf;
    return ok;
}
// The check stage on the side stream, the error word clear and the values staged: the values into rows [M, M + n) of the
// value array, the batch sorted, its gaps and every check -- one host wait, after which the batch is refused with nothing
// of the tree or the caller's changed, or accepted.
static int bulk_checks(imt_itree* t, PlanSet& P, const uint8_t* d_vals, size_t n, double& wait_ms) {
    imt_ctx* c = t->ctx;
    hipStream_t ps = t->up_stream;
    P.ws.part_mod = t->part_mod;
    P.ws.part_res = t->part_res;
    IMT_HIP(c, prep::bulk_check(ps, P.ws, d_vals, t->d_val, t->d_sorted[t->sorted_cur], (uint32_t)t->size, (uint32_t)n));
    IMT_HIP(c, hipMemcpyAsync(t->h_err_pin, P.ws.err, sizeof(int), hipMemcpyDeviceToHost, ps));
    const HostTimer w;
    IMT_HIP(c, hipStreamSynchronize(ps));
    wait_ms += w.ms();
    return insertion_verdict(t, *t->h_err_pin, "batch");
}
// Behind the sweep's last write-back on stream s the stored tree holds every rewritten low leaf and nothing of the batch's
// own leaves: the proof of the first free slot M, Z[l] wherever the sibling lies to the right.
static void bulk_frontier(imt_itree* t, hipStream_t s, uint64_t M, uint8_t* append_sib, unsigned fmt) {
    if (!append_sib) return;
    imt_ctx* c = t->ctx;
    launch::gather_frontier(s, launch::TreeView{t->d_nodes, t->d_off, t->d_len, c->d_zero}, M, t->depth, append_sib, fmt);
}
// The append: leaves M .. M + n - 1 from their final preimages (rows [n, 2n) of P.d_pre) and every node above them once --
// apply_hashes over the dense table of the new leaves, in the plan set's tables, which the sweep on s has done with.
static int bulk_append(imt_itree* t, PlanSet& P, hipStream_t s, uint64_t M, size_t n, unsigned L0) {
    imt_ctx* c = t->ctx;
    IMT_HIP(c, prep::append_table(s, (uint32_t)M, (uint32_t)n, P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][2], P.d_tab[0][3]));
    const int rc = apply_hashes(t, P, s, n, L0, t->d_apply_stats);
    if (rc) return rc;
    t->apply_seen = true;
    t->apply_stats_set = nullptr;
    return IMT_OK;
}
// stored_root: d.root is the stored root, converted here; false: a replay's builder has written it there already
static int bulk_deliver_outputs(imt_itree* t, hipStream_t s, const imt_bulk_out* o, const BulkDev& d, size_t n, unsigned flags,
                                bool stored_root = true) {
    imt_ctx* c = t->ctx;
    const unsigned fmt = flags & IMT_FMT_MASK;
    if (fmt != IMT_FMT_CANONICAL) {
        if (d.hashfree.low_leaf) launch::convert(s, d.hashfree.low_leaf, d.hashfree.low_leaf, n * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
        if (d.hashfree.new_leaf) launch::convert(s, d.hashfree.new_leaf, d.hashfree.new_leaf, n * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
    }
    if (d.root && stored_root) launch::convert(s, t->nodes(t->depth), d.root, 1, IMT_FMT_DEVICE, fmt, c->d_err);
    if (flags & IMT_DEVICE_PTRS) return IMT_OK;
    auto back = [&](void* user, const void* from, size_t bytes) -> int {
        if (user && from) IMT_HIP(c, hipMemcpyAsync(user, from, bytes, hipMemcpyDeviceToHost, s));
        return IMT_OK;
    };
    int rc;
    if ((rc = back(o->order, d.hashfree.order, n * 8)) || (rc = back(o->low_index, d.hashfree.low_index, n * 8)) ||
        (rc = back(o->is_largest, d.hashfree.is_largest, n)) || (rc = back(o->low_leaf, d.hashfree.low_leaf, n * 96)) ||
        (rc = back(o->new_leaf, d.hashfree.new_leaf, n * 96)) || (rc = back(o->root_before, d.sweep.old_root, n * 32)) ||
        (rc = back(o->root_after, d.sweep.interim_root, n * 32)) ||
        (rc = back(o->low_sib, d.sweep.low_sib, (size_t)t->depth * n * 32)) ||
        (rc = back(o->append_sib, d.append_sib, (size_t)t->depth * 32)) || (rc = back(o->root, d.root, 32)))
        return rc;
    IMT_HIP(c, hipStreamSynchronize(s));
    return IMT_OK;
}

extern "C" int imt_itree_insert_bulk(imt_itree* t, const void* vals, size_t n, const imt_bulk_out* out, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (n == 0) return IMT_OK;
    if (!vals) return c->fail(IMT_ERR_ARG, "null vals");
    int rc;
    if ((rc = check_mixed_mode(t, flags, BULK_BATCH)) || (rc = check_batch_call(t, n, flags))) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    if ((rc = check_fe_ptrs(c, dev, {vals}))) return rc;
    if (out && (rc = check_fe_ptrs(c, dev, {out->low_leaf, out->root_before, out->root_after, out->low_sib, out->new_leaf,
                                            out->append_sib, out->root})))
        return rc;
    if (dev && out && (((uintptr_t)out->order | (uintptr_t)out->low_index) & 7u))
        return c->fail(IMT_ERR_ARG, "device order / low_index array is not 8-byte aligned");
    if ((rc = check_room(t, n)) || (rc = ensure_device_index(t))) return rc;
    const uint64_t M = t->size;
    const HostTimer host;
    double waited_ms = 0;

    // ---- plan buffers: n events, and the new leaves' preimages behind theirs ----
    PlanSet& P = t->plan[t->cur];
    if ((rc = acquire_plan(t, 2 * n, 0, waited_ms))) return rc;

    // ---- the checks (side stream): nothing of the caller's is written before the batch is accepted ----
    hipStream_t ps = t->up_stream;
    if ((rc = order_behind_caller(t, ps, flags))) return rc;
    size_t slot = 2;
    const uint8_t* d_vals = nullptr;
    uint8_t* up = dev ? nullptr : (uint8_t*)c->dev_scratch(slot++, n * 32);
    if ((rc = stage_canonical(c, ps, vals, n, flags, up, P.d_canon, P.ws.err, &d_vals))) return rc;
    if ((rc = bulk_checks(t, P, d_vals, n, waited_ms))) return rc;

    // ---- accepted: rows, events, tables, merged index, hash-free outputs ----
    BulkDev d;
    if (out && !bulk_stage_outputs(c, dev, slot, out, n, t->depth, d)) return IMT_ERR_HIP;
    uint32_t* erow = P.d_slot;
    IMT_HIP(c, prep::bulk_events(ps, P.ws, t->d_val, t->d_sorted[t->sorted_cur], t->d_sorted[t->sorted_cur ^ 1], (uint32_t)M,
                                 (uint32_t)n, P.d_pre, P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][2], P.d_tab[0][3], erow,
                                 d.hashfree));
    IMT_HIP(c, hipEventRecord(t->up_done, ps));

    // ---- hashing on the context's stream, behind every batch in flight: the rows' sweep over the levels the stored M
    // leaves occupy (above them every event climbs alone against Z[l]), the frontier, the append ----
    hipStream_t s;
    WitnessSweep w;
    if ((rc = hashing_stream(t, false, s, w.pipe))) return rc;
    IMT_HIP(c, hipStreamWaitEvent(s, t->up_done, 0));
    const bool item_major = flags & IMT_SIB_ITEM_MAJOR;
    const launch::SibLayout lay = item_major ? launch::SibLayout{1, t->depth} : launch::SibLayout{n, 1};
    const launch::MixedRoute route{erow, nullptr};
    w.route = &route;
    w.bulk = true;
    const unsigned L0_stored = std::min(ceil_log2(M), t->depth), L0 = std::min(ceil_log2(M + n), t->depth);
    if ((rc = witness_sweep(t, P, s, n, L0_stored, d.sweep, lay, fmt, w))) return rc;
    bulk_frontier(t, s, M, d.append_sib, fmt);
    if ((rc = bulk_append(t, P, s, M, n, L0))) return rc;

    // ---- record, commit, outputs: a batch like any other ----
    IMT_HIP(c, hipMemcpyAsync(P.d_root, t->nodes(t->depth), 32, hipMemcpyDeviceToDevice, s));
    if ((rc = plan_launched(t, P, s, L0, false, false))) return rc;
    index_committed(t, M + n);
    if (c->profiling) {
        c->prof_ms[IMT_PROF_HOST] += host.ms() - waited_ms;
        c->prof_n[IMT_PROF_HOST] += 1;
    }
    if (out) return bulk_deliver_outputs(t, s, out, d, n, flags);
    if (!dev) IMT_HIP(c, hipStreamSynchronize(s));
    return IMT_OK;
}

// The filtered twin: prep::mixed_filter classifies the operations on the side stream, one wait brings back
// the two counts and the error bits, and the accepted operations -- compacted into the plan set, P.fw.acc / aop -- are a
// mixed batch of their own with the caller's level stride.  status / leaf_index are classified into the plan set's
// staging whatever the pointers are: a device-pointer caller's op bytes are checked by the class kernel, and a bad one
// must leave the caller's arrays as they were.  apply != NULL: imt_itree_apply_mixed_filtered -- the accepted operations
// are a witness-free mixed batch instead, and a call that changes nothing still reports the root.
static int mixed_filtered_call(imt_itree* t, const void* vals, const uint8_t* op, size_t n, uint8_t* status, uint64_t* leaf_index,
                               const imt_insert_out* ins, const imt_read_out* rd, uint64_t* n_inserted, uint64_t* n_read,
                               unsigned flags, const ApplyReq* apply) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    if (n_inserted) *n_inserted = 0;        // the counts are 0 on every error
    if (n_read) *n_read = 0;
    IMT_NOT_SLICED(t);
    if (!status || !n_inserted || !n_read) return c->fail(IMT_ERR_ARG, "null status / n_inserted / n_read");
    void* const root_out = apply ? apply->root_out : nullptr;     // nothing inserted: an apply call still reports the root
    if (n == 0) return report_unchanged_root(t, root_out, flags);
    if (!vals || !op) return c->fail(IMT_ERR_ARG, "null vals / op");
    int rc;
    if ((rc = check_mixed_mode(t, flags, MIXED_BATCH)) || (rc = check_batch_call(t, n, flags))) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((rc = check_mixed_ptrs(c, dev, vals, ins, rd))) return rc;
    if (dev && ((uintptr_t)leaf_index & 7u)) return c->fail(IMT_ERR_ARG, "device leaf_index array is not 8-byte aligned");
    if ((rc = check_fe_ptrs(c, dev, {root_out})) || (rc = check_host_ops(c, dev, op, n, flags))) return rc;
    if ((rc = ensure_device_index(t))) return rc;
    double waited_ms = 0;
    PlanSet& P = t->plan[t->cur];
    if ((rc = acquire_plan(t, 2 * n, 0, waited_ms))) return rc;

    // ---- the classification: nothing of the caller's is written before the op bytes are known to be good ----
    hipStream_t ps = t->up_stream;
    if ((rc = order_behind_caller(t, ps, flags))) return rc;
    size_t slot = 2;
    const uint8_t* d_vals = nullptr;
    // the plan's own buffer for the upload as well, as gpu_filter has it
    if ((rc = stage_canonical(c, ps, vals, n, flags, P.d_canon, P.d_canon, P.ws.err, &d_vals))) return rc;
    const uint8_t* d_op = nullptr;
    if ((rc = stage_ops(c, ps, dev, op, n, slot, &d_op))) return rc;
    uint64_t* d_leaf = leaf_index ? P.fw.leaf : nullptr;
    IMT_HIP(c, prep::mixed_filter(ps, P.fw, d_vals, d_op, (uint32_t)n, mixed_max_op(flags), t->d_val, t->d_sorted[t->sorted_cur],
                                  (uint32_t)t->size, t->index_base, P.fw.status, d_leaf, P.ws.err));
    IMT_HIP(c, hipMemcpyAsync(t->h_cnt_pin, P.fw.count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ps));
    IMT_HIP(c, hipMemcpyAsync(t->h_err_pin, P.ws.err, sizeof(int), hipMemcpyDeviceToHost, ps));
    if (!dev) IMT_HIP(c, hipMemcpyAsync(status, P.fw.status, n, hipMemcpyDeviceToHost, ps));     // its op bytes were checked above
    IMT_HIP(c, hipStreamSynchronize(ps));
    if (*t->h_err_pin & prep::ERR_OP) return c->fail(IMT_ERR_ARG, "an op byte is %s", mixed_op_kinds(flags));
    if (dev) IMT_HIP(c, hipMemcpyAsync(status, P.fw.status, n, hipMemcpyDeviceToDevice, ps));
    const size_t n_ins = t->h_cnt_pin[0], n_rd = t->h_cnt_pin[1], n_acc = n_ins + n_rd;
    if (*t->h_err_pin & prep::ERR_NONCANONICAL) rc = c->fail(IMT_ERR_NONCANONICAL, "a value is not reduced (>= p)");
    else rc = check_room(t, n_ins);
    const hipMemcpyKind to_user = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (rc || !n_acc) {       // refused, or nothing to carry out: the classification is the whole answer
        if (leaf_index) IMT_HIP(c, hipMemcpyAsync(leaf_index, d_leaf, n * 8, to_user, ps));
        IMT_HIP(c, hipStreamSynchronize(ps));
        return rc ? rc : report_unchanged_root(t, root_out, flags);
    }

    // ---- the accepted operations: a mixed batch with the caller's dimensions ----
    MixedFiltered fl{nullptr, nullptr, n};
    if (leaf_index) {
        if (dev) {      // the rest of the classification now, the low leaves of the READs straight into the caller's array
            IMT_HIP(c, hipMemcpyAsync(leaf_index, d_leaf, n * 8, to_user, ps));
            fl.d_leaf = leaf_index;
        } else {
            fl.d_leaf = d_leaf;
            fl.h_leaf = leaf_index;
        }
    }
    rc = apply ? apply_mixed_core(t, P, P.fw.acc, P.fw.aop, n_acc, slot, nullptr, nullptr, flags, &fl, *apply)
               : mixed_core(t, P, P.fw.acc, P.fw.aop, n_acc, n, slot, ins, rd, nullptr, nullptr, flags, &fl);
    if (rc) return rc;
    *n_inserted = n_ins;
    *n_read = n_rd;
    return IMT_OK;
}

extern "C" int imt_itree_mixed_filtered(imt_itree* t, const void* vals, const uint8_t* op, size_t n, uint8_t* status,
                                        uint64_t* leaf_index, const imt_insert_out* ins, const imt_read_out* rd,
                                        uint64_t* n_inserted, uint64_t* n_read, unsigned flags) {
    return mixed_filtered_call(t, vals, op, n, status, leaf_index, ins, rd, n_inserted, n_read, flags, nullptr);
}

extern "C" int imt_itree_apply_mixed_filtered(imt_itree* t, const void* vals, const uint8_t* op, size_t n, uint8_t* status,
                                              uint64_t* leaf_index, uint64_t* n_inserted, uint64_t* n_read, void* root_out,
                                              unsigned flags) {
    const ApplyReq req{root_out};
    return mixed_filtered_call(t, vals, op, n, status, leaf_index, nullptr, nullptr, n_inserted, n_read, flags, &req);
}

// ------------------------------------------------------------------------------------
// going back (imt_rewind.hpp)
// ------------------------------------------------------------------------------------
extern "C" int imt_itree_rewind(imt_itree* t, uint64_t new_size, void* root_out, uint64_t* hashes, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (flags & IMT_PIPELINE) return c->fail(IMT_ERR_ARG, "a rewind is not pipelined (IMT_PIPELINE)");
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (new_size == 0 || new_size > t->size)
        return c->fail(IMT_ERR_RANGE, "cannot rewind a tree of %llu leaves to %llu", (unsigned long long)t->size,
                       (unsigned long long)new_size);
    if (slice_open(t)) return c->fail(IMT_ERR_ARG, "a slice is open (issue its remaining units first)");
    if (t->pending.active) return c->fail(IMT_ERR_ARG, "a sharded batch is open (imt_itree_batch_end first)");
    int rc = c->set_device();
    if (rc) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    if ((rc = check_fe_ptrs(c, dev, {root_out}))) return rc;
    const uint64_t M = t->size, S = new_size;
    if (S == M) {
        if (hashes) std::memset(hashes, 0, (t->depth + 1) * 8);
        return report_unchanged_root(t, root_out, flags);
    }
    // ---- behind everything in flight, the caller's stream included: from here on the tree is this call's alone ----
    if ((rc = ensure_device_index(t))) return rc;
    if ((rc = join_top(t))) return rc;
    for (auto& pl : t->plan)
        if (pl.in_flight) { IMT_HIP(c, hipEventSynchronize(pl.done)); pl.in_flight = false; pl.pipelined = false; }
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    hipStream_t s = c->stream;
    const unsigned L0 = std::min(ceil_log2(M), t->depth);       // of the size the call finds: the nodes in use reach that high
    const size_t max_rows = (size_t)std::min(M - S, S) + 1;
    const ScratchTrim trim{c, 3, 3};        // the scan's places are 8 bytes per leaf of the tree: not something a context keeps
    const size_t ws_bytes = prep::rewind_ws_bytes((size_t)M, max_rows);
    void* ws = c->dev_scratch(3, ws_bytes);
    uint8_t* d_root = (root_out && !dev) ? (uint8_t*)c->dev_scratch(0, 32) : (uint8_t*)root_out;
    if (!ws || (root_out && !d_root)) return IMT_ERR_HIP;
    // ---- the index of the earlier tree into the other buffer, and how many leaves are relinked ----
    const uint32_t* sorted_old = t->d_sorted[t->sorted_cur];
    uint32_t* sorted_new = t->d_sorted[t->sorted_cur ^ 1];
    const uint32_t* d_relinked = nullptr;
    uint32_t R = 0;
    IMT_HIP(c, prep::rewind_compact(s, ws, ws_bytes, sorted_old, sorted_new, (uint32_t)M, (uint32_t)S, &d_relinked));
    IMT_HIP(c, hipMemcpyAsync(&R, d_relinked, sizeof(R), hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipStreamSynchronize(s));
    if ((size_t)R + 1 > max_rows) return c->fail(IMT_ERR_INTERNAL, "rewind: %u relinked leaves, at most %zu expected", R, max_rows - 1);
    const size_t E = (size_t)R + 1;                             // one event per touched leaf: the relinked ones and slot S
    // ---- a plan set owns the tables and the lists; nothing of the tree has been written up to here ----
    PlanSet& P = t->plan[t->cur];
    double waited = 0;
    if ((rc = acquire_plan(t, E, 0, waited))) return rc;
    IMT_HIP(c, prep::rewind_table(s, ws, ws_bytes, t->d_val, sorted_old, sorted_new, (uint32_t)M, (uint32_t)S, t->index_base,
                                  (uint32_t)E, P.d_tab[1][0], P.d_tab[1][1], P.d_pre, P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][2],
                                  P.d_tab[0][3]));
    prep::rewind_refill(s, t->d_nodes, t->d_off, t->d_len, c->d_zero, S, M, L0);
    if ((rc = apply_hashes(t, P, s, E, L0, t->d_rewind_stats))) return rc;
    if (root_out) launch::convert(s, t->nodes(t->depth), d_root, 1, IMT_FMT_DEVICE, fmt, c->d_err);
    if (root_out && !dev) IMT_HIP(c, hipMemcpyAsync(root_out, d_root, 32, hipMemcpyDeviceToHost, s));
    if (hashes) IMT_HIP(c, hipMemcpyAsync(hashes, t->d_rewind_stats, (t->depth + 1) * 8, hipMemcpyDeviceToHost, s));
    // ---- everything is enqueued: the earlier tree is the tree ----
    t->sorted_cur ^= 1;
    t->size = S;
    t->pre.clear();
    t->pre.shrink_to_fit();
    t->sorted.clear();
    t->sorted.shrink_to_fit();
    t->mirror_valid = false;
    t->dev_index_valid = true;
    t->gen++;
    for (auto& pl : t->plan) pl.has_root = pl.has_root2 = false;
    IMT_HIP(c, hipStreamSynchronize(s));
    return IMT_OK;
}

// ------------------------------------------------------------------------------------
// filtered batch insertion and value lookup (imt_filter_logic.hpp)
// ------------------------------------------------------------------------------------
namespace {

// position in t->sorted of the first stored value >= v
size_t find_ge(const imt_itree* t, const U256& v) {
    size_t lo = 0, hi = t->sorted.size();
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (cmp_ent(t, t->sorted[mid], v) < 0) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The classification on the device (prep::filter), on the side stream behind everything the batches before this one
// enqueued there: the index it reads is the one committed when the last of them was prepared.  The accepted values end
// up in P.fw.acc; one synchronisation for their number and the error bits.
int gpu_filter(imt_itree* t, PlanSet& P, const void* vals, size_t n, unsigned flags, uint8_t* status,
               uint64_t* leaf_index, size_t& n_acc) {
    imt_ctx* c = t->ctx;
    const bool dev = flags & IMT_DEVICE_PTRS;
    int rc = ensure_device_index(t);
    if (rc) return rc;
    hipStream_t ps = t->up_stream;
    const uint8_t* d_vals = nullptr;
    // the plan's own buffer for the upload as well, not context scratch (see gpu_prepare)
    if ((rc = stage_canonical(c, ps, vals, n, flags, P.d_canon, P.d_canon, P.ws.err, &d_vals))) return rc;
    uint8_t* d_st = dev ? status : P.fw.status;
    uint64_t* d_leaf = leaf_index ? (dev ? leaf_index : P.fw.leaf) : nullptr;
    IMT_HIP(c, prep::filter(ps, P.fw, d_vals, (uint32_t)n, t->d_val, t->d_sorted[t->sorted_cur], (uint32_t)t->size,
                            t->index_base, t->part_mod, t->part_res, d_st, d_leaf, P.ws.err));
    IMT_HIP(c, hipMemcpyAsync(t->h_cnt_pin, P.fw.count, sizeof(uint32_t), hipMemcpyDeviceToHost, ps));
    IMT_HIP(c, hipMemcpyAsync(t->h_err_pin, P.ws.err, sizeof(int), hipMemcpyDeviceToHost, ps));
    if (!dev) {
        IMT_HIP(c, hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, ps));
        if (leaf_index) IMT_HIP(c, hipMemcpyAsync(leaf_index, d_leaf, n * 8, hipMemcpyDeviceToHost, ps));
    }
    IMT_HIP(c, hipStreamSynchronize(ps));
    if (*t->h_err_pin & prep::ERR_NONCANONICAL) return c->fail(IMT_ERR_NONCANONICAL, "a value is not reduced (>= p)");
    n_acc = *t->h_cnt_pin;
    return IMT_OK;
}

// IMT_HOST_PREP: the same rule over the host mirror -- a binary search per value, a sort of the batch -- stated
// independently of the kernels.  The accepted values, canonical, go to `acc` in input order.
int host_filter(imt_itree* t, const void* vals, size_t n, unsigned flags, uint8_t* status, uint64_t* leaf_index,
                std::vector<U256>& acc) {
    imt_ctx* c = t->ctx;
    const bool dev = flags & IMT_DEVICE_PTRS;
    int rc = ensure_mirror(t);
    if (rc) return rc;
    std::vector<U256> v;
    if ((rc = fetch_canonical(c, dev ? t->up_stream : c->stream, vals, n, flags, v))) return rc;
    const uint64_t M = t->size, base = t->index_base;
    std::vector<uint8_t> st(n);
    std::vector<uint64_t> aux(n, 0), leaf(n);
    std::vector<uint32_t> ord;
    for (size_t i = 0; i < n; i++) {
        st[i] = prep::filter_class(reinterpret_cast<const uint8_t*>(v[i].data()), t->part_mod, t->part_res);
        if (st[i] != prep::VAL_NEW) continue;
        const size_t q = find_ge(t, v[i]);
        if (q < t->sorted.size() && cmp_ent(t, t->sorted[q], v[i]) == 0) {
            st[i] = prep::VAL_PRESENT;
            aux[i] = t->sorted[q].idx;
        } else {
            ord.push_back((uint32_t)i);
        }
    }
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return lt256(v[a], v[b]) || (v[a] == v[b] && a < b); });
    for (size_t r = 1, head = 0; r < ord.size(); r++) {
        if (v[ord[r]] != v[ord[head]]) { head = r; continue; }
        st[ord[r]] = prep::VAL_REPEATED;
        aux[ord[r]] = ord[head];
    }
    acc.clear();
    std::vector<uint64_t> rank(n, 0);
    for (size_t i = 0; i < n; i++)
        if (st[i] == prep::VAL_NEW) {
            rank[i] = acc.size();
            acc.push_back(v[i]);
        }
    for (size_t i = 0; i < n; i++) {
        switch (st[i]) {
            case prep::VAL_NEW: leaf[i] = base + M + rank[i]; break;
            case prep::VAL_REPEATED: leaf[i] = base + M + rank[aux[i]]; break;
            case prep::VAL_PRESENT: leaf[i] = base + aux[i]; break;
            case prep::VAL_ZERO: leaf[i] = base; break;
            default: leaf[i] = prep::LEAF_NONE;
        }
    }
    if (dev) {
        IMT_HIP(c, hipMemcpyAsync(status, st.data(), n, hipMemcpyHostToDevice, t->up_stream));
        if (leaf_index) IMT_HIP(c, hipMemcpyAsync(leaf_index, leaf.data(), n * 8, hipMemcpyHostToDevice, t->up_stream));
        IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    } else {
        std::memcpy(status, st.data(), n);
        if (leaf_index) std::memcpy(leaf_index, leaf.data(), n * 8);
    }
    return IMT_OK;
}

}  // namespace

// the body of imt_itree_insert_filtered and (apply != NULL) imt_itree_apply_filtered
static int filtered_core(imt_itree* t, const void* vals, size_t n, uint8_t* status, uint64_t* leaf_index,
                         uint64_t* n_inserted, const imt_insert_out* out, unsigned flags, const ApplyReq* apply) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (!status || !n_inserted) return c->fail(IMT_ERR_ARG, "null status / n_inserted");
    if (apply && (flags & IMT_PIPELINE)) return c->fail(IMT_ERR_ARG, "apply batches are not pipelined (IMT_PIPELINE)");
    void* const root_out = apply ? apply->root_out : nullptr;     // nothing inserted: an apply call still reports the root
    if (n == 0) {
        *n_inserted = 0;
        return report_unchanged_root(t, root_out, flags);
    }
    if (!vals) return c->fail(IMT_ERR_ARG, "null vals");
    int rc = check_batch_call(t, n, flags);
    if (rc) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((rc = check_fe_ptrs(c, dev, {vals})) || (rc = check_out_ptrs(c, dev, out))) return rc;
    if (dev && ((uintptr_t)leaf_index & 7u)) return c->fail(IMT_ERR_ARG, "device leaf_index array is not 8-byte aligned");
    *n_inserted = 0;

    // the plan set the batch will run on: its buffers hold the classification too
    double waited_ms = 0;            // not part of any profile: the host time of the insertion starts in insert_core
    PlanSet& P = t->plan[t->cur];
    if ((rc = acquire_plan(t, 2 * n, 0, waited_ms))) return rc;
    if (dev && (flags & IMT_PIPELINE) && (rc = reserve_all_plans(t, 2 * n))) return rc;
    if ((rc = order_behind_caller(t, t->up_stream, flags))) return rc;
    size_t n_acc = 0;
    const void* acc = nullptr;       // the accepted values, canonical: in the plan set (device), or in h_acc (host)
    unsigned acc_flags = 0;
    std::vector<U256> h_acc;
    if (flags & IMT_HOST_PREP) {
        rc = host_filter(t, vals, n, flags, status, leaf_index, h_acc);
        acc = h_acc.data();
        acc_flags = IMT_FMT_CANONICAL;
        n_acc = h_acc.size();
    } else {
        rc = gpu_filter(t, P, vals, n, flags, status, leaf_index, n_acc);
        acc = P.fw.acc;
        acc_flags = IMT_FMT_CANONICAL | IMT_DEVICE_PTRS;
    }
    if (rc) return rc;
    if (!n_acc) {
        if ((rc = report_unchanged_root(t, root_out, flags))) return rc;
    } else {
        if ((rc = check_fe_ptrs(c, dev, {root_out})) || (rc = check_room(t, n_acc))) return rc;
        // The insertion of the accepted values, on the plan set taken above: insert_core's own acquire_plan finds it idle
        // and reserved for 2 * n >= 2 * n_acc events, so P.fw.acc stays where it is, and its order_behind_caller repeats
        // the one above.  The outputs keep the caller's dimensions: level stride n, not n_acc.
        if ((rc = insert_core(t, acc, acc_flags, n_acc, out, flags, n, apply))) return rc;
    }
    *n_inserted = n_acc;
    return IMT_OK;
}

extern "C" int imt_itree_insert_filtered(imt_itree* t, const void* vals, size_t n, uint8_t* status, uint64_t* leaf_index,
                                         uint64_t* n_inserted, const imt_insert_out* out, unsigned flags) {
    return filtered_core(t, vals, n, status, leaf_index, n_inserted, out, flags, nullptr);
}

extern "C" int imt_itree_apply_filtered(imt_itree* t, const void* vals, size_t n, uint8_t* status, uint64_t* leaf_index,
                                        uint64_t* n_inserted, void* root_out, unsigned flags) {
    const ApplyReq req{root_out};
    return filtered_core(t, vals, n, status, leaf_index, n_inserted, nullptr, flags, &req);
}

static int lookup_batch(imt_itree* t, const imt_itree_view* v, const void* vals, size_t n, uint8_t* status,
                        uint64_t* leaf_index, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (!status) return c->fail(IMT_ERR_ARG, "null status");
    if (n == 0) return IMT_OK;
    if (!vals) return c->fail(IMT_ERR_ARG, "null vals");
    int rc = c->set_device();
    if (rc) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    if ((rc = check_fe_ptrs(c, dev, {vals}))) return rc;
    if (fmt == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (n > ((size_t)1 << 31)) return c->fail(IMT_ERR_RANGE, "batch too large");
    if (dev && ((uintptr_t)leaf_index & 7u)) return c->fail(IMT_ERR_ARG, "device leaf_index array is not 8-byte aligned");
    if ((rc = ensure_device_index(t))) return rc;
    if ((rc = join_top(t))) return rc;
    hipStream_t s = c->stream;
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    const uint8_t* d_vals = nullptr;
    int* d_perr = (int*)c->dev_scratch(2, sizeof(int));
    if (!d_perr) return IMT_ERR_HIP;
    uint8_t* buf = (!dev || fmt != IMT_FMT_CANONICAL) ? (uint8_t*)c->dev_scratch(0, n * 32) : nullptr;
    if ((rc = stage_canonical(c, s, vals, n, flags, buf, buf, d_perr, &d_vals))) return rc;
    uint8_t* d_st = dev ? status : (uint8_t*)c->dev_scratch(3, n);
    uint64_t* d_leaf = (dev || !leaf_index) ? leaf_index : (uint64_t*)c->dev_scratch(1, n * 8);
    if (!d_st || (leaf_index && !d_leaf)) return IMT_ERR_HIP;
    prep::lookup(s, d_vals, t->d_val, read_index(t, v), (uint32_t)read_size(t, v), (uint32_t)n, t->index_base,
                 t->part_mod, t->part_res, d_st, d_leaf, d_perr);
    int perr = 0;
    IMT_HIP(c, hipMemcpyAsync(&perr, d_perr, sizeof(int), hipMemcpyDeviceToHost, s));
    if (!dev) {
        IMT_HIP(c, hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, s));
        if (leaf_index) IMT_HIP(c, hipMemcpyAsync(leaf_index, d_leaf, n * 8, hipMemcpyDeviceToHost, s));
    }
    IMT_HIP(c, hipStreamSynchronize(s));
    if (perr & prep::ERR_NONCANONICAL) return c->fail(IMT_ERR_NONCANONICAL, "a value is not reduced (>= p)");
    return IMT_OK;
}
extern "C" int imt_itree_lookup_batch(imt_itree* t, const void* vals, size_t n, uint8_t* status, uint64_t* leaf_index,
                                      unsigned flags) {
    return lookup_batch(t, nullptr, vals, n, status, leaf_index, flags);
}

// ------------------------------------------------------------------------------------
// read-only views at an earlier size (imt_view.hpp)
// ------------------------------------------------------------------------------------
// The views that exist.  A view handle is looked up here before anything is read through it, so a handle that is not a
// live view -- a freed one, a tree's -- is an argument error like a NULL one and never a wild read.
static std::mutex g_views_mu;
static std::unordered_set<const imt_itree_view*> g_views;
static bool view_alive(const imt_itree_view* v) {
    std::lock_guard<std::mutex> lock(g_views_mu);
    return v && g_views.count(v) != 0;
}

// what imt_itree_rewind refuses for the state the tree is in, in its words
static int check_view_call(imt_itree* t, unsigned flags) {
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (flags & IMT_PIPELINE) return c->fail(IMT_ERR_ARG, "a view is not pipelined (IMT_PIPELINE)");
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (slice_open(t)) return c->fail(IMT_ERR_ARG, "a slice is open (issue its remaining units first)");
    if (t->pending.active) return c->fail(IMT_ERR_ARG, "a sharded batch is open (imt_itree_batch_end first)");
    return c->set_device();
}

static void view_release_build(imt_itree_view* v) {
    for (void* q : {(void*)v->d_tab[0], (void*)v->d_tab[1], (void*)v->d_tab[2], (void*)v->d_tab[3], (void*)v->d_src,
                    (void*)v->d_pre, (void*)v->d_list, (void*)v->d_side})
        if (q) hipFree(q);
    for (auto& q : v->d_tab) q = nullptr;
    v->d_src = nullptr;
    v->d_pre = nullptr;
    v->d_list = nullptr;
    v->d_side = nullptr;
    v->rows_cap = 0;
    v->levels_cap = 0;
}

// the view's buffers for a build of `rows` table rows and `levels` list levels
static int view_reserve(imt_itree_view* v, size_t rows, unsigned levels) {
    if (v->rows_cap >= rows && v->levels_cap >= levels) return IMT_OK;
    imt_ctx* c = v->t->ctx;
    view_release_build(v);
    const size_t E = rows + rows / 4;
    hipError_t e = hipSuccess;
    auto A = [&](void** ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(ptr, bytes);
    };
    for (auto& q : v->d_tab) A((void**)&q, E * 4);
    A((void**)&v->d_src, E * 4);
    A((void**)&v->d_pre, E * 96);
    A((void**)&v->d_list, (size_t)levels * E * 4);
    A((void**)&v->d_side, (size_t)levels * E * 32);
    if (e != hipSuccess) {
        view_release_build(v);
        return c->hip_fail(e, "hipMalloc(view)");
    }
    v->rows_cap = E;
    v->levels_cap = levels;
    return IMT_OK;
}

// The context's stream behind everything in flight on the tree, with the device index current: what a view's build and
// a replay read -- stored nodes, d_val, the index -- is then the tree's committed state.
static int view_behind_tree(imt_itree* t) {
    imt_ctx* c = t->ctx;
    int rc;
    if ((rc = ensure_device_index(t))) return rc;
    if ((rc = join_top(t))) return rc;
    for (const auto& pl : t->plan)                              // and behind whatever else a plan set still has in flight: the
        if (pl.in_flight) IMT_HIP(c, hipStreamWaitEvent(c->stream, pl.done, 0));   // sets themselves stay as they are
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));             // the index is written on the side stream
    return IMT_OK;
}

// The cache for (v->size, the tree as it is): the index of the earlier tree and the side table, on the context's stream
// behind everything in flight on the tree.  imt_itree_rewind's sequence with two differences: every output goes to the
// view's memory, and nothing is refilled or written back -- the hashes read their children through the rule instead.
static int view_build(imt_itree_view* v) {
    imt_itree* t = v->t;
    imt_ctx* c = t->ctx;
    const uint64_t M = t->size, S = v->size;
    int rc;
    if (S == M) {                                               // the tree answers: nothing to compute, nothing cached
        std::memset(v->h_hashes, 0, sizeof(v->h_hashes));
        v->current = true;
        v->gen = t->gen;
        v->builds++;
        return IMT_OK;
    }
    if ((rc = view_behind_tree(t))) return rc;
    hipStream_t s = c->stream;
    const unsigned L0 = std::min(ceil_log2(M), t->depth);
    const size_t max_rows = (size_t)std::min(M - S, S) + 1;
    const ScratchTrim trim{c, 3, 3};
    const size_t ws_bytes = prep::rewind_ws_bytes((size_t)M, max_rows);
    void* ws = c->dev_scratch(3, ws_bytes);
    if (!ws) return IMT_ERR_HIP;
    const uint32_t* sorted_now = t->d_sorted[t->sorted_cur];
    const uint32_t* d_relinked = nullptr;
    uint32_t R = 0;
    IMT_HIP(c, prep::rewind_compact(s, ws, ws_bytes, sorted_now, v->d_sorted, (uint32_t)M, (uint32_t)S, &d_relinked));
    IMT_HIP(c, hipMemcpyAsync(&R, d_relinked, sizeof(R), hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipStreamSynchronize(s));
    if ((size_t)R + 1 > max_rows) return c->fail(IMT_ERR_INTERNAL, "view: %u relinked leaves, at most %zu expected", R, max_rows - 1);
    const size_t E = (size_t)R + 1;
    if ((rc = view_reserve(v, E, L0))) return rc;
    const size_t stride = v->rows_cap;
    // scratch of the build alone: the unsorted table, the scans' places and their temporary storage
    const size_t tmp_bytes = prep::apply_lists_tmp_bytes(E);
    const size_t pos_bytes = ((size_t)L0 * stride * 4 + 255) & ~(size_t)255, key_bytes = (E * 4 + 255) & ~(size_t)255;
    uint8_t* scr = (uint8_t*)c->dev_scratch(0, pos_bytes + 2 * key_bytes + tmp_bytes);
    if (!scr) return IMT_ERR_HIP;
    uint32_t* pos = (uint32_t*)scr;
    uint32_t* key = (uint32_t*)(scr + pos_bytes);
    uint32_t* row = (uint32_t*)(scr + pos_bytes + key_bytes);
    void* tmp = scr + pos_bytes + 2 * key_bytes;
    IMT_HIP(c, prep::rewind_table(s, ws, ws_bytes, t->d_val, sorted_now, v->d_sorted, (uint32_t)M, (uint32_t)S, t->index_base,
                                  (uint32_t)E, key, row, v->d_pre, v->d_tab[0], v->d_tab[1], v->d_tab[2], v->d_tab[3]));
    const apply::Lists lists{v->d_list, v->d_src, v->d_count, stride};
    IMT_HIP(c, prep::apply_lists(s, tmp, tmp_bytes, v->d_tab[0], v->d_tab[1], v->d_tab[3], (uint32_t)E, L0, t->depth, pos, lists));
    v->top = L0;
    const view::Side side = v->side();
    launch::view_leaves(s, lists.count, apply::bound((uint32_t)E, L0, 0), lists.node, lists.src, v->d_pre, IMT_FMT_CANONICAL,
                        c->d_err, v->d_side, t->h_len[0], c->coop_max_events);
    for (unsigned l = 0; l + 1 < L0; l++)
        launch::view_level(s, side, l, apply::bound((uint32_t)E, L0, l + 1), t->nodes(l), t->h_len[l],
                           c->d_zero + (size_t)l * 32, v->d_side + (size_t)(l + 1) * stride * 32, t->h_len[l + 1],
                           c->coop_max_events);
    launch::view_top(s, side, launch::TreeView{t->d_nodes, t->d_off, t->d_len, c->d_zero, t->index_base}, v->d_chain, L0 - 1,
                     t->depth);
    IMT_HIP(c, hipMemcpyAsync(v->h_hashes, v->d_count, (t->depth + 1) * 8, hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipStreamSynchronize(s));
    v->current = false;
    v->gen = t->gen;
    v->builds++;
    return IMT_OK;
}

// every query starts here: the refusals, then the cache brought up to the tree
static int view_enter(imt_itree_view* v, unsigned flags) {
    if (!view_alive(v)) return IMT_ERR_ARG;
    imt_itree* t = v->t;
    int rc = check_view_call(t, flags);
    if (rc) return rc;
    if (t->size < v->size)
        return t->ctx->fail(IMT_ERR_RANGE, "the tree holds %llu leaves, fewer than the view's %llu", (unsigned long long)t->size,
                            (unsigned long long)v->size);
    return v->gen == t->gen ? IMT_OK : view_build(v);
}
// the view a query is answered from: none when the tree itself is the answer
static const imt_itree_view* view_source(const imt_itree_view* v) { return v->current ? nullptr : v; }

extern "C" int imt_itree_view_create(imt_itree* t, uint64_t size, imt_itree_view** out) {
    if (!t || !out) return IMT_ERR_ARG;
    *out = nullptr;
    imt_ctx* c = t->ctx;
    int rc = check_view_call(t, 0);
    if (rc) return rc;
    if (size == 0 || size > t->size)
        return c->fail(IMT_ERR_RANGE, "no view at %llu leaves of a tree of %llu", (unsigned long long)size, (unsigned long long)t->size);
    imt_itree_view* v = new (std::nothrow) imt_itree_view();
    if (!v) return c->fail(IMT_ERR_ALLOC, "out of host memory");
    v->t = t;
    v->size = size;
    hipError_t e;
    if ((e = hipMalloc((void**)&v->d_sorted, size * 4)) != hipSuccess ||
        (e = hipMalloc((void**)&v->d_count, (IMT_MAX_DEPTH + 1) * 8)) != hipSuccess ||
        (e = hipMalloc((void**)&v->d_chain, (IMT_MAX_DEPTH + 1) * 32)) != hipSuccess) {
        for (void* q : {(void*)v->d_sorted, (void*)v->d_count, (void*)v->d_chain})
            if (q) hipFree(q);
        delete v;
        return c->hip_fail(e, "hipMalloc(view)");
    }
    {
        std::lock_guard<std::mutex> lock(g_views_mu);
        g_views.insert(v);
    }
    *out = v;
    return IMT_OK;
}

extern "C" void imt_itree_view_free(imt_itree_view* v) {
    {
        std::lock_guard<std::mutex> lock(g_views_mu);
        if (!v || !g_views.erase(v)) return;
    }
    imt_ctx* c = v->t->ctx;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    view_release_build(v);
    plan_free(v->plan);
    for (void* q : {(void*)v->d_sorted, (void*)v->d_count, (void*)v->d_chain})
        if (q) hipFree(q);
    delete v;
}

extern "C" uint64_t imt_itree_view_size(const imt_itree_view* v) { return view_alive(v) ? v->size : 0; }

// ------------------------------------------------------------------------------------
// another capacity for the tree that exists (imt_resize.hpp)
// ------------------------------------------------------------------------------------
extern "C" uint64_t imt_itree_capacity(const imt_itree* t) { return t ? t->cap : 0; }

static int reserve_alloc(imt_ctx* c, void** q, size_t bytes, const char* what);
static void reserve_free(void* q);
// A workspace's temporary storage was sized for (cap_n values, the capacity of the day): large enough for new_cap, the
// rest of the workspace -- and of the plan set around it, d_root above all -- left where it is.  Nothing is in flight.
static int ws_fit(imt_ctx* c, prep::Workspace& w, size_t new_cap) {
    if (!w.cap_n) return IMT_OK;
    const size_t need = prep::temp_bytes_needed(w.cap_n, new_cap);
    if (need <= w.tmp_bytes) return IMT_OK;
    void* q = nullptr;
    int rc = reserve_alloc(c, &q, need, "a batch workspace");
    if (rc) return rc;
    if (w.tmp) reserve_free(w.tmp);
    w.tmp = q;
    w.tmp_bytes = need;
    return IMT_OK;
}

// host milliseconds the running imt_itree_reserve has spent in hipMalloc and hipFree (imt_itree_reserve_stats)
static thread_local double g_reserve_mem_ms = 0;
static void reserve_free(void* q) {
    const HostTimer w;
    hipFree(q);
    g_reserve_mem_ms += w.ms();
}
static int reserve_alloc(imt_ctx* c, void** q, size_t bytes, const char* what) {
    const HostTimer w;
    const hipError_t e = hipMalloc(q, bytes);
    g_reserve_mem_ms += w.ms();
    if (e == hipSuccess) return IMT_OK;
    (void)hipGetLastError();
    *q = nullptr;
    return c->fail(IMT_ERR_ALLOC, "imt_itree_reserve: no %zu bytes for %s", bytes, what);
}
// `rows` rows of `row_bytes` into a new array of new_cap rows -- q if the caller has it already -- and the old array
// freed once the copy has left the stream: the new one exists before the old one goes, so the peak is one array more,
// and a failure leaves *arr as it was.
template <class T>
static int reserve_rows(imt_ctx* c, T** arr, void* have, size_t new_cap, size_t rows, size_t row_bytes, const char* what) {
    T* q = (T*)have;
    int rc;
    if (!q && (rc = reserve_alloc(c, (void**)&q, new_cap * row_bytes, what))) return rc;
    hipError_t e = hipSuccess;
    if (rows) e = hipMemcpyAsync(q, *arr, rows * row_bytes, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        hipFree(q);
        return c->hip_fail(e, "imt_itree_reserve copy");
    }
    reserve_free(*arr);
    *arr = q;
    return IMT_OK;
}

extern "C" int imt_itree_reserve(imt_itree* t, uint64_t new_capacity, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (flags & IMT_PIPELINE) return c->fail(IMT_ERR_ARG, "a reserve is not pipelined (IMT_PIPELINE)");
    if (flags) return c->fail(IMT_ERR_ARG, "imt_itree_reserve takes no flags");
    const uint64_t C = new_capacity;
    if (C < 2 || (C & (C - 1)) || C > ((uint64_t)1 << 31))
        return c->fail(IMT_ERR_RANGE, "capacity must be a power of two in [2, 2^31]");
    if (t->depth < 63 && C > ((uint64_t)1 << t->depth)) return c->fail(IMT_ERR_RANGE, "capacity exceeds 2^depth");
    if (C < t->size)
        return c->fail(IMT_ERR_RANGE, "a tree of %llu leaves does not fit a capacity of %llu", (unsigned long long)t->size,
                       (unsigned long long)C);
    if (slice_open(t)) return c->fail(IMT_ERR_ARG, "a slice is open (issue its remaining units first)");
    if (t->pending.active) return c->fail(IMT_ERR_ARG, "a sharded batch is open (imt_itree_batch_end first)");
    int rc = c->set_device();
    if (rc) return rc;
    if (C == t->cap) return IMT_OK;
    const HostTimer whole;
    g_reserve_mem_ms = 0;
    float kernel_ms = 0;
    // ---- behind everything in flight, the caller's stream included (imt_itree_rewind's sequence) ----
    if ((rc = join_top(t))) return rc;
    for (auto& pl : t->plan)
        if (pl.in_flight) { IMT_HIP(c, hipEventSynchronize(pl.done)); pl.in_flight = false; pl.pipelined = false; }
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    hipStream_t s = c->stream;
    IMT_HIP(c, hipStreamSynchronize(s));
    const unsigned D = t->depth;
    const uint64_t total = resize::total_nodes(C, D);
    // A shrinking tree must not be left with its capacity over an array of the smaller one, so every new array exists
    // before the first old one goes (together they are at most half the old tree).  A growing tree takes one at a time.
    void *q_val = nullptr, *q_sorted[2] = {nullptr, nullptr}, *q_extra = nullptr;
    if (C < t->cap) {
        if ((rc = reserve_alloc(c, &q_val, C * 32, "the values")) || (rc = reserve_alloc(c, &q_sorted[0], C * 4, "the index")) ||
            (rc = reserve_alloc(c, &q_sorted[1], C * 4, "the index")) ||
            (t->d_sorted_extra && (rc = reserve_alloc(c, &q_extra, C * 4, "the index")))) {
            for (void* q : {q_val, q_sorted[0], q_sorted[1], q_extra})
                if (q) hipFree(q);
            return rc;
        }
    }
    // ---- the nodes: every level of the new layout in one launch, Z[l] where the old layout has no node ----
    {
        std::vector<uint64_t> off(D + 1), len(D + 1);
        for (unsigned l = 0; l <= D; l++) {
            off[l] = resize::level_off(C, l);
            len[l] = resize::level_len(C, l);
        }
        uint8_t* nodes = nullptr;
        uint64_t *d_off = nullptr, *d_len = nullptr;
        hipError_t e;
        if ((rc = reserve_alloc(c, (void**)&nodes, total * 32, "the nodes")) || (rc = reserve_alloc(c, (void**)&d_off, (D + 1) * 8, "the offsets")) ||
            (rc = reserve_alloc(c, (void**)&d_len, (D + 1) * 8, "the lengths"))) {
            for (void* q : {(void*)nodes, (void*)d_off, (void*)d_len, q_val, q_sorted[0], q_sorted[1], q_extra})
                if (q) hipFree(q);
            return rc;
        }
        hipEvent_t k0 = nullptr, k1 = nullptr;          // the kernel's own time, for imt_itree_reserve_stats; optional
        if (hipEventCreate(&k0) != hipSuccess || hipEventCreate(&k1) != hipSuccess) {
            (void)hipGetLastError();
            if (k0) hipEventDestroy(k0);
            k0 = k1 = nullptr;
        }
        if ((e = hipMemcpyAsync(d_off, off.data(), (D + 1) * 8, hipMemcpyHostToDevice, s)) == hipSuccess &&
            (e = hipMemcpyAsync(d_len, len.data(), (D + 1) * 8, hipMemcpyHostToDevice, s)) == hipSuccess) {
            if (k0) hipEventRecord(k0, s);
            launch::restride_levels(s, t->d_nodes, t->d_off, t->d_len, nodes, d_off, total, c->d_zero, D);
            e = hipGetLastError();
            if (k1) hipEventRecord(k1, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e == hipSuccess && k1 && hipEventElapsedTime(&kernel_ms, k0, k1) != hipSuccess) kernel_ms = 0;
        }
        if (k0) hipEventDestroy(k0);
        if (k1) hipEventDestroy(k1);
        if (e != hipSuccess) {
            for (void* q : {(void*)nodes, (void*)d_off, (void*)d_len, q_val, q_sorted[0], q_sorted[1], q_extra})
                if (q) hipFree(q);
            return c->hip_fail(e, "imt_itree_reserve nodes");
        }
        // The nodes are in the new layout from here on.  Should a later array of a growing tree fail, the tree keeps its
        // capacity over a node array of the larger one: every reader and writer goes through h_len / d_len, and between
        // the two layouts the nodes differ only where both read Z[l].
        for (void* q : {(void*)t->d_nodes, (void*)t->d_off, (void*)t->d_len}) reserve_free(q);
        t->d_nodes = nodes;
        t->d_off = d_off;
        t->d_len = d_len;
        t->h_off = off;
        t->h_len = len;
    }
    // ---- one array at a time: the values, the index buffers (only the current one holds anything), the third one ----
    rc = reserve_rows(c, &t->d_val, q_val, C, t->size, 32, "the values");
    q_val = nullptr;                // the tree's now, or freed
    for (int b = 0; b < 2 && !rc; b++) {
        rc = reserve_rows(c, &t->d_sorted[b], q_sorted[b], C, b == t->sorted_cur ? t->size : 0, 4, "the index");
        q_sorted[b] = nullptr;
    }
    if (t->d_sorted_extra && !rc) {
        rc = reserve_rows(c, &t->d_sorted_extra, q_extra, C, 0, 4, "the index");
        q_extra = nullptr;
    }
    if (rc) {
        for (void* q : {q_val, q_sorted[0], q_sorted[1], q_extra})
            if (q) hipFree(q);
        return rc;
    }
    // ---- workspaces sized from the capacity: the tree's plan sets, each view's own, the slices' ----
    if (C > t->cap) {
        for (auto& pl : t->plan)
            if ((rc = ws_fit(c, pl.ws, C))) return rc;
        if ((rc = ws_fit(c, t->fws, C))) return rc;
        std::lock_guard<std::mutex> lock(g_views_mu);
        for (const imt_itree_view* cv : g_views) {
            imt_itree_view* v = const_cast<imt_itree_view*>(cv);
            if (v->t == t && (rc = ws_fit(c, v->plan.ws, C))) return rc;
        }
    }
    t->cap = C;
    t->reserve_ms[0] = whole.ms();
    t->reserve_ms[1] = kernel_ms;
    t->reserve_ms[2] = g_reserve_mem_ms;
    return IMT_OK;
}

extern "C" int imt_itree_reserve_stats(const imt_itree* t, double* ms) {
    if (!t || !ms) return IMT_ERR_ARG;
    for (int i = 0; i < 3; i++) ms[i] = t->reserve_ms[i];
    return IMT_OK;
}

extern "C" int imt_itree_view_root(imt_itree_view* v, void* root, unsigned flags) {
    if (!view_alive(v) || !root) return IMT_ERR_ARG;
    int rc = view_enter(v, flags);
    if (rc) return rc;
    imt_itree* t = v->t;
    if (v->current) return imt_itree_root(t, root, flags);
    imt_ctx* c = t->ctx;
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((rc = check_fe_ptrs(c, dev, {root}))) return rc;
    const uint8_t* src = v->d_chain + (size_t)t->depth * 32;
    uint8_t* d = dev ? (uint8_t*)root : (uint8_t*)c->dev_scratch(0, 32);
    if (!d) return IMT_ERR_HIP;
    launch::convert(c->stream, src, d, 1, IMT_FMT_DEVICE, flags & IMT_FMT_MASK, c->d_err);
    if (dev) return IMT_OK;
    IMT_HIP(c, hipMemcpyAsync(root, d, 32, hipMemcpyDeviceToHost, c->stream));
    IMT_HIP(c, hipStreamSynchronize(c->stream));
    return IMT_OK;
}

extern "C" int imt_itree_view_lookup_batch(imt_itree_view* v, const void* vals, size_t n, uint8_t* status, uint64_t* leaf_index,
                                           unsigned flags) {
    int rc = view_enter(v, flags);
    return rc ? rc : lookup_batch(v->t, view_source(v), vals, n, status, leaf_index, flags);
}

extern "C" int imt_itree_view_get_leaves(imt_itree_view* v, const uint64_t* index, size_t n, void* preimage, unsigned flags) {
    int rc = view_enter(v, flags);
    return rc ? rc : get_leaves(v->t, view_source(v), index, n, preimage, flags);
}

// the refusals of view_enter without its build: the values of the earlier tree are the first rows of d_val as they are
extern "C" int imt_itree_view_get_values(imt_itree_view* v, uint64_t first, size_t n, void* vals, unsigned flags) {
    if (!view_alive(v)) return IMT_ERR_ARG;
    imt_itree* t = v->t;
    int rc = check_view_call(t, flags);
    if (rc) return rc;
    if (t->size < v->size)
        return t->ctx->fail(IMT_ERR_RANGE, "the tree holds %llu leaves, fewer than the view's %llu", (unsigned long long)t->size,
                            (unsigned long long)v->size);
    return get_values(t, v->size, first, n, vals, flags);
}

extern "C" int imt_itree_view_get_proof_batch(imt_itree_view* v, const uint64_t* index, size_t n, void* sib, unsigned flags) {
    int rc = view_enter(v, flags);
    return rc ? rc : get_proof_batch(v->t, view_source(v), index, n, sib, flags);
}

extern "C" int imt_itree_view_non_membership_witness(imt_itree_view* v, const void* vals, size_t n, uint64_t* low_index,
                                                     void* low_leaf, uint8_t* is_largest, void* low_sib, unsigned flags) {
    int rc = view_enter(v, flags);
    return rc ? rc : non_membership_witness(v->t, view_source(v), vals, n, low_index, low_leaf, is_largest, low_sib, flags);
}

// The witnesses of the n insertions that followed the view's size (imt_replay.hpp), behind view_enter and the range
// check: imt_itree_insert_batch's sequence on the context's stream with the view in the tree's place.  The preparation
// runs against the view's index over the values where they are, the tables and versions live in the view's own plan
// set, every base sibling is read as of the view's size, and there is no write-back, no stored root and no commit.
static int view_replay(imt_itree_view* v, size_t n, const imt_insert_out* out, unsigned flags) {
    imt_itree* t = v->t;
    imt_ctx* c = t->ctx;
    const bool dev = flags & IMT_DEVICE_PTRS, item_major = flags & IMT_SIB_ITEM_MAJOR;
    const unsigned fmt = flags & IMT_FMT_MASK;
    const uint64_t S = v->size;
    const size_t E = 2 * n;
    const unsigned L0 = std::min(ceil_log2(S + n), t->depth);       // of the tree the insertions were made into
    int rc;
    if ((rc = view_behind_tree(t))) return rc;
    hipStream_t s = c->stream;
    PlanSet& P = v->plan;
    if (P.cap_events < E || P.cap_levels < t->depth) IMT_HIP(c, hipStreamSynchronize(s));   // an earlier replay may still use it
    if ((rc = plan_reserve(c, P, E, t->depth, t->cap))) return rc;
    const ScratchTrim trim{c, 3, 3};        // the merged index is 4 bytes per leaf of the tree as of size + n: like a build's scratch
    uint32_t* merged = (uint32_t*)c->dev_scratch(3, (size_t)(S + n) * 4);
    if (!merged) return IMT_ERR_HIP;
    // ---- where each requested output is written: the caller's array, or scratch copied back at the end ----
    size_t slot = 4;
    imt_insert_out d = {};
    const size_t sib_bytes = (size_t)t->global_depth * n * 32;
    if (!stage_insert_outputs(c, dev, slot, out, n, sib_bytes, d)) return IMT_ERR_HIP;
    // ---- hash-free part: the values are rows [S, S + n) of d_val, the index is the view's ----
    IMT_HIP(c, hipMemsetAsync(P.ws.err, 0, sizeof(int), s));
    P.ws.part_mod = t->part_mod;
    P.ws.part_res = t->part_res;
    IMT_HIP(c, prep::run(s, P.ws, nullptr, t->d_val, v->d_sorted, merged, (uint32_t)S, (uint32_t)n, t->index_base, P.d_pre,
                         P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][2], P.d_tab[0][3], d.low_index, d.is_largest,
                         (uint8_t*)d.low_leaf, (uint8_t*)d.new_leaf));
    // ---- hashing: the levels below L0 against the view, nothing written back or stored; old_root[0] is the view's root,
    // the other roots are the events' top values ----
    const launch::SibLayout lay = item_major ? launch::SibLayout{1, t->global_depth} : launch::SibLayout{n, 1};
    const view::Side side = v->side();
    WitnessSweep w;
    w.side = &side;
    w.store = false;
    w.view_root = v->d_chain + (size_t)t->depth * 32;
    if ((rc = witness_sweep(t, P, s, E, L0, d, lay, fmt, w))) return rc;
    // ---- outputs ----
    const HostPlan hp;
    if ((rc = deliver_hashfree_outputs(t, s, n, out, d, hp, flags, slot))) return rc;
    if (dev) return IMT_OK;
    if ((rc = deliver_witness_outputs(t, s, n, out, d, item_major, n))) return rc;
    IMT_HIP(c, hipStreamSynchronize(s));
    return IMT_OK;
}

extern "C" int imt_itree_view_insert_witness(imt_itree_view* v, size_t n, const imt_insert_out* out, unsigned flags) {
    if (!view_alive(v)) return IMT_ERR_ARG;
    imt_itree* t = v->t;
    imt_ctx* c = t->ctx;
    if (!out) return c->fail(IMT_ERR_ARG, "null outputs");
    int rc = view_enter(v, flags);
    if (rc) return rc;
    if (n == 0) return IMT_OK;
    if (n > t->size - v->size)
        return c->fail(IMT_ERR_RANGE, "the tree holds %llu leaves: no %zu insertions follow the view's %llu", (unsigned long long)t->size,
                       n, (unsigned long long)v->size);
    if ((rc = check_out_ptrs(c, flags & IMT_DEVICE_PTRS, out))) return rc;
    return view_replay(v, n, out, flags & ~(unsigned)IMT_HOST_PREP);
}

// The witnesses of a mixed block the tree has already applied at the view's size, behind view_enter and the
// argument checks: mixed_core's sequence with view_replay's differences.  Everything runs on the context's stream behind
// the tree, in the view's own plan set; the INSERT values are compared with the rows they went to instead of written
// there, the neighbours are searched in the view's index, the base siblings below L0 are read as of the view's size, and
// there is no write-back, no stored root, no rotation of plan sets and no commit.  A view at the tree's current size has
// no side table: the stored tree is the tree as of that size, the list can hold no INSERT, and the live LEVEL launch reads
// the siblings where they are -- still without the write-back.
static int view_replay_mixed(imt_itree_view* v, const void* vals, const uint8_t* op, size_t n, const imt_insert_out* ins,
                             const imt_read_out* rd, uint64_t* n_inserted, uint64_t* bad_op, unsigned flags) {
    imt_itree* t = v->t;
    imt_ctx* c = t->ctx;
    const bool dev = flags & IMT_DEVICE_PTRS, item_major = flags & IMT_SIB_ITEM_MAJOR;
    const unsigned fmt = flags & IMT_FMT_MASK;
    const uint64_t S = v->size;
    int rc;
    if ((rc = view_behind_tree(t))) return rc;
    hipStream_t s = c->stream;
    PlanSet& P = v->plan;
    if (P.cap_events < 2 * n || P.cap_levels < t->depth) IMT_HIP(c, hipStreamSynchronize(s));   // an earlier replay may still use it
    if ((rc = plan_reserve(c, P, 2 * n, t->depth, t->cap))) return rc;      // 2n events hold any mix

    // ---- ranks, the range, then the checks: nothing of the caller's is written before the list is accepted ----
    size_t slot = 4;
    const uint8_t* d_vals = nullptr;
    uint8_t* up = dev ? nullptr : (uint8_t*)c->dev_scratch(slot++, n * 32);
    if ((rc = stage_canonical(c, s, vals, n, flags, up, P.d_canon, P.ws.err, &d_vals))) return rc;
    const uint8_t* d_op = nullptr;
    if ((rc = stage_ops(c, s, dev, op, n, slot, &d_op))) return rc;
    const prep::MixedWs mx = mixed_scratch(P);
    size_t n_ins = 0;
    if ((rc = mixed_rank_stage(t, P, mx, s, d_op, n, flags, n_ins))) return rc;
    const size_t n_rd = n - n_ins;
    if (n_ins > t->size - S)
        return c->fail(IMT_ERR_RANGE, "the tree holds %llu leaves: no %zu insertions follow the view's %llu", (unsigned long long)t->size,
                       n_ins, (unsigned long long)S);
    const uint32_t* index = v->current ? t->d_sorted[t->sorted_cur] : v->d_sorted;
    P.ws.part_mod = t->part_mod;
    P.ws.part_res = t->part_res;
    IMT_HIP(c, prep::mixed_check_view(s, P.ws, mx, d_vals, d_op, t->d_val, index, (uint32_t)S, (uint32_t)n, (uint32_t)n_ins));
    if ((rc = mixed_check_verdict(t, P, mx, s))) return rc;
    const int perr = *t->h_err_pin;
    if (perr & prep::ERR_NONCANONICAL) return c->fail(IMT_ERR_NONCANONICAL, "a value is not reduced (>= p)");
    if (perr & (prep::ERR_ZERO | prep::ERR_FOREIGN | prep::ERR_DUPLICATE | prep::ERR_MISMATCH | prep::ERR_ABSENT)) {
        const uint32_t bad = *t->h_cnt_pin;
        if (bad_op && bad < n) *bad_op = bad;
        // which of the two it is at that position: an INSERT that matches its row has nothing else wrong with it
        uint32_t is_ins = 0, rank = 0;
        uint8_t given[32], held[32];
        if (bad >= n) return c->fail(IMT_ERR_INTERNAL, "the checks refuse the list (bits %#x) and name no position", perr);
        IMT_HIP(c, hipMemcpyAsync(&is_ins, mx.flag + bad, 4, hipMemcpyDeviceToHost, s));
        IMT_HIP(c, hipMemcpyAsync(&rank, mx.rank + bad, 4, hipMemcpyDeviceToHost, s));
        IMT_HIP(c, hipStreamSynchronize(s));
        if (is_ins) {
            IMT_HIP(c, hipMemcpyAsync(given, d_vals + (size_t)bad * 32, 32, hipMemcpyDeviceToHost, s));
            IMT_HIP(c, hipMemcpyAsync(held, t->d_val + (size_t)(S + rank) * 32, 32, hipMemcpyDeviceToHost, s));
            IMT_HIP(c, hipStreamSynchronize(s));
            if (std::memcmp(given, held, 32) != 0)
                return c->fail(IMT_ERR_VALUE, "operation %u: INSERT %u of the list is not the value stored at leaf %llu", bad, rank,
                               (unsigned long long)(S + rank));
        }
        if (flags & IMT_MEMBER_OPS)
            return c->fail(IMT_ERR_VALUE, "operation %u: refused as of its place in the list (0, stored at the view's size, or "
                           "inserted earlier in the list; a MEMBER: 0, or neither of the two)", bad);
        return c->fail(IMT_ERR_VALUE, "operation %u: refused as of its place in the list (0, stored at the view's size, or inserted "
                       "earlier in the list)", bad);
    }

    // ---- accepted: events, tables, hash-free outputs ----
    const size_t E = n + n_ins;
    const unsigned L0 = std::min(ceil_log2(S + n_ins), t->depth);       // of the tree the block was applied to
    const ScratchTrim trim{c, 3, 3};        // the merged index is computed and dropped: borrowed, like a build's scratch
    uint32_t* merged = (uint32_t*)c->dev_scratch(3, (size_t)(S + n_ins) * 4);
    if (!merged) return IMT_ERR_HIP;
    imt_insert_out d = {};
    imt_read_out r = {};
    if (!mixed_stage_outputs(c, dev, slot, ins, rd, n_ins, n_rd, (size_t)t->depth * n * 32, d, r)) return IMT_ERR_HIP;
    IMT_HIP(c, prep::mixed_events(s, P.ws, mx, t->d_val, index, merged, (uint32_t)S, (uint32_t)n, (uint32_t)n_ins, t->index_base,
                                  P.d_pre, P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][2], P.d_tab[0][3], d.low_index, d.is_largest,
                                  (uint8_t*)d.low_leaf, (uint8_t*)d.new_leaf,
                                  prep::ReadOut{r.low_index, r.is_largest, (uint8_t*)r.low_leaf}));

    // ---- hashing: the levels below L0 against the view -- against the stored tree as it is for a view at its size --
    // and nothing written back or stored.  old_root[0] is the view's root (an INSERT means the view is not at the tree's
    // size: the chain exists); the other roots, a READ's before the first INSERT included, are the events' top values ----
    const launch::SibLayout lay = item_major ? launch::SibLayout{1, t->depth} : launch::SibLayout{n, 1};
    const launch::MixedRoute route{mx.erow, (uint8_t*)r.low_sib};
    const view::Side side = v->side();
    WitnessSweep w;
    w.route = &route;
    w.n_ins = n_ins;
    w.read_root = (uint8_t*)r.root;
    w.side = v->current ? nullptr : &side;
    w.store = false;
    w.view_root = v->d_chain + (size_t)t->depth * 32;
    if ((rc = witness_sweep(t, P, s, E, L0, d, lay, fmt, w))) return rc;
    if (n_inserted) *n_inserted = n_ins;
    return mixed_deliver_outputs(t, s, ins, rd, d, r, n_ins, n_rd, n, flags);
}

extern "C" int imt_itree_view_mixed_witness(imt_itree_view* v, const void* vals, const uint8_t* op, size_t n,
                                            const imt_insert_out* ins, const imt_read_out* rd, uint64_t* n_inserted,
                                            uint64_t* bad_op, unsigned flags) {
    if (!view_alive(v)) return IMT_ERR_ARG;
    imt_itree* t = v->t;
    imt_ctx* c = t->ctx;
    if (n && (!vals || !op)) return c->fail(IMT_ERR_ARG, "null vals / op");
    int rc;
    if ((rc = check_mixed_mode(t, flags, MIXED_REPLAY))) return rc;
    if (n > ((size_t)1 << 30)) return c->fail(IMT_ERR_RANGE, "list too large");
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((rc = check_mixed_ptrs(c, dev, vals, ins, rd)) || (rc = check_host_ops(c, dev, op, n, flags))) return rc;
    if ((rc = view_enter(v, flags))) return rc;
    if (n == 0) {
        if (n_inserted) *n_inserted = 0;
        return IMT_OK;
    }
    return view_replay_mixed(v, vals, op, n, ins, rd, n_inserted, bad_op, flags);
}

// The bulk witness of the n insertions that followed the view's size, behind view_enter and the argument
// checks: imt_itree_insert_bulk's sequence with view_replay's differences.  The rows come from the view's index over the
// values where they are, with no verdict to wait for; the sweep reads its base siblings as of the view's size and writes
// nothing back, so the frontier of slot S is picked up between the level launches (imt_replay.hpp) instead of gathered from
// the stored tree; and the append runs on borrowed scratch through imt_frontier_append_root's builder, whose root is the
// root as of S + n.  No write-back, no stored root, no rotation of plan sets, no commit.
static int view_replay_bulk(imt_itree_view* v, size_t n, const imt_bulk_out* out, unsigned flags) {
    imt_itree* t = v->t;
    imt_ctx* c = t->ctx;
    const bool dev = flags & IMT_DEVICE_PTRS, item_major = flags & IMT_SIB_ITEM_MAJOR;
    const unsigned fmt = flags & IMT_FMT_MASK;
    const uint64_t S = v->size;
    int rc;
    if ((rc = view_behind_tree(t))) return rc;
    hipStream_t s = c->stream;
    PlanSet& P = v->plan;
    if (P.cap_events < 2 * n || P.cap_levels < t->depth) IMT_HIP(c, hipStreamSynchronize(s));   // an earlier replay may still use it
    if ((rc = plan_reserve(c, P, 2 * n, t->depth, t->cap))) return rc;
    const ScratchTrim trim{c, 3, 4};        // the merged index and the append's rows: borrowed, like a build's scratch
    uint32_t* merged = (uint32_t*)c->dev_scratch(3, (size_t)(S + n) * 4);
    if (!merged) return IMT_ERR_HIP;

    // ---- the append's scratch: the level builder's rows, its frontier and path indices, and the frontier as picked up ----
    launch::FrontierArgs a{};
    a.fmt_in = IMT_FMT_DEVICE;
    a.err = c->d_err;
    a.start = S;
    a.n = n;
    a.depth = t->depth;
    a.zero = c->d_zero;
    const size_t rows_bytes = (size_t)launch::frontier_rows(a) * 32, fsib_bytes = ((size_t)t->depth + 1) * 32;
    uint8_t* scr = (uint8_t*)c->dev_scratch(4, rows_bytes + 2 * fsib_bytes + 16);
    if (!scr) return IMT_ERR_HIP;
    uint8_t* frontier = scr;
    a.sib = frontier;
    a.fsib = scr + fsib_bytes;
    a.idx = (uint64_t*)(scr + 2 * fsib_bytes);
    a.rows = scr + 2 * fsib_bytes + 16;

    // ---- rows, events, tables, hash-free outputs: the batch sorted and its gaps against the view's index, then bulk_row ----
    size_t slot = 5;
    BulkDev d;
    if (!bulk_stage_outputs(c, dev, slot, out, n, t->depth, d)) return IMT_ERR_HIP;
    P.ws.part_mod = t->part_mod;
    P.ws.part_res = t->part_res;
    uint32_t* erow = P.d_slot;
    IMT_HIP(c, prep::bulk_check(s, P.ws, nullptr, t->d_val, v->d_sorted, (uint32_t)S, (uint32_t)n));
    IMT_HIP(c, prep::bulk_events(s, P.ws, t->d_val, v->d_sorted, merged, (uint32_t)S, (uint32_t)n, P.d_pre, P.d_tab[0][0],
                                 P.d_tab[0][1], P.d_tab[0][2], P.d_tab[0][3], erow, d.hashfree));

    // ---- the sweep over the levels the S leaves occupy, against the view, nothing written back or stored; the frontier
    // starts as the view's and takes the final version of every node an event rewrote ----
    const bool want_frontier = d.append_sib || d.root;
    const launch::SibLayout lay = item_major ? launch::SibLayout{1, t->depth} : launch::SibLayout{n, 1};
    const launch::MixedRoute route{erow, nullptr};
    const view::Side side = v->side();
    WitnessSweep w;
    w.route = &route;
    w.bulk = true;
    w.side = &side;
    w.store = false;
    w.view_root = v->d_chain + (size_t)t->depth * 32;
    if (want_frontier) {
        launch::bulk_frontier_base(s, side, launch::TreeView{t->d_nodes, t->d_off, t->d_len, c->d_zero}, t->depth, frontier);
        w.frontier = frontier;
        w.frontier_size = S;
    }
    const unsigned L0_stored = std::min(ceil_log2(S), t->depth);
    if ((rc = witness_sweep(t, P, s, n, L0_stored, d.sweep, lay, fmt, w))) return rc;

    // ---- frontier and append ----
    if (d.append_sib) launch::convert(s, frontier, d.append_sib, t->depth, IMT_FMT_DEVICE, fmt, c->d_err);
    if (d.root)
        launch::frontier_append(s, a, P.d_pre + n * 96, true, IMT_FMT_CANONICAL, nullptr, d.root, fmt, c->coop_max_events);
    return bulk_deliver_outputs(t, s, out, d, n, flags, false);
}

extern "C" int imt_itree_view_bulk_witness(imt_itree_view* v, size_t n, const imt_bulk_out* out, unsigned flags) {
    if (!view_alive(v)) return IMT_ERR_ARG;
    imt_itree* t = v->t;
    imt_ctx* c = t->ctx;
    if (!out) return c->fail(IMT_ERR_ARG, "null outputs");
    int rc;
    if ((rc = check_mixed_mode(t, flags & ~(unsigned)(IMT_HOST_PREP | IMT_INPUTS_READY), BULK_BATCH))) return rc;
    if ((rc = view_enter(v, flags))) return rc;
    if (n == 0) return IMT_OK;
    if (n > t->size - v->size)
        return c->fail(IMT_ERR_RANGE, "the tree holds %llu leaves: no %zu insertions follow the view's %llu", (unsigned long long)t->size,
                       n, (unsigned long long)v->size);
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((rc = check_fe_ptrs(c, dev, {out->low_leaf, out->root_before, out->root_after, out->low_sib, out->new_leaf, out->append_sib,
                                     out->root})))
        return rc;
    if (dev && (((uintptr_t)out->order | (uintptr_t)out->low_index) & 7u))
        return c->fail(IMT_ERR_ARG, "device order / low_index array is not 8-byte aligned");
    return view_replay_bulk(v, n, out, flags & ~(unsigned)(IMT_HOST_PREP | IMT_INPUTS_READY));
}

extern "C" int imt_itree_view_stats(imt_itree_view* v, uint64_t* hashes, uint64_t* builds) {
    if (!view_alive(v)) return IMT_ERR_ARG;
    if (hashes) std::memcpy(hashes, v->h_hashes, (v->t->depth + 1) * 8);
    if (builds) *builds = v->builds;
    return IMT_OK;
}

// ------------------------------------------------------------------------------------
// e: one tree on several GPUs, sequential semantics (imt_itree_batch_*)
// ------------------------------------------------------------------------------------
extern "C" int imt_itree_batch_begin(imt_itree* t, const void* vals, size_t n, unsigned flags, uint32_t* events_out,
                                     uint32_t* l0_out) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    IMT_NOT_SLICED(t);
    if (!vals || n == 0) return c->fail(IMT_ERR_ARG, "null / empty batch");
    if (t->pending.active) return c->fail(IMT_ERR_ARG, "a sharded batch is already open");
    int rc = check_batch_call(t, n, flags);
    if (rc) return rc;
    const uint64_t M = t->size;
    if ((rc = check_room(t, n))) return rc;
    if ((rc = join_top(t))) return rc;
    if ((rc = ensure_device_index(t))) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    if ((rc = check_fe_ptrs(c, dev, {vals}))) return rc;
    const unsigned fmt = flags & IMT_FMT_MASK;
    const size_t E = 2 * n;
    const unsigned L0 = std::min(ceil_log2(M + n), t->depth);
    PlanSet& P = t->plan[t->cur];
    double waited_ms = 0;       // no profile counts a sharded batch's host time
    if ((rc = acquire_plan(t, E, 0, waited_ms))) return rc;
    hipStream_t s = c->stream;
    // context scratch is safe here, unlike in gpu_prepare: everything runs on the context's own stream, behind
    // whatever used those slots last
    size_t slot = 2;
    const uint8_t* d_vals = nullptr;
    uint8_t* up = dev ? nullptr : (uint8_t*)c->dev_scratch(slot++, n * 32);
    uint8_t* can = fmt == IMT_FMT_CANONICAL ? nullptr : (uint8_t*)c->dev_scratch(slot++, n * 32);
    if ((rc = stage_canonical(c, s, vals, n, flags, up, can, P.ws.err, &d_vals))) return rc;
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    P.ws.part_mod = t->part_mod;
    P.ws.part_res = t->part_res;
    IMT_HIP(c, prep::run(s, P.ws, d_vals, t->d_val, t->d_sorted[t->sorted_cur], t->d_sorted[t->sorted_cur ^ 1], (uint32_t)M,
                         (uint32_t)n, t->index_base, P.d_pre, P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][2], P.d_tab[0][3],
                         P.ws.o_low, P.ws.o_largest, P.ws.o_lowleaf, P.ws.o_newleaf));
    IMT_HIP(c, hipMemcpyAsync(t->h_err_pin, P.ws.err, sizeof(int), hipMemcpyDeviceToHost, s));
    IMT_HIP(c, hipStreamSynchronize(s));
    if ((rc = insertion_verdict(t, *t->h_err_pin, "batch"))) return rc;
    // index phase for every level, with the slot of every event per level
    launch::slot0(s, P.d_tab[0][1], P.d_slot, (uint32_t)E);
    index_phase(P, s, E, L0, P.d_slot);
    t->pending.active = true;
    t->pending.n = n;
    t->pending.l0 = L0;
    t->pending.set = t->cur;
    if (events_out) *events_out = (uint32_t)E;
    if (l0_out) *l0_out = L0;
    return IMT_OK;
}

#define IMT_PENDING(t, c)                                                                   \
    if (!(t)) return IMT_ERR_ARG;                                                           \
    imt_ctx* c = (t)->ctx;                                                                  \
    if (!(t)->pending.active) return c->fail(IMT_ERR_ARG, "no sharded batch is open");      \
    { int rc__ = c->set_device(); if (rc__) return rc__; }                                  \
    PlanSet& P = (t)->plan[(t)->pending.set];                                               \
    const size_t E = 2 * (t)->pending.n;                                                    \
    const unsigned L0 = (t)->pending.l0;                                                    \
    (void)E; (void)L0; (void)P

extern "C" int imt_itree_batch_leaves(imt_itree* t, void* val0, uint32_t k_begin, uint32_t k_count) {
    IMT_PENDING(t, c);
    if (!val0 || (size_t)k_begin + k_count > E) return c->fail(IMT_ERR_RANGE, "slot range outside the batch");
    if (int rc = check_fe_ptrs(c, true, {val0})) return rc;
    launch::sweep_leaves(c->stream, P.d_pre, P.d_tab[0][1], (uint8_t*)val0, k_begin, k_count, IMT_FMT_CANONICAL, c->d_err,
                         c->coop_max_events);
    return IMT_OK;
}

extern "C" int imt_itree_batch_level(imt_itree* t, unsigned level, const void* val_in, void* val_out, uint32_t k_begin,
                                     uint32_t k_count) {
    IMT_PENDING(t, c);
    if (level >= L0) return c->fail(IMT_ERR_RANGE, "level %u >= l0 %u", level, L0);
    if (!val_in || !val_out || (size_t)k_begin + k_count > E) return c->fail(IMT_ERR_RANGE, "slot range outside the batch");
    if (int rc = check_fe_ptrs(c, true, {val_in, val_out})) return rc;
    const PlanSet::Level row = P.level(level);
    launch::sweep_level(c->stream, (const uint8_t*)val_in, (uint8_t*)val_out, row.from, row.sibsrc, row.nodeb, row.timen,
                        t->nodes(level), t->h_len[level], c->d_zero + (size_t)level * 32,
                        k_begin, k_count, nullptr, nullptr, launch::SibLayout{0, 0}, level, IMT_FMT_DEVICE,
                        c->coop_max_events);
    return IMT_OK;
}

extern "C" int imt_itree_batch_top(imt_itree* t, const void* val_l0, uint32_t e_begin, uint32_t e_count, void* roots,
                                   void* top_path) {
    IMT_PENDING(t, c);
    if (!val_l0 || !roots || !top_path || (size_t)e_begin + e_count > E)
        return c->fail(IMT_ERR_RANGE, "event range outside the batch");
    if (int rc = check_fe_ptrs(c, true, {val_l0, roots, top_path})) return rc;
    // levels [L0, depth) for this rank's events, ping-ponging through the plan's value scratch; the rank whose range
    // holds the last event fills top_path with that event's node at every level >= L0
    const uint8_t* vin = (const uint8_t*)val_l0;
    uint8_t* tp = (uint8_t*)top_path;
    for (unsigned l = L0; l < t->depth; l++) {
        uint8_t* vout = P.d_val[l & 1];
        launch::sweep_upper(c->stream, vin, vout, c->d_zero + (size_t)l * 32, e_begin, e_count, (uint32_t)E - 1,
                            l == L0 ? tp : nullptr, tp + (size_t)(l + 1 - L0) * 32, nullptr, nullptr,
                            launch::SibLayout{0, 0}, l, IMT_FMT_DEVICE, c->coop_max_events);
        vin = vout;
    }
    launch::emit_roots(c->stream, vin, e_begin, e_count, (uint32_t)E, nullptr, nullptr, nullptr, IMT_FMT_DEVICE,
                       (uint8_t*)roots, L0 == t->depth ? tp : nullptr);
    return IMT_OK;
}

extern "C" int imt_itree_batch_extract(imt_itree* t, const void* const* val_levels, const void* roots, uint32_t ins_begin,
                                       uint32_t ins_count, const imt_insert_out* out, unsigned flags) {
    IMT_PENDING(t, c);
    if (!val_levels || !roots || !out) return c->fail(IMT_ERR_ARG, "null argument");
    if (!(flags & IMT_DEVICE_PTRS)) return c->fail(IMT_ERR_ARG, "imt_itree_batch_extract takes device pointers");
    if ((size_t)ins_begin + ins_count > t->pending.n) return c->fail(IMT_ERR_RANGE, "insertion range outside the batch");
    if (ins_count == 0) return IMT_OK;
    if (int rc = check_fe_ptrs(c, true, {roots})) return rc;
    if (int rc = check_out_ptrs(c, true, out)) return rc;
    for (unsigned l = 0; l <= L0; l++)
        if (int rc = check_fe_ptrs(c, true, {val_levels[l]})) return rc;
    const unsigned fmt = flags & IMT_FMT_MASK;
    hipStream_t s = c->stream;
    IMT_HIP(c, hipMemcpyAsync(P.d_valptr, val_levels, (size_t)(L0 + 1) * sizeof(void*), hipMemcpyHostToDevice, s));
    launch::ExtractParams p{};
    p.val = P.d_valptr;
    p.slot = P.d_slot;
    p.sibsrc = P.d_sibsrc;
    p.node_below = P.d_nodeb;
    p.stride = P.cap_events;
    p.tree_nodes = t->d_nodes;
    p.tree_off = t->d_off;
    p.tree_len = t->d_len;
    p.zero = c->d_zero;
    p.roots = (const uint8_t*)roots;
    p.l0 = L0;
    p.depth = t->depth;
    p.ins_begin = ins_begin;
    p.ins_count = ins_count;
    p.n_total = (uint32_t)t->pending.n;
    p.old_root = (uint8_t*)out->old_root;
    p.interim_root = (uint8_t*)out->interim_root;
    p.new_root = (uint8_t*)out->new_root;
    p.low_sib = (uint8_t*)out->low_sib;
    p.new_sib = (uint8_t*)out->new_sib;
    p.lay = (flags & IMT_SIB_ITEM_MAJOR) ? launch::SibLayout{1, t->global_depth} : launch::SibLayout{ins_count, 1};
    p.fmt_out = fmt;
    launch::extract(s, p);
    if (out->low_index)
        IMT_HIP(c, hipMemcpyAsync(out->low_index, P.ws.o_low + ins_begin, (size_t)ins_count * 8, hipMemcpyDeviceToDevice, s));
    if (out->is_largest)
        IMT_HIP(c, hipMemcpyAsync(out->is_largest, P.ws.o_largest + ins_begin, ins_count, hipMemcpyDeviceToDevice, s));
    if (out->low_leaf)
        launch::convert(s, P.ws.o_lowleaf + (size_t)ins_begin * 96, (uint8_t*)out->low_leaf, (size_t)ins_count * 3,
                        IMT_FMT_CANONICAL, fmt, c->d_err);
    if (out->new_leaf)
        launch::convert(s, P.ws.o_newleaf + (size_t)ins_begin * 96, (uint8_t*)out->new_leaf, (size_t)ins_count * 3,
                        IMT_FMT_CANONICAL, fmt, c->d_err);
    return IMT_OK;
}

extern "C" int imt_itree_batch_abort(imt_itree* t) {
    if (!t) return IMT_ERR_ARG;
    // nothing of an open batch has touched the stored tree, the committed index or the size: rows
    // [size, size + n) of the value array and the spare sorted index are simply overwritten next time
    t->pending.active = false;
    return IMT_OK;
}

extern "C" int imt_itree_batch_end(imt_itree* t, const void* const* val_levels, const void* top_path) {
    IMT_PENDING(t, c);
    if (!val_levels || !top_path) return c->fail(IMT_ERR_ARG, "null argument");
    if (int rc = check_fe_ptrs(c, true, {top_path})) return rc;
    for (unsigned l = 0; l < L0; l++)
        if (int rc = check_fe_ptrs(c, true, {val_levels[l]})) return rc;
    hipStream_t s = c->stream;
    for (unsigned l = 0; l < L0; l++)
        launch::writeback(s, (const uint8_t*)val_levels[l], P.level(l).from, P.level(l).nodeb, t->nodes(l), (uint32_t)E);
    launch::store_top_path(s, (const uint8_t*)top_path, t->d_nodes, t->d_off, L0, t->depth);
    IMT_HIP(c, hipMemcpyAsync(P.d_root, t->nodes(t->depth), 32, hipMemcpyDeviceToDevice, s));
    P.has_root = true;
    P.reads_only = false;
    IMT_HIP(c, hipEventRecord(P.done, s));
    P.in_flight = true;
    P.pipelined = false;
    P.l0 = L0;
    t->sorted_cur ^= 1;
    t->size += t->pending.n;
    t->mirror_valid = false;
    t->cur = (t->cur + 1) % imt_itree::NSETS;
    t->batch_no++;
    t->pending.active = false;
    t->gen++;
    return IMT_OK;
}

// ------------------------------------------------------------------------------------
// e: one tree on several GPUs, sequential semantics, time-sliced (imt_itree_slice_*)
// ------------------------------------------------------------------------------------
// A step's insertions are cut into consecutive slices, one per GPU.  A slice is an ordinary batch for the GPU that
// hashes it -- same plan, same kernels, same 2 + 2 * depth hashes per insertion, proofs and roots written directly --
// except that its level sweeps are issued one UNIT at a time on the caller's stream, so that between units the caller
// can exchange with the other GPUs what each unit wrote back to the stored tree (the "payload" of a unit) and apply
// theirs (imt_itree_slice_apply).  Unit 0 = the leaf hashes, unit 1 + l = level l -> l + 1.  A slice's level l may run
// once every earlier slice's level l has been applied here, and nothing later: the caller's schedule (sharded.py,
// SlicedIndexedTree) guarantees both.  The values other GPUs hash only enter this replica's index (sort + merge, no
// events, no hashing).
namespace {
constexpr size_t SLICE_HDR = 128;      // payload header: node at l0 (32 B), node above (32 B), root (32 B), count (4 B), pad
constexpr size_t SLICE_COUNT_AT = 96;

// (node, value) pairs a slice of n insertions into a tree of size_before leaves can write back at level l: one per
// event at most, and no more than the level has nodes under the leaves in use
inline size_t slice_pairs(uint64_t size_before, size_t n, unsigned l) {
    const uint64_t nodes = l < 63 ? ((size_before + n - 1) >> l) + 1 : 1;
    return (size_t)std::min<uint64_t>(2 * (uint64_t)n, nodes);
}
// bytes of the payload of unit 1 + l: header, values, node ids, rounded to 16
inline size_t slice_unit_bytes(uint64_t size_before, size_t n, unsigned unit, unsigned depth) {
    if (unit == 0) return SLICE_HDR;
    const unsigned l = unit - 1;
    const unsigned L0 = std::min(ceil_log2(size_before + n), depth);
    if (l >= L0) return SLICE_HDR;
    return (SLICE_HDR + 36 * slice_pairs(size_before, n, l) + 15) & ~(size_t)15;
}

int fws_reserve(imt_itree* t, size_t n) {
    imt_ctx* c = t->ctx;
    prep::Workspace& w = t->fws;
    const size_t tmp_need = prep::temp_bytes_needed(n, t->cap);
    if (w.cap_n >= n && w.tmp_bytes >= tmp_need) return IMT_OK;
    IMT_HIP(c, hipStreamSynchronize(t->up_stream));
    for (void* q : {(void*)w.iota, (void*)w.bsorted, (void*)w.gap, (void*)w.st, w.tmp})
        if (q) hipFree(q);
    w = prep::Workspace();
    const size_t N = n + n / 4;
    hipError_t e = hipSuccess;
    auto A = [&](void** ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(ptr, bytes);
    };
    A((void**)&w.iota, N * 4);
    A((void**)&w.bsorted, N * 4);
    A((void**)&w.gap, N * 4);
    A((void**)&w.st, N * 4);
    w.tmp_bytes = prep::temp_bytes_needed(N, t->cap);
    A(&w.tmp, w.tmp_bytes);
    if (e != hipSuccess) {
        for (void* q : {(void*)w.iota, (void*)w.bsorted, (void*)w.gap, (void*)w.st, w.tmp})
            if (q) hipFree(q);
        w = prep::Workspace();
        return c->hip_fail(e, "hipMalloc(slice index workspace)");
    }
    w.cap_n = N;
    return IMT_OK;
}
}  // namespace

extern "C" size_t imt_itree_slice_payload_bytes(size_t n) { return (SLICE_HDR + 72 * n + 15) & ~(size_t)15; }

extern "C" size_t imt_itree_slice_unit_bytes(const imt_itree* t, uint64_t size_before, size_t n, unsigned unit) {
    if (!t || n == 0 || unit > t->depth) return 0;
    return slice_unit_bytes(size_before, n, unit, t->depth);
}

extern "C" int imt_itree_slice_prepare(imt_itree* t, const void* vals, size_t n_before, size_t n_own, size_t n_after,
                                       const imt_insert_out* out, unsigned flags, int* slice_out, uint32_t* l0_out) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    if (!vals || n_own == 0 || !slice_out) return c->fail(IMT_ERR_ARG, "null / empty slice");
    if (!(flags & IMT_DEVICE_PTRS)) return c->fail(IMT_ERR_ARG, "imt_itree_slice_prepare takes device pointers");
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (t->index_base || t->part_mod > 1) return c->fail(IMT_ERR_ARG, "a placed / partitioned tree is not sliced");
    if (t->pending.active) return c->fail(IMT_ERR_ARG, "a sharded batch is open (imt_itree_batch_end first)");
    const size_t n_all = n_before + n_own + n_after;
    if (n_all > ((size_t)1 << 30)) return c->fail(IMT_ERR_RANGE, "step too large");
    const uint64_t M0 = t->size;
    int rc = check_room(t, n_all);
    if (rc) return rc;
    if ((rc = c->set_device())) return rc;
    if ((rc = ensure_device_index(t))) return rc;
    if ((rc = check_fe_ptrs(c, true, {vals})) || (rc = check_out_ptrs(c, true, out))) return rc;
    const unsigned fmt = flags & IMT_FMT_MASK;
    const int set = t->cur;
    PlanSet& P = t->plan[set];
    if (P.open) return c->fail(IMT_ERR_ARG, "too many slices prepared ahead (%d plan sets)", imt_itree::NSETS);
    double waited_ms = 0;
    rc = acquire_plan(t, 2 * n_own, t->slice_wait_limit_ms, waited_ms);
    t->slice_wait_ms += waited_ms;
    t->slice_backpressure_ms += waited_ms;
    if (rc) return rc;
    if ((rc = reserve_all_plans(t, 2 * n_own))) return rc;
    if (n_before || n_after)
        if ((rc = fws_reserve(t, std::max(n_before, n_after)))) return rc;
    // The side stream, or a stream the sliced schedule names (imt_itree_set_slice_prep_stream: the NEW round's own stream,
    // whose hardware queue is idle -- the side stream shares one with some round's stream, and a hardware queue runs what
    // it holds in submission order: the preparation then stood behind a whole period of that round's hash kernels and the
    // host's wait for the verdict lasted until the GPU had run dry).  Preparations of consecutive steps are ordered by the
    // host: each is waited for (the verdict) before the call returns.
    hipStream_t ps = t->slice_prep_stream ? t->slice_prep_stream : t->up_stream;
    if (t->slice_prep_stream) IMT_HIP(c, hipStreamSynchronize(t->up_stream));      // whatever an earlier call left there
    if ((rc = order_behind_caller(t, ps, flags))) return rc;
    // the whole step's values go through a buffer of the tree's own: the plan set's holds one slice, and context scratch
    // is not safe on this stream (see gpu_prepare)
    if (fmt != IMT_FMT_CANONICAL && t->canon_all_cap < n_all * 32) {
        IMT_HIP(c, hipStreamSynchronize(ps));
        if (t->d_canon_all) hipFree(t->d_canon_all);
        t->d_canon_all = nullptr;
        t->canon_all_cap = 0;
        IMT_HIP(c, hipMalloc((void**)&t->d_canon_all, n_all * 40));
        t->canon_all_cap = n_all * 40;
    }
    const uint8_t* d_vals = nullptr;
    if ((rc = stage_canonical(c, ps, vals, n_all, flags, nullptr, t->d_canon_all, P.ws.err, &d_vals))) return rc;
    // ---- the index, in the order of the step: the slices before this one, this one (with its events), those after.
    // Up to three merges, none of which may write the committed index (a refused step leaves the tree as it was): they
    // go committed -> ... -> spare, through a third buffer when there are two or three of them.
    if (!t->d_sorted_extra) IMT_HIP(c, hipMalloc((void**)&t->d_sorted_extra, t->cap * 4));
    const int n_merges = 1 + (n_before ? 1 : 0) + (n_after ? 1 : 0);
    uint32_t* const committed = t->d_sorted[t->sorted_cur];
    uint32_t* const spare = t->d_sorted[t->sorted_cur ^ 1];
    uint32_t* chain[4] = {committed, spare, spare, spare};
    if (n_merges == 2) chain[1] = t->d_sorted_extra;
    if (n_merges == 3) chain[2] = t->d_sorted_extra;
    int link = 0;
    uint64_t M = M0;
    t->fws.err = P.ws.err;
    t->fws.part_mod = t->fws.part_res = 0;
    P.ws.part_mod = P.ws.part_res = 0;
    if (n_before) {
        IMT_HIP(c, prep::index_only(ps, t->fws, d_vals, t->d_val, chain[link], chain[link + 1], (uint32_t)M,
                                    (uint32_t)n_before));
        link++;
        M += n_before;
    }
    const uint64_t M_own = M;
    IMT_HIP(c, prep::run(ps, P.ws, d_vals + n_before * 32, t->d_val, chain[link], chain[link + 1], (uint32_t)M,
                         (uint32_t)n_own, 0, P.d_pre, P.d_tab[0][0], P.d_tab[0][1], P.d_tab[0][2], P.d_tab[0][3],
                         out ? out->low_index : nullptr, out ? out->is_largest : nullptr,
                         out ? (uint8_t*)out->low_leaf : nullptr, out ? (uint8_t*)out->new_leaf : nullptr));
    link++;
    M += n_own;
    if (n_after) {
        IMT_HIP(c, prep::index_only(ps, t->fws, d_vals + (n_before + n_own) * 32, t->d_val, chain[link], chain[link + 1],
                                    (uint32_t)M, (uint32_t)n_after));
        link++;
    }
    IMT_HIP(c, hipMemcpyAsync(t->h_err_pin, P.ws.err, sizeof(int), hipMemcpyDeviceToHost, ps));
    // ---- this slice's index phase (no hashing) on the side stream as well ----
    const size_t E = 2 * n_own;
    const unsigned L0 = std::min(ceil_log2(M_own + n_own), t->depth);
    index_phase(P, ps, E, L0, nullptr);
    if (out && fmt != IMT_FMT_CANONICAL) {
        if (out->low_leaf) launch::convert(ps, (uint8_t*)out->low_leaf, (uint8_t*)out->low_leaf, n_own * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
        if (out->new_leaf) launch::convert(ps, (uint8_t*)out->new_leaf, (uint8_t*)out->new_leaf, n_own * 3, IMT_FMT_CANONICAL, fmt, c->d_err);
    }
    // The slice's units run on streams the caller names and read / write the stored levels: they must come behind
    // every ORDINARY batch still in flight on this tree (pipelined or on the context's stream), whose sweeps write the
    // same levels.  Unit 0 waits for prep_done, so ordering the side stream behind those batches orders the units.
    // Earlier slices are not waited for here: the sliced schedule orders slices among themselves level by level.
    for (auto& pl : t->plan)
        if (&pl != &P && pl.in_flight && !pl.sliced) IMT_HIP(c, hipStreamWaitEvent(ps, pl.done, 0));
    IMT_HIP(c, hipEventRecord(P.prep_done, ps));
    {
        const HostTimer w;
        rc = bounded_wait(c, t->slice_wait_limit_ms, [&] { return hipStreamQuery(ps); }, [&] { return hipStreamSynchronize(ps); },
                          "the step's preparation (its value check)");
        t->slice_wait_ms += w.ms();
        if (rc) return rc;
    }
    // the same verdict on every GPU: they all see all values of the step (none is foreign: a sliced tree has no partition)
    if ((rc = insertion_verdict(t, *t->h_err_pin, "step"))) return rc;
    // ---- commit the index; the hashing follows unit by unit ----
    t->sorted_cur ^= 1;          // chain[n_merges] == spare
    t->size = M0 + n_all;
    t->mirror_valid = false;
    t->gen++;
    P.open = true;
    P.sliced = true;
    P.slice_n = n_own;
    P.slice_out = out ? *out : imt_insert_out{};
    P.slice_fmt = fmt;
    P.slice_next_unit = 0;
    P.slice_size_before = M_own;
    P.slice_lay = (flags & IMT_SIB_ITEM_MAJOR) ? launch::SibLayout{1, t->depth} : launch::SibLayout{n_own, 1};
    P.l0 = L0;
    P.has_root = false;
    P.reads_only = false;
    t->cur = (t->cur + 1) % imt_itree::NSETS;
    t->batch_no++;
    *slice_out = set;
    if (l0_out) *l0_out = L0;
    return IMT_OK;
}

extern "C" int imt_itree_slice_unit(imt_itree* t, int slice, unsigned unit, void* payload, void* hip_stream) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    if (slice < 0 || slice >= imt_itree::NSETS || !t->plan[slice].open) return c->fail(IMT_ERR_ARG, "no such open slice");
    PlanSet& P = t->plan[slice];
    if (unit != P.slice_next_unit) return c->fail(IMT_ERR_ARG, "slice unit %u out of order (next is %u)", unit, P.slice_next_unit);
    int rc = c->set_device();
    if (rc) return rc;
    if ((rc = check_fe_ptrs(c, true, {payload}))) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const size_t n = P.slice_n, E = 2 * n;
    const unsigned L0 = P.l0, depth = t->depth, fmt = P.slice_fmt;
    const imt_insert_out& o = P.slice_out;
    uint8_t* pl = (uint8_t*)payload;
    P.slice_next_unit = unit + 1;
    if (unit == 0) {
        IMT_HIP(c, hipStreamWaitEvent(s, P.prep_done, 0));
        sweep_leaf_hashes(t, P, s, E);
        return IMT_OK;
    }
    const unsigned l = unit - 1;
    if (l < L0) {
        sweep_one_level(t, P, s, l, E, o, P.slice_lay, fmt);
        const PlanSet::Level row = P.level(l);
        const uint8_t* vin = P.d_val[l & 1];
        const int pf = c->prof_begin(IMT_PROF_WRITEBACK, s);
        if (pl) {       // the write-back, and what the other replicas need to repeat it: (node, value) pairs, packed
            const size_t cap = slice_pairs(P.slice_size_before, n, l);
            IMT_HIP(c, hipMemsetAsync(pl + SLICE_COUNT_AT, 0, 4, s));
            // the pack is the last kernel of this unit (unless it is the round's last, or a profile brackets it): it can
            // signal the tick's event itself
            hipEvent_t tail = (l + 1 != depth && pf < 0) ? t->slice_tail_event : nullptr;
            launch::pack_writeback(s, vin, row.from, row.nodeb, (uint32_t)E, t->nodes(l), pl + SLICE_HDR,
                                   (uint32_t*)(pl + SLICE_HDR + cap * 32), (uint32_t*)(pl + SLICE_COUNT_AT), (uint32_t)cap, tail);
            if (tail) t->slice_tail_attached = true;
        } else {
            launch::writeback(s, vin, row.from, row.nodeb, t->nodes(l), (uint32_t)E);
        }
        c->prof_end(pf, s);
    } else {
        if (l + 1 == depth) read_old_root(t, s, o, fmt);
        sweep_one_upper(t, P, s, l, E, L0, o, P.slice_lay, fmt);
        if (pl) {       // the two nodes the launch stored: the one at L0 (its own input), the one above
            if (l == L0) IMT_HIP(c, hipMemcpyAsync(pl, t->nodes(l), 32, hipMemcpyDeviceToDevice, s));
            IMT_HIP(c, hipMemcpyAsync(pl + 32, t->nodes(l + 1), 32, hipMemcpyDeviceToDevice, s));
        }
    }
    if (l + 1 == depth) {       // the last unit: roots of every event, the batch's root, done
        if (L0 == depth) read_old_root(t, s, o, fmt);
        finish_roots(t, P, s, E, L0, o, fmt);
        if (pl && L0 == depth) IMT_HIP(c, hipMemcpyAsync(pl + 64, t->nodes(depth), 32, hipMemcpyDeviceToDevice, s));
        P.has_root = false;         // the root after THIS slice is a mid-step root on every rank but the last: not offered
        IMT_HIP(c, hipEventRecord(P.done, s));
        P.in_flight = true;
        P.pipelined = true;         // not on the context's stream: join_top orders that stream behind it
        P.applied = false;
        P.l0 = 0;                   // no per-level events were recorded: a pipelined batch that follows waits for `done`
        t->pipe_pending = true;
        P.open = false;
    }
    return IMT_OK;
}

extern "C" int imt_itree_slice_apply(imt_itree* t, uint64_t size_before, size_t n, unsigned unit, const void* payload,
                                     void* hip_stream) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    if (!payload || n == 0) return c->fail(IMT_ERR_ARG, "null / empty payload");
    if (unit > t->depth) return c->fail(IMT_ERR_RANGE, "unit %u beyond depth %u", unit, t->depth);
    if (size_before + n > t->cap) return c->fail(IMT_ERR_RANGE, "slice outside the tree's capacity");
    if (unit == 0) return IMT_OK;          // leaf hashes: nothing is stored yet
    int rc = c->set_device();
    if (rc) return rc;
    if ((rc = check_fe_ptrs(c, true, {payload}))) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const unsigned depth = t->depth, l = unit - 1;
    const unsigned L0 = std::min(ceil_log2(size_before + n), depth);
    const uint8_t* pl = (const uint8_t*)payload;
    if (l < L0) {
        const size_t cap = slice_pairs(size_before, n, l);
        launch::apply_packed(s, pl + SLICE_HDR, (const uint32_t*)(pl + SLICE_HDR + cap * 32), (const uint32_t*)(pl + SLICE_COUNT_AT),
                             (uint32_t)cap, t->nodes(l), t->h_len[l]);
    } else {
        if (l == L0) IMT_HIP(c, hipMemcpyAsync(t->nodes(l), pl, 32, hipMemcpyDeviceToDevice, s));
        IMT_HIP(c, hipMemcpyAsync(t->nodes(l + 1), pl + 32, 32, hipMemcpyDeviceToDevice, s));
    }
    if (l + 1 == depth && L0 == depth)
        IMT_HIP(c, hipMemcpyAsync(t->nodes(depth), pl + 64, 32, hipMemcpyDeviceToDevice, s));
    return IMT_OK;
}

extern "C" int imt_itree_slice_apply_gathered(imt_itree* t, const void* gathered, size_t stride, size_t count,
                                              const uint64_t* size_before, const uint64_t* n, const int32_t* unit,
                                              void* hip_stream) {
    if (!t) return IMT_ERR_ARG;
    if (!gathered || !size_before || !n || !unit) return t->ctx->fail(IMT_ERR_ARG, "null argument");
    imt_ctx* c = t->ctx;
    int rc = c->set_device();
    if (rc) return rc;
    if ((rc = check_fe_ptrs(c, true, {gathered})) || (stride & 15u))
        return rc ? rc : c->fail(IMT_ERR_ARG, "payload stride must be a multiple of 16 bytes");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const unsigned depth = t->depth;
    launch::ApplyJobs jobs{};
    jobs.poison = t->slice_poison;
    for (size_t r = 0; r < count; r++) {
        if (unit[r] < 0) continue;
        if ((unsigned)unit[r] > depth) return c->fail(IMT_ERR_RANGE, "unit %d beyond depth %u", unit[r], depth);
        if (n[r] == 0 || size_before[r] + n[r] > t->cap) return c->fail(IMT_ERR_RANGE, "slice outside the tree's capacity");
        if (unit[r] == 0) continue;
        // the kernel reads the counter and the node ids at offsets computed from (size_before, n, unit): a payload
        // slot shorter than that would make it read the neighbouring payload
        if (count > 1 && stride < slice_unit_bytes(size_before[r], (size_t)n[r], (unsigned)unit[r], depth))
            return c->fail(IMT_ERR_ARG, "payload stride %zu is smaller than the %zu bytes unit %d of slot %zu uses", stride,
                           slice_unit_bytes(size_before[r], (size_t)n[r], (unsigned)unit[r], depth), unit[r], r);
        const unsigned l = (unsigned)unit[r] - 1;
        const unsigned L0 = std::min(ceil_log2(size_before[r] + n[r]), depth);
        launch::ApplyJobs::Job& j = jobs.j[jobs.n_jobs++];
        j = launch::ApplyJobs::Job{};
        j.payload = (const uint8_t*)gathered + r * stride;
        if (l < L0) {
            j.pairs = 1;
            j.cap = (uint32_t)slice_pairs(size_before[r], (size_t)n[r], l);
            j.tree_l = t->nodes(l);
            j.len_l = t->h_len[l];
        } else {
            if (l == L0) j.node_in = t->nodes(l);
            j.node_out = t->nodes(l + 1);
        }
        if (l + 1 == depth && L0 == depth) {
            if (j.pairs) {      // pairs and the root from one payload: the root goes as a job of its own
                if (jobs.n_jobs == 16) { launch::apply_gathered(s, jobs); jobs.n_jobs = 0; }
                launch::ApplyJobs::Job& k = jobs.j[jobs.n_jobs++];
                k = launch::ApplyJobs::Job{};
                k.payload = (const uint8_t*)gathered + r * stride;
                k.root = t->nodes(depth);
            } else {
                j.root = t->nodes(depth);
            }
        }
        if (jobs.n_jobs >= 15) { launch::apply_gathered(s, jobs); jobs.n_jobs = 0; }
    }
    if (jobs.n_jobs && t->slice_tail_event) {
        launch::apply_gathered(s, jobs, t->slice_tail_event);
        t->slice_tail_attached = true;
    } else {
        launch::apply_gathered(s, jobs);
    }
    return IMT_OK;
}

// ------------------------------------------------------------------------------------
// e: the tree as one subtree of a deeper tree (leaf-index-range sharding)
// ------------------------------------------------------------------------------------
extern "C" int imt_itree_set_placement(imt_itree* t, unsigned global_depth, uint64_t subtree_index) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    if (t->size != 1 || t->batch_no != 0) return c->fail(IMT_ERR_ARG, "placement must be set on an empty tree");
    if (global_depth < t->depth || global_depth > IMT_MAX_DEPTH)
        return c->fail(IMT_ERR_RANGE, "global depth %u outside [%u, %d]", global_depth, t->depth, IMT_MAX_DEPTH);
    const unsigned up = global_depth - t->depth;
    if (up < 64 && (subtree_index >> up) != 0) return c->fail(IMT_ERR_RANGE, "subtree index does not fit the global tree");
    if (global_depth > 63 && subtree_index != 0) return c->fail(IMT_ERR_RANGE, "leaf indices must fit 64 bits");
    t->global_depth = global_depth;
    t->sub_index = subtree_index;
    t->index_base = t->depth < 64 ? subtree_index << t->depth : 0;
    return IMT_OK;
}

extern "C" int imt_itree_set_value_partition(imt_itree* t, uint32_t modulus, uint32_t residue) {
    if (!t) return IMT_ERR_ARG;
    if (modulus > 1 && residue >= modulus) return t->ctx->fail(IMT_ERR_ARG, "residue %u >= modulus %u", residue, modulus);
    t->part_mod = modulus;
    t->part_res = residue;
    return IMT_OK;
}

extern "C" int imt_itree_lift_batch(imt_itree* t, const void* roots_before, const void* roots_after, size_t n_subtrees,
                                    size_t n, const imt_insert_out* out, unsigned flags) {
    if (!t) return IMT_ERR_ARG;
    imt_ctx* c = t->ctx;
    if (!out) return c->fail(IMT_ERR_ARG, "null outputs");
    if ((flags & IMT_FMT_MASK) == 3) return c->fail(IMT_ERR_ARG, "unknown field-element format");
    if (n_subtrees == 0 || (n_subtrees & (n_subtrees - 1)) || n_subtrees > 65536)
        return c->fail(IMT_ERR_ARG, "n_subtrees must be a power of two (<= 65536)");
    unsigned k = 0;
    while (((size_t)1 << k) < n_subtrees) k++;
    const unsigned levels = t->global_depth - t->depth;
    if (k > levels) return c->fail(IMT_ERR_RANGE, "depth + log2(n_subtrees) exceeds the global depth");
    if (t->sub_index >= n_subtrees) return c->fail(IMT_ERR_RANGE, "this tree is subtree %llu of %zu",
                                                   (unsigned long long)t->sub_index, n_subtrees);
    if (n_subtrees > 1 && (!roots_before || !roots_after)) return c->fail(IMT_ERR_ARG, "null subtree roots");
    if (n == 0 || levels == 0) return IMT_OK;
    if (n > ((size_t)1 << 30)) return c->fail(IMT_ERR_RANGE, "batch too large");
    int rc = c->set_device();
    if (rc) return rc;
    const bool dev = flags & IMT_DEVICE_PTRS;
    const unsigned fmt = flags & IMT_FMT_MASK;
    hipStream_t s = c->stream;
    if ((rc = check_fe_ptrs(c, dev, {roots_before, roots_after})) || (rc = check_out_ptrs(c, dev, out))) return rc;
    if (!dev && (rc = c->clear_err())) return rc;
    size_t slot = 2;
    auto scratch = [&](size_t bytes) { return (uint8_t*)c->dev_scratch(slot++, bytes); };
    // ---- the `levels` siblings above this subtree's root: constant for the whole batch ----
    uint8_t* tree_buf = scratch(2 * n_subtrees * 32);       // dense tree over the mixed roots
    uint8_t* top = scratch((size_t)levels * 32);            // device format
    if (!tree_buf || !top) return IMT_ERR_HIP;
    if (n_subtrees > 1) {
        const uint8_t *d_b = (const uint8_t*)roots_before, *d_a = (const uint8_t*)roots_after;
        if (!dev) {
            uint8_t* up = scratch(2 * n_subtrees * 32);
            if (!up) return IMT_ERR_HIP;
            IMT_HIP(c, hipMemcpyAsync(up, roots_before, n_subtrees * 32, hipMemcpyHostToDevice, s));
            IMT_HIP(c, hipMemcpyAsync(up + n_subtrees * 32, roots_after, n_subtrees * 32, hipMemcpyHostToDevice, s));
            d_b = up;
            d_a = up + n_subtrees * 32;
        }
        // subtrees left of this one (lower leaf indices) are taken AFTER the step, those right of it BEFORE:
        // within a step the insertions of subtree 0 come first, then subtree 1's, ...
        launch::mix_roots(s, d_b, d_a, tree_buf, (uint32_t)n_subtrees, (uint32_t)t->sub_index, fmt, c->d_err);
        size_t off = 0;
        for (size_t m = n_subtrees; m > 1; m >>= 1) {
            launch::tree_level(s, tree_buf + off * 32, tree_buf + (off + m) * 32, m / 2, c->coop_max_events);
            off += m;
        }
    }
    launch::pick_top(s, tree_buf, (uint32_t)n_subtrees, (uint32_t)t->sub_index, k, levels, c->d_zero, t->depth, top);
    const uint64_t pos_bits = t->sub_index;                 // bit j: the ancestor at height depth + j is a right child
    // ---- roots, in place ----
    uint8_t* d_roots[3] = {(uint8_t*)out->old_root, (uint8_t*)out->interim_root, (uint8_t*)out->new_root};
    void* h_roots[3] = {out->old_root, out->interim_root, out->new_root};
    if (!dev)
        for (int j = 0; j < 3; j++)
            if (h_roots[j]) {
                d_roots[j] = scratch(n * 32);
                if (!d_roots[j]) return IMT_ERR_HIP;
                IMT_HIP(c, hipMemcpyAsync(d_roots[j], h_roots[j], n * 32, hipMemcpyHostToDevice, s));
            }
    launch::lift_roots(s, d_roots[0], d_roots[1], d_roots[2], (uint32_t)n, top, pos_bits, levels, fmt, c->d_err);
    // ---- sibling rows [depth, global_depth) ----
    const bool item_major = flags & IMT_SIB_ITEM_MAJOR;
    launch::SibLayout lay = item_major ? launch::SibLayout{1, t->global_depth} : launch::SibLayout{n, 1};
    if (dev) {
        launch::fill_sib_rows(s, (uint8_t*)out->low_sib, lay, t->depth, levels, (uint32_t)n, top, fmt);
        launch::fill_sib_rows(s, (uint8_t*)out->new_sib, lay, t->depth, levels, (uint32_t)n, top, fmt);
        return IMT_OK;
    }
    for (int j = 0; j < 3; j++)
        if (h_roots[j]) IMT_HIP(c, hipMemcpyAsync(h_roots[j], d_roots[j], n * 32, hipMemcpyDeviceToHost, s));
    std::vector<uint8_t> h_top((size_t)levels * 32);
    if (out->low_sib || out->new_sib) {
        uint8_t* top_fmt = scratch((size_t)levels * 32);
        if (!top_fmt) return IMT_ERR_HIP;
        launch::convert(s, top, top_fmt, levels, IMT_FMT_DEVICE, fmt, c->d_err);
        IMT_HIP(c, hipMemcpyAsync(h_top.data(), top_fmt, (size_t)levels * 32, hipMemcpyDeviceToHost, s));
    }
    if ((rc = c->sync_and_check())) return rc;
    for (void* sibv : {out->low_sib, out->new_sib}) {
        uint8_t* sib = (uint8_t*)sibv;
        if (!sib) continue;
        for (unsigned j = 0; j < levels; j++)
            for (size_t i = 0; i < n; i++)
                std::memcpy(sib + ((uint64_t)(t->depth + j) * lay.level_stride + i * lay.item_stride) * 32,
                            &h_top[(size_t)j * 32], 32);
    }
    return IMT_OK;
}
