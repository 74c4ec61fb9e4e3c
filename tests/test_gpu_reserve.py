"""GPU (MI355X): another capacity for a live tree (imt_itree_reserve / imt_itree_capacity).

The claim under test is an identity: after reserve(C) a tree cannot be told, through any call, from a tree made with
capacity C (same depth, placement, partition) that received the same values in the same order.  Expected values are the
sequential oracle's (tests/insert_corpus.py, oracle.sparse_insert) or such a twin's; every comparison is bit-exact.

  test_reserve_scenarios            every scenario of the corpus from capacity 2, reserving the smallest power of two
                                    that holds size + n before each batch: witness rows and roots against the oracle's
                                    records, the stored tree against a twin made at the scenario's capacity.
  test_reserve_every_pair           depth 5, every ordered pair of capacities 2 .. 32, sizes 1, min - 1, min: every leaf
                                    and proof at every index below the new capacity.
  test_reserved_tree_goes_on        300 values at capacity 512, reserve 2^18, 300 and 5000 more (plan sets reserved under
                                    the small capacity), then every kind of call against the twin.
  test_reserve_with_work_in_flight  four pipelined blocks of the four kinds, reserve with no sync, two more blocks.
  test_reserve_under_views          a view across a grow and a shrink: same answers, no rebuild; root_lagged unchanged.
  test_reserve_shrink_after_rewind  grow, 3000 values, rewind to 100, reserve 128; FULL, then reserve 256 and the batch.
  test_reserve_refusals             every documented refusal leaves size, root, leaves and capacity alone.
  test_sliced_world_goes_on_after_reserve   world 2: steps, flush, both replicas reserved alike, more steps.
  test_reserve_large                2^16 + 3 values across 2^10 -> 2^14 -> 2^17 against a twin of 2^17.
  test_grow_demo_example            examples/grow_demo.c: its final root against the oracle's.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import insert_corpus as ic
import oracle_lib
import test_gpu_insert_matrix as tm  # noqa: F401  (the corpus' conversions; imported as test_gpu_load_values does)
from oracle_lib import P, ints_to_arr
from test_gpu_load_values import P_, new_tree, same_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = ("low_index", "is_largest", "low_leaf", "new_leaf", "old_root", "interim_root", "new_root", "new_index")


def pow2_for(leaves):
    """the smallest capacity imt_itree_new accepts that holds `leaves`"""
    c = 2
    while c < leaves:
        c *= 2
    return c


def every_slot(t, upto=None):
    """(leaves, proofs) at every index below `upto` (default: the capacity), the empty slots included"""
    idx = np.arange(upto if upto is not None else t.capacity, dtype=np.uint64) + np.uint64(t.index_base)
    return t.get_leaves(idx), t.get_proof_batch(idx)


def state(t):
    lv, pr = every_slot(t)
    return t.size, t.root(), t.capacity, lv.tobytes(), pr.tobytes()


def raw_reserve(imt, t, cap, flags=0):
    return imt.lib.imt_itree_reserve(t.h if t is not None else None, cap, flags)


def same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- the corpus
@pytest.mark.parametrize("name", [s.name for s in ic.SCENARIOS])
def test_reserve_scenarios(imt, ctx, name):
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    rec, vals = exp["rec"], ints_to_arr(exp["vals"])
    t = imt.IndexedTree(ctx, sc.depth, 2)
    if sc.placement:
        t.set_placement(*sc.placement)
    twin = new_tree(imt, ctx, sc)
    try:
        assert t.capacity == 2
        for j, (a, b) in enumerate(ic.batch_bounds(sc)):
            want_cap = pow2_for(t.size + (b - a))
            t.reserve(want_cap)
            assert t.capacity == want_cap and t.size == a + 1
            res = t.insert_batch(vals[a:b])
            for k in REC:
                bad = np.nonzero((res[k] != rec[k][a:b]).reshape(b - a, -1).any(axis=1))[0]
                assert bad.size == 0, f"{k}: first differing insertion {a + bad[0]} (batch {j}, capacity {want_cap})"
            for k in ("low_sib", "new_sib"):
                got = res[k][:sc.depth].transpose(1, 0, 2)
                bad = np.argwhere((got != rec[k][a:b]).any(axis=2))
                assert bad.size == 0, f"{k}: insertion {a + bad[0][0]} level {bad[0][1]} (batch {j}, capacity {want_cap})"
            assert t.root() == exp["batch_roots"][j + 1]
        t.reserve(sc.cap)
        assert t.capacity == sc.cap
        twin.apply_batch(vals)
        same_tree(t, twin)
        fin = exp["final"]
        assert (t.get_proof_batch(fin["index"], item_major=True) == fin["proofs"]).all()
        assert (t.get_leaves(fin["index"]) == fin["preimages"]).all()
    finally:
        t.close()
        twin.close()


def test_reserve_every_pair(imt, ctx):
    depth, caps = 5, (2, 4, 8, 16, 32)
    vals = ints_to_arr(oracle_lib.synth_values(31, 0x52535600))
    twins = {}                                            # (capacity, size) -> what a tree made there answers at every slot

    def twin_slots(cap, size):
        if (cap, size) not in twins:
            tw = imt.IndexedTree(ctx, depth, cap)
            if size > 1:
                tw.apply_batch(vals[:size - 1])
            twins[(cap, size)] = (tw.root(),) + every_slot(tw)
            tw.close()
        return twins[(cap, size)]

    for old in caps:
        for new in caps:
            for size in sorted({1, min(old, new) - 1, min(old, new)} - {0}):
                t = imt.IndexedTree(ctx, depth, old)
                try:
                    if size > 1:
                        t.apply_batch(vals[:size - 1])
                    t.reserve(new)
                    assert (t.capacity, t.size) == (new, size)
                    root, leaves, proofs = twin_slots(new, size)
                    got_leaves, got_proofs = every_slot(t)
                    assert t.root() == root, (old, new, size)
                    assert (got_leaves == leaves).all() and (got_proofs == proofs).all(), (old, new, size)
                    if size < new:                        # and it goes on as the twin does
                        assert t.apply_batch(vals[size - 1:size]) == twin_slots(new, size + 1)[0]
                finally:
                    t.close()


# ---------------------------------------------------------------- the reserved tree goes on
def test_reserved_tree_goes_on(imt, ctx):
    import torch
    f = imt._ffi
    depth = 32
    allv = oracle_lib.synth_values(7000, 0x52535601)
    a, b = imt.IndexedTree(ctx, depth, 512), imt.IndexedTree(ctx, depth, 1 << 18)
    try:
        for k in range(0, 300, 60):                # five batches: every plan set of `a` is reserved under capacity 512
            assert a.apply_batch(allv[k:k + 60]) == b.apply_batch(allv[k:k + 60])
        a.reserve(1 << 18)
        assert a.capacity == b.capacity == 1 << 18
        same_tree(a, b)
        # the plan sets keep their 1024 events, so none is reserved anew: their workspaces must fit the larger tree now
        assert a.apply_batch(allv[300:600]) == b.apply_batch(allv[300:600])
        assert a.apply_batch(allv[600:5600]) == b.apply_batch(allv[600:5600])
        same_tree(a, b)
        at = 5600
        for host_prep in (False, True):
            same_dict(a.insert_batch(allv[at:at + 130], host_prep=host_prep), b.insert_batch(allv[at:at + 130], host_prep=host_prep))
            at += 130
        mixed = [0, allv[3], allv[6900], allv[6900], allv[5605], allv[6901], 0, allv[6902]]
        fa, fb = a.insert_filtered(mixed), b.insert_filtered(mixed)
        assert fa["n_inserted"] == fb["n_inserted"] == 3
        same_dict(fa, fb)
        dv = torch.from_numpy(ints_to_arr(allv[at:at + 200])).cuda()
        roots = torch.zeros((2, 32), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        a.apply_pipelined(dv.data_ptr(), 200, roots[0].data_ptr())
        b.apply_pipelined(dv.data_ptr(), 200, roots[1].data_ptr())
        ctx.sync()
        r = roots.cpu().numpy()
        assert (r[0] == r[1]).all() and imt.to_int(r[0]) == a.root() == b.root()
        at += 200
        # INSERT / READ / MEMBER in one block
        blk = [allv[at], allv[6950], allv[10], allv[at + 1], allv[at], allv[6951], allv[at + 2]]
        ops = [f.OP_INSERT, f.OP_READ, f.OP_MEMBER, f.OP_INSERT, f.OP_MEMBER, f.OP_READ, f.OP_INSERT]
        (ia, ra), (ib, rb) = a.mixed_batch(blk, ops, members=True), b.mixed_batch(blk, ops, members=True)
        same_dict(ia, ib)
        same_dict(ra, rb)
        at += 3
        probe = ints_to_arr([allv[0], allv[299], allv[300], allv[at - 1], 0, allv[6990], allv[6991], P - 1])
        sa, sb = a.lookup(probe), b.lookup(probe)
        assert (sa[0] == sb[0]).all() and (sa[1] == sb[1]).all()
        assert sa[0].tolist() == [f.VAL_PRESENT] * 4 + [f.VAL_ZERO] + [f.VAL_NEW] * 3
        assert (a.find_low(probe[5:]) == b.find_low(probe[5:])).all()
        for x, y in zip(a.non_membership_witness(probe[5:]), b.non_membership_witness(probe[5:])):
            assert (x == y).all()
        same_tree(a, b)
        # the snapshot of the one loaded into the other and back; the value log likewise
        snap = a.snapshot()
        assert (snap == b.snapshot()).all()
        a.load(snap)
        b.load(snap)
        same_tree(a, b)
        log = ints_to_arr(allv[:at])
        a.load_values(log)
        b.load_values(log)
        same_tree(a, b)
        assert a.apply_batch(allv[6100:6200]) == b.apply_batch(allv[6100:6200])
        same_tree(a, b)
    finally:
        a.close()
        b.close()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- work in flight
class Blocks:
    """The six blocks of test_reserve_with_work_in_flight on one tree, all on device pointers: outputs in zeroed device
    buffers, so a row a call does not write compares equal too."""

    def __init__(self, imt, ctx, t, vals, absent):
        import torch
        self.imt, self.ctx, self.t, self.torch = imt, ctx, t, torch
        self.n, self.d = 96, t.depth
        self.dv = torch.from_numpy(ints_to_arr(vals)).cuda()
        f = imt._ffi
        # a mixed block: INSERTs of new values, READs of values no tree ever holds, MEMBERs of values of the first block
        n = self.n
        self.mixed = {}
        for which, first in (("mixed", 2 * n), ("apply_mixed", 3 * n)):
            mv, ops = [], []
            for i in range(n):
                kind = (f.OP_INSERT, f.OP_READ, f.OP_MEMBER)[i % 3]
                mv.append(vals[first + i] if kind == f.OP_INSERT else absent[i] if kind == f.OP_READ else vals[i])
                ops.append(kind)
            self.mixed[which] = (torch.from_numpy(ints_to_arr(mv)).cuda(), torch.tensor(ops, dtype=torch.uint8).cuda())
        self.out = []
        self.args = [self._prepare(k) for k in range(6)]
        torch.cuda.synchronize()                   # the zero fills are torch's, on torch's stream: done before any block

    def _buf(self, *shape):
        b = self.torch.zeros(shape, dtype=self.torch.uint8, device="cuda")
        self.out.append(b)
        return b

    def _insert_out(self, n):
        d = self.d
        return dict(low_index=self._buf(n, 8), low_leaf=self._buf(n, 96), is_largest=self._buf(n), old_root=self._buf(n, 32),
                    interim_root=self._buf(n, 32), new_root=self._buf(n, 32), new_leaf=self._buf(n, 96),
                    low_sib=self._buf(d, n, 32), new_sib=self._buf(d, n, 32))

    def _read_out(self, n):
        return dict(low_index=self._buf(n, 8), low_leaf=self._buf(n, 96), is_largest=self._buf(n), root=self._buf(n, 32),
                    low_sib=self._buf(self.d, n, 32))

    def _prepare(self, k):
        """the output addresses of block k"""
        n = self.n
        if k in (0, 4):
            return {key: b.data_ptr() for key, b in self._insert_out(n).items()}
        if k == 2:
            return ({key: b.data_ptr() for key, b in self._insert_out(n).items()},
                    {key: b.data_ptr() for key, b in self._read_out(n).items()})
        return self._buf(32).data_ptr()

    def step(self, k):
        """enqueue block k; nothing here waits for the GPU beyond what the call itself does"""
        imt, f, t, n, args = self.imt, self.imt._ffi, self.t, self.n, self.args[k]
        if k in (0, 4):                            # insert_batch | IMT_PIPELINE
            first = 0 if k == 0 else 4 * n
            out = f.InsertOut(**args)
            rc = imt.lib.imt_itree_insert_batch(t.h, P_(self.dv, first * 32), n, ctypes.byref(out), f.DEVICE_PTRS | f.PIPELINE)
            assert rc == 0, imt.lib.imt_last_error(self.ctx.h)
        elif k in (1, 5):                          # apply_pipelined
            first = n if k == 1 else 5 * n
            t.apply_pipelined(self.dv.data_ptr() + first * 32, n, args)
        elif k == 2:                               # mixed_pipelined
            mv, ops = self.mixed["mixed"]
            assert t.mixed_pipelined(mv.data_ptr(), ops.data_ptr(), n, args[0], args[1], members=True) == n // 3
        else:                                      # apply_mixed_pipelined
            mv, ops = self.mixed["apply_mixed"]
            assert t.apply_mixed_pipelined(mv.data_ptr(), ops.data_ptr(), n, args, members=True) == n // 3

    def results(self):
        self.ctx.sync()
        self.torch.cuda.synchronize()
        return [b.cpu().numpy() for b in self.out]


def test_reserve_with_work_in_flight(imt, ctx):
    import torch
    depth, n = 32, 96
    vals = oracle_lib.synth_values(6 * n, 0x52535602)
    absent = oracle_lib.synth_values(n, 0x52535603)
    start = oracle_lib.synth_values(700, 0x52535604)
    a, b = imt.IndexedTree(ctx, depth, 1024), imt.IndexedTree(ctx, depth, 4096)
    try:
        a.apply_batch(start)
        b.apply_batch(start)
        ra, rb = Blocks(imt, ctx, a, vals, absent), Blocks(imt, ctx, b, vals, absent)
        for k in range(4):                         # nothing waits between these calls and the reserve
            ra.step(k)
        assert a.size + 2 * n > a.capacity         # the last two blocks need the room
        a.reserve(4096)
        ra.step(4)
        ra.step(5)
        got = ra.results()
        for k in range(6):                         # the twin never has two things in flight
            rb.step(k)
            ctx.sync()
        want = rb.results()
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert (g == w).all(), f"output buffer {i}"
        # both mixed blocks insert a third of their operations
        assert a.size == b.size == 701 + 4 * n + 2 * (n // 3) and a.capacity == b.capacity == 4096
        same_tree(a, b)
        lag = np.empty((2, 2, 32), np.uint8)
        for i, t in enumerate((a, b)):
            for k in (0, 1):
                assert imt.lib.imt_itree_root_lagged(t.h, k, P_(lag[i, k]), 0) == 0
        assert (lag[0] == lag[1]).all()
    finally:
        a.close()
        b.close()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- views and lagged roots
def test_reserve_under_views(imt, ctx):
    depth, S = 32, 250
    allv = oracle_lib.synth_values(700, 0x52535605)
    t = imt.IndexedTree(ctx, depth, 1024)
    try:
        t.apply_batch(allv[:300])
        t.apply_batch(allv[300:600])
        v = t.view(S)
        idx = np.array([0, 1, 100, S - 1, S, S + 1, 600, 1023], np.uint64)
        absent = ints_to_arr(allv[600:620] + [P - 1])

        def lagged():
            out = np.empty((2, 32), np.uint8)
            for k in (0, 1):
                assert imt.lib.imt_itree_root_lagged(t.h, k, P_(out[k]), 0) == 0
            return out.tobytes()

        def answers(index):
            w = v.insert_witness(40)
            nm = v.non_membership_witness(absent)
            return (v.root(), v.get_leaves(index).tobytes(), v.get_proof_batch(index).tobytes(), tuple(x.tobytes() for x in nm),
                    tuple(w[k].tobytes() for k in sorted(w)), v.values().tobytes())

        first, lag0 = answers(idx), lagged()
        builds = v.stats()[1]
        assert builds == 1
        t.reserve(8192)
        assert t.capacity == 8192
        assert answers(idx) == first and v.stats()[1] == builds and lagged() == lag0
        t.reserve(1024)
        assert t.capacity == 1024
        assert answers(idx) == first and v.stats()[1] == builds and lagged() == lag0
        # the view follows the tree as before: a batch later it rebuilds once and answers the same
        t.reserve(2048)
        t.apply_batch(allv[620:700])
        assert answers(idx) == first and v.stats()[1] == builds + 1
        v.close()
    finally:
        t.close()


# ---------------------------------------------------------------- memory back
def test_reserve_shrink_after_rewind(imt, ctx, oracle):
    depth = 32
    allv = oracle_lib.synth_values(3100, 0x52535606)
    t, twin = imt.IndexedTree(ctx, depth, 2), imt.IndexedTree(ctx, depth, 128)
    h = oracle.sparse_new(depth, 256)
    try:
        t.reserve(1 << 12)
        t.apply_batch(allv[:3000])
        t.rewind(100)
        t.reserve(128)
        twin.apply_batch(allv[:99])
        assert (t.capacity, t.size) == (128, 100) and t.root() == twin.root()
        for got, want in zip(every_slot(t), every_slot(twin)):
            assert (got == want).all()
        assert (t.values() == twin.values()).all()
        # 100 + 29 leaves do not fit 128
        batch = allv[3000:3029]
        before = state(t)
        root = np.empty(32, np.uint8)
        assert imt.lib.imt_itree_apply_batch(t.h, P_(ints_to_arr(batch)), 29, P_(root), 0) == imt._ffi.ERR["FULL"]
        assert b"(imt_itree_reserve)" in imt.lib.imt_last_error(ctx.h)
        with pytest.raises(imt.ImtError) as ei:
            t.insert_batch(batch)
        assert ei.value.code == imt._ffi.ERR["FULL"] and state(t) == before
        t.reserve(256)
        res = t.insert_batch(batch)
        for x in allv[:99]:
            assert oracle.sparse_insert(h, depth, x)["rc"] == 0
        for i, x in enumerate(batch):
            old = oracle.sparse_root(h)
            o = oracle.sparse_insert(h, depth, x)
            assert o["rc"] == 0 and int(res["low_index"][i]) == o["low"] and int(res["is_largest"][i]) == o["largest"]
            assert imt.to_int(res["old_root"][i]) == old and imt.to_int(res["interim_root"][i]) == o["interim_root"]
            assert imt.to_int(res["new_root"][i]) == o["new_root"] and (res["low_leaf"][i] == o["low_leaf"]).all()
            assert (res["low_sib"][:, i] == o["low_proof"]).all() and (res["new_sib"][:, i] == o["new_proof"]).all()
        assert t.root() == oracle.sparse_root(h) and t.size == 129 and t.capacity == 256
    finally:
        oracle.sparse_free(h)
        t.close()
        twin.close()


# ---------------------------------------------------------------- refusals
def test_reserve_refusals(imt, ctx):
    import torch
    import test_gpu_sliced as ts
    f, lib = imt._ffi, imt.lib
    depth = 32
    good = oracle_lib.synth_values(60, 0x52535607)
    t, small = imt.IndexedTree(ctx, depth, 64), imt.IndexedTree(ctx, 4, 16)
    try:
        t.apply_batch(good[:20])
        small.apply_batch(good[:5])
        before, sbefore = state(t), state(small)
        for cap in (0, 1, 3, 48, (1 << 31) + 1, 1 << 32, 1 << 63, 16):          # 16 < the 21 leaves
            assert raw_reserve(imt, t, cap) == f.ERR["RANGE"], cap
            assert state(t) == before
        assert raw_reserve(imt, t, 3) == f.ERR["RANGE"] and b"capacity must be a power of two in [2, 2^31]" in lib.imt_last_error(ctx.h)
        assert raw_reserve(imt, small, 32) == f.ERR["RANGE"] and b"capacity exceeds 2^depth" in lib.imt_last_error(ctx.h)
        assert raw_reserve(imt, small, 4) == f.ERR["RANGE"]                       # below its 6 leaves
        assert state(small) == sbefore
        for flags in (f.PIPELINE, 0x8000, f.DEVICE_PTRS, 1):
            assert raw_reserve(imt, t, 128, flags) == f.ERR["ARG"], flags
            assert raw_reserve(imt, t, 64, flags) == f.ERR["ARG"], flags          # also where nothing would change
        assert raw_reserve(imt, None, 128) == f.ERR["ARG"] and lib.imt_itree_capacity(None) == 0
        assert state(t) == before
        assert raw_reserve(imt, t, 64) == 0 and state(t) == before                # the capacity it has: nothing runs
        # between imt_itree_batch_begin and _end
        ev, l0 = ctypes.c_uint32(), ctypes.c_uint32()
        more = ints_to_arr(good[20:24])
        assert lib.imt_itree_batch_begin(t.h, P_(more), 4, 0, ctypes.byref(ev), ctypes.byref(l0)) == 0
        assert raw_reserve(imt, t, 128) == f.ERR["ARG"] and b"sharded batch" in lib.imt_last_error(ctx.h)
        assert lib.imt_itree_capacity(t.h) == 64
        assert lib.imt_itree_batch_abort(t.h) == 0
        assert state(t) == before
        # an open slice
        dvals = torch.from_numpy(ints_to_arr(good[30:38])).cuda()
        pay = torch.zeros(int(lib.imt_itree_slice_payload_bytes(8)) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sl = ctypes.c_int(-1)
        assert lib.imt_itree_slice_prepare(t.h, P_(dvals), 0, 8, 0, None, f.DEVICE_PTRS, ctypes.byref(sl), None) == 0
        assert raw_reserve(imt, t, 128) == f.ERR["ARG"] and b"a slice is open" in lib.imt_last_error(ctx.h)
        assert raw_reserve(imt, t, 32) == f.ERR["ARG"] and lib.imt_itree_capacity(t.h) == 64
        for q in range(depth + 1):
            assert lib.imt_itree_slice_unit(t.h, sl.value, q, P_(pay), None) == 0
        ctx.sync()
        assert t.size == before[0] + 8 and t.rewind(before[0]) == before[1] and state(t) == before
        # and now it may
        t.reserve(128)
        assert t.capacity == 128 and t.root() == before[1]
    finally:
        t.close()
        small.close()
    # a replica of a sliced world with steps in flight
    sl_mod = ts.load_sliced()
    world, batch = 2, 50
    vals = oracle_lib.synth_values(world * batch, 0x52535608)
    w = sl_mod.SlicedTree(imt, 0, depth, 1 << 10, batch, world, n_local=world, nbuf=8)
    try:
        w.step(torch.from_numpy(ints_to_arr(vals)).cuda())
        for tr in w.trees:
            assert raw_reserve(imt, tr, 1 << 11) == f.ERR["ARG"] and lib.imt_itree_capacity(tr.h) == 1 << 10
            assert b"sliced steps in flight" in lib.imt_last_error(tr.ctx.h)
        w.flush()
        assert all(tr.size == world * batch + 1 and tr.capacity == 1 << 10 for tr in w.trees)
    finally:
        w.close()


def test_sliced_world_goes_on_after_reserve(imt, oracle):
    """after imt_sliced_flush the host reserves every replica alike, as it rewinds every replica alike"""
    import torch
    import test_gpu_sliced as ts
    sl = ts.load_sliced()
    depth, cap, world, batch, rounds = 32, 512, 2, 80, 6
    step = world * batch
    vals = oracle_lib.synth_values(rounds * step, 0x52535609)
    h = oracle.sparse_new(depth, 2 * cap)
    rows = [oracle.sparse_insert(h, depth, x) for x in vals]
    want_root = oracle.sparse_root(h)
    oracle.sparse_free(h)
    assert all(r["rc"] == 0 for r in rows)
    arr = torch.from_numpy(ints_to_arr(vals)).cuda()
    w = sl.SlicedTree(imt, 0, depth, cap, batch, world, n_local=world, nbuf=rounds)
    try:
        for r in range(3):
            assert w.step(arr[r * step:(r + 1) * step]) == r
        w.flush()
        assert all(t.size == 3 * step + 1 for t in w.trees)         # 481 of 512: the next step does not fit
        for t in w.trees:
            t.reserve(2 * cap)
        for r in range(3, rounds):
            assert w.step(arr[r * step:(r + 1) * step]) == r
        w.flush()
        for r in range(rounds):
            for k in range(world):
                o = w.outputs(r, k)
                base = r * step + k * batch
                new_root, old_root = o["new_root"].cpu().numpy(), o["old_root"].cpu().numpy()
                low_sib = o["low_sib"].cpu().numpy()
                for j in range(batch):
                    e = rows[base + j]
                    assert imt.to_int(new_root[j]) == e["new_root"], (r, k, j)
                    assert base + j == 0 or imt.to_int(old_root[j]) == rows[base + j - 1]["new_root"], (r, k, j)
                    assert (low_sib[:, j] == e["low_proof"]).all(), (r, k, j)
        assert all(t.root() == want_root and t.capacity == 2 * cap for t in w.trees)
    finally:
        w.close()


# ---------------------------------------------------------------- a size users run
def test_reserve_large(imt, ctx):
    import torch
    depth, n = 32, (1 << 16) + 3
    vals = ints_to_arr(oracle_lib.synth_values(n, 0x5253560A))
    a, b = imt.IndexedTree(ctx, depth, 1 << 10), imt.IndexedTree(ctx, depth, 1 << 17)
    try:
        a.apply_batch(vals[:1000])
        a.reserve(1 << 14)
        a.apply_batch(vals[1000:16383])                   # exactly full: 16384 leaves
        assert a.size == a.capacity == 1 << 14
        a.reserve(1 << 17)
        a.apply_batch(vals[16383:])
        assert b.apply_batch(vals) == a.root()
        same_tree(a, b)
    finally:
        a.close()
        b.close()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- the C example
def test_grow_demo_example(imt, oracle):
    """examples/grow_demo.c meets IMT_ERR_FULL twice on the way to ten blocks, reserves and goes on, then rewinds to three
    blocks and shrinks to fit; given the oracle's root as its argument it compares and fails on a difference."""
    exe = os.path.join(ROOT, "examples", "grow_demo")
    csrc = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "grow_demo.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    depth, h = 32, oracle.sparse_new(32, 4096)
    roots = {}
    for x in range(1, 3001):
        assert oracle.sparse_insert(h, depth, 1 + 7919023757 * x % ((1 << 61) - 1))["rc"] == 0
        if x in (900, 3000):
            roots[x] = oracle.sparse_root(h)
    oracle.sparse_free(h)
    r = subprocess.run([exe, f"{roots[900]:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "block 3: full at 901 of 1024 leaves; capacity now 2048, root unchanged" in r.stdout
    assert "block 6: full at 1801 of 2048 leaves; capacity now 4096, root unchanged" in r.stdout
    assert f"follower: 3001 leaves of 4096, root {roots[3000]:064x}" in r.stdout
    assert f"after the reorg: 901 leaves of 1024, root {roots[900]:064x}" in r.stdout
    assert "is the root again" in r.stdout and "refused, the tree as it was" in r.stdout
    assert "final root equals the expected one" in r.stdout
    r = subprocess.run([exe, f"{roots[900] ^ 1:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "DIFFERS" in r.stdout
