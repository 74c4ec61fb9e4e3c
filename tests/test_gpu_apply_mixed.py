"""GPU: imt_itree_apply_mixed and imt_itree_apply_mixed_filtered (include/imt.h) -- mixed blocks without witnesses.

The definition is the pair of calls that write witnesses: apply_mixed is mixed_batch with ins == rd == NULL, and
apply_mixed_filtered is mixed_filtered with ins == rd == NULL, plus root_out.  So every test plays a block on twin trees,
one through the new call and one through the call that defines it, and compares what both report and the trees they
leave; the plain Python walk (test_mixed_filter_logic.filtered_walk) and the sequential oracle (test_gpu_mixed.oracle_walk)
pin both.  The cost is part of the contract and is checked through imt_itree_apply_stats.  Every buffer, root_out
included, is filled with a sentinel byte before the call.

  test_twin_trees_filtered   == mixed_filtered: result, status, leaf_index, counts, root, state, every proof; walk and oracle
  test_twin_trees_strict     == mixed_batch on the accepted sub-scripts; the refused scripts: code, *bad_op, nothing written
  test_hash_counts           apply_stats == apply_batch of the carried-out INSERT values; READs add nothing, change nothing
  test_refusals, test_refused_while_sliced   every error, misaligned device buffers included: result, counts, tree and
                             root_out untouched, and on IMT_ERR_ARG status and leaf_index too
  test_formats_and_pointers  MONT256 / DEVICE, host and device pointers, NULL root_out, NULL leaf_index
  test_apply_now_prove_later a view at the size before the block replays the rows mixed_filtered wrote on the twin
  test_many_blocks_of_threads, test_one_long_run     2^12 + 3 operations, a third refused; 1 024 operations on one value
  test_neighbours            behind pipelined batches in flight, insert_batch with witnesses behind it, a rewind
  test_python_wrappers, test_apply_block_example     the upper layers
"""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib
import test_gpu_insert_matrix as tm
from oracle_lib import P, arr_ints, ints_to_arr
from test_gpu_mixed import INS_FIELDS, RD_FIELDS, SENTINEL, Raw, oracle_walk
from test_gpu_mixed_filtered import EXAMPLE_BLOCK, SENT64, RawF, noisy_script, scripts_for, split, state, tree_with
from test_gpu_rewind import forms  # noqa: F401  (the fixture: one context per hash form)
from test_mixed_filter_logic import NEW, PRESENT, REPEATED, ZERO, filtered_walk
from test_mixed_logic import ADVERSARIAL, INSERT, READ, walk

pytestmark = pytest.mark.gpu


class Out:
    """status / leaf_index / root_out buffers of one call, host or device, every one pre-filled with the sentinel byte"""

    def __init__(self, imt, n, dev=False, leaf=True, root=True):
        self.imt, self.n, self.dev = imt, n, dev
        self.status = self._buf(np.full(n, SENTINEL, np.uint8))
        self.leaf = self._buf(np.full(n, SENT64, np.uint64)) if leaf else None
        self.root = self._buf(np.full(32, SENTINEL, np.uint8)) if root else None

    def _buf(self, a):
        if not self.dev:
            return a
        import torch
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()

    def ptr(self, x, offset=0):
        if x is None:
            return None
        return ctypes.c_void_p((x.data_ptr() if self.dev else x.ctypes.data) + offset)

    def inputs(self, vals, ops):
        """(pointer to vals, pointer to ops); the arrays are kept alive in self.keep"""
        if self.dev:
            import torch
            self.keep = (torch.from_numpy(np.ascontiguousarray(vals)).cuda(), torch.from_numpy(np.asarray(ops, np.uint8)).cuda())
            return tuple(ctypes.c_void_p(x.data_ptr()) for x in self.keep)
        self.keep = (np.ascontiguousarray(vals), np.asarray(ops, np.uint8))
        return tuple(x.ctypes.data_as(ctypes.c_void_p) for x in self.keep)

    def finish(self, t):
        if self.dev:
            import torch
            t.ctx.sync()
            torch.cuda.synchronize()

    def host(self, x):
        if x is None or not self.dev:
            return x
        a = x.cpu().numpy()
        return a.view(np.uint64) if a.dtype == np.int64 else a

    def got_status(self):
        return self.host(self.status).tolist()

    def got_leaf(self):
        return self.host(self.leaf).tolist()

    def got_root(self):
        return self.host(self.root)

    def root_untouched(self):
        return self.root is None or (self.got_root() == SENTINEL).all()

    def classification_untouched(self):
        return set(self.got_status()) <= {SENTINEL} and (self.leaf is None or set(self.got_leaf()) <= {SENT64})


class RawAF(Out):
    """imt_itree_apply_mixed_filtered"""

    def call(self, t, vals, ops, flags=0, leaf_offset=0, root_offset=0):
        pv, po = self.inputs(vals, ops)
        self.n_ins, self.n_rd = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
        flags |= self.imt._ffi.DEVICE_PTRS if self.dev else 0
        rc = self.imt.lib.imt_itree_apply_mixed_filtered(t.h, pv, po, self.n, self.ptr(self.status), self.ptr(self.leaf, leaf_offset),
                                                         ctypes.byref(self.n_ins), ctypes.byref(self.n_rd),
                                                         self.ptr(self.root, root_offset), flags)
        self.finish(t)
        return rc

    def counts(self):
        return self.n_ins.value, self.n_rd.value


class RawA(Out):
    """imt_itree_apply_mixed"""

    def __init__(self, imt, n, dev=False, root=True):
        super().__init__(imt, 0, dev, False, root)
        self.n = n

    def call(self, t, vals, ops, flags=0, root_offset=0):
        pv, po = self.inputs(vals, ops)
        self.n_ins, self.bad = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
        flags |= self.imt._ffi.DEVICE_PTRS if self.dev else 0
        rc = self.imt.lib.imt_itree_apply_mixed(t.h, pv, po, self.n, self.ptr(self.root, root_offset), ctypes.byref(self.n_ins),
                                                ctypes.byref(self.bad), flags)
        self.finish(t)
        return rc


def root_arr(root, fmt=0):
    a = ints_to_arr([root])
    return (tm.to_fmt(a, fmt) if fmt else a)[0]


def all_proofs(t):
    return t.get_proof_batch(np.arange(t.size))


def carried_out(stored, script):
    """(status, leaf, accepted positions, accepted sub-script, its INSERT values) by the plain walk"""
    status, _, leaf, _, acc = filtered_walk([0] + list(stored), script)
    sub = [script[p] for p in acc]
    return status, leaf, acc, sub, [v for op, v in sub if op == INSERT]


def vals_ops(script):
    if not script:
        return np.zeros((0, 32), np.uint8), []
    return split(script)


_ORACLE = {}


def oracle_final(oracle, depth, name):
    """(root, preimages) of the sequential oracle after the accepted sub-script of scripts_for(depth)[name], computed once"""
    if (depth, name) not in _ORACLE:
        stored, script = scripts_for(depth)[name]
        _ORACLE[depth, name] = oracle_walk(oracle, depth, 1 << min(depth, 7), stored, carried_out(stored, script)[3])[2]
    return _ORACLE[depth, name]


def same_tree(a, b, tag=""):
    assert state(a) == state(b), tag
    assert (all_proofs(a) == all_proofs(b)).all(), tag


# ---------------------------------------------------------------- 1. twin trees, filtered
@pytest.mark.parametrize("form", ["thread", "quad"])
@pytest.mark.parametrize("depth", [3, 8, 32])
def test_twin_trees_filtered(imt, forms, oracle, depth, form):
    c, cap = forms[form], 1 << min(depth, 7)
    cases = scripts_for(depth)
    assert len(cases) >= 10 and "random" in cases and "one value 64 times" in cases and "nothing accepted" in cases
    for name, (stored, script) in cases.items():
        tag = f"{name} depth {depth} {form}"
        status, leaf, acc, sub, _ = carried_out(stored, script)
        a, b = tree_with(imt, c, depth, cap, stored), tree_with(imt, c, depth, cap, stored)
        try:
            vals, ops = split(script)
            ra, rb = RawAF(imt, len(script)), RawF(imt, depth, len(script))
            assert ra.call(a, vals, ops) == rb.call(b, vals, ops, 0) == 0, (tag, imt.lib.imt_last_error(c.h))
            assert ra.counts() == (rb.n_ins.value, rb.n_rd.value), tag
            assert ra.got_status() == rb.got_status() == status and ra.got_leaf() == rb.got_leaf() == leaf, tag
            assert arr_ints(ra.got_root()) == [b.root()], tag
            same_tree(a, b, tag)
            root, pre = oracle_final(oracle, depth, name)
            assert a.root() == root and a.size == pre.shape[0] and (a.snapshot() == pre).all(), tag
        finally:
            a.close()
            b.close()


# ---------------------------------------------------------------- 2. twin trees, strict
@pytest.mark.parametrize("form", ["thread", "quad"])
@pytest.mark.parametrize("depth", [3, 8, 32])
def test_twin_trees_strict(imt, forms, oracle, depth, form):
    c, cap, E = forms[form], 1 << min(depth, 7), imt._ffi.ERR
    for name, (stored, script) in scripts_for(depth).items():
        tag = f"{name} depth {depth} {form}"
        sub = carried_out(stored, script)[3]
        a, b = tree_with(imt, c, depth, cap, stored), tree_with(imt, c, depth, cap, stored)
        try:
            vals, ops = vals_ops(sub)
            ra, rb = RawA(imt, len(sub)), Raw(imt, depth, len(sub))
            assert ra.call(a, vals, ops) == rb.call(b, vals, ops, 0) == 0, (tag, imt.lib.imt_last_error(c.h))
            assert ra.n_ins.value == rb.n_ins.value == ops.count(INSERT) and ra.bad.value == rb.bad.value == 0xDEAD, tag
            assert arr_ints(ra.got_root()) == [b.root()], tag
            same_tree(a, b, tag)
            root, pre = oracle_final(oracle, depth, name)
            assert a.root() == root and a.size == pre.shape[0] and (a.snapshot() == pre).all(), tag
        finally:
            a.close()
            b.close()
    refused = {k: (st[1:], sc) for k, (st, sc) in ADVERSARIAL.items() if walk(st, sc)[1] >= 0 and max(x for _, x in sc) < P}
    assert len(refused) >= 6
    for name, (stored, script) in refused.items():
        tag = f"refused: {name} depth {depth} {form}"
        a, b = tree_with(imt, c, depth, cap, stored), tree_with(imt, c, depth, cap, stored)
        try:
            before = state(a)
            vals, ops = split(script)
            ra, rb = RawA(imt, len(script)), Raw(imt, depth, len(script), ins_fields=None, rd_fields=None)
            rc = ra.call(a, vals, ops)
            assert rc == rb.call(b, vals, ops, 0) and rc in (E["VALUE"], E["FULL"]), tag
            assert ra.bad.value == rb.bad.value and ra.n_ins.value == rb.n_ins.value == 0xDEAD, tag
            if rc == E["VALUE"]:
                assert ra.bad.value == walk([0] + stored, script)[1], tag
            assert state(a) == before == state(b) and ra.root_untouched(), tag
        finally:
            a.close()
            b.close()


# ---------------------------------------------------------------- 3. the cost
def counts_block():
    vals = [v for v in oracle_lib.synth_values(700, 0x41504D03) if 0 < v < P]
    stored, fresh = vals[:100], vals[100:]
    script = noisy_script(random.Random(0x41504D03), stored, fresh, 300, 200)
    return vals, stored, script


def test_hash_counts(imt, ctx):
    depth, cap, lib = 32, 1024, imt.lib
    vals, stored, script = counts_block()
    status, leaf, acc, sub, inserted = carried_out(stored, script)
    assert 60 <= len(inserted) and 60 <= len(sub) - len(inserted) and 60 <= len(script) - len(sub)
    trees = [tree_with(imt, ctx, depth, cap, stored) for _ in range(5)]
    a, s, c3, d, e = trees
    try:
        ra = RawAF(imt, len(script))
        assert ra.call(a, *split(script)) == 0 and ra.counts() == (len(inserted), len(sub) - len(inserted))
        want_root = c3.apply_batch(inserted)
        want = c3.apply_stats()
        assert want[0] >= len(inserted) and (want[1:] >= 1).all()
        assert (a.apply_stats() == want).all() and arr_ints(ra.got_root()) == [want_root]
        # the strict call on the accepted sub-script; the same block with its READs removed, through both calls
        rs = RawA(imt, len(sub))
        assert rs.call(s, *split(sub)) == 0 and (s.apply_stats() == want).all()
        no_reads = [(op, v) for op, v in script if op == INSERT]
        rd_ = RawAF(imt, len(no_reads))
        assert rd_.call(d, *split(no_reads)) == 0 and rd_.counts() == (len(inserted), 0) and (d.apply_stats() == want).all()
        re_ = RawA(imt, len(inserted))
        assert re_.call(e, ints_to_arr(inserted), [INSERT] * len(inserted)) == 0 and (e.apply_stats() == want).all()
        for t in (s, d, e):
            same_tree(t, c3)
        same_tree(a, c3)
        # a READs-only block afterwards: no hash, no change, the view stays fresh, the lagged root does not move
        v = a.view(50)
        view_root, builds = v.root(), v.stats()[1]
        before, proofs = state(a), all_proofs(a)
        lagged, again = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
        assert lib.imt_itree_root_lagged(a.h, 0, lagged.ctypes.data_as(ctypes.c_void_p), 0) == 0
        reads = [(READ, x) for x in vals[600:660]] + [(READ, stored[3]), (INSERT, inserted[0]), (READ, 0), (INSERT, stored[5])]
        for call_reads in (reads, reads[:60]):
            r = RawAF(imt, len(call_reads))
            assert r.call(a, *split(call_reads)) == 0 and r.counts() == (0, 60)
            assert r.got_status() == filtered_walk([0] + stored + inserted, call_reads)[0]
            assert arr_ints(r.got_root()) == [before[0]]
            r2 = RawA(imt, 60)
            assert r2.call(a, *split(reads[:60])) == 0 and r2.n_ins.value == 0 and arr_ints(r2.got_root()) == [before[0]]
            assert (a.apply_stats() == want).all()
            assert state(a) == before and (all_proofs(a) == proofs).all()
            assert v.root() == view_root and v.stats()[1] == builds
            assert lib.imt_itree_root_lagged(a.h, 0, again.ctypes.data_as(ctypes.c_void_p), 0) == 0 and (again == lagged).all()
        v.close()
        # on a tree no apply call has inserted into, a READs-only block is no apply call either
        fresh = imt.IndexedTree(ctx, depth, cap)
        trees.append(fresh)
        hashes = (ctypes.c_uint64 * (depth + 1))()
        for r in (RawAF(imt, 60), RawA(imt, 60)):
            assert r.call(fresh, *split(reads[:60])) == 0 and arr_ints(r.got_root()) == [fresh.root()]
            assert lib.imt_itree_apply_stats(fresh.h, hashes) == imt._ffi.ERR["ARG"]
        fresh.insert_batch(stored[:4])
        assert RawAF(imt, 60).call(fresh, *split(reads[:60])) == 0 and lib.imt_itree_apply_stats(fresh.h, hashes) == imt._ffi.ERR["ARG"]
    finally:
        for t in trees:
            t.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals(imt, forms):
    import torch
    c, f, lib = forms["default"], imt._ffi, imt.lib
    depth, cap = 32, 64
    E = f.ERR
    stored = [10, 20, 30]
    t = imt.IndexedTree(c, depth, cap)
    try:
        t.apply_batch(stored)
        before = state(t)

        def refused(script, want_rc, flags=0, dev=False, tree=t, classified=False, tag=""):
            """both calls: the result, the counts, tree and root_out untouched; status as the error case says"""
            was = before if tree is t else state(tree)
            r = RawAF(imt, len(script), dev)
            rc = r.call(tree, *split(script), flags)
            assert rc == want_rc, (tag, script, rc, lib.imt_last_error(c.h))
            assert r.counts() == (0, 0) and r.root_untouched(), (tag, script)
            if classified:
                assert r.got_status() == filtered_walk([0] + stored, script)[0], (tag, script)
            else:
                assert r.classification_untouched(), (tag, script)
            assert state(tree) == was, (tag, script)
            return r

        def refused_strict(script, want_rc, flags=0, dev=False, tree=t, bad=0xDEAD, tag=""):
            was = before if tree is t else state(tree)
            r = RawA(imt, len(script), dev)
            rc = r.call(tree, *split(script), flags)
            assert rc == want_rc, (tag, script, rc, lib.imt_last_error(c.h))
            assert r.n_ins.value == 0xDEAD and r.bad.value == bad and r.root_untouched(), (tag, script)
            assert state(tree) == was, (tag, script)

        # IMT_ERR_NONCANONICAL: malformed input, whatever else the block holds; status is the classification
        refused([(READ, 7), (READ, P), (INSERT, 0), (INSERT, 20)], E["NONCANONICAL"], classified=True)
        refused([(INSERT, P + 1), (READ, 7), (INSERT, 7), (READ, 7)], E["NONCANONICAL"], dev=True, classified=True)
        refused_strict([(READ, 7), (READ, P), (INSERT, 8)], E["NONCANONICAL"])
        refused_strict([(INSERT, P + 1), (READ, 7)], E["NONCANONICAL"], dev=True)
        # IMT_ERR_VALUE is the strict call's alone, with the first offender
        refused_strict([(INSERT, 5), (READ, 6), (READ, 5), (INSERT, 0)], E["VALUE"], bad=2)
        refused_strict([(READ, 6), (INSERT, 20), (READ, 0)], E["VALUE"], dev=True, bad=1)
        # IMT_ERR_FULL counts the accepted INSERTs only: the raw INSERTs exceed the room, the accepted ones too
        room = cap - t.size
        full = [(INSERT, 1000 + i) for i in range(room + 1)]
        refused(full, E["FULL"], classified=True)
        refused([(READ, 500 + i) for i in range(80)] + full + [(INSERT, 1000), (INSERT, 0)], E["FULL"], dev=True, classified=True)
        refused_strict([(READ, 500 + i) for i in range(80)] + full, E["FULL"])
        # ... and the reverse: the raw INSERTs exceed the room, the accepted ones fill it exactly
        twin = imt.IndexedTree(c, depth, cap)
        twin.apply_batch(stored)
        fits = full[:room] + [(INSERT, 1000 + i) for i in range(room)] + [(INSERT, 10), (INSERT, 0)] + [(READ, 500 + i) for i in range(2 * cap)]
        assert sum(op == INSERT for op, _ in fits) > room
        r = RawAF(imt, len(fits))
        assert r.call(twin, *split(fits)) == 0 and r.counts() == (room, 2 * cap) and twin.size == cap
        assert r.got_status() == [NEW] * room + [REPEATED] * room + [PRESENT, ZERO] + [NEW] * (2 * cap)
        assert arr_ints(r.got_root()) == [twin.root()]
        twin.rewind(1 + len(stored))
        r = RawA(imt, room + 2 * cap)
        assert r.call(twin, *split(full[:room] + fits[-2 * cap:])) == 0 and r.n_ins.value == room and twin.size == cap
        twin.close()
        # IMT_ERR_ARG: op bytes through both kinds of pointer
        for dev in (False, True):
            for ops in ([0, 2], [255, 1]):
                r = RawAF(imt, 2, dev)
                assert r.call(t, ints_to_arr([5, 6]), ops) == E["ARG"] and r.classification_untouched() and r.root_untouched()
                assert r.counts() == (0, 0)
                r = RawA(imt, 2, dev)
                assert r.call(t, ints_to_arr([5, 6]), ops) == E["ARG"] and r.root_untouched()
                assert (r.n_ins.value, r.bad.value) == (0xDEAD, 0xDEAD)
        assert state(t) == before
        # the three refused flags, an unknown format
        ok = [(INSERT, 5), (READ, 6)]
        for flags in (f.PIPELINE, f.PIPELINE | f.DEVICE_PTRS, f.HOST_PREP, f.INPUTS_READY | f.DEVICE_PTRS, f.INPUTS_READY, 3):
            refused(ok, E["ARG"], flags=flags & ~f.DEVICE_PTRS, dev=bool(flags & f.DEVICE_PTRS), tag=f"flags {flags}")
            refused_strict(ok, E["ARG"], flags=flags & ~f.DEVICE_PTRS, dev=bool(flags & f.DEVICE_PTRS), tag=f"flags {flags}")
        # NULL arguments
        one, op1, st1, root1 = ints_to_arr([5]), np.zeros(1, np.uint8), np.full(1, SENTINEL, np.uint8), np.full(32, SENTINEL, np.uint8)
        pv, po, ps, pr = (x.ctypes.data_as(ctypes.c_void_p) for x in (one, op1, st1, root1))
        k1, k2 = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
        n1, n2 = ctypes.byref(k1), ctypes.byref(k2)
        call, strict = lib.imt_itree_apply_mixed_filtered, lib.imt_itree_apply_mixed
        assert call(t.h, None, po, 1, ps, None, n1, n2, pr, 0) == E["ARG"]
        assert call(t.h, pv, None, 1, ps, None, n1, n2, pr, 0) == E["ARG"]
        assert call(t.h, pv, po, 1, None, None, n1, n2, pr, 0) == E["ARG"]
        assert call(t.h, pv, po, 1, ps, None, None, n2, pr, 0) == E["ARG"]
        assert call(t.h, pv, po, 1, ps, None, n1, None, pr, 0) == E["ARG"]
        assert call(None, pv, po, 1, ps, None, n1, n2, pr, 0) == E["ARG"]
        assert strict(t.h, None, po, 1, pr, n1, n2, 0) == E["ARG"] and strict(t.h, pv, None, 1, pr, n1, n2, 0) == E["ARG"]
        assert strict(None, pv, po, 1, pr, n1, n2, 0) == E["ARG"]
        assert st1[0] == SENTINEL and (root1 == SENTINEL).all() and state(t) == before
        # n == 0: IMT_OK, the counts 0, the current root
        k1.value = k2.value = 0xDEAD
        assert call(t.h, None, None, 0, ps, None, n1, n2, pr, 0) == 0 and (k1.value, k2.value) == (0, 0)
        assert arr_ints(root1) == [before[0]] and st1[0] == SENTINEL
        root1[:] = SENTINEL
        k1.value = k2.value = 0xDEAD
        assert strict(t.h, None, None, 0, pr, n1, n2, 0) == 0 and (k1.value, k2.value) == (0, 0xDEAD) and arr_ints(root1) == [before[0]]
        assert call(t.h, None, None, 0, ps, None, n1, n2, None, 0) == 0 and strict(t.h, None, None, 0, None, None, None, 0) == 0
        # misaligned device buffers: vals, leaf_index, root_out
        r = RawAF(imt, 2, dev=True)
        assert r.call(t, ints_to_arr([5, 6]), [0, 1], leaf_offset=4) == E["ARG"] and r.classification_untouched() and r.root_untouched()
        r = RawAF(imt, 2, dev=True)
        assert r.call(t, ints_to_arr([5, 6]), [0, 1], root_offset=8) == E["ARG"] and r.classification_untouched() and r.root_untouched()
        big = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
        r = RawA(imt, 2, dev=True)
        r.root = big
        assert r.call(t, ints_to_arr([5, 6]), [0, 1], root_offset=8) == E["ARG"] and (big.cpu().numpy() == SENTINEL).all()
        dvals = torch.from_numpy(ints_to_arr([5, 6, 7])).cuda()
        dops = torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
        r = RawAF(imt, 2, dev=True)
        off = ctypes.c_void_p(dvals.data_ptr() + 8)
        assert call(t.h, off, ctypes.c_void_p(dops.data_ptr()), 2, r.ptr(r.status), r.ptr(r.leaf), n1, n2, r.ptr(r.root), f.DEVICE_PTRS) == E["ARG"]
        assert strict(t.h, off, ctypes.c_void_p(dops.data_ptr()), 2, r.ptr(r.root), n1, n2, f.DEVICE_PTRS) == E["ARG"]
        c.sync()
        assert r.classification_untouched() and r.root_untouched() and state(t) == before
        # a placed tree, a partitioned tree
        placed = imt.IndexedTree(c, 8, 64)
        placed.set_placement(10, 1)
        refused(ok, E["ARG"], tree=placed)
        refused_strict(ok, E["ARG"], tree=placed)
        placed.close()
        part = imt.IndexedTree(c, depth, cap)
        c._check(lib.imt_itree_set_value_partition(part.h, 3, 1))
        refused([(INSERT, 4), (READ, 7)], E["ARG"], tree=part)
        refused_strict([(INSERT, 4), (READ, 7)], E["ARG"], tree=part)
        assert part.size == 1
        part.close()
        # between imt_itree_batch_begin and _end; an open slice
        ev, l0 = ctypes.c_uint32(), ctypes.c_uint32()
        more = ints_to_arr([71, 72, 73, 74])
        assert lib.imt_itree_batch_begin(t.h, more.ctypes.data_as(ctypes.c_void_p), 4, 0, ctypes.byref(ev), ctypes.byref(l0)) == 0
        for r in (RawAF(imt, 2), RawA(imt, 2)):
            assert r.call(t, ints_to_arr([5, 6]), [0, 1]) == E["ARG"] and r.classification_untouched() and r.root_untouched()
        assert lib.imt_itree_batch_abort(t.h) == 0
        assert state(t) == before
        dv8 = torch.from_numpy(ints_to_arr([81, 82, 83, 84, 85, 86, 87, 88])).cuda()
        pay = torch.zeros(int(lib.imt_itree_slice_payload_bytes(8)) + 64, dtype=torch.uint8, device="cuda")
        sl = ctypes.c_int(-1)
        assert lib.imt_itree_slice_prepare(t.h, ctypes.c_void_p(dv8.data_ptr()), 0, 8, 0, None, f.DEVICE_PTRS, ctypes.byref(sl), None) == 0
        for r in (RawAF(imt, 2), RawA(imt, 2)):
            assert r.call(t, ints_to_arr([5, 6]), [0, 1]) == E["ARG"] and r.classification_untouched() and r.root_untouched()
        for q in range(depth + 1):
            assert lib.imt_itree_slice_unit(t.h, sl.value, q, ctypes.c_void_p(pay.data_ptr()), None) == 0
        c.sync()
        assert t.size == before[1] + 8
        status, leaf, n_ins, n_rd, root = t.apply_mixed_filtered([5, 6, 5], [INSERT, READ, READ])      # and afterwards the call works
        assert status.tolist() == [NEW, NEW, REPEATED] and leaf.tolist() == [t.size - 1] * 3 and (n_ins, n_rd) == (1, 1)
        assert root == t.root()
    finally:
        t.close()


def test_refused_while_sliced(imt, ctx):
    """world 2 over the local transport: a replica with steps in flight takes no block, after the flush it does"""
    import torch
    import test_gpu_sliced as ts
    sl = ts.load_sliced()
    depth, cap, world, batch = 32, 1 << 10, 2, 40
    vals = oracle_lib.synth_values(world * batch + 4, 0x41504D53)
    w = sl.SlicedTree(imt, 0, depth, cap, batch, world, n_local=world, nbuf=8)
    try:
        w.step(torch.from_numpy(ints_to_arr(vals[:world * batch])).cuda())
        for t in w.trees:
            r = RawAF(imt, 2)
            assert r.call(t, ints_to_arr(vals[-2:]), [0, 1]) == imt._ffi.ERR["ARG"] and r.counts() == (0, 0)
            assert r.classification_untouched() and r.root_untouched()
            r = RawA(imt, 2)
            assert r.call(t, ints_to_arr(vals[-2:]), [0, 1]) == imt._ffi.ERR["ARG"] and r.root_untouched()
        w.flush()
        roots = {t.root() for t in w.trees}
        assert len(roots) == 1
        t = w.trees[0]
        status, leaf, n_ins, n_rd, root = t.apply_mixed_filtered([vals[-2], vals[-1], vals[0]], [READ, INSERT, INSERT])
        assert status.tolist() == [NEW, NEW, PRESENT] and (n_ins, n_rd) == (1, 1) and root == t.root() and root not in roots
        assert t.size == world * batch + 2
    finally:
        w.close()


# ---------------------------------------------------------------- 5. formats and pointers
def test_formats_and_pointers(imt, forms):
    c, f = forms["default"], imt._ffi
    depth, cap = 32, 256
    vals = [v for v in oracle_lib.synth_values(120, 0x41504D05) if 0 < v < P]
    stored, script = vals[:30], [(READ if i % 3 == 1 else INSERT, vals[40 + i]) for i in range(50)]
    script += [(READ, vals[41]), (READ, vals[100]), (INSERT, 0), (READ, vals[3]), (INSERT, vals[40]), (READ, vals[42]), (READ, 0),
               (INSERT, vals[7])]
    v_arr, ops = split(script)
    n = len(script)
    want_status, want_leaf, acc, sub, inserted = carried_out(stored, script)
    k, m = len(inserted), len(sub) - len(inserted)
    assert 0 < k and 0 < m and len(acc) == n - 6
    sub_vals, sub_ops = split(sub)
    trees = []

    def fresh():
        trees.append(tree_with(imt, c, depth, cap, stored))
        return trees[-1]

    try:
        ref = fresh()
        rb = RawF(imt, depth, n)
        assert rb.call(ref, v_arr, ops, 0) == 0 and rb.got_status() == want_status and rb.got_leaf() == want_leaf
        final, root = state(ref), ref.root()
        for fmt in (f.FMT_CANONICAL, f.FMT_MONT256, f.FMT_DEVICE):
            for dev in (False, True):
                for with_leaf, with_root in ((True, True), (False, True), (True, False), (False, False)):
                    tag = f"fmt {fmt} dev {dev} leaf {with_leaf} root {with_root}"
                    t, r = fresh(), RawAF(imt, n, dev, with_leaf, with_root)
                    assert r.call(t, tm.to_fmt(v_arr, fmt), ops, fmt) == 0 and r.counts() == (k, m), tag
                    assert r.got_status() == want_status and (not with_leaf or r.got_leaf() == want_leaf), tag
                    assert not with_root or (r.got_root() == root_arr(root, fmt)).all(), tag
                    assert state(t) == final, tag
                    t.close()
                for with_root in (True, False):
                    tag = f"strict fmt {fmt} dev {dev} root {with_root}"
                    t, r = fresh(), RawA(imt, len(sub), dev, with_root)
                    assert r.call(t, tm.to_fmt(sub_vals, fmt), sub_ops, fmt) == 0 and r.n_ins.value == k, tag
                    assert not with_root or (r.got_root() == root_arr(root, fmt)).all(), tag
                    assert state(t) == final, tag
                    t.close()
    finally:
        for t in trees:
            t.close()


# ---------------------------------------------------------------- 6. the loop the feature exists for
def test_apply_now_prove_later(imt, ctx):
    depth, cap = 32, 1024
    vals = [v for v in oracle_lib.synth_values(500, 0x41504D06) if 0 < v < P]
    stored = vals[:100]
    script = [(READ if i % 4 == 1 else INSERT, vals[100 + i] if i % 9 else (0, vals[i], vals[100 + i - 1])[i % 3]) for i in range(200)]
    script[5], script[6] = (READ, vals[100 + 150]), (READ, vals[100 + 150])            # two READs of a value inserted later
    status, leaf, acc, sub, inserted = carried_out(stored, script)
    k, m = len(inserted), len(sub) - len(inserted)
    assert k >= 100 and m >= 30 and len(script) - len(sub) >= 15
    a, b = tree_with(imt, ctx, depth, cap, stored), tree_with(imt, ctx, depth, cap, stored)
    try:
        size0 = a.size
        got_status, got_leaf, n_ins, n_rd, root1 = a.apply_mixed_filtered(*split(script))
        assert got_status.tolist() == status and got_leaf.tolist() == leaf and (n_ins, n_rd) == (k, m)
        root2 = a.apply_batch(vals[400:450])                                           # the tree moves on
        want_ins, want_rd, b_status, b_leaf = b.mixed_filtered(*split(script))
        assert b.root() == root1 != root2 and (b_status == got_status).all() and (b_leaf == got_leaf).all()
        v = a.view(size0)
        ins, rd = v.mixed_witness(*split(sub))
        compared = 0
        for got, want, fields in ((ins, want_ins, INS_FIELDS), (rd, want_rd, RD_FIELDS)):
            for key in fields:
                assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), key
                compared += 1
        assert compared == 14 and arr_ints(ins["new_root"][-1]) == [root1]
        v.close()
        assert a.root() == root2 and a.size == size0 + k + 50
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 7. more than one block of threads, one long run
def test_many_blocks_of_threads(imt, forms):
    """2^12 + 3 operations behind 300 stored values: 17 blocks of threads for the operations, more than one for the INSERT
    events, more than one merge-sort tile.  About a third refused; everything against the mixed_filtered twin and the walk"""
    c = forms["default"]
    depth, cap, n = 32, 1 << 13, (1 << 12) + 3
    vals = [v for v in oracle_lib.synth_values(5000, 0x41504D07) if 0 < v < P]
    stored, fresh = vals[:300], vals[300:]
    script = noisy_script(random.Random(0x41504D07), stored, fresh, n, cap - 301)
    for p in range(100, n, 500):                               # behind 300 stored values the noise hardly ever draws a 0
        script[p], script[p + 1] = (INSERT, 0), (READ, 0)
    status, leaf, acc, sub, inserted = carried_out(stored, script)
    assert n // 4 <= n - len(acc) <= 2 * n // 5 and len(inserted) > 1024 and len(sub) - len(inserted) > 1024
    assert {(op, s) for (op, _), s in zip(script, status)} == {(o, s) for o in (INSERT, READ) for s in (NEW, ZERO, PRESENT, REPEATED)}
    a, b, c3 = (tree_with(imt, c, depth, cap, stored) for _ in range(3))
    try:
        vals_arr, ops = split(script)
        ra, rb = RawAF(imt, n), RawF(imt, depth, n)
        assert ra.call(a, vals_arr, ops) == rb.call(b, vals_arr, ops, 0) == 0
        assert ra.counts() == (rb.n_ins.value, rb.n_rd.value) == (len(inserted), len(sub) - len(inserted))
        assert ra.got_status() == rb.got_status() == status and ra.got_leaf() == rb.got_leaf() == leaf
        assert arr_ints(ra.got_root()) == [b.root()]
        same_tree(a, b)
        assert c3.apply_batch(inserted) == a.root() and (c3.apply_stats() == a.apply_stats()).all()
    finally:
        for t in (a, b, c3):
            t.close()


def test_one_long_run(imt, ctx):
    """1 024 operations on one value -- READ, INSERT, then alternating"""
    depth, cap, n = 32, 64, 1024
    a, b = tree_with(imt, ctx, depth, cap, [10, 90]), tree_with(imt, ctx, depth, cap, [10, 90])
    try:
        script = [(READ, 50), (INSERT, 50)] + [(p & 1, 50) for p in range(n - 2)]
        ra, rb = RawAF(imt, n), RawF(imt, depth, n, ins_fields=("new_root",), rd_fields=("root",))
        assert ra.call(a, *split(script)) == rb.call(b, *split(script), 0) == 0 and ra.counts() == (1, 1)
        assert ra.got_status() == rb.got_status() == [NEW, NEW] + [REPEATED] * (n - 2)
        assert ra.got_leaf() == rb.got_leaf() == [1] + [3] * (n - 1)
        assert arr_ints(ra.got_root()) == [b.root()] and a.apply_stats()[0] == 2
        same_tree(a, b)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 8. neighbours
def test_neighbours(imt, forms):
    """behind two pipelined insert batches still in flight, with no synchronisation by the caller; insert_batch with
    witnesses directly behind it; a rewind to the size before the block"""
    import torch
    c, f, lib = forms["default"], imt._ffi, imt.lib
    depth, cap, nb = 32, 1 << 14, 2048
    vals = [v for v in oracle_lib.synth_values(2 * nb + 200, 0x41504D08) if 0 < v < P]
    a, b = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    try:
        d = torch.from_numpy(ints_to_arr(vals[:2 * nb])).cuda()
        for j in range(2):
            part = d[j * nb:(j + 1) * nb]
            assert lib.imt_itree_insert_batch(a.h, ctypes.c_void_p(part.data_ptr()), nb, None, f.DEVICE_PTRS | f.PIPELINE) == 0
        script = [(READ if i % 3 == 0 else INSERT, vals[2 * nb + i]) for i in range(60)]
        script += [(READ, vals[2 * nb - 1]), (INSERT, vals[nb + 5]), (READ, vals[2 * nb + 1]), (INSERT, vals[2 * nb + 2]), (READ, 0)]
        ra = RawAF(imt, len(script))
        assert ra.call(a, *split(script)) == 0
        after = a.insert_batch(vals[2 * nb + 100:2 * nb + 140])
        b.apply_batch(ints_to_arr(vals[:2 * nb]))
        before = state(b)
        rb = RawF(imt, depth, len(script))
        assert rb.call(b, *split(script), 0) == 0
        assert ra.got_status() == rb.got_status() == [NEW] * 60 + [PRESENT, PRESENT, REPEATED, REPEATED, ZERO]
        assert ra.got_leaf() == rb.got_leaf() and ra.counts() == (rb.n_ins.value, rb.n_rd.value) == (40, 20)
        assert arr_ints(ra.got_root()) == [b.root()] == arr_ints(after["old_root"][0])
        want = b.insert_batch(vals[2 * nb + 100:2 * nb + 140])
        for key in want:
            assert (after[key] == want[key]).all(), key
        same_tree(a, b)
        assert a.rewind(before[1]) == before[0] and state(a) == before
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 9. the upper layers
def test_python_wrappers(imt, ctx):
    depth, cap = 32, 256
    vals, stored, script = counts_block()
    script = script[:120]
    status, leaf, acc, sub, inserted = carried_out(stored, script)
    a, b, s = (tree_with(imt, ctx, depth, cap, stored) for _ in range(3))
    try:
        got = a.apply_mixed_filtered(*split(script))
        assert got[0].tolist() == status and got[1].tolist() == leaf and got[2:4] == (len(inserted), len(sub) - len(inserted))
        assert got[4] == b.apply_batch(inserted) == a.root()
        assert s.apply_mixed(*split(sub)) == (len(inserted), a.root()) and state(s) == state(a) == state(b)
        with pytest.raises(ValueError) as e:                   # the block again, on the tree that now holds its INSERTs
            s.apply_mixed([v for _, v in script], [op for op, _ in script])
        assert e.value.bad_op == walk([0] + stored + inserted, script)[1] and state(s) == state(a)
        for wrapper in (s.apply_mixed, s.apply_mixed_filtered):
            with pytest.raises(ValueError):
                wrapper([5, 6], [INSERT])
    finally:
        for t in (a, b, s):
            t.close()


def test_apply_block_example(imt, oracle):
    """examples/apply_block_demo.c applies the block of filtered_block_demo.c without witnesses, prints one line per
    operation and the applied root, then proves the accepted operations through a view and prints their roots"""
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, csrc = os.path.join(root_dir, "examples", "apply_block_demo"), os.path.join(root_dir, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(root_dir, "include"),
                        os.path.join(root_dir, "examples", "apply_block_demo.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    status, _, leaf, _, acc = filtered_walk([0], EXAMPLE_BLOCK)
    assert status == [NEW, NEW, NEW, REPEATED, REPEATED, NEW, NEW, NEW, NEW, ZERO]
    want_ins, want_rd, (root, _) = oracle_walk(oracle, 8, 64, [], [EXAMPLE_BLOCK[p] for p in acc])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    names = {NEW: "carried out", ZERO: "skipped: zero", PRESENT: "skipped: stored before the block", REPEATED: "skipped: spent earlier in the block"}
    for p, ((op, v), s) in enumerate(zip(EXAMPLE_BLOCK, status)):
        assert f"op {p}: {'READ' if op else 'INSERT'} {v}: {names[s]}, leaf {leaf[p]}\n" in r.stdout, (p, r.stdout)
    assert f"{len(want_ins)} inserted, {len(want_rd)} read, {len(EXAMPLE_BLOCK) - len(acc)} skipped; applied root {root:064x}" in r.stdout
    ins, rd = iter(want_ins), iter(want_rd)
    for p in acc:
        line = f"new root {next(ins)['new_root']:064x}" if EXAMPLE_BLOCK[p][0] == INSERT else f"against root {next(rd)['root']:064x}"
        assert f"proved op {p}: {line}\n" in r.stdout, (p, r.stdout)
    assert f"final root {root:064x}" in r.stdout
