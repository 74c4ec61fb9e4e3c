"""GPU: imt_itree_mixed_filtered (include/imt.h) -- a mixed block whose refused operations are skipped with a status.

The definition is the walk of imt_itree_mixed_batch with the operations it would refuse skipped: the plain Python walk of
test_mixed_filter_logic (filtered_walk) says which operations are accepted, with which status and leaf; the rows of the
accepted ones are the sequential oracle's walk (test_gpu_mixed.oracle_walk) over the accepted sub-script.  Every buffer
is filled with a sentinel byte before the call.

  test_oracle_rows           both structs, status, leaf_index, the counts, root, leaves: depths 3, 8, 32, both forms, both layouts
  test_twin_trees            == imt_itree_mixed_batch of the accepted sub-script, all 14 arrays byte for byte (257 operations)
  test_clean_block, test_inserts_only     the two identities: == mixed_batch, == insert_filtered
  test_nothing_changes       nothing accepted, only READs accepted: tree, view and lagged root as before
  test_refusals, test_refused_while_sliced   every error: result, counts 0, tree and ins / rd buffers untouched
  test_formats_and_pointers  MONT256 / DEVICE, device pointers, NULL fields, NULL structs, NULL leaf_index
  test_many_blocks_of_threads, test_one_long_run   2^12 + 3 operations through the oracle-pinned checkers; 1 024 of one value
  test_behind_a_pipelined_batch, test_rewind_and_view_afterwards   the neighbours
  test_python_wrapper, test_filtered_block_example   the upper layers
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
from test_gpu_mixed import INS_FIELDS, RD_FIELDS, SENTINEL, Raw, check_rows, cut, oracle_walk
from test_gpu_rewind import forms  # noqa: F401  (the fixture: one context per hash form)
from test_mixed_filter_logic import HANDWRITTEN, NEW, PRESENT, REPEATED, ZERO, filtered_walk
from test_mixed_logic import ADVERSARIAL, INSERT, READ

pytestmark = pytest.mark.gpu

SENT64 = 0xA5A5A5A5A5A5A5A5


class RawF(Raw):
    """imt_itree_mixed_filtered with buffers of its own, every one pre-filled with the sentinel byte"""

    def __init__(self, imt, depth, n, item_major=False, dev=False, ins_fields=INS_FIELDS, rd_fields=RD_FIELDS, leaf=True):
        super().__init__(imt, depth, n, item_major, dev, ins_fields, rd_fields)
        self.status = self._buf((n,), "status")
        self.leaf = self._buf((n,), "low_index") if leaf else None

    def call(self, t, vals, ops, flags):
        f, lib = self.imt._ffi, self.imt.lib
        if self.dev:
            import torch
            self.keep = (torch.from_numpy(np.ascontiguousarray(vals)).cuda(), torch.from_numpy(np.asarray(ops, np.uint8)).cuda())
            pv, po = (ctypes.c_void_p(x.data_ptr()) for x in self.keep)
            flags |= f.DEVICE_PTRS
        else:
            self.keep = (np.ascontiguousarray(vals), np.asarray(ops, np.uint8))
            pv, po = (x.ctypes.data_as(ctypes.c_void_p) for x in self.keep)
        out = None if self.ins is None else ctypes.byref(f.InsertOut(**{k: self._ptr(x) for k, x in self.ins.items()}))
        rout = None if self.rd is None else ctypes.byref(f.ReadOut(**{k: self._ptr(x) for k, x in self.rd.items()}))
        self.n_ins, self.n_rd = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
        rc = lib.imt_itree_mixed_filtered(t.h, pv, po, self.n, ctypes.c_void_p(self._ptr(self.status)),
                                          None if self.leaf is None else ctypes.c_void_p(self._ptr(self.leaf)), out, rout,
                                          ctypes.byref(self.n_ins), ctypes.byref(self.n_rd), flags)
        if self.dev:
            t.ctx.sync()
            import torch
            torch.cuda.synchronize()
        return rc

    def got_status(self):
        return (self.status.cpu().numpy() if self.dev else self.status).tolist()

    def got_leaf(self):
        return (self.leaf.cpu().numpy().view(np.uint64) if self.dev else self.leaf).tolist()

    def classification_untouched(self):
        return set(self.got_status()) == {SENTINEL} and (self.leaf is None or set(self.got_leaf()) == {SENT64})


def split(script):
    return ints_to_arr([v for _, v in script]), [op for op, _ in script]


def state(t):
    return t.root(), t.size, t.snapshot().tobytes()


def tree_with(imt, c, depth, cap, stored):
    t = imt.IndexedTree(c, depth, cap)
    if len(stored):
        t.apply_batch(stored)
    return t


def noisy_script(rng, stored, fresh, n, max_ins):
    """n operations over fresh values, about a third of them refused: 0, a stored value or a value inserted earlier"""
    script, inserted, pending = [], [], list(fresh)
    for _ in range(n):
        op = READ if rng.random() < 0.45 else INSERT
        if rng.random() < 0.34:
            v = rng.choice([0] + list(stored) + inserted + inserted)
        elif op == INSERT and len(inserted) >= max_ins:
            op, v = READ, rng.choice(pending)
        else:
            v = rng.choice(pending[:12])                      # a small window: READs meet the values inserted later
            if op == INSERT:
                pending.remove(v)
                inserted.append(v)
        script.append((op, v))
    return script


def scripts_for(depth):
    """name -> (stored values, script); the accepted INSERTs of every script fit the capacity 2^min(depth, 7)"""
    cap = 1 << min(depth, 7)
    out = {k: (st[1:], sc) for k, (st, sc) in list(ADVERSARIAL.items()) + list(HANDWRITTEN.items()) if max(x for _, x in sc) < P}
    fresh = [v for v in oracle_lib.synth_values(120, 0x4D464900 + depth) if 0 < v < P]
    rng = random.Random(0x4D4646 + depth)
    out["random"] = (fresh[:2], noisy_script(rng, fresh[:2], fresh[10:], 12 if depth == 3 else 64, 4 if depth == 3 else 40))
    fits = lambda st, sc: 1 + len(st) + sum(script_op == INSERT for script_op, _ in [sc[p] for p in filtered_walk([0] + st, sc)[4]]) <= cap
    return {k: v for k, v in out.items() if fits(*v)}


# ---------------------------------------------------------------- 1. the oracle, row by row
@pytest.mark.parametrize("form", ["thread", "quad"])
@pytest.mark.parametrize("depth", [3, 8, 32])
def test_oracle_rows(imt, forms, oracle, depth, form):
    c, cap = forms[form], 1 << min(depth, 7)
    cases = scripts_for(depth)
    assert len(cases) >= 10 and "random" in cases and "one value 64 times" in cases and "nothing accepted" in cases
    refused = 0
    for j, (name, (stored, script)) in enumerate(cases.items()):
        item_major = bool(j & 1)
        tag = f"{name} depth {depth} {form}"
        status, _, leaf, _, acc = filtered_walk([0] + stored, script)
        refused += len(script) - len(acc)
        sub = [script[p] for p in acc]
        k = sum(op == INSERT for op, _ in sub)
        want_ins, want_rd, (root, pre) = oracle_walk(oracle, depth, cap, stored, sub)
        t = tree_with(imt, c, depth, cap, stored)
        try:
            vals, ops = split(script)
            r = RawF(imt, depth, len(script), item_major)
            assert r.call(t, vals, ops, imt._ffi.SIB_ITEM_MAJOR if item_major else 0) == 0, (tag, imt.lib.imt_last_error(c.h))
            assert (r.n_ins.value, r.n_rd.value) == (k, len(sub) - k), tag
            assert r.got_status() == status and r.got_leaf() == leaf, tag
            ins, rd = cut(r.ins, k, len(script), item_major), cut(r.rd, len(sub) - k, len(script), item_major)
            check_rows(ins, rd, want_ins, want_rd, item_major, tag)
            assert t.root() == root and t.size == pre.shape[0] == imt.lib.imt_itree_size(t.h), tag
            assert (t.snapshot() == pre).all(), tag
        finally:
            t.close()
    assert refused >= 40
    if depth > 3:
        st = filtered_walk([0] + cases["random"][0], cases["random"][1])[0]
        assert 12 <= sum(s != NEW for s in st) <= 32 and {ZERO, PRESENT, REPEATED} <= set(st)


# ---------------------------------------------------------------- 2. twin trees
def block_257():
    vals = [v for v in oracle_lib.synth_values(400, 0x4D464902) if 0 < v < P]
    stored, fresh = vals[:40], vals[40:]
    rng = random.Random(0x4D464902)
    script = [(READ if p % 3 == 1 else INSERT, fresh[p]) for p in range(257)]
    for p in rng.sample(range(8, 257), 60):                    # 60 offenders, ten of each kind at least
        kind, op = p % 3, rng.choice((INSERT, READ))
        earlier = [v for o, v in script[:p] if o == INSERT and v and v not in stored]
        script[p] = (op, (0, rng.choice(stored), rng.choice(earlier))[kind])
    return stored, script


def test_twin_trees(imt, ctx):
    depth, cap = 32, 1024
    stored, script = block_257()
    status, _, leaf, _, acc = filtered_walk([0] + stored, script)
    kinds = {(op, s) for (op, _), s in zip(script, status)}
    assert len(script) == 257 and 50 <= 257 - len(acc) <= 60 and len(kinds) == 8
    sub = [script[p] for p in acc]
    k = sum(op == INSERT for op, _ in sub)
    a, b = tree_with(imt, ctx, depth, cap, stored), tree_with(imt, ctx, depth, cap, stored)
    try:
        ra, rb = RawF(imt, depth, 257), Raw(imt, depth, len(sub))
        assert ra.call(a, *split(script), 0) == 0 and rb.call(b, *split(sub), 0) == 0
        assert (ra.n_ins.value, ra.n_rd.value, rb.n_ins.value) == (k, len(sub) - k, k)
        assert ra.got_status() == status and ra.got_leaf() == leaf
        compared = 0
        for got, want, m in ((ra.ins, rb.ins, k), (ra.rd, rb.rd, len(sub) - k)):
            got, want = cut(got, m, 257, False), cut(want, m, len(sub), False)        # level stride 257 on a, |A| on b
            for key in want:
                assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), key
                compared += 1
        assert compared == 14
        assert state(a) == state(b)
        assert (a.get_proof_batch(np.arange(a.size)) == b.get_proof_batch(np.arange(b.size))).all()
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 3. the identities
def test_clean_block(imt, ctx):
    depth, cap = 32, 1024
    vals = [v for v in oracle_lib.synth_values(330, 0x4D464903) if 0 < v < P]
    stored, script = vals[:30], [(READ if p % 4 == 2 else INSERT, vals[30 + p]) for p in range(257)]
    script[7], script[9] = (READ, vals[30 + 200]), (READ, vals[30 + 200])          # two READs of a value inserted later
    a, b = tree_with(imt, ctx, depth, cap, stored), tree_with(imt, ctx, depth, cap, stored)
    try:
        v, ops = split(script)
        ins, rd, status, leaf = a.mixed_filtered(v, ops)
        want_ins, want_rd = b.mixed_batch(v, ops)
        assert (status == NEW).all()
        for got, want in ((ins, want_ins), (rd, want_rd)):
            assert set(got) == set(want)
            for key in want:
                assert got[key].shape == want[key].shape and (got[key] == want[key]).all(), key
        is_rd = np.array(ops) == READ
        assert (leaf[is_rd] == rd["low_index"]).all() and (leaf[~is_rd] == ins["new_index"]).all()
        assert state(a) == state(b)
    finally:
        a.close()
        b.close()


def test_inserts_only(imt, ctx):
    depth, cap, n = 32, 1024, 257
    vals = [v for v in oracle_lib.synth_values(n + 20, 0x4D464904) if 0 < v < P]
    stored, block = vals[:20], list(vals[20:20 + n])
    rng = random.Random(0x4D464904)
    for p in rng.sample(range(5, n), 45):
        block[p] = (0, rng.choice(stored), block[rng.randrange(p)])[p % 3]
    a, b = tree_with(imt, ctx, depth, cap, stored), tree_with(imt, ctx, depth, cap, stored)
    try:
        ins, rd, status, leaf = a.mixed_filtered(block, [INSERT] * n)
        want = b.insert_filtered(block)
        assert {ZERO, PRESENT, REPEATED, NEW} == set(want["status"].tolist())
        assert (status == want["status"]).all() and (leaf == want["leaf_index"]).all()
        assert ins["low_index"].shape[0] == want["n_inserted"] < n and rd["low_index"].shape[0] == 0
        for key in INS_FIELDS + ("new_index",):
            assert ins[key].shape == want[key].shape and (ins[key] == want[key]).all(), key
        assert state(a) == state(b)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 4. blocks that change nothing
def test_nothing_changes(imt, ctx):
    depth, cap = 32, 1024
    vals = [v for v in oracle_lib.synth_values(500, 0x4D464905) if 0 < v < P]
    t = imt.IndexedTree(ctx, depth, cap)
    try:
        t.apply_batch(vals[:150])
        v = t.view(100)
        v.root()
        t.insert_batch(vals[150:250])
        view_root, builds = v.root(), v.stats()[1]
        before, proofs = state(t), t.get_proof_batch(np.arange(t.size))
        lagged = np.zeros(32, np.uint8)
        assert imt.lib.imt_itree_root_lagged(t.h, 0, lagged.ctypes.data_as(ctypes.c_void_p), 0) == 0
        nothing = [(p & 1, (0, vals[p], vals[100 + p])[p % 3]) for p in range(90)]
        reads = [(READ, vals[300 + p]) for p in range(60)] + [(INSERT, vals[p]) for p in range(20)] + [(READ, 0), (INSERT, 0)]
        low, leaves, sib, largest = t.non_membership_witness(vals[300:360])
        for script, n_rd in ((nothing, 0), (reads, 60)):
            r = RawF(imt, depth, len(script))
            assert r.call(t, *split(script), 0) == 0 and (r.n_ins.value, r.n_rd.value) == (0, n_rd)
            status, _, leaf, _, acc = filtered_walk([0] + vals[:250], script)
            assert len(acc) == n_rd and r.got_status() == status and r.got_leaf() == leaf
            assert all((a.view(np.uint8) == SENTINEL).all() for a in r.ins.values())
            rd = cut(r.rd, n_rd, len(script), False)
            if n_rd:
                assert (rd["low_index"] == low).all() and (rd["low_leaf"] == leaves).all() and (rd["is_largest"] == largest).all()
                assert (rd["low_sib"] == sib).all() and arr_ints(rd["root"]) == [before[0]] * n_rd
            assert state(t) == before and (t.get_proof_batch(np.arange(t.size)) == proofs).all()
            assert v.root() == view_root and v.stats()[1] == builds          # not counted as a change: the view stays fresh
            again = np.zeros(32, np.uint8)
            assert imt.lib.imt_itree_root_lagged(t.h, 0, again.ctypes.data_as(ctypes.c_void_p), 0) == 0 and (again == lagged).all()
        t.insert_batch([vals[400]])                                         # and the tree goes on as if nothing had been asked
        assert t.size == before[1] + 1
        v.close()
    finally:
        t.close()


# ---------------------------------------------------------------- 5. refusals
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
            was = before if tree is t else state(tree)
            r = RawF(imt, tree.depth, len(script), bool(flags & f.SIB_ITEM_MAJOR), dev)
            rc = r.call(tree, *split(script), flags)
            assert rc == want_rc, (tag, script, rc, lib.imt_last_error(c.h))
            assert r.untouched() and (r.n_ins.value, r.n_rd.value) == (0, 0), (tag, script)
            if classified:
                assert r.got_status() == filtered_walk([0] + stored, script)[0], (tag, script)
            else:
                assert r.classification_untouched(), (tag, script)
            assert state(tree) == was, (tag, script)

        # IMT_ERR_NONCANONICAL: malformed input, whatever else the block holds; status is the classification
        refused([(READ, 7), (READ, P), (INSERT, 0), (INSERT, 20)], E["NONCANONICAL"], classified=True)
        refused([(INSERT, P + 1), (READ, 7), (INSERT, 7), (READ, 7)], E["NONCANONICAL"], dev=True, classified=True)
        # IMT_ERR_FULL counts the accepted INSERTs only
        room = cap - t.size
        full = [(INSERT, 1000 + i) for i in range(room + 1)]
        refused(full, E["FULL"], classified=True)
        refused([(READ, 500 + i) for i in range(80)] + full + [(INSERT, 1000), (INSERT, 0)], E["FULL"], dev=True, classified=True)
        twin = imt.IndexedTree(c, depth, cap)
        twin.apply_batch(stored)
        fits = full[:room] + [(INSERT, 1000 + i) for i in range(room)] + [(INSERT, 10), (INSERT, 0)] + [(READ, 500 + i) for i in range(2 * cap)]
        assert sum(op == INSERT for op, _ in fits) > room               # the raw INSERTs exceed the room, the accepted ones fill it
        ins, rd, status, leaf = twin.mixed_filtered(*split(fits), proofs=False)
        assert twin.size == cap and ins["low_index"].shape[0] == room and rd["root"].shape[0] == 2 * cap
        assert status.tolist() == [NEW] * room + [REPEATED] * room + [PRESENT, ZERO] + [NEW] * (2 * cap)
        twin.close()
        # IMT_ERR_ARG: op bytes through both kinds of pointer, NULL arguments, flags, misaligned device buffers
        for dev in (False, True):
            for ops in ([0, 2], [255, 1]):
                r = RawF(imt, depth, 2, False, dev)
                assert r.call(t, ints_to_arr([5, 6]), ops, 0) == E["ARG"] and r.untouched() and r.classification_untouched()
                assert (r.n_ins.value, r.n_rd.value) == (0, 0)
        ok = [(INSERT, 5), (READ, 6)]
        for flags in (f.PIPELINE, f.PIPELINE | f.DEVICE_PTRS, f.HOST_PREP, f.INPUTS_READY | f.DEVICE_PTRS, 3):
            refused(ok, E["ARG"], flags=flags, dev=bool(flags & f.DEVICE_PTRS))
        one, op1, st1 = ints_to_arr([5]), np.zeros(1, np.uint8), np.full(1, SENTINEL, np.uint8)
        pv, po, ps = (x.ctypes.data_as(ctypes.c_void_p) for x in (one, op1, st1))
        k1, k2 = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
        n1, n2 = ctypes.byref(k1), ctypes.byref(k2)
        call = lib.imt_itree_mixed_filtered
        assert call(t.h, None, po, 1, ps, None, None, None, n1, n2, 0) == E["ARG"]
        assert call(t.h, pv, None, 1, ps, None, None, None, n1, n2, 0) == E["ARG"]
        assert call(t.h, pv, po, 1, None, None, None, None, n1, n2, 0) == E["ARG"]
        assert call(t.h, pv, po, 1, ps, None, None, None, None, n2, 0) == E["ARG"]
        assert call(t.h, pv, po, 1, ps, None, None, None, n1, None, 0) == E["ARG"]
        assert call(None, pv, po, 1, ps, None, None, None, n1, n2, 0) == E["ARG"]
        assert st1[0] == SENTINEL
        k1.value = k2.value = 0xDEAD
        assert call(t.h, None, None, 0, ps, None, None, None, n1, n2, 0) == 0 and (k1.value, k2.value) == (0, 0)       # n == 0
        dbuf = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
        dvals = torch.from_numpy(ints_to_arr([5, 6])).cuda()
        dops = torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
        at = lambda off: dbuf.data_ptr() + off
        dv, do, dst = (ctypes.c_void_p(x) for x in (dvals.data_ptr(), dops.data_ptr(), at(2048)))
        for ins_kw, rd_kw in ((dict(new_root=at(8)), {}), (dict(low_sib=at(24)), {}), ({}, dict(root=at(8))), ({}, dict(low_sib=at(4))),
                              ({}, dict(low_leaf=at(40))), (dict(low_index=at(4)), {}), ({}, dict(low_index=at(12)))):
            rc = call(t.h, dv, do, 2, dst, None, ctypes.byref(f.InsertOut(**ins_kw)), ctypes.byref(f.ReadOut(**rd_kw)), n1, n2, f.DEVICE_PTRS)
            assert rc == E["ARG"], (ins_kw, rd_kw)
        assert call(t.h, dv, do, 2, dst, ctypes.c_void_p(at(1028)), None, None, n1, n2, f.DEVICE_PTRS) == E["ARG"]      # leaf_index
        assert call(t.h, ctypes.c_void_p(dvals.data_ptr() + 8), do, 1, dst, None, None, None, n1, n2, f.DEVICE_PTRS) == E["ARG"]
        c.sync()
        assert (dbuf.cpu().numpy() == SENTINEL).all() and state(t) == before
        # a placed tree, a partitioned tree
        placed = imt.IndexedTree(c, 8, 64)
        placed.set_placement(10, 1)
        refused(ok, E["ARG"], tree=placed)
        placed.close()
        part = imt.IndexedTree(c, depth, cap)
        c._check(lib.imt_itree_set_value_partition(part.h, 3, 1))
        refused([(INSERT, 4), (READ, 7)], E["ARG"], tree=part)
        assert part.size == 1
        part.close()
        # between imt_itree_batch_begin and _end; an open slice
        ev, l0 = ctypes.c_uint32(), ctypes.c_uint32()
        more = ints_to_arr([71, 72, 73, 74])
        assert lib.imt_itree_batch_begin(t.h, more.ctypes.data_as(ctypes.c_void_p), 4, 0, ctypes.byref(ev), ctypes.byref(l0)) == 0
        r = RawF(imt, depth, 2)
        assert r.call(t, ints_to_arr([5, 6]), [0, 1], 0) == E["ARG"] and r.untouched() and r.classification_untouched()
        assert lib.imt_itree_batch_abort(t.h) == 0
        assert state(t) == before
        dv8 = torch.from_numpy(ints_to_arr([81, 82, 83, 84, 85, 86, 87, 88])).cuda()
        pay = torch.zeros(int(lib.imt_itree_slice_payload_bytes(8)) + 64, dtype=torch.uint8, device="cuda")
        sl = ctypes.c_int(-1)
        assert lib.imt_itree_slice_prepare(t.h, ctypes.c_void_p(dv8.data_ptr()), 0, 8, 0, None, f.DEVICE_PTRS, ctypes.byref(sl), None) == 0
        r = RawF(imt, depth, 2)
        assert r.call(t, ints_to_arr([5, 6]), [0, 1], 0) == E["ARG"] and r.untouched() and r.classification_untouched()
        for q in range(depth + 1):
            assert lib.imt_itree_slice_unit(t.h, sl.value, q, ctypes.c_void_p(pay.data_ptr()), None) == 0
        c.sync()
        assert t.size == before[1] + 8
        ins, rd, status, leaf = t.mixed_filtered([5, 6, 5], [INSERT, READ, READ])          # and afterwards the call works
        assert status.tolist() == [NEW, NEW, REPEATED] and leaf.tolist() == [t.size - 1, t.size - 1, t.size - 1]
    finally:
        t.close()


def test_refused_while_sliced(imt, ctx):
    """world 2 over the local transport: a replica with steps in flight takes no filtered block, after the flush it does"""
    import torch
    import test_gpu_sliced as ts
    sl = ts.load_sliced()
    depth, cap, world, batch = 32, 1 << 10, 2, 40
    vals = oracle_lib.synth_values(world * batch + 4, 0x4D464953)
    w = sl.SlicedTree(imt, 0, depth, cap, batch, world, n_local=world, nbuf=8)
    try:
        w.step(torch.from_numpy(ints_to_arr(vals[:world * batch])).cuda())
        for t in w.trees:
            r = RawF(imt, depth, 2)
            assert r.call(t, ints_to_arr(vals[-2:]), [0, 1], 0) == imt._ffi.ERR["ARG"] and r.untouched()
            assert r.classification_untouched() and (r.n_ins.value, r.n_rd.value) == (0, 0)
        w.flush()
        roots = {t.root() for t in w.trees}
        assert len(roots) == 1
        ins, rd, status, leaf = w.trees[0].mixed_filtered([vals[-2], vals[-1], vals[0]], [READ, INSERT, INSERT])
        assert status.tolist() == [NEW, NEW, PRESENT] and arr_ints(rd["root"]) == list(roots)
        assert w.trees[0].size == world * batch + 2
    finally:
        w.close()


# ---------------------------------------------------------------- 6. formats and pointers
def test_formats_and_pointers(imt, forms):
    c, f = forms["default"], imt._ffi
    depth, cap = 32, 256
    vals = [v for v in oracle_lib.synth_values(120, 0x4D464906) if 0 < v < P]
    stored, script = vals[:30], [(READ if i % 3 == 1 else INSERT, vals[40 + i]) for i in range(50)]
    script += [(READ, vals[41]), (READ, vals[100]), (INSERT, 0), (READ, vals[3]), (INSERT, vals[40]), (READ, vals[42]), (READ, 0),
               (INSERT, vals[7])]
    v_arr, ops = split(script)
    n = len(script)
    want_status, _, want_leaf, _, acc = filtered_walk([0] + stored, script)
    k = sum(script[p][0] == INSERT for p in acc)
    m = len(acc) - k
    assert 0 < k and 0 < m and len(acc) == n - 6
    trees = []

    def fresh():
        trees.append(tree_with(imt, c, depth, cap, stored))
        return trees[-1]

    try:
        ref = fresh()
        want_ins, want_rd, status, leaf = ref.mixed_filtered(v_arr, ops)
        assert status.tolist() == want_status and leaf.tolist() == want_leaf
        want_ins.pop("new_index")
        final = state(ref)
        lm = lambda a: a.transpose(1, 0, 2)                       # [depth][rows] -> [rows][depth]
        for fmt, item_major, dev in ((f.FMT_MONT256, True, False), (f.FMT_DEVICE, False, False), (f.FMT_CANONICAL, False, True),
                                     (f.FMT_MONT256, False, True), (f.FMT_DEVICE, True, True)):
            tag = f"fmt {fmt} item_major {item_major} dev {dev}"
            t, r = fresh(), RawF(imt, depth, n, item_major, dev)
            assert r.call(t, tm.to_fmt(v_arr, fmt), ops, fmt | (f.SIB_ITEM_MAJOR if item_major else 0)) == 0, tag
            assert (r.n_ins.value, r.n_rd.value) == (k, m) and state(t) == final, tag
            assert r.got_status() == want_status and r.got_leaf() == want_leaf, tag
            for got, want, rows in ((cut(r.host(r.ins), k, n, item_major), want_ins, k), (cut(r.host(r.rd), m, n, item_major), want_rd, m)):
                for key, a in got.items():
                    w = want[key]
                    if key.endswith("_sib") and item_major:
                        w = lm(w)
                    if key not in ("low_index", "is_largest"):
                        w = tm.to_fmt(np.ascontiguousarray(w), fmt)
                    assert a.shape == w.shape and (a == w).all(), f"{tag}: {key}"
        # NULL fields are skipped, either struct may be missing altogether, and so may leaf_index
        for ins_f, rd_f, dev, with_leaf in ((("new_root", "low_sib"), ("root",), False, True), (None, RD_FIELDS, True, False),
                                            (INS_FIELDS, None, False, False), (None, None, True, True),
                                            (("is_largest",), ("low_sib", "low_index"), True, True)):
            tag = f"fields {ins_f} {rd_f} dev {dev} leaf {with_leaf}"
            t, r = fresh(), RawF(imt, depth, n, False, dev, ins_f, rd_f, with_leaf)
            assert r.call(t, v_arr, ops, 0) == 0 and (r.n_ins.value, r.n_rd.value) == (k, m), tag
            assert state(t) == final and r.got_status() == want_status and (not with_leaf or r.got_leaf() == want_leaf), tag
            for got, want, rows in ((r.host(r.ins), want_ins, k), (r.host(r.rd), want_rd, m)):
                for key, a in (cut(got, rows, n, False) if got else {}).items():
                    assert (a == want[key]).all(), f"{tag}: {key}"
    finally:
        for t in trees:
            t.close()


# ---------------------------------------------------------------- 7. more than one block of threads, one long run
def test_many_blocks_of_threads(imt, forms):
    """2^12 + 3 operations on 2^13 leaves: 17 blocks of threads and more than one merge-sort tile.  About an eighth refused,
    of every kind; status and leaf_index against the walk, the rows through the two oracle-pinned checkers, the chain of
    roots, the final tree against a twin that applied the accepted INSERTs"""
    c = forms["default"]
    depth, cap, M, n = 32, 1 << 14, 1 << 13, (1 << 12) + 3
    vals = [v for v in oracle_lib.synth_values(M + n + 40, 0x4D464907) if 0 < v < P]
    base, fresh = vals[:M - 1], vals[M - 1:]
    rng = random.Random(0x4D464907)
    script = [(READ if p % 4 == 3 else INSERT, fresh[p]) for p in range(n)]
    for p in rng.sample(range(16, n), n // 8):
        kind, op = p % 3, rng.choice((INSERT, READ))
        script[p] = (op, (0, rng.choice(base), fresh[4 * rng.randrange(p // 4)])[kind])
    status, _, leaf, _, acc = filtered_walk([0] + base, script)
    assert {(op, s) for (op, _), s in zip(script, status)} == {(o, s) for o in (INSERT, READ) for s in (NEW, ZERO, PRESENT, REPEATED)}
    assert n // 10 <= n - len(acc) <= n // 8
    a, b = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    try:
        for t in (a, b):
            t.apply_batch(ints_to_arr(base))
        root0 = a.root()
        v_arr, ops = split(script)
        ins, rd, got_status, got_leaf = a.mixed_filtered(v_arr, ops)
        assert got_status.tolist() == status and got_leaf.tolist() == leaf
        sub_ops = np.array([script[p][0] for p in acc], np.uint8)
        sub_vals = v_arr[acc]
        k = int((sub_ops == INSERT).sum())
        assert ins["low_index"].shape[0] == k and rd["low_index"].shape[0] == len(acc) - k
        fail = c.non_membership(rd["root"], rd["low_leaf"], rd["low_index"], rd["low_sib"], depth, sub_vals[sub_ops == READ], rd["is_largest"])
        assert not fail.any(), np.nonzero(fail)[0][:5]
        fail = c.insert_witness(ins["old_root"], ins["low_leaf"], ins["low_index"], ins["low_sib"], ins["new_root"], ins["new_leaf"],
                                ins["new_index"], ins["new_sib"], ins["is_largest"], depth)
        assert not fail.any(), np.nonzero(fail)[0][:5]
        assert arr_ints(ins["old_root"][0]) == [root0] and (ins["old_root"][1:] == ins["new_root"][:-1]).all()
        ranks = np.cumsum(sub_ops == INSERT)[sub_ops == READ]
        assert (ranks > 0).all() and (rd["root"] == ins["new_root"][ranks - 1]).all()
        assert (sub_vals[sub_ops == INSERT] == ins["new_leaf"][:, 0]).all()
        assert b.apply_batch(sub_vals[sub_ops == INSERT]) == a.root() == arr_ints(ins["new_root"][-1])[0]
        assert a.size == b.size == M + k and (a.snapshot() == b.snapshot()).all()
    finally:
        a.close()
        b.close()


def test_one_long_run(imt, ctx):
    """1 024 operations on one value -- READ, INSERT, then alternating: no thread may walk the run"""
    depth, cap, n = 32, 64, 1024
    t = imt.IndexedTree(ctx, depth, cap)
    try:
        t.apply_batch([10, 90])
        script = [(READ, 50), (INSERT, 50)] + [(p & 1, 50) for p in range(n - 2)]
        ins, rd, status, leaf = t.mixed_filtered(*split(script), proofs=False)
        assert status.tolist() == [NEW, NEW] + [REPEATED] * (n - 2) and leaf.tolist() == [1] + [3] * (n - 1)
        assert ins["low_index"].tolist() == [1] and rd["low_index"].tolist() == [1] and t.size == 4
    finally:
        t.close()


# ---------------------------------------------------------------- 8. neighbours
def test_behind_a_pipelined_batch(imt, forms):
    """a filtered block right behind pipelined insert batches still in flight orders itself behind them"""
    import torch
    c, f, lib = forms["default"], imt._ffi, imt.lib
    depth, cap, nb = 32, 1 << 14, 2048
    vals = [v for v in oracle_lib.synth_values(3 * nb + 60, 0x4D464908) if 0 < v < P]
    a, b = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    try:
        d = torch.from_numpy(ints_to_arr(vals[:3 * nb])).cuda()
        for j in range(3):
            part = d[j * nb:(j + 1) * nb]
            assert lib.imt_itree_insert_batch(a.h, ctypes.c_void_p(part.data_ptr()), nb, None, f.DEVICE_PTRS | f.PIPELINE) == 0
        script = [(READ if i % 3 == 0 else INSERT, vals[3 * nb + i]) for i in range(40)]
        script += [(READ, vals[3 * nb - 1]), (INSERT, vals[2 * nb + 5]), (READ, vals[3 * nb + 1]), (INSERT, vals[3 * nb + 2])]
        v_arr, ops = split(script)
        ins, rd, status, leaf = a.mixed_filtered(v_arr, ops)
        b.apply_batch(ints_to_arr(vals[:3 * nb]))
        want_ins, want_rd = b.mixed_batch(v_arr[:40], ops[:40])
        assert status.tolist() == [NEW] * 40 + [PRESENT, PRESENT, REPEATED, REPEATED]
        assert leaf[40:].tolist() == [3 * nb, 2 * nb + 6, int(ins["new_index"][0]), int(ins["new_index"][1])]
        for key in want_ins:
            assert (ins[key] == want_ins[key]).all(), key
        for key in want_rd:
            assert (rd[key] == want_rd[key]).all(), key
        assert state(a) == state(b)
    finally:
        a.close()
        b.close()


def test_rewind_and_view_afterwards(imt, ctx):
    """a view at the size before a filtered block replays its INSERT rows; a rewind to that size gives the tree back"""
    depth, cap = 32, 1024
    vals = [v for v in oracle_lib.synth_values(400, 0x4D464909) if 0 < v < P]
    t = imt.IndexedTree(ctx, depth, cap)
    try:
        t.apply_batch(vals[:100])
        before = state(t)
        script = [(READ if i % 4 == 1 else INSERT, vals[100 + i] if i % 9 else (0, vals[i], vals[100 + i - 1])[i % 3]) for i in range(200)]
        v_arr, ops = split(script)
        ins, rd, status, leaf = t.mixed_filtered(v_arr, ops)
        k = ins["low_index"].shape[0]
        assert 0 < k and (status != NEW).sum() >= 15 and t.size == before[1] + k
        v = t.view(before[1])
        assert v.root() == before[0]
        replay = v.insert_witness(k)
        for key in INS_FIELDS + ("new_index",):
            assert (replay[key] == ins[key]).all(), key
        v.close()
        lagged = np.zeros(32, np.uint8)
        assert imt.lib.imt_itree_root_lagged(t.h, 0, lagged.ctypes.data_as(ctypes.c_void_p), 0) == 0
        assert arr_ints(lagged) == [t.root()]
        assert t.rewind(before[1]) == before[0] and state(t) == before
        ins2, rd2, status2, leaf2 = t.mixed_filtered(v_arr, ops)
        assert all((ins2[key] == ins[key]).all() for key in ins) and all((rd2[key] == rd[key]).all() for key in rd)
        assert (status2 == status).all() and (leaf2 == leaf).all()
    finally:
        t.close()


# ---------------------------------------------------------------- 9. the upper layers
def test_python_wrapper(imt, ctx):
    depth, cap = 32, 256
    stored, script = block_257()
    script = script[:120]
    for item_major in (False, True):
        a, b = tree_with(imt, ctx, depth, cap, stored), tree_with(imt, ctx, depth, cap, stored)
        try:
            ins, rd, status, leaf = a.mixed_filtered(*split(script), item_major=item_major)
            r = RawF(imt, depth, len(script), item_major)
            assert r.call(b, *split(script), imt._ffi.SIB_ITEM_MAJOR if item_major else 0) == 0
            assert status.tolist() == r.got_status() and leaf.tolist() == r.got_leaf()
            assert (ins["low_index"].shape[0], rd["low_index"].shape[0]) == (r.n_ins.value, r.n_rd.value)
            for got, raw, m in ((ins, r.ins, r.n_ins.value), (rd, r.rd, r.n_rd.value)):
                for key, w in cut(raw, m, len(script), item_major).items():
                    assert got[key].shape == w.shape and (got[key] == w).all(), key
            assert ins["new_index"].tolist() == list(range(1 + len(stored), a.size)) and state(a) == state(b)
            no_proofs = tree_with(imt, ctx, depth, cap, stored)
            ins2, rd2, status2, _ = no_proofs.mixed_filtered(*split(script), proofs=False)
            assert "low_sib" not in ins2 and "low_sib" not in rd2 and (status2 == status).all() and state(no_proofs) == state(a)
            no_proofs.close()
        finally:
            a.close()
            b.close()
    with pytest.raises(ValueError):
        t = imt.IndexedTree(ctx, depth, cap)
        try:
            t.mixed_filtered([5, 6], [INSERT])
        finally:
            t.close()


EXAMPLE_BLOCK = list(zip([0, 1, 0, 0, 1, 0, 1, 0, 1, 0], [30, 45, 10, 30, 10, 70, 65, 45, 25, 0]))


def test_filtered_block_example(imt, oracle):
    """examples/filtered_block_demo.c plays a block with a double spend (30), a READ of a value spent two transactions
    earlier (10) and a READ of a value spent later (45), prints one line per operation and the final root"""
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, csrc = os.path.join(root_dir, "examples", "filtered_block_demo"), os.path.join(root_dir, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(root_dir, "include"),
                        os.path.join(root_dir, "examples", "filtered_block_demo.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    status, _, leaf, _, acc = filtered_walk([0], EXAMPLE_BLOCK)
    assert status == [NEW, NEW, NEW, REPEATED, REPEATED, NEW, NEW, NEW, NEW, ZERO]
    want_ins, want_rd, (root, _) = oracle_walk(oracle, 8, 64, [], [EXAMPLE_BLOCK[p] for p in acc])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    names = {NEW: "carried out", ZERO: "skipped: zero", PRESENT: "skipped: stored before the block", REPEATED: "skipped: spent earlier in the block"}
    for p, ((op, v), s) in enumerate(zip(EXAMPLE_BLOCK, status)):
        assert f"op {p}: {'READ' if op else 'INSERT'} {v}: {names[s]}, leaf {leaf[p]}" in r.stdout, (p, r.stdout)
    for o in want_ins:
        assert f"new root {o['new_root']:064x}" in r.stdout, r.stdout
    for o in want_rd:
        assert f"against root {o['root']:064x}" in r.stdout, r.stdout
    assert f"final root {root:064x}" in r.stdout
    assert f"{len(want_ins)} inserted, {len(want_rd)} read, {len(EXAMPLE_BLOCK) - len(acc)} skipped" in r.stdout
