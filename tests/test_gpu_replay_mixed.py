"""GPU: imt_itree_view_mixed_witness (include/imt.h) -- the witnesses of a mixed block the tree has already applied.

The definition is a fresh tree: fed the first size - 1 values the tree holds, imt_itree_mixed_batch of the list writes what
this call writes, byte for byte, provided the INSERTs of the list are the values the tree holds from `size` on.  So the
expectation is test_gpu_mixed's walk on the sequential oracle over the STORED PREFIX, while the tree under test has applied
the block's insertions witness-free and has been built upon.

  test_oracle_rows            depths 3, 8, 32, both kernel forms, both layouts, every accepted script of test_gpu_mixed:
                              every field of both output structs; the tree as it was; one build
  test_twin                   4096 + 1 leaves, 1024 operations with a READ at every fourth, 1024 later insertions: replay
                              against live imt_itree_mixed_batch on a twin, on three contexts; READ events read their
                              sibling from every source (asserted from the order of the values alone)
  test_identities             INSERTs only, READs only, the view's root, a READ of a tail value, n == 0, the view at the
                              current size
  test_refusals               every refusal: result, *bad_op, outputs, tree and view untouched
  test_refused_while_sliced   a replica of a sliced world with steps in flight
  test_formats_and_pointers   MONT256 / DEVICE, item-major, host and device pointers, NULL fields, ins == NULL, rd == NULL
  test_follows                behind pipelined batches in flight, after a live mixed batch, two views on consecutive blocks
  test_example                examples/late_block_demo.c: its roots against the oracle's
"""
import bisect
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import test_gpu_insert_matrix as tm
import test_gpu_mixed as tg
from oracle_lib import P, arr_ints, ints_to_arr
from test_gpu_mixed import INS_FIELDS, RD_FIELDS, check_rows, oracle_walk, scripts_for
from test_gpu_rewind import forms  # noqa: F401  (the fixture: one context per hash form)
from test_mixed_logic import ADVERSARIAL, INSERT, READ, walk

pytestmark = pytest.mark.gpu

EMPTY, SIDE, STORED, BATCH = 0, 1, 2, 3


def split(script):
    return [v for _, v in script], [op for op, _ in script]


def inserts_of(script):
    return [v for op, v in script if op == INSERT]


def tail_for(stored, script, room, pool):
    """up to `room` later values, none of them in the tree; the first one lands right above a kept value, so it relinks a
    kept leaf (its low leaf is a leaf of the view)"""
    if room <= 0:
        return []
    present = {0} | set(stored) | set(inserts_of(script))
    order = sorted(present)
    first = None
    for k in sorted({0} | set(stored), reverse=True):
        v = k + 1
        if v not in present and v < P and order[bisect.bisect_left(order, v) - 1] == k:
            first = v
            break
    assert first is not None
    rest = [v for v in pool if v not in present and v != first]
    return [first] + rest[:min(room - 1, 12)]


def tree_state(t):
    return t.root(), t.size, t.snapshot().tobytes()


# ---------------------------------------------------------------- 1. the oracle, row by row
_walks = {}


def walk_of(oracle, depth, cap, name, stored, script):
    key = (depth, name)
    if key not in _walks:
        _walks[key] = oracle_walk(oracle, depth, cap, stored, script)[:2]
    return _walks[key]


@pytest.mark.parametrize("form", ["thread", "quad"])
@pytest.mark.parametrize("depth", [3, 8, 32])
def test_oracle_rows(imt, forms, oracle, depth, form):
    c, cap = forms[form], 1 << min(depth, 7)
    cases = scripts_for(depth)
    assert len(cases) >= 8
    pool = [v for v in oracle_lib.synth_values(40, 0x564D4F00 + depth) if 0 < v < P]
    relinking = 0
    for j, (name, (stored, script)) in enumerate(cases.items()):
        item_major = bool(j & 1)
        tag = f"{name} depth {depth} {form}"
        want_ins, want_rd = walk_of(oracle, depth, cap, name, stored, script)
        t = imt.IndexedTree(c, depth, cap)
        try:
            if stored:
                t.apply_batch(stored)
            if inserts_of(script):
                t.apply_batch(inserts_of(script))
            tail = tail_for(stored, script, cap - t.size, pool)
            if tail:
                t.apply_batch(tail)
                relinking += 1
            before = tree_state(t)
            s = 1 + len(stored)
            v = t.view(s)
            ins, rd = v.mixed_witness(*split(script), item_major=item_major)
            check_rows(ins, rd, want_ins, want_rd, item_major, tag)
            assert ins["new_index"].tolist() == list(range(s, s + len(want_ins))), tag
            assert tree_state(t) == before, tag
            assert v.stats()[1] == 1, tag
            v.close()
        finally:
            t.close()
    assert relinking >= (1 if depth == 3 else 8)


# ---------------------------------------------------------------- 2. against a live twin, every sibling source
TWIN = dict(depth=32, cap=1 << 14, base=4096, n=1024, tail=1024, seed=0x564D5831)


def twin_values():
    """(base, script, tail): a READ at every fourth position; the READs in turn of a value nobody ever inserts, of a value
    a later INSERT of the block puts in, of a value nobody inserts, of a value the tail puts in"""
    base_n, n, tail_n = TWIN["base"], TWIN["n"], TWIN["tail"]
    n_rd = n // 4
    n_ins = n - n_rd
    allv = oracle_lib.synth_values(base_n + n_ins + tail_n + n_rd, TWIN["seed"])
    base, block = allv[:base_n], allv[base_n:base_n + n_ins]
    tail, never = allv[base_n + n_ins:base_n + n_ins + tail_n], allv[base_n + n_ins + tail_n:]
    script, r = [], 0
    for p in range(n):
        if p % 4 != 3:
            script.append((INSERT, block[r]))
            r += 1
            continue
        q = p // 4
        if q % 2 == 0:
            v = never[q]
        elif q % 4 == 1 and r + 7 < n_ins:
            v = block[r + 7]                    # inserted a few operations later
        else:
            v = tail[(q * 37) % tail_n]
        script.append((READ, v))
    return base, script, tail


def read_coverage(base, script, tail, levels):
    """From the sorted order of the values alone: per level l < levels, how many READ events of the replay read their
    sibling from each source (replay_coverage of test_gpu_replay, over the events of a mixed list)."""
    s = 1 + len(base)
    order = [(0, 0)] + sorted((v, i + 1) for i, v in enumerate(base))
    pos, is_read, n_ins = [], [], 0
    for op, v in script:
        k = bisect.bisect_left(order, (v, -1))
        assert v != 0 and (k == len(order) or order[k][0] != v)
        pos.append(order[k - 1][1])
        is_read.append(op == READ)
        if op == INSERT:
            pos.append(s + n_ins)
            is_read.append(False)
            order.insert(k, (v, s + n_ins))
            n_ins += 1
    # S_0: the kept leaves whose successor in the tree of everything is not kept, and slot s
    full = [0] + list(base) + inserts_of(script) + list(tail)
    by_val = sorted(range(len(full)), key=full.__getitem__)
    S = {s} | {by_val[j] for j in range(len(by_val) - 1) if by_val[j] < s <= by_val[j + 1]}
    out = []
    for l in range(levels):
        fill = -(-s // (1 << l))
        seen, count = set(), {BATCH: 0, EMPTY: 0, SIDE: 0, STORED: 0}
        for p, rd in zip(pos, is_read):
            y = (p >> l) ^ 1
            cls = BATCH if y in seen else EMPTY if y >= fill else SIDE if y in S else STORED
            seen.add(p >> l)
            if rd:
                count[cls] += 1
        out.append(count)
        S = {x >> 1 for x in S}
    return out


def test_twin(imt, forms):
    depth, cap = TWIN["depth"], TWIN["cap"]
    base, script, tail = twin_values()
    assert len(script) == 1024 and sum(op == READ for op, _ in script) == 256
    cover = read_coverage(base, script, tail, 13)               # L0 = ceil_log2(4097 + 768) = 13
    for l in range(4):
        assert all(cover[l][k] > 0 for k in (BATCH, SIDE, STORED)), f"level {l}: READ events by source {cover[l]}"
    assert any(c[EMPTY] > 0 for c in cover), "no READ event meets an empty sibling"
    vals, ops = split(script)
    v_arr = ints_to_arr(vals)
    s = 1 + len(base)
    b = imt.IndexedTree(forms["default"], depth, cap)
    try:
        b.apply_batch(ints_to_arr(base))
        want_ins, want_rd = b.mixed_batch(v_arr, ops)
        for form in ("default", "thread", "quad"):
            a = imt.IndexedTree(forms[form], depth, cap)
            try:
                a.apply_batch(ints_to_arr(base))
                a.apply_batch(ints_to_arr(inserts_of(script)))
                assert a.root() == b.root()
                head = a.apply_batch(ints_to_arr(tail))
                view = a.view(s)
                ins, rd = view.mixed_witness(v_arr, ops)
                for got, want in ((ins, want_ins), (rd, want_rd)):
                    assert set(got) == set(want)
                    for k in want:
                        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), f"{form}: {k}"
                assert a.root() == head and a.size == s + 768 + len(tail) and view.stats()[1] == 1
                view.close()
            finally:
                a.close()
    finally:
        b.close()


# ---------------------------------------------------------------- 3. what follows from the definition
def test_identities(imt, forms):
    c, lib = forms["default"], imt.lib
    depth, cap = 32, 1024
    vals = [v for v in oracle_lib.synth_values(420, 0x564D4903) if 0 < v < P]
    base, block, tail, never = vals[:100], vals[100:200], vals[200:300], vals[300:400]
    t = imt.IndexedTree(c, depth, cap)
    try:
        t.apply_batch(base)
        root_s = t.root()
        t.apply_batch(block)
        t.apply_batch(tail)
        before = tree_state(t)
        s = 1 + len(base)
        v = t.view(s)
        assert v.root() == root_s != t.root()
        # INSERTs only
        ins, rd = v.mixed_witness(block[:60], [INSERT] * 60)
        want = v.insert_witness(60)
        for k in INS_FIELDS + ("new_index",):
            assert ins[k].shape == want[k].shape and (ins[k] == want[k]).all(), k
        assert all(rd[k].shape[1 if k == "low_sib" else 0] == 0 for k in RD_FIELDS)
        # READs only: of values never inserted, of values the block inserts, of values the tail inserts, one value twice
        reads = never[:40] + block[:10] + tail[:10] + never[:1]
        ins, rd = v.mixed_witness(reads, [READ] * len(reads))
        low, leaves, sib, largest = v.non_membership_witness(reads)
        assert (rd["low_index"] == low).all() and (rd["low_leaf"] == leaves).all() and (rd["is_largest"] == largest).all()
        assert (rd["low_sib"] == sib).all() and arr_ints(rd["root"]) == [root_s] * len(reads)
        assert ins["low_index"].shape[0] == 0 and ins["new_index"].shape[0] == 0
        # a READ before the first INSERT carries the view's root, and so does old_root of that INSERT
        script = [(READ, never[5]), (READ, tail[3]), (INSERT, block[0]), (READ, tail[3]), (INSERT, block[1]), (READ, block[7])]
        ins, rd = v.mixed_witness(*split(script))
        assert arr_ints(rd["root"][:2]) == [root_s, root_s] and arr_ints(ins["old_root"][:1]) == [root_s]
        assert (rd["root"][2] == ins["new_root"][0]).all() and (rd["root"][3] == ins["new_root"][1]).all()
        fail = c.non_membership(rd["root"], rd["low_leaf"], rd["low_index"], rd["low_sib"], depth,
                                ints_to_arr([x for op, x in script if op == READ]), rd["is_largest"])
        assert not fail.any()
        # n == 0
        k = ctypes.c_uint64(0xDEAD)
        assert lib.imt_itree_view_mixed_witness(v.h, None, None, 0, None, None, ctypes.byref(k), None, 0) == 0 and k.value == 0
        assert v.stats()[1] == 1 and tree_state(t) == before
        # the view at the current size: READs only, the tree's own answers
        head = t.view(t.size)
        reads = never[:30]
        ins, rd = head.mixed_witness(reads, [READ] * 30, item_major=True)
        low, leaves, sib, largest = t.non_membership_witness(reads)
        assert (rd["low_index"] == low).all() and (rd["low_leaf"] == leaves).all() and (rd["is_largest"] == largest).all()
        assert (rd["low_sib"].transpose(1, 0, 2) == sib).all() and arr_ints(rd["root"]) == [before[0]] * 30
        assert tree_state(t) == before
        t.insert_batch(never[90:92])                                       # and the tree goes on: its nodes were not rewritten
        assert t.get_proof_batch(np.arange(4)).shape[1] == 4
        head.close()
        v.close()
    finally:
        t.close()


# ---------------------------------------------------------------- raw calls
class RawV(tg.Raw):
    """imt_itree_view_mixed_witness with buffers of its own, every one pre-filled with a sentinel byte"""

    def call(self, view, vals, ops, flags):
        f, lib = self.imt._ffi, self.imt.lib
        h = view.h if hasattr(view, "h") else view
        ctx = view.ctx if hasattr(view, "ctx") else None
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
        self.n_ins, self.bad = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
        rc = lib.imt_itree_view_mixed_witness(h, pv, po, self.n, out, rout, ctypes.byref(self.n_ins), ctypes.byref(self.bad), flags)
        if self.dev:
            import torch
            if ctx is not None:
                ctx.sync()
            torch.cuda.synchronize()
        return rc


# ---------------------------------------------------------------- 4. refusals
def test_refusals(imt, forms):
    import torch
    c, f, lib = forms["default"], imt._ffi, imt.lib
    depth, cap = 32, 64
    E = f.ERR
    stored, block, tail = [10, 20, 30], [5, 50, 40, 25], [60, 15]
    idx = np.arange(cap, dtype=np.uint64)
    t = imt.IndexedTree(c, depth, cap)
    try:
        t.apply_batch(stored)
        t.apply_batch(block)
        t.apply_batch(tail)
        s = 1 + len(stored)
        v = t.view(s)
        v.root()

        def vstate(view):
            return view.root(), view.get_leaves(idx).tobytes(), view.get_proof_batch(idx).tobytes(), view.stats()[1]

        def refused(script, want_rc, want_bad=None, flags=0, dev=False, view=v, tag=""):
            tree = view.tree
            before, vb = tree_state(tree), vstate(view)
            r = RawV(imt, depth, len(script), bool(flags & f.SIB_ITEM_MAJOR), dev)
            rc = r.call(view, ints_to_arr([x for _, x in script]), [op for op, _ in script], flags)
            assert rc == want_rc, (tag, script, rc, lib.imt_last_error(c.h))
            assert r.untouched(), (tag, script)
            assert r.n_ins.value == 0xDEAD
            assert r.bad.value == (0xDEAD if want_bad is None else want_bad), (tag, script, r.bad.value)
            assert tree_state(tree) == before and vstate(view) == vb, (tag, script)

        ok = [(INSERT, 5), (READ, 6), (INSERT, 50), (READ, 60), (INSERT, 40), (READ, 7), (INSERT, 25)]
        r = RawV(imt, depth, len(ok))
        assert r.call(v, ints_to_arr([x for _, x in ok]), [op for op, _ in ok], 0) == 0 and r.n_ins.value == 4
        # IMT_ERR_VALUE from the walk: a READ of 0, of a stored value, of a value an earlier INSERT of the list put in
        for script, bad in (([(INSERT, 5), (READ, 20)], 1), ([(READ, 7), (READ, 0), (INSERT, 5)], 1),
                            ([(INSERT, 5), (READ, 6), (READ, 5), (INSERT, 50)], 2),
                            ([(INSERT, 5), (INSERT, 50), (READ, 45), (INSERT, 40), (READ, 50)], 4),
                            ([(READ, 30), (INSERT, 5)], 0)):
            assert walk([0] + stored, script)[1] == bad
            refused(script, E["VALUE"], bad)
            refused(script, E["VALUE"], bad, dev=True, flags=f.SIB_ITEM_MAJOR)
        # the scripts of the CPU test that the walk refuses, each against a tree that applied what it could
        seen = 0
        for name, (st, script) in ADVERSARIAL.items():
            bad = walk(st, script)[1]
            if bad < 0 or max(x for _, x in script) >= P:
                continue
            own = imt.IndexedTree(c, depth, cap)
            applied, present = [], set(st)
            for x in st[1:] + inserts_of(script[:bad]):
                applied.append(x)
                present.add(x)
            later = [x for x in inserts_of(script[bad:]) if x not in present and x != 0]
            later = list(dict.fromkeys(later)) + [7777 + i for i in range(8)]     # rows enough for every INSERT of the script
            own.apply_batch(applied + later)
            ov = own.view(len(st))
            # the first refusal of the walk, or the first INSERT that is not the stored one, whichever comes first
            rank, first_diff = 0, None
            stored_rows = (applied + later)[len(st) - 1:]
            for p, (op, x) in enumerate(script):
                if op == INSERT:
                    if rank >= len(stored_rows) or stored_rows[rank] != x:
                        first_diff = p
                        break
                    rank += 1
            want_bad = bad if first_diff is None else min(bad, first_diff)
            assert sum(op == INSERT for op, _ in script) <= own.size - len(st)
            for dev in (False, True):
                refused(script, E["VALUE"], want_bad, dev=dev, view=ov, tag=name)
            seen += 1
            ov.close()
            own.close()
        assert seen >= 5
        # an altered INSERT: alone, two of them, behind a READ the walk refuses, and in front of one
        for script, bad in (([(INSERT, 5), (READ, 6), (INSERT, 51), (INSERT, 40)], 2),
                            ([(INSERT, 6), (READ, 7), (INSERT, 50), (INSERT, 41)], 0),
                            ([(READ, 8), (INSERT, 5), (INSERT, 50), (INSERT, 41), (INSERT, 26)], 3),
                            ([(INSERT, 5), (READ, 20), (INSERT, 51)], 1),
                            ([(INSERT, 5), (INSERT, 51), (READ, 20)], 1),
                            ([(INSERT, 5), (READ, 5), (INSERT, 50), (INSERT, 41)], 1),
                            ([(INSERT, 50), (INSERT, 5)], 0),                      # the block's values in another order
                            ([(INSERT, 5), (INSERT, 50), (INSERT, 40), (INSERT, 25), (INSERT, 61)], 4),   # the tail's row differs
                            ([(INSERT, 5), (INSERT, 0)], 1), ([(INSERT, 5), (INSERT, 20)], 1)):
            refused(script, E["VALUE"], bad)
            refused(script, E["VALUE"], bad, dev=True)
        r = RawV(imt, depth, 2)
        assert r.call(v, ints_to_arr([5, 51]), [INSERT, INSERT], 0) == E["VALUE"] and r.bad.value == 1
        assert b"not the value stored at leaf 5" in lib.imt_last_error(c.h), lib.imt_last_error(c.h)
        # IMT_ERR_NONCANONICAL outranks a bad value elsewhere in the list
        refused([(READ, 7), (READ, P), (INSERT, 6)], E["NONCANONICAL"])
        refused([(INSERT, P + 1), (READ, 7)], E["NONCANONICAL"], dev=True)
        # IMT_ERR_RANGE: one INSERT more than the tree holds beyond the view
        all_in = [(INSERT, x) for x in block + tail]
        r = RawV(imt, depth, len(all_in))
        assert r.call(v, ints_to_arr([x for _, x in all_in]), [INSERT] * len(all_in), 0) == 0
        refused(all_in + [(READ, 9), (INSERT, 70)], E["RANGE"])
        refused([(READ, 9)] + all_in + [(INSERT, 70)], E["RANGE"], dev=True)
        head = t.view(t.size)
        refused([(READ, 9), (INSERT, 70)], E["RANGE"], view=head)
        head.close()
        # IMT_ERR_ARG: op bytes, NULL vals / op, flags, misaligned device buffers, a handle that is no view
        for dev in (False, True):
            r = RawV(imt, depth, 2, False, dev)
            assert r.call(v, ints_to_arr([5, 6]), [0, 2], 0) == E["ARG"] and r.untouched() and r.bad.value == 0xDEAD
            r = RawV(imt, depth, 2, False, dev)
            assert r.call(v, ints_to_arr([5, 6]), [255, 1], 0) == E["ARG"] and r.untouched()
        for flags in (f.PIPELINE, f.PIPELINE | f.DEVICE_PTRS, f.HOST_PREP, f.INPUTS_READY | f.DEVICE_PTRS, 3):
            refused(ok[:2], E["ARG"], flags=flags, dev=bool(flags & f.DEVICE_PTRS))
        one, op1 = ints_to_arr([5]), np.zeros(1, np.uint8)
        pv, po = one.ctypes.data_as(ctypes.c_void_p), op1.ctypes.data_as(ctypes.c_void_p)
        assert lib.imt_itree_view_mixed_witness(v.h, None, po, 1, None, None, None, None, 0) == E["ARG"]
        assert lib.imt_itree_view_mixed_witness(v.h, pv, None, 1, None, None, None, None, 0) == E["ARG"]
        assert lib.imt_itree_view_mixed_witness(None, pv, po, 1, None, None, None, None, 0) == E["ARG"]
        assert lib.imt_itree_view_mixed_witness(t.h, pv, po, 1, None, None, None, None, 0) == E["ARG"]     # a tree's handle
        dbuf = torch.full((4096,), tg.SENTINEL, dtype=torch.uint8, device="cuda")
        dvals = torch.from_numpy(ints_to_arr([5, 6])).cuda()
        dops = torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
        at = lambda off: dbuf.data_ptr() + off
        for ins_kw, rd_kw in ((dict(new_root=at(8)), {}), (dict(low_sib=at(24)), {}), ({}, dict(root=at(8))), ({}, dict(low_sib=at(4))),
                              ({}, dict(low_leaf=at(40))), (dict(low_index=at(4)), {}), ({}, dict(low_index=at(12)))):
            rc = lib.imt_itree_view_mixed_witness(v.h, ctypes.c_void_p(dvals.data_ptr()), ctypes.c_void_p(dops.data_ptr()), 2,
                                                  ctypes.byref(f.InsertOut(**ins_kw)), ctypes.byref(f.ReadOut(**rd_kw)), None, None,
                                                  f.DEVICE_PTRS)
            assert rc == E["ARG"], (ins_kw, rd_kw)
        rc = lib.imt_itree_view_mixed_witness(v.h, ctypes.c_void_p(dvals.data_ptr() + 8), ctypes.c_void_p(dops.data_ptr()), 1, None,
                                              None, None, None, f.DEVICE_PTRS)
        assert rc == E["ARG"]
        c.sync()
        assert (dbuf.cpu().numpy() == tg.SENTINEL).all()
        # a placed tree, a partitioned tree
        placed = imt.IndexedTree(c, 8, 64)
        placed.set_placement(10, 1)
        placed.apply_batch([4, 9])
        pview = placed.view(2)
        r = RawV(imt, 8, 2)
        assert r.call(pview, ints_to_arr([9, 7]), [0, 1], 0) == E["ARG"] and r.untouched()
        pview.close()
        placed.close()
        part = imt.IndexedTree(c, depth, cap)
        c._check(lib.imt_itree_set_value_partition(part.h, 3, 1))
        part.apply_batch([4, 7])
        pview = part.view(2)
        r = RawV(imt, depth, 2)
        assert r.call(pview, ints_to_arr([7, 10]), [0, 1], 0) == E["ARG"] and r.untouched()
        pview.close()
        part.close()
        # between imt_itree_batch_begin and _end; an open slice
        before, vb = tree_state(t), vstate(v)
        ev, l0 = ctypes.c_uint32(), ctypes.c_uint32()
        more = ints_to_arr([71, 72, 73, 74])
        assert lib.imt_itree_batch_begin(t.h, more.ctypes.data_as(ctypes.c_void_p), 4, 0, ctypes.byref(ev), ctypes.byref(l0)) == 0
        r = RawV(imt, depth, 2)
        assert r.call(v, ints_to_arr([5, 6]), [0, 1], 0) == E["ARG"] and r.untouched()
        assert lib.imt_itree_batch_abort(t.h) == 0
        assert tree_state(t) == before and vstate(v) == vb
        dv8 = torch.from_numpy(ints_to_arr([81, 82, 83, 84, 85, 86, 87, 88])).cuda()
        pay = torch.zeros(int(lib.imt_itree_slice_payload_bytes(8)) + 64, dtype=torch.uint8, device="cuda")
        sl = ctypes.c_int(-1)
        assert lib.imt_itree_slice_prepare(t.h, ctypes.c_void_p(dv8.data_ptr()), 0, 8, 0, None, f.DEVICE_PTRS, ctypes.byref(sl), None) == 0
        r = RawV(imt, depth, 2)
        assert r.call(v, ints_to_arr([5, 6]), [0, 1], 0) == E["ARG"] and r.untouched()
        for q in range(depth + 1):
            assert lib.imt_itree_slice_unit(t.h, sl.value, q, ctypes.c_void_p(pay.data_ptr()), None) == 0
        c.sync()
        assert t.size == before[1] + 8
        ins, rd = v.mixed_witness(*split(ok))                              # and afterwards the call works, after one rebuild
        assert ins["low_index"].shape[0] == 4 and v.stats()[1] == vb[3] + 1
        # the tree rewound below the view; then grown again along another history
        t.rewind(2)
        builds = v.stats()[1]
        r = RawV(imt, depth, len(ok))
        assert r.call(v, ints_to_arr([x for _, x in ok]), [op for op, _ in ok], 0) == E["RANGE"] and r.untouched()
        assert r.n_ins.value == 0xDEAD and r.bad.value == 0xDEAD and v.stats()[1] == builds and t.size == 2
        t.apply_batch([20, 30, 5, 50, 41, 25, 90])                          # leaves 2 .. 8: the third INSERT of the block differs
        refused(ok, E["VALUE"], 4)
        ins, rd = v.mixed_witness(*split(ok[:4]))                          # the part both histories share still replays
        assert ins["low_index"].shape[0] == 2 and rd["low_index"].shape[0] == 2
        # a handle that is not a live view
        stale = ctypes.c_void_p(v.h.value)
        v.close()
        assert lib.imt_itree_view_mixed_witness(stale, pv, po, 1, None, None, None, None, 0) == E["ARG"]
    finally:
        t.close()


def test_refused_while_sliced(imt, ctx):
    """world 2 over the local transport: a replica with steps in flight replays nothing, after the flush it does"""
    import torch
    import test_gpu_sliced as ts
    sl = ts.load_sliced()
    depth, cap, world, batch = 32, 1 << 10, 2, 40
    vals = oracle_lib.synth_values(world * batch + 4, 0x564D5300)
    w = sl.SlicedTree(imt, 0, depth, cap, batch, world, n_local=world, nbuf=8)
    try:
        views = [t.view(1) for t in w.trees]
        w.step(torch.from_numpy(ints_to_arr(vals[:world * batch])).cuda())
        script = [(READ, vals[-1]), (INSERT, vals[0]), (READ, vals[1]), (INSERT, vals[1])]
        for view in views:
            r = RawV(imt, depth, len(script))
            assert r.call(view, ints_to_arr([x for _, x in script]), [op for op, _ in script], 0) == imt._ffi.ERR["ARG"]
            assert r.untouched()
        w.flush()
        rows = [view.mixed_witness(*split(script)) for view in views]
        for k in rows[0][0]:
            assert (rows[0][0][k] == rows[1][0][k]).all(), k
        assert rows[0][0]["low_index"].shape[0] == 2 and rows[0][1]["low_index"].shape[0] == 2
        for view in views:
            view.close()
    finally:
        w.close()


# ---------------------------------------------------------------- 5. formats and pointers
def test_formats_and_pointers(imt, forms):
    c, f = forms["default"], imt._ffi
    depth, cap = 32, 256
    vals = [v for v in oracle_lib.synth_values(160, 0x564D4605) if 0 < v < P]
    stored, script = vals[:30], [(READ if i % 3 == 1 else INSERT, vals[40 + i]) for i in range(50)]
    script += [(READ, vals[41]), (READ, vals[100]), (READ, vals[130])]
    tail = vals[120:150]
    v_arr, ops, n = ints_to_arr([v for _, v in script]), [op for op, _ in script], len(script)
    k = ops.count(INSERT)
    ref, t = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    try:
        ref.apply_batch(stored)
        want_ins, want_rd = ref.mixed_batch(v_arr, ops)
        want_ins.pop("new_index")
        t.apply_batch(stored)
        t.apply_batch(inserts_of(script))
        t.apply_batch(tail)
        state = tree_state(t)
        view = t.view(1 + len(stored))
        lm = lambda a: a.transpose(1, 0, 2)                       # [depth][rows] -> [rows][depth]
        for fmt, item_major, dev in ((f.FMT_MONT256, True, False), (f.FMT_DEVICE, True, False), (f.FMT_CANONICAL, False, True),
                                     (f.FMT_MONT256, False, True), (f.FMT_DEVICE, True, True), (f.FMT_DEVICE, False, False)):
            tag = f"fmt {fmt} item_major {item_major} dev {dev}"
            r = RawV(imt, depth, n, item_major, dev)
            assert r.call(view, tm.to_fmt(v_arr, fmt), ops, fmt | (f.SIB_ITEM_MAJOR if item_major else 0)) == 0, tag
            assert r.n_ins.value == k and tree_state(t) == state, tag
            for got, want, m in ((tg.cut(r.host(r.ins), k, n, item_major), want_ins, k),
                                 (tg.cut(r.host(r.rd), n - k, n, item_major), want_rd, n - k)):
                for key, a in got.items():
                    w = want[key]
                    if key.endswith("_sib") and item_major:
                        w = lm(w)
                    if key not in ("low_index", "is_largest"):
                        w = tm.to_fmt(np.ascontiguousarray(w), fmt)
                    assert a.shape == w.shape and (a == w).all(), f"{tag}: {key}"
        # NULL fields are skipped, either struct may be missing altogether
        for ins_f, rd_f, dev in ((("new_root", "low_sib"), ("root",), False), (None, RD_FIELDS, True), (INS_FIELDS, None, False),
                                 (None, None, True), (("is_largest", "old_root"), ("low_sib", "low_index"), True)):
            tag = f"fields {ins_f} {rd_f} dev {dev}"
            r = RawV(imt, depth, n, False, dev, ins_f, rd_f)
            assert r.call(view, v_arr, ops, 0) == 0 and r.n_ins.value == k, tag
            assert tree_state(t) == state, tag
            for got, want, m in ((r.host(r.ins), want_ins, k), (r.host(r.rd), want_rd, n - k)):
                for key, a in (tg.cut(got, m, n, False) if got else {}).items():
                    assert (a == want[key]).all(), f"{tag}: {key}"
        assert view.stats()[1] == 1
        view.close()
    finally:
        ref.close()
        t.close()


# ---------------------------------------------------------------- 6. the replay follows the tree
def test_follows(imt, forms):
    import torch
    c, f, lib = forms["default"], imt._ffi, imt.lib
    depth, cap, nb = 32, 1 << 14, 2048
    vals = oracle_lib.synth_values(3 * nb + 400, 0x564D4606)
    base, rest = vals[:3 * nb], vals[3 * nb:]
    block1 = [(READ if i % 3 == 0 else INSERT, rest[i]) for i in range(90)]
    block2 = [(READ if i % 4 == 1 else INSERT, rest[100 + i]) for i in range(80)]
    block2 += [(READ, rest[3]), (READ, rest[300])]
    a, b = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    try:
        b.apply_batch(ints_to_arr(base[:nb]))
        a.apply_batch(ints_to_arr(base[:nb]))
        s1 = a.size
        # block 1 is the head of the second batch of values; two more pipelined batches are left in flight behind it
        seq = inserts_of(block1) + base[nb:]
        d = torch.from_numpy(ints_to_arr(seq)).cuda()
        v1 = a.view(s1)
        at = 0
        for m in (len(inserts_of(block1)), nb, nb):
            part = d[at:at + m]
            assert lib.imt_itree_insert_batch(a.h, ctypes.c_void_p(part.data_ptr()), m, None, f.DEVICE_PTRS | f.PIPELINE) == 0
            at += m
        ins, rd = v1.mixed_witness(*split(block1))
        want_ins, want_rd = b.mixed_batch(*split(block1))
        for k in want_ins:
            assert (ins[k] == want_ins[k]).all(), k
        for k in want_rd:
            assert (rd[k] == want_rd[k]).all(), k
        assert v1.stats()[1] == 1
        b.apply_batch(ints_to_arr(base[nb:]))
        assert a.root() == b.root()
        # a live mixed batch on the same tree: block 2; a view made before it replays it
        s2 = a.size
        v2 = a.view(s2)
        live_ins, live_rd = a.mixed_batch(*split(block2))
        ins, rd = v2.mixed_witness(*split(block2))
        for k in live_ins:
            assert (ins[k] == live_ins[k]).all(), k
        for k in live_rd:
            assert (rd[k] == live_rd[k]).all(), k
        builds = (v1.stats()[1], v2.stats()[1])
        assert builds == (1, 1)                                   # v1 is rebuilt at its next query only
        # a batch of READs only changes nothing: neither view rebuilds
        ins, rd = v1.mixed_witness(*split(block1))
        assert v1.stats()[1] == 2
        a.mixed_batch([rest[350], rest[351]], [READ, READ])
        ins1, rd1 = v1.mixed_witness(*split(block1))
        ins2, rd2 = v2.mixed_witness(*split(block2))
        assert (v1.stats()[1], v2.stats()[1]) == (2, 1)
        # two views, two consecutive blocks, in turn
        for k in want_ins:
            assert (ins1[k] == want_ins[k]).all(), k
        for k in live_rd:
            assert (rd2[k] == live_rd[k]).all() and (rd1[k] == want_rd[k]).all(), k
        assert arr_ints(ins2["old_root"][:1]) == [v2.root()] and v2.root() == b.root()
        v1.close()
        v2.close()
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 7. the C example
def test_example(imt, oracle):
    """examples/late_block_demo.c: a sequencer applies a mixed block's insertions and the next block's, a prover then replays
    the first block through a view at its start.  The demo prints the roots."""
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, csrc = os.path.join(root_dir, "examples", "late_block_demo"), os.path.join(root_dir, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(root_dir, "include"),
                        os.path.join(root_dir, "examples", "late_block_demo.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    stored = [20, 40]
    script = list(zip([0, 1, 0, 0, 1, 0, 1, 0, 1, 0], [30, 45, 10, 60, 65, 70, 65, 45, 25, 5]))
    nxt = [15, 35, 55, 65]
    want_ins, want_rd, (root1, _) = oracle_walk(oracle, 8, 64, stored, script)
    _, _, (root2, _) = oracle_walk(oracle, 8, 64, stored + inserts_of(script), [(INSERT, x) for x in nxt])
    _, _, (root0, _) = oracle_walk(oracle, 8, 64, stored, [])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"root before the block {root0:064x}" in r.stdout, r.stdout
    assert f"root after the block {root1:064x}" in r.stdout and f"root after the next block {root2:064x}" in r.stdout, r.stdout
    assert f"the view's root {root0:064x}" in r.stdout
    for o in want_ins:
        assert f"low leaf {o['low']}, new root {o['new_root']:064x}" in r.stdout, r.stdout
    for o in want_rd:
        assert f"low leaf {o['low']}{' (the largest)' if o['largest'] else ''}, against root {o['root']:064x}" in r.stdout, r.stdout
    assert "6 insert_leaf and 4 verify_non_inclusion witnesses, all satisfied" in r.stdout
    assert f"the tree is where it was: root {root2:064x}" in r.stdout
    assert "altered block: refused at operation 3" in r.stdout
