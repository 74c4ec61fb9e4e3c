"""GPU: IMT_OP_MEMBER under IMT_MEMBER_OPS (include/imt.h "PRESENCE READS") -- presence reads inside mixed blocks, in order.

The definition is the walk: a MEMBER of v asks lookup of v on the tree at that moment, the answer must be PRESENT at a leaf
L, and its `rd` row is L, get_leaves(L) then, the root then and get_proof_batch(L) then.  The expectation of every test is
that walk played once on the sequential CPU oracle (sparse_insert per INSERT; sparse_root, sparse_preimage and sparse_proof
at every READ and MEMBER, the leaf named by tests/member_model.py) or the strict call on a twin tree that was itself
compared with the oracle.  Every comparison is bit-exact.

  test_stories              depth 3, {10, 30} stored: the six stories of the issue in all eight forms (host / device
                            pointers, level- / item-major, canonical / MONT256) against the oracle; the tree afterwards
                            against a twin fed the INSERTs alone; every MEMBER row through imt_verify_proof_batch
  test_entry_points_agree   depth 32, 2^10 operations a third of each kind: apply_mixed, both pipelined forms as four
                            blocks enqueued before one synchronisation, the replay after the tree has moved on -- each
                            against strict mixed_batch on a twin, one 64-operation block against the oracle; apply_stats
  test_refusals             *bad_op, outputs and tree untouched, views fresh; op 3 and 255 with the flag, op 2 without
  test_filtered_twins       every status under every kind: status, leaf_index and counts against the model, the rows
                            against the strict call on the carried-out operations
  test_member_example       examples/member_reads_demo.c: its rows and root against the oracle's
"""
import ctypes

import numpy as np
import pytest

import oracle_lib
import test_gpu_insert_matrix as tm
from member_model import OP_MEMBER, MemberModel
from oracle_lib import P, arr_ints, ints_to_arr
from test_gpu_mixed import INS_FIELDS, RD_FIELDS, SENTINEL, check_rows, cut
from test_gpu_mixed_pipelined import same_tree, sync
from test_gpu_rewind import forms  # noqa: F401  (the fixture: one context per hash form)
from tree_model import NEW, NONE, OP_INSERT, OP_READ, PRESENT, REPEATED, ZERO

pytestmark = pytest.mark.gpu

I, R, M = OP_INSERT, OP_READ, OP_MEMBER
UNSET = 0xDEAD
CALLS = ("mixed", "mixed_filtered", "apply_mixed", "apply_mixed_filtered", "mixed_pipelined", "apply_mixed_pipelined", "view")
TODAY = b"neither IMT_OP_INSERT nor IMT_OP_READ"
ALL_THREE = b"neither IMT_OP_INSERT, IMT_OP_READ nor IMT_OP_MEMBER"


def split(script):
    return ints_to_arr([v for _, v in script]), [op for op, _ in script]


def oracle_walk(orc, depth, cap, stored, script):
    """(ins rows, rd rows, final root, final preimages) of the walk on the sequential oracle: test_gpu_mixed.oracle_walk
    with the third kind -- the leaf of a READ or a MEMBER is the one the model names, and the oracle's preimage of that
    leaf is the row"""
    m = MemberModel(depth, cap)
    h = orc.sparse_new(depth, cap)
    for v in stored:
        m.insert([v])
        assert orc.sparse_insert(h, depth, v)["rc"] == 0
    ins, rd = [], []
    for op, v in script:
        root = orc.sparse_root(h)
        if op == I:
            o = orc.sparse_insert(h, depth, v)
            assert o["rc"] == 0
            o["old_root"] = root
            o["new_leaf"] = orc.sparse_preimage(h, m.size)
            ins.append(o)
            m.insert([v])
            continue
        low, leaf, largest = m.nm_witness(v) if op == R else m.member_witness(v)
        pre = orc.sparse_preimage(h, low)
        assert arr_ints(pre) == list(leaf) and (op == R or leaf[0] == v)
        rd.append(dict(low=low, low_leaf=pre, largest=largest, root=root, low_proof=orc.sparse_proof(h, depth, low)))
    final = (orc.sparse_root(h), np.stack([orc.sparse_preimage(h, i) for i in range(m.size)]))
    orc.sparse_free(h)
    return ins, rd, final


class Call:
    """One of the seven calls with buffers of its own, every one pre-filled with the sentinel byte 0xA5: the nine arrays
    of imt_insert_out, the five of imt_read_out, root_out, status and leaf_index."""

    def __init__(self, imt, depth, n, dev=False, item_major=False):
        self.imt, self.dev, self.n, self.depth, self.item_major = imt, dev, n, depth, item_major
        rows = max(n, 1)
        sib = (rows, depth, 32) if item_major else (depth, rows, 32)
        shapes = dict(low_index=(rows,), low_leaf=(rows, 3, 32), new_leaf=(rows, 3, 32), is_largest=(rows,), old_root=(rows, 32),
                      interim_root=(rows, 32), new_root=(rows, 32), root=(rows, 32), low_sib=sib, new_sib=sib)
        self.ins = {k: self._buf(shapes[k], k == "low_index") for k in INS_FIELDS}
        self.rd = {k: self._buf(shapes[k], k == "low_index") for k in RD_FIELDS}
        self.extra = dict(root_out=self._buf((32,)), status=self._buf((rows,)), leaf_index=self._buf((rows,), True))

    def _buf(self, shape, u64=False):
        a = np.full(shape, 0xA5A5A5A5A5A5A5A5, np.uint64) if u64 else np.full(shape, SENTINEL, np.uint8)
        if not self.dev:
            return a
        import torch
        return torch.from_numpy(a.view(np.int64) if u64 else a).cuda()

    def _ptr(self, x):
        return ctypes.c_void_p(x.data_ptr() if self.dev else x.ctypes.data)

    def _host(self, x):
        if not self.dev:
            return x
        a = x.cpu().numpy()
        return a.view(np.uint64) if a.dtype == np.int64 else a

    def host(self):
        return {name: {k: self._host(x) for k, x in d.items()} for name, d in (("ins", self.ins), ("rd", self.rd), ("extra", self.extra))}

    def untouched(self):
        return all((a.view(np.uint8) == SENTINEL).all() for d in self.host().values() for a in d.values())

    def run(self, which, handle, vals, ops, flags, wait=True):
        """handle: the tree's, or the view's for `view`; returns rc and leaves n_ins, n_rd (filtered) and bad"""
        f, lib = self.imt._ffi, self.imt.lib
        vals, ops = np.ascontiguousarray(vals), np.asarray(ops, np.uint8)
        if self.dev:
            import torch
            self.keep = (torch.from_numpy(vals).cuda(), torch.from_numpy(ops).cuda())
            flags |= f.DEVICE_PTRS
        else:
            self.keep = (vals, ops)
        pv, po = (self._ptr(x) for x in self.keep)
        ins = ctypes.byref(f.InsertOut(**{k: self._ptr(x).value for k, x in self.ins.items()}))
        rd = ctypes.byref(f.ReadOut(**{k: self._ptr(x).value for k, x in self.rd.items()}))
        root, status, leaf = (self._ptr(self.extra[k]) for k in ("root_out", "status", "leaf_index"))
        a, b = ctypes.c_uint64(UNSET), ctypes.c_uint64(UNSET)
        n = self.n
        if which in ("mixed", "mixed_pipelined", "view"):
            fn = dict(mixed=lib.imt_itree_mixed_batch, mixed_pipelined=lib.imt_itree_mixed_pipelined, view=lib.imt_itree_view_mixed_witness)
            rc = fn[which](handle, pv, po, n, ins, rd, ctypes.byref(a), ctypes.byref(b), flags)
        elif which in ("apply_mixed", "apply_mixed_pipelined"):
            fn = lib.imt_itree_apply_mixed if which == "apply_mixed" else lib.imt_itree_apply_mixed_pipelined
            rc = fn(handle, pv, po, n, root, ctypes.byref(a), ctypes.byref(b), flags)
        elif which == "mixed_filtered":
            rc = lib.imt_itree_mixed_filtered(handle, pv, po, n, status, leaf, ins, rd, ctypes.byref(a), ctypes.byref(b), flags)
        else:
            rc = lib.imt_itree_apply_mixed_filtered(handle, pv, po, n, status, leaf, ctypes.byref(a), ctypes.byref(b), root, flags)
        filtered = which.endswith("filtered")
        self.n_ins, self.n_rd, self.bad = a.value, (b.value if filtered else None), (None if filtered else b.value)
        if self.dev and wait:
            import torch
            torch.cuda.synchronize()
        return rc


def state_of(t):
    return (t.root(), t.size, t.snapshot().tobytes())


def arrays_of(want_ins, want_rd, depth):
    """the oracle's rows as the arrays of the two structs, siblings item-major"""
    ins = dict(low_index=np.array([o["low"] for o in want_ins], np.uint64), is_largest=np.array([o["largest"] for o in want_ins], np.uint8))
    for k, src in (("low_leaf", "low_leaf"), ("new_leaf", "new_leaf"), ("low_sib", "low_proof"), ("new_sib", "new_proof")):
        ins[k] = np.stack([o[src] for o in want_ins]) if want_ins else np.zeros((0, depth if "sib" in k else 3, 32), np.uint8)
    for k in ("old_root", "interim_root", "new_root"):
        ins[k] = ints_to_arr([o[k] for o in want_ins]) if want_ins else np.zeros((0, 32), np.uint8)
    rd = dict(low_index=np.array([o["low"] for o in want_rd], np.uint64), is_largest=np.array([o["largest"] for o in want_rd], np.uint8))
    rd["low_leaf"] = np.stack([o["low_leaf"] for o in want_rd]) if want_rd else np.zeros((0, 3, 32), np.uint8)
    rd["low_sib"] = np.stack([o["low_proof"] for o in want_rd]) if want_rd else np.zeros((0, depth, 32), np.uint8)
    rd["root"] = ints_to_arr([o["root"] for o in want_rd]) if want_rd else np.zeros((0, 32), np.uint8)
    return ins, rd


def same_rows(got, want, m, n, item_major, fmt, tag):
    """rows [0, m) of every array of one struct against `want` (canonical, siblings item-major), nothing beyond them written"""
    for k, a in cut(got, m, max(n, 1), item_major).items():
        w = want[k]
        if k.endswith("_sib") and not item_major:
            w = w.transpose(1, 0, 2)
        if k not in ("low_index", "is_largest"):
            w = tm.to_fmt(np.ascontiguousarray(w), fmt)
        assert a.shape == w.shape and (a == w).all(), f"{tag}: {k}"


# ---------------------------------------------------------------- 1. the stories at depth 3
STORED = [10, 30]
STORIES = {
    "a stored value": [(M, 10)],
    "the largest value": [(M, 30)],
    "the value the operation before it inserted": [(I, 20), (M, 20)],
    "two MEMBERs, an INSERT between them becomes the successor": [(I, 20), (M, 20), (I, 25), (M, 20)],
    "interleaved": [(M, 10), (R, 15), (I, 15), (M, 15), (R, 40), (I, 40), (M, 40), (M, 30), (R, 12), (M, 10)],
    "MEMBERs only": [(M, 10), (M, 30), (M, 10)],
}
_STORY_WANT = {}


def story_want(orc, name):
    if name not in _STORY_WANT:
        _STORY_WANT[name] = oracle_walk(orc, 3, 8, STORED, STORIES[name])
    return _STORY_WANT[name]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("item_major", [False, True], ids=["level-major", "item-major"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["canonical", "mont256"])
def test_stories(imt, forms, oracle, dev, item_major, fmt):
    c, f = forms["default"], imt._ffi
    depth, cap = 3, 8
    for name, script in STORIES.items():
        tag = f"{name}, dev {dev} item_major {item_major} fmt {fmt}"
        want_ins, want_rd, (root, pre) = story_want(oracle, name)
        # the rows the definition gives a MEMBER: the leaf holds the value, and is_largest says its successor is nothing
        kinds = [op for op, _ in script if op != I]
        for (op, v), o in zip([x for x in script if x[0] != I], want_rd):
            if op == M:
                assert arr_ints(o["low_leaf"])[0] == v and o["largest"] == int(arr_ints(o["low_leaf"])[1] == 0), tag
        w_ins, w_rd = arrays_of(want_ins, want_rd, depth)
        v_arr, ops = split(script)
        n, k = len(script), ops.count(I)
        t, twin = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
        try:
            for x in (t, twin):
                x.apply_batch(STORED)
            call = Call(imt, depth, n, dev, item_major)
            rc = call.run("mixed", t.h, tm.to_fmt(v_arr, fmt), ops, fmt | f.MEMBER_OPS | (f.SIB_ITEM_MAJOR if item_major else 0))
            assert rc == 0 and call.n_ins == k and call.bad == UNSET, (tag, rc, imt.lib.imt_last_error(c.h))
            got = call.host()
            same_rows(got["ins"], w_ins, k, n, item_major, fmt, tag + ": ins")
            same_rows(got["rd"], w_rd, n - k, n, item_major, fmt, tag + ": rd")
            assert all((a.view(np.uint8) == SENTINEL).all() for a in got["extra"].values()), tag
            # the tree afterwards: the oracle's, and a twin fed the INSERTs alone -- root, all leaves, all proofs
            assert t.root() == root and t.size == pre.shape[0] and (t.snapshot() == pre).all(), tag
            if k:
                twin.apply_batch([v for op, v in script if op == I])
            same_tree(t, twin, tag)
            # every MEMBER row is a membership proof of hash3(low_leaf)
            rows = [q for q, op in enumerate(kinds) if op == M]
            rd = cut(got["rd"], n - k, n, item_major)
            leaf = c.hash3(rd["low_leaf"][rows], fmt=fmt)
            sib = rd["low_sib"][rows] if item_major else np.ascontiguousarray(rd["low_sib"][:, rows])
            ok = c.verify_proof_batch(leaf, rd["low_index"][rows], rd["root"][rows], sib, depth, item_major=item_major, fmt=fmt)
            assert ok.all(), tag
        finally:
            t.close()
            twin.close()


# ---------------------------------------------------------------- 2. the seven entry points agree at depth 32
def big_script(n, stored, fresh, seed):
    """n operations, a third of each kind, every one accepted: a MEMBER draws from what is there by then, a READ from
    what is not (values inserted later included)"""
    import random
    rng = random.Random(seed)
    there, later, script = list(stored), list(fresh[:n // 3 + 1]), []
    absent = list(fresh[n // 3 + 1:])
    for p in range(n):
        kind = p % 3
        if kind == 0:
            v = later.pop(0)
            there.append(v)
            script.append((I, v))
        elif kind == 1:
            script.append((R, rng.choice(later[:8] + absent[:64])))
        else:
            script.append((M, rng.choice(there[-6:] + there[:40])))
    return script


def test_entry_points_agree(imt, forms, oracle):
    import torch
    c, f = forms["default"], imt._ffi
    depth, cap, n, nb = 32, 1 << 12, 1 << 10, 4
    vals = [v for v in oracle_lib.synth_values(2400, 0x4D454D01) if 0 < v < P]
    stored, fresh = vals[:300], vals[300:]
    script = big_script(n, stored, fresh, 0x4D454D02)
    assert [sum(op == k for op, _ in script) for k in (I, R, M)] == [342, 341, 341]
    v_arr, ops = split(script)
    k = ops.count(I)
    flags = f.MEMBER_OPS
    trees = [imt.IndexedTree(c, depth, cap) for _ in range(6)]
    ref, ta, tp, tap, small, base = trees
    try:
        for t in trees:
            t.apply_batch(stored)
        # the reference: strict mixed_batch on a twin, whole and block by block
        want_ins, want_rd = ref.mixed_batch(v_arr, ops, members=True)
        assert ref.size == 1 + len(stored) + k
        # ... pinned by the oracle on one 64-operation block
        o_ins, o_rd, (o_root, o_pre) = oracle_walk(oracle, depth, cap, stored, script[:64])
        s_ins, s_rd = small.mixed_batch(v_arr[:64], ops[:64], members=True)
        check_rows(s_ins, s_rd, o_ins, o_rd, False, "64 operations against the oracle")
        assert small.root() == o_root and (small.snapshot() == o_pre).all()
        for key in RD_FIELDS:
            m = len(o_rd)
            assert (want_rd[key][:, :m] == s_rd[key]).all() if key == "low_sib" else (want_rd[key][:m] == s_rd[key]).all(), key

        # apply_mixed: the same tree, no rows, the stats of the INSERTs alone
        n_ins, root = ta.apply_mixed(v_arr, ops, members=True)
        assert n_ins == k and root == ref.root()
        same_tree(ta, ref, "apply_mixed")
        stats = ta.apply_stats().copy()
        base.apply_batch([v for op, v in script if op == I])
        assert (stats == base.apply_stats()).all() and base.root() == root

        # four blocks of 256 through each pipelined form, all enqueued before one synchronisation
        q = n // nb
        for which, t in (("mixed_pipelined", tp), ("apply_mixed_pipelined", tap)):
            calls, sizes = [], []
            for j in range(nb):
                call = Call(imt, depth, q, dev=True)
                rc = call.run(which, t.h, v_arr[j * q:(j + 1) * q], ops[j * q:(j + 1) * q], flags, wait=False)
                assert rc == 0 and call.bad == UNSET, (which, j, rc, imt.lib.imt_last_error(c.h))
                calls.append(call)
                sizes.append(t.size)
            sync(c)
            same_tree(t, ref, which)
            at_i = at_r = 0
            for j, call in enumerate(calls):
                kj = ops[j * q:(j + 1) * q].count(I)
                assert call.n_ins == kj and sizes[j] == 1 + len(stored) + at_i + kj, (which, j)
                got = call.host()
                if which == "mixed_pipelined":
                    for part, want, lo, m in (("ins", want_ins, at_i, kj), ("rd", want_rd, at_r, q - kj)):
                        for key, a in cut(got[part], m, q, False).items():
                            w = want[key][:, lo:lo + m] if key.endswith("_sib") else want[key][lo:lo + m]
                            assert (a == w).all(), f"{which} block {j}: {part}.{key}"
                    assert (got["extra"]["root_out"] == SENTINEL).all()
                else:
                    assert arr_ints(got["extra"]["root_out"]) == arr_ints(want_ins["new_root"][at_i + kj - 1]), (which, j)
                    assert all((a.view(np.uint8) == SENTINEL).all() for part in ("ins", "rd") for a in got[part].values())
                at_i, at_r = at_i + kj, at_r + q - kj
            if which == "apply_mixed_pipelined":
                last = [v for op, v in script[(nb - 1) * q:] if op == I]
                before = [v for op, v in script[:(nb - 1) * q] if op == I]
                twin = imt.IndexedTree(c, depth, cap)
                trees.append(twin)
                twin.apply_batch(stored + before)
                twin.apply_batch(last)
                assert (t.apply_stats() == twin.apply_stats()).all()

        # the replay, after the tree has moved a block on: a MEMBER of a value the tree received later is refused, the block
        # itself replays byte for byte
        late = fresh[-40:]
        ta.apply_batch(late)
        view = ta.view(1 + len(stored))
        trees.append(view)
        ins, rd = view.mixed_witness(v_arr, ops, members=True)
        for part, want in ((ins, want_ins), (rd, want_rd)):
            for key, a in part.items():
                assert a.shape == want[key].shape and (a == want[key]).all(), f"replay: {key}"
        with pytest.raises(ValueError) as e:
            view.mixed_witness(np.concatenate([v_arr, ints_to_arr([late[0]])]), ops + [M], members=True)
        assert e.value.bad_op == n
    finally:
        sync(c)
        for t in reversed(trees):
            t.close()


# ---------------------------------------------------------------- 3. refusals
def test_refusals(imt, forms):
    c, f, lib = forms["default"], imt._ffi, imt.lib
    E = f.ERR
    depth, cap = 32, 8
    stored = [10, 20, 30]
    t = imt.IndexedTree(c, depth, cap)
    view = None
    try:
        t.apply_batch(stored[:2])
        view = t.view(3)
        view.root()
        t.apply_batch(stored[2:])
        view_root = view.root()
        builds = view.stats()[1]
        before = state_of(t)

        def refused(which, script, want_rc, want_bad, flags, dev, words=None, tag=""):
            handle = view.h if which == "view" else t.h
            v_arr, ops = split(script)
            call = Call(imt, depth, len(script), dev or "pipelined" in which)
            rc = call.run(which, handle, v_arr, ops, flags)
            tag = (which, script, dev, tag, rc, lib.imt_last_error(c.h))
            assert rc == want_rc, tag
            assert call.untouched(), tag
            if which.endswith("filtered"):
                assert call.n_ins == 0 and call.n_rd == 0, tag            # the counts are 0 on every error
            else:
                assert call.n_ins == UNSET and call.bad == (UNSET if want_bad is None else want_bad), tag
            if words:
                assert words in lib.imt_last_error(c.h), tag
            assert state_of(t) == before and view.root() == view_root and view.stats()[1] == builds, tag

        strict = [w for w in CALLS if not w.endswith("filtered")]
        # IMT_ERR_VALUE with the flag; the view holds {10, 20}, so 30 counts as an in-list INSERT there
        for dev in (False, True):
            for which in strict:
                if which == "view":
                    # the list of a replay starts with the INSERT the tree made: leaf 3 = 30
                    cases = [([(I, 30), (M, 0)], 1), ([(M, 30), (I, 30)], 0), ([(I, 30), (M, 30), (M, 40)], 2),
                             ([(R, 5), (M, 10), (R, 10)], 2), ([(M, 10), (M, 5), (M, 0)], 1)]
                else:
                    cases = [([(M, 10), (M, 0)], 1),                                   # 0
                             ([(M, 5)], 0),                                            # neither stored nor inserted
                             ([(M, 40), (I, 40)], 0),                                  # a later INSERT does not help
                             ([(I, 40), (M, 40), (M, 41), (R, 40)], 2),                # the smallest position over all kinds
                             ([(I, 40), (R, 40), (M, 41)], 1),
                             ([(M, 10), (I, 10), (M, 11)], 1),                         # the INSERT rule is unchanged
                             ([(M, 30), (R, 30)], 1)]                                  # and so is the READ rule
                for script, bad in cases:
                    refused(which, script, E["VALUE"], bad, f.MEMBER_OPS, dev)
        # IMT_ERR_FULL counts INSERTs only: five leaves free ... four, the tree holds 4 of 8
        for which in ("mixed", "apply_mixed"):
            refused(which, [(I, 40 + i) for i in range(5)] + [(M, 10)], E["FULL"], None, f.MEMBER_OPS, False)
        ok = Call(imt, depth, 7)
        twin = imt.IndexedTree(c, depth, cap)
        twin.apply_batch(stored)
        assert ok.run("apply_mixed", twin.h, *split([(I, 40 + i) for i in range(4)] + [(M, 10), (M, 43), (M, 30)]), f.MEMBER_OPS) == 0
        assert ok.n_ins == 4 and twin.size == 8
        twin.close()
        # with the flag op 3 and op 255 are IMT_ERR_ARG through both kinds of pointer, by all seven calls
        for dev in (False, True):
            for which in CALLS:
                for byte in (3, 255):
                    refused(which, [(M, 10), (byte, 11)], E["ARG"], None, f.MEMBER_OPS, dev, ALL_THREE)
        # without the flag op 2 is refused by all seven, in today's words
        for dev in (False, True):
            for which in CALLS:
                refused(which, [(R, 11), (M, 10)], E["ARG"], None, 0, dev, TODAY)
                assert ALL_THREE not in lib.imt_last_error(c.h)
        # placed and partitioned trees stay refused either way
        placed = imt.IndexedTree(c, 8, 64)
        placed.set_placement(10, 1)
        call = Call(imt, 8, 1)
        assert call.run("mixed", placed.h, *split([(M, 10)]), f.MEMBER_OPS) == E["ARG"] and call.untouched()
        placed.close()
        # and the calls work afterwards
        n_ins, root = t.apply_mixed(*split([(M, 30), (I, 40), (M, 40)]), members=True)
        assert n_ins == 1 and t.size == 5
    finally:
        if view is not None:
            view.close()
        t.close()


# ---------------------------------------------------------------- 4. the filtered twins
def test_filtered_twins(imt, forms):
    c, f = forms["default"], imt._ffi
    depth, cap = 32, 64
    stored = [10, 20, 30]
    # every status under every kind: ZERO, PRESENT, REPEATED, NEW x INSERT, READ, MEMBER; 50 is inserted at position 3
    script = [(I, 0), (R, 0), (M, 0),
              (I, 50), (I, 20), (R, 30), (M, 10),
              (I, 50), (R, 50), (M, 50),
              (I, 60), (R, 70), (M, 80),
              (M, 70), (I, 70), (M, 70), (M, 30), (R, 25), (M, 60), (I, 25), (M, 25), (R, 26)]
    v_arr, ops = split(script)
    n = len(script)
    model = MemberModel(depth, cap)
    model.insert(stored)
    status, leaf, carried, (acc, reads) = model.mixed_filtered([v for _, v in script], ops)
    assert {(op, s) for (op, _), s in zip(script, status)} == {(k, s) for k in (I, R, M) for s in (ZERO, PRESENT, REPEATED, NEW)}
    assert NONE in leaf
    n_ins, n_rd = len(acc), len(carried) - len(acc)
    trees = [imt.IndexedTree(c, depth, cap) for _ in range(6)]
    try:
        for t in trees:
            t.apply_batch(stored)
        strict_t, a_t = trees[0], trees[1]
        # the strict call on the carried-out operations, with the same flags
        want_ins, want_rd = strict_t.mixed_batch(v_arr[carried], [ops[p] for p in carried], members=True)
        assert [int(x) for x in want_rd["low_index"]] == [low for _, low, _, _, _ in reads]
        for j, (dev, item_major) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            tag = f"dev {dev} item_major {item_major}"
            t = trees[2 + j]
            call = Call(imt, depth, n, dev, item_major)
            rc = call.run("mixed_filtered", t.h, v_arr, ops, f.MEMBER_OPS | (f.SIB_ITEM_MAJOR if item_major else 0))
            assert rc == 0, (tag, imt.lib.imt_last_error(c.h))
            got = call.host()
            assert got["extra"]["status"].tolist() == status and got["extra"]["leaf_index"].tolist() == leaf, tag
            assert (call.n_ins, call.n_rd) == (n_ins, n_rd), tag
            for part, want, m in (("ins", want_ins, n_ins), ("rd", want_rd, n_rd)):
                for key, a in cut(got[part], m, n, item_major).items():
                    w = want[key]
                    if key.endswith("_sib") and item_major:
                        w = w.transpose(1, 0, 2)
                    assert a.shape == w.shape and (a == w).all(), f"{tag}: {part}.{key}"
            same_tree(t, strict_t, tag)
        # the witness-free twin: the same classification, counts, tree and root
        st, lf, a_ins, a_rd, root = a_t.apply_mixed_filtered(v_arr, ops, members=True)
        assert st.tolist() == status and lf.tolist() == leaf and (a_ins, a_rd) == (n_ins, n_rd) and root == strict_t.root()
        same_tree(a_t, strict_t, "apply_mixed_filtered")
        # the Python wrapper of the witness form cuts the rows to the carried-out operations
        ins, rd, st, lf = a_t.mixed_filtered(ints_to_arr([10, 70, 90, 91]), [M, M, M, I], members=True)
        assert st.tolist() == [PRESENT, PRESENT, NEW, NEW] and int(lf[2]) == NONE and rd["low_index"].shape[0] == 2
        assert arr_ints(rd["low_leaf"][:, 0]) == [10, 70]
    finally:
        for t in trees:
            t.close()


# ---------------------------------------------------------------- the C example
def test_member_example(imt, oracle):
    """examples/member_reads_demo.c emits a value and proves it present in one block, checks every row as a consumer would,
    and has a block whose MEMBER comes before its INSERT refused: its rows against the oracle's"""
    import os
    import subprocess
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, csrc = os.path.join(root_dir, "examples", "member_reads_demo"), os.path.join(root_dir, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(root_dir, "include"),
                        os.path.join(root_dir, "examples", "member_reads_demo.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    script = list(zip([R, I, I, M, M, M], [45, 45, 50, 45, 30, 60]))
    _, want_rd, (root, _) = oracle_walk(oracle, 8, 64, [30, 60], script)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for (op, v), o in zip([x for x in script if x[0] != I], want_rd):
        word = "present" if op == M else "absent "
        val, nxt = arr_ints(o["low_leaf"])[:2]
        line = f"{v} is {word}: leaf {o['low']} {{{val} -> {nxt}}}{' (the largest)' if o['largest'] else ''}, against root {o['root']:064x}"
        assert line in r.stdout, (line, r.stdout)
    assert "block of 6: 2 inserted, 4 rows, 0 bad" in r.stdout and "second block refused: operation 0" in r.stdout
    assert f"root {root:064x}\nmember reads demo ok" in r.stdout
