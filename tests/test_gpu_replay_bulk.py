"""GPU (MI355X): imt_itree_view_bulk_witness -- the bulk witness of a block the tree applied earlier.

The claim is an identity: the replay through a view at S writes byte for byte what imt_itree_insert_bulk writes on a fresh
tree fed the first S - 1 values and given the values of leaves [S, S + n), and no call can tell the tree from one that was
never replayed.  Expected values are tests/bulk_model.py's (the walk over a sparse tree of the oracle's hashes), a live
imt_itree_insert_bulk, a later view of the same tree, or the stateless checkers; every comparison is bit-exact.

  test_model                       every shape of test_gpu_bulk.shapes(): depths 3, 8, 32, thread and quad forms, the tree
                                   further on and exactly at S + n; the tree the same before and after
  test_equals_live                 the bytes of the live call, again after the tree grew three ways, after reserve, after rewind
  test_cut_differently             blocks that went in as 20 + 13 replayed as 33, one of 33 replayed as 20 + 13
  test_frontier_is_the_later_tree  append_sib against the proof of slot S in the view at S + n, and the empty subtrees
  test_stateless_checks            2^12 values behind 2^14 leaves through the stateless calls alone, device pointers
  test_formats_and_pointers        both formats, both layouts, host and device pointers, NULL fields, the bytes behind
  test_arguments                   every refusal with outputs and tree untouched
  test_follows_and_coexists        two views in turn, between the other replays of one view, behind batches in flight
  test_example                     examples/late_bulk_demo.c
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bulk_model as bm
import test_gpu_insert_matrix as tm
from oracle_lib import arr_ints, ints_to_arr
from test_gpu_bulk import FIELDS, check_model, fresh, shapes
from test_gpu_rewind import forms  # noqa: F401  (the fixture: one context per hash form)

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64                      # bytes of FILL behind every output array
WIDE = ("order", "low_index")


def field_shapes(n, depth, item_major):
    return dict(order=(n, 8), low_index=(n, 8), low_leaf=(n, 3, 32), is_largest=(n,), root_before=(n, 32), root_after=(n, 32),
                low_sib=(n, depth, 32) if item_major else (depth, n, 32), new_leaf=(n, 3, 32), append_sib=(depth, 32),
                root=(32,))


class Raw:
    """imt_itree_view_bulk_witness into buffers of its own: every byte FILL, PAD more bytes of FILL behind each array"""

    def __init__(self, imt, depth, n, item_major=False, dev=False, fields=FIELDS):
        self.imt, self.dev, self.item = imt, dev, item_major
        self.shapes = {k: field_shapes(max(n, 1), depth, item_major)[k] for k in (fields or ())}
        self.null = fields is None
        flat = {k: np.full(int(np.prod(s)) + PAD, FILL, np.uint8) for k, s in self.shapes.items()}
        if dev:
            import torch
            flat = {k: torch.from_numpy(a).cuda() for k, a in flat.items()}
        self.flat = flat

    def call(self, vh, n, flags=0):
        f, lib = self.imt._ffi, self.imt.lib
        ptr = (lambda x: x.data_ptr()) if self.dev else (lambda x: x.ctypes.data)
        out = None if self.null else ctypes.byref(f.BulkOut(**{k: ptr(x) for k, x in self.flat.items()}))
        return lib.imt_itree_view_bulk_witness(vh, n, out, flags | (f.DEVICE_PTRS if self.dev else 0) |
                                               (f.SIB_ITEM_MAJOR if self.item else 0))

    def host(self, ctx=None):
        """the arrays in the shapes of IndexedTree.insert_bulk's dict; the padding must be as it was"""
        if self.dev:
            import torch
            ctx.sync()
            torch.cuda.synchronize()
        res = {}
        for k, a in self.flat.items():
            a = a.cpu().numpy() if self.dev else a
            assert (a[-PAD:] == FILL).all(), f"bytes behind {k} were written"
            b = a[:-PAD].reshape(self.shapes[k])
            res[k] = b.view(np.uint64).reshape(-1) if k in WIDE else b
        return res

    def untouched(self, ctx=None):
        if self.dev:
            import torch
            ctx.sync()
            torch.cuda.synchronize()
        return all(((a.cpu().numpy() if self.dev else a) == FILL).all() for a in self.flat.values())


def tree_state(t):
    return t.size, t.root(), t.snapshot().tobytes(), t.values().tobytes()


def same(a, b, tag=""):
    assert a.keys() == b.keys(), tag
    for k in a:
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), f"{tag}: {k}"


# ---------------------------------------------------------------- 1. the model, byte for byte
@pytest.mark.parametrize("form", ["thread", "quad"])
@pytest.mark.parametrize("depth", [3, 8, 32])
def test_model(imt, forms, oracle, depth, form):
    c, cap = forms[form], 1 << min(depth, 7)
    extra = fresh(5, 0x52424C00 + depth)
    for j, (name, (stored, vals)) in enumerate(shapes(depth).items()):
        tag, item_major = f"{name} depth {depth} {form}", bool(j & 1)
        want = bm.bulk_witness(oracle, depth, [0] + stored, vals)
        S, n = 1 + len(stored), len(vals)
        t = imt.IndexedTree(c, depth, cap)
        try:
            if stored:
                t.apply_batch(stored)
            t.apply_batch(vals)
            v = t.view(S)
            # the tree exactly at S + n, then 5 values further on -- as many of them as a tree of 2^3 leaves has room for
            for further in (False, True):
                if further:
                    more = [x for x in extra if x not in stored and x not in vals][:min(5, cap - t.size)]
                    if not more:
                        continue
                    t.apply_batch(more)
                before = tree_state(t)
                res = v.bulk_witness(n, item_major=item_major)
                check_model(res, want, n, item_major, f"{tag} further {further}")
                assert tree_state(t) == before, tag
                assert (res["root_before"][1:] == res["root_after"][:-1]).all(), tag
        finally:
            t.close()


# ---------------------------------------------------------------- 2. the live call's bytes, whatever the tree does next
def test_equals_live(imt, forms):
    import torch
    c, depth, cap = forms["default"], 32, 512
    f = fresh(400, 0x52424C10)
    stored, vals, more = f[:36], f[36:100], f[100:]
    t = imt.IndexedTree(c, depth, cap)
    try:
        t.apply_batch(stored)
        M = t.size
        assert M == 37
        live = t.insert_bulk(vals)
        v = t.view(M)
        same(v.bulk_witness(64), live, "right behind the live call")
        t.insert_batch(more[:30])
        d = torch.from_numpy(ints_to_arr(more[30:90])).cuda()
        t.apply_pipelined(d.data_ptr(), 60)
        t.insert_bulk(more[90:120])
        same(v.bulk_witness(64), live, "after three more batches")
        t.reserve(2 * cap)
        same(v.bulk_witness(64), live, "after reserve")
        t.rewind(M + 64)
        same(v.bulk_witness(64), live, "after the rewind to M + 64")
        same(v.bulk_witness(64, item_major=True), {k: (a.transpose(1, 0, 2) if k == "low_sib" else a) for k, a in live.items()},
             "item-major")
    finally:
        t.close()


# ---------------------------------------------------------------- 3. the blocks cut differently
def test_cut_differently(imt, forms, oracle):
    c, depth, cap = forms["default"], 32, 128
    f = fresh(60, 0x52424C20)
    stored, vals = f[:10], f[10:43]
    S = 11
    a, b = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    try:
        for t in (a, b):
            t.apply_batch(stored)
        a.apply_batch(vals[:20])
        a.apply_batch(vals[20:])
        b.apply_batch(vals)
        for t in (a, b):
            t.apply_batch(f[43:50])
        check_model(a.view(S).bulk_witness(33), bm.bulk_witness(oracle, depth, [0] + stored, vals), 33, False, "20 + 13 as 33")
        first, second = b.view(S).bulk_witness(20), b.view(S + 20).bulk_witness(13)
        check_model(first, bm.bulk_witness(oracle, depth, [0] + stored, vals[:20]), 20, False, "33 as 20")
        check_model(second, bm.bulk_witness(oracle, depth, [0] + stored + vals[:20], vals[20:]), 13, False, "33 as 13")
        assert (second["root_before"][0] == first["root"]).all()
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 4. the frontier is a row of the later tree
def test_frontier_is_the_later_tree(imt, forms):
    c, depth, cap = forms["default"], 32, 64
    f = fresh(50, 0x52424C30)
    Z = c.zero_hashes(depth)
    t = imt.IndexedTree(c, depth, cap)
    try:
        t.apply_batch(f[:40])
        for S in (1, 2, 7, 16, 21):
            for n in (1, 9):
                res = t.view(S).bulk_witness(n)
                later = t.view(S + n)
                proof = later.get_proof_batch(np.array([S], np.uint64))[:, 0]
                for l in range(depth):
                    want = proof[l] if (S >> l) & 1 else Z[l]
                    assert (res["append_sib"][l] == want).all(), (S, n, l)
                assert imt.to_int(res["root"]) == later.root(), (S, n)
    finally:
        t.close()


# ---------------------------------------------------------------- 5. the larger shape through the stateless calls
def test_stateless_checks(imt, forms):
    import torch
    c, depth, cap = forms["thread"], 32, 1 << 15
    S, n = 1 << 14, 1 << 12
    f = fresh(S - 1 + 2 * n, 0x52424C40)
    t = imt.IndexedTree(c, depth, cap)
    try:
        t.apply_batch(f[:S - 1])
        t.apply_batch(f[S - 1:S - 1 + n])
        t.apply_batch(f[S - 1 + n:])
        assert t.size == S + 2 * n
        v_arr = ints_to_arr(f[S - 1:S - 1 + n])
        before = tree_state(t)
        v = t.view(S)
        r = Raw(imt, depth, n, dev=True)
        assert r.call(v.h, n) == 0, imt.lib.imt_last_error(c.h)
        res = r.host(c)
        assert tree_state(t) == before
        order = res["order"].astype(np.int64)
        assert sorted(order.tolist()) == list(range(n)) and all(f[S - 1 + order[k]] > f[S - 1 + order[k + 1]] for k in range(n - 1))
        fail, root_out = c.non_membership(res["root_before"], res["low_leaf"], res["low_index"], res["low_sib"], depth,
                                          v_arr[order], res["is_largest"], want_root=True)
        assert not fail.any() and (root_out == res["root_before"]).all()
        rewritten = res["low_leaf"].copy()
        rewritten[:, 1] = v_arr[order]
        rewritten[:, 2] = ints_to_arr([S + int(i) for i in order])
        assert (c.path_root(c.hash3(rewritten), res["low_index"], res["low_sib"], depth) == res["root_after"]).all()
        assert (res["root_before"][1:] == res["root_after"][:-1]).all()
        root_before, root_after = c.frontier_append_root(res["append_sib"], S, depth, leaf3=res["new_leaf"])
        assert (root_before == res["root_after"][n - 1]).all() and (root_after == res["root"]).all()
        later = t.view(S + n)
        assert imt.to_int(res["root"]) == later.root() and imt.to_int(res["root_before"][0]) == v.root()
        assert (res["new_leaf"] == later.get_leaves(np.arange(S, S + n, dtype=np.uint64))).all()
    finally:
        t.close()


# ---------------------------------------------------------------- 6. the call surface
def test_formats_and_pointers(imt, forms):
    c, f = forms["default"], imt._ffi
    depth, cap = 32, 128
    vals = fresh(70, 0x52424C50)
    stored, batch = vals[:21], vals[21:60]
    n, S = len(batch), 22
    t = imt.IndexedTree(c, depth, cap)
    try:
        t.apply_batch(stored)
        want = t.insert_bulk(batch)
        t.apply_batch(vals[60:])
        before = tree_state(t)
        v = t.view(S)
        for fmt, item_major, dev in ((f.FMT_MONT256, True, False), (f.FMT_DEVICE, False, False), (f.FMT_CANONICAL, False, True),
                                     (f.FMT_MONT256, False, True), (f.FMT_DEVICE, True, True), (f.FMT_CANONICAL, True, False)):
            tag = f"fmt {fmt} item_major {item_major} dev {dev}"
            r = Raw(imt, depth, n, item_major, dev)
            assert r.call(v.h, n, fmt) == 0, tag
            for key, a in r.host(c).items():
                w = want[key]
                if key == "low_sib" and item_major:
                    w = w.transpose(1, 0, 2)
                if key not in ("order", "low_index", "is_largest"):
                    w = tm.to_fmt(np.ascontiguousarray(w), fmt)
                assert a.shape == w.shape and (a == w).all(), f"{tag}: {key}"
        # each pointer NULL in turn, and every other NULL
        for j, k in enumerate(FIELDS):
            for fields in (tuple(x for x in FIELDS if x != k), (k,)):
                dev = bool(j & 1)
                r = Raw(imt, depth, n, False, dev, fields)
                assert r.call(v.h, n) == 0, f"fields {fields}"
                for key, a in r.host(c).items():
                    assert (a == want[key]).all(), f"fields {fields}: {key}"
        r = Raw(imt, depth, n, False, False, ())
        assert r.call(v.h, n) == 0                              # a struct of NULLs: a call that writes nothing
        assert tree_state(t) == before
    finally:
        t.close()


def test_arguments(imt, forms):
    import torch
    c, f, lib, E = forms["default"], imt._ffi, imt.lib, imt._ffi.ERR
    depth, cap = 32, 64
    vals = fresh(50, 0x52424C60)
    t = imt.IndexedTree(c, depth, cap)
    placed, parted = imt.IndexedTree(c, 8, 16), imt.IndexedTree(c, 8, 16)
    try:
        t.apply_batch(vals[:30])
        before = tree_state(t)
        v, head = t.view(11), t.view(31)

        def refused(vh, code, n, flags=0, dev=False, null=False, d=depth):
            r = Raw(imt, d, min(n, cap), dev=dev, fields=None if null else FIELDS)
            rc = r.call(vh, n, flags)
            assert rc == (0 if code is None else E[code]), (rc, code, n, flags, lib.imt_last_error(c.h))
            assert r.untouched(c), (code, n, flags)

        refused(v.h, "ARG", 5, null=True)
        refused(v.h, "ARG", 0, null=True)
        refused(v.h, None, 0)
        refused(head.h, None, 0)
        refused(v.h, "RANGE", 21)                               # one past the tree's size
        refused(v.h, "RANGE", 1 << 40)
        refused(head.h, "RANGE", 1)                             # the view at the current size: nothing follows it
        for flags, dev in ((f.PIPELINE, False), (f.PIPELINE, True), (3, False)):
            refused(v.h, "ARG", 5, flags, dev=dev)
        refused(None, "ARG", 5)
        refused(t.h, "ARG", 5)                                  # a tree's handle is no view
        # IMT_HOST_PREP and IMT_INPUTS_READY change nothing
        want = v.bulk_witness(20)
        for flags in (f.HOST_PREP, f.INPUTS_READY):
            r = Raw(imt, depth, 20)
            assert r.call(v.h, 20, flags) == 0
            same(r.host(), want, f"flags {flags:#x}")
        # misaligned device order / low_index
        buf = torch.full((20 * 8 + 64,), FILL, dtype=torch.uint8, device="cuda")
        for field in ("order", "low_index"):
            o = f.BulkOut(**{field: buf.data_ptr() + 4})
            assert lib.imt_itree_view_bulk_witness(v.h, 20, ctypes.byref(o), f.DEVICE_PTRS) == E["ARG"], field
        for field in ("low_leaf", "root_before", "root_after", "low_sib", "new_leaf", "append_sib", "root"):
            o = f.BulkOut(**{field: buf.data_ptr() + 8})
            assert lib.imt_itree_view_bulk_witness(v.h, 1, ctypes.byref(o), f.DEVICE_PTRS) == E["ARG"], field
        c.sync()
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == FILL).all()
        assert tree_state(t) == before
        # a view ahead of a rewound tree, which answers again once the tree has grown
        w = t.view(25)
        want_w = w.bulk_witness(6)
        t.rewind(20)
        refused(w.h, "RANGE", 3)
        refused(w.h, "RANGE", 0)
        t.apply_batch(vals[19:30])
        same(w.bulk_witness(6), want_w, "the tree grown again")
        assert tree_state(t) == before
        # a placed tree and a partitioned tree: refused as imt_itree_insert_bulk refuses them
        placed.set_placement(12, 3)
        placed.apply_batch(vals[:6])
        pv = placed.view(3)
        refused(pv.h, "ARG", 2, d=8)
        assert b"bulk batches are not available on a placed or partitioned tree" in lib.imt_last_error(c.h)
        assert lib.imt_itree_set_value_partition(parted.h, 4, 1) == 0
        mine = [x for x in vals if x % 4 == 1][:4]
        parted.apply_batch(mine)
        qv = parted.view(2)
        refused(qv.h, "ARG", 2, d=8)
        # a freed view handle
        h = ctypes.c_void_p(v.h.value)
        v.close()
        refused(h, "ARG", 5)
    finally:
        for x in (t, placed, parted):
            x.close()


def test_follows_and_coexists(imt, forms):
    import torch
    c, f, lib = forms["default"], imt._ffi, imt.lib
    depth, cap = 32, 4096
    vals = fresh(1700, 0x52424C70)
    t, twin = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    try:
        t.apply_batch(vals[:40])
        twin.apply_batch(vals[:20])
        want_a = twin.insert_bulk(vals[20:40])                  # what the view at 21 replays
        twin.rewind(31)
        want_b = twin.insert_bulk(vals[30:40])                  # and the view at 31
        a, b = t.view(21), t.view(31)
        stats = t.apply_stats().tolist()
        for view, want, n in ((a, want_a, 20), (b, want_b, 10), (a, want_a, 20), (b, want_b, 10)):
            same(view.bulk_witness(n), want, f"view at {view.size}")
        # between the other two replays of the same view: one plan set serves all three
        ops = [0] * 20
        m1 = a.mixed_witness(vals[20:40], ops)[0]
        same(a.bulk_witness(20), want_a, "behind a mixed replay")
        i1 = a.insert_witness(20)
        same(a.bulk_witness(7), twin_rows(imt, c, depth, vals[:20], vals[20:27]), "a shorter one")
        m2 = a.mixed_witness(vals[20:40], ops)[0]
        same(m1, m2, "the mixed replay again")
        same(i1, a.insert_witness(20), "the insertion replay again")
        assert t.apply_stats().tolist() == stats
        assert a.stats()[1] == 1 and b.stats()[1] == 1, "one build serves every replay of an unchanged tree"
        # right behind pipelined batches still in flight: nothing synchronised by the caller
        d1, d2 = (torch.from_numpy(ints_to_arr(x)).cuda() for x in (vals[40:640], vals[640:1240]))
        rc = lib.imt_itree_insert_batch(t.h, ctypes.c_void_p(d1.data_ptr()), 600, None, f.DEVICE_PTRS | f.PIPELINE)
        assert rc == 0
        t.apply_pipelined(d2.data_ptr(), 600)
        res = a.bulk_witness(20 + 1200)
        same(res, twin_rows(imt, c, depth, vals[:20], vals[20:1240]), "behind batches in flight")
        assert t.size == 1241
    finally:
        t.close()
        twin.close()


def twin_rows(imt, c, depth, stored, vals):
    """imt_itree_insert_bulk of vals on a fresh tree fed `stored`"""
    t = imt.IndexedTree(c, depth, 4096)
    try:
        t.apply_batch(stored)
        return t.insert_bulk(vals)
    finally:
        t.close()


def test_example(imt, forms, oracle):
    """examples/late_bulk_demo.c: a sequencer applies three blocks without witnesses, a prover then takes the bulk witness of
    the second through a view and re-checks it with the stateless calls alone; its roots against the model's"""
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, csrc = os.path.join(root_dir, "examples", "late_bulk_demo"), os.path.join(root_dir, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(root_dir, "include"),
                        os.path.join(root_dir, "examples", "late_bulk_demo.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    b1, b2, b3 = [20, 50, 90], [30, 70, 45, 10, 65, 25], [15, 85, 60]
    want = bm.bulk_witness(oracle, 8, [0] + b1, b2)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for k, row in enumerate(want["rows"]):
        assert f"row {k}: value {b2[row['order']]} (position {row['order']}), low leaf {row['low_index']} " in r.stdout, r.stdout
        assert f"root after {row['root_after']:064x}" in r.stdout, r.stdout
    assert f"append of 6 leaves at slot 4, root {want['root']:064x}" in r.stdout, r.stdout
    after3 = bm.bulk_witness(oracle, 8, [0] + b1 + b2, b3)["root"]
    assert f"sequencer: 3 blocks applied, 13 leaves, root {after3:064x}" in r.stdout, r.stdout
    assert "late bulk witness of block 2: 6 rows and the append of 6 leaves, all satisfied" in r.stdout
