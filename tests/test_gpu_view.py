"""GPU (MI355X): imt_itree_view_* -- the tree read as it was at an earlier size while it stays where it is.

The claim under test is an identity: through no query can a view at size s be told from a fresh tree that received the
first s - 1 values, and through no call can the tree be told from one that never had a view.  Expected values are the
sequential oracle's (tests/insert_corpus.py, test_gpu_rewind.prefix_trees) or a twin tree's; every comparison is bit-exact.

  test_view_scenarios   every scenario of the corpus on the three hash forms, apply and witness batches taking turns.  After
                        every batch the views at size 1 and at every earlier batch boundary -- created once, when the tree
                        had that size -- answer root, get_leaves and get_proof_batch at query_indices as the oracle's
                        prefix tree does, and have hashed what the definition says.  At the end the tree is the corpus's.
  test_view_formats     one scenario through IMT_FMT_MONT256, IMT_FMT_DEVICE, and level-major with device pointers.
  test_view_witnesses   lookup and non_membership_witness of a view at the middle boundary against a twin that holds only
                        that prefix; the witnesses verify against the view's root; a present candidate is refused.
  test_view_follows     a view while the tree grows (pipelined device batches left in flight, apply batches), is rewound
                        above and below the view's size, and grows again along another history.
  test_view_large       a view 2^16 insertions behind a tree of 2^20 + 2^16 + 1 leaves against a twin without them, both
                        forms of the hash kernels; the queried siblings cover side table, stored nodes and empty subtrees.
  test_view_arguments   every refusal with tree and view untouched, the view at the current size, two views, NULL.
  test_view_sliced      creation refused on a replica with steps in flight, works after the flush.
  test_finalized_reads_example   examples/finalized_reads_demo.c: its roots against the oracle's.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import insert_corpus as ic
import oracle_lib
import test_gpu_insert_matrix as tm
import test_gpu_rewind as tr
from oracle_lib import arr_ints, ints_to_arr
from test_gpu_rewind import forms  # noqa: F401  (the fixture: one context per hash form)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64p = ctypes.POINTER(ctypes.c_uint64)


def check_view(v, sc, want, idx, tag):
    """every query of the view against the oracle's tree of that size"""
    assert v.root() == want["root"], f"{tag}: root"
    gidx = np.array(idx, np.uint64) + np.uint64(sc.index_base)
    pre = v.get_leaves(gidx)
    bad = np.nonzero((pre != want["preimages"]).reshape(len(idx), -1).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: preimage of leaf {idx[bad[0]]}"
    proofs = v.get_proof_batch(gidx, item_major=True)
    bad = np.argwhere((proofs != want["proofs"]).any(axis=2))
    assert bad.size == 0, f"{tag}: proof of leaf {idx[bad[0][0]]} level {bad[0][1]}"


def grow(t, vals, bounds, first=0):
    """the corpus's batches from `first` on, apply and witness batches taking turns; yields the size after each"""
    for j, (a, b) in enumerate(bounds):
        if j < first:
            continue
        if j % 2 == 0:
            t.apply_batch(ints_to_arr(vals[a:b]))
        else:
            t.insert_batch(ints_to_arr(vals[a:b]))
        yield j, b + 1


# ---------------------------------------------------------------- every scenario, every boundary
@pytest.mark.parametrize("name,form", tr._scenario_cases())
def test_view_scenarios(imt, forms, name, form):
    sc, exp, trees = ic.BY_NAME[name], ic.expected(name), tr.prefix_trees(name)
    vals, idx = exp["vals"], tr.query_indices(sc, len(exp["vals"]))
    t = tr.new_tree(imt, forms[form], sc)
    try:
        views, born = {1: t.view(1)}, {1: 0}                 # size -> view, and the batches applied when it was made
        assert views[1].stats()[1] == 0
        for j, M in grow(t, vals, ic.batch_bounds(sc)):
            for s, v in views.items():
                tag = f"{name} view at {s} of {M}"
                check_view(v, sc, trees[s], idx, tag)
                hashes, builds = v.stats()
                assert hashes.tolist() == tr.rewind_counts(trees[M], trees[s], idx, M, s, sc.depth), f"{tag}: hashes per level"
                assert builds == j + 1 - born[s] + (s > 1), f"{tag}: one rebuild per batch since it was made"
            v = views[M] = t.view(M)                          # at the current size: the tree answers, nothing is hashed
            born[M] = j + 1
            check_view(v, sc, trees[M], idx, f"{name} view at the current size {M}")
            assert v.stats()[0].tolist() == [0] * (sc.depth + 1) and v.stats()[1] == 1
        # the views wrote nothing: the tree is the corpus's final tree
        fin = exp["final"]
        assert t.size == fin["size"] and t.root() == fin["root"]
        assert (t.get_leaves(fin["index"]) == fin["preimages"]).all()
        assert (t.get_proof_batch(fin["index"], item_major=True) == fin["proofs"]).all()
    finally:
        t.close()


def test_view_formats(imt, forms):
    """d32_between, the view at the middle boundary of the finished tree: the raw calls with IMT_FMT_MONT256 and
    IMT_FMT_DEVICE (item-major, host pointers) and canonical level-major with device pointers"""
    import torch
    name = "d32_between"
    sc, exp, trees = ic.BY_NAME[name], ic.expected(name), tr.prefix_trees(name)
    c, f, lib = forms["default"], imt._ffi, imt.lib
    vals, bounds = exp["vals"], ic.batch_bounds(sc)
    idx = tr.query_indices(sc, len(vals))
    s = bounds[len(bounds) // 2][0] + 1
    want, n, d = trees[s], len(idx), sc.depth
    t = tr.new_tree(imt, c, sc)
    try:
        list(grow(t, vals, bounds))
        v = t.view(s)
        gidx = np.array(idx, np.uint64)
        P_ = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for fmt in (f.FMT_MONT256, f.FMT_DEVICE):
            root, pre, sib = np.zeros(32, np.uint8), np.zeros((n, 3, 32), np.uint8), np.zeros((n, d, 32), np.uint8)
            assert lib.imt_itree_view_root(v.h, P_(root), fmt) == 0
            assert lib.imt_itree_view_get_leaves(v.h, P_(gidx), n, P_(pre), fmt) == 0
            assert lib.imt_itree_view_get_proof_batch(v.h, P_(gidx), n, P_(sib), fmt | f.SIB_ITEM_MAJOR) == 0
            assert (root == tm.to_fmt(ints_to_arr([want["root"]]), fmt)[0]).all(), fmt
            assert (pre == tm.to_fmt(want["preimages"], fmt)).all(), fmt
            assert (sib == tm.to_fmt(want["proofs"], fmt)).all(), fmt
        dev = lambda x: ctypes.c_void_p(x.data_ptr())
        d_idx = torch.from_numpy(gidx.view(np.int64)).cuda()
        d_root = torch.zeros(32, dtype=torch.uint8, device="cuda")
        d_pre = torch.zeros((n, 3, 32), dtype=torch.uint8, device="cuda")
        d_sib = torch.zeros((d, n, 32), dtype=torch.uint8, device="cuda")
        assert lib.imt_itree_view_root(v.h, dev(d_root), f.DEVICE_PTRS) == 0
        assert lib.imt_itree_view_get_leaves(v.h, dev(d_idx), n, dev(d_pre), f.DEVICE_PTRS) == 0
        assert lib.imt_itree_view_get_proof_batch(v.h, dev(d_idx), n, dev(d_sib), f.DEVICE_PTRS) == 0
        c.sync()
        torch.cuda.synchronize()
        assert arr_ints(d_root.cpu().numpy())[0] == want["root"]
        assert (d_pre.cpu().numpy() == want["preimages"]).all()
        assert (d_sib.cpu().numpy().transpose(1, 0, 2) == want["proofs"]).all()
        assert v.stats()[1] == 1
    finally:
        t.close()


# ---------------------------------------------------------------- witnesses
@pytest.mark.parametrize("name", ["d32_between", "placed_g5"])
def test_view_witnesses(imt, forms, name):
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    c, f = forms["default"], imt._ffi
    vals, bounds = exp["vals"], ic.batch_bounds(sc)
    s = bounds[len(bounds) // 2][0] + 1
    kept, later = vals[:s - 1], vals[s - 1:]
    allv = set(vals)
    between = [x + 1 for x in sorted(kept) if x + 1 not in allv and x + 1 < oracle_lib.P][:24]
    above = max(kept) + 1
    while above in allv:
        above += 1
    assert above < oracle_lib.P
    absent = later + between + [above]
    t, twin = tr.new_tree(imt, c, sc), tr.new_tree(imt, c, sc)
    try:
        list(grow(t, vals, bounds))
        twin.apply_batch(ints_to_arr(kept))
        v = t.view(s)
        assert v.root() == twin.root() == exp["batch_roots"][len(bounds) // 2]
        # lookup: every class, the twin's answer
        st, leaf = v.lookup(ints_to_arr(kept + absent + [0]))
        st2, leaf2 = twin.lookup(ints_to_arr(kept + absent + [0]))
        assert (st == st2).all() and (leaf == leaf2).all()
        assert (st[:len(kept)] == f.VAL_PRESENT).all() and (st[len(kept):-1] == f.VAL_NEW).all() and st[-1] == f.VAL_ZERO
        assert (leaf[len(kept):-1] - np.uint64(sc.index_base) < s).all(), "a low leaf is a kept leaf"
        # witnesses of the absent values: the twin's, and they verify against the view's root
        got, want = v.non_membership_witness(ints_to_arr(absent)), twin.non_membership_witness(ints_to_arr(absent))
        for g, w, what in zip(got, want, ("low_index", "low_leaf", "low_sib", "is_largest")):
            assert (g == w).all(), what
        low, leaves, sib, largest = got
        assert largest[-1] == 1 and largest[:-1].sum() == sum(x > max(kept) for x in absent[:-1])
        fail = c.non_membership(ints_to_arr([v.root()])[0], leaves, low - np.uint64(sc.index_base), sib, sc.depth,
                                ints_to_arr(absent), largest)
        assert not fail.any(), fail
        # a present value, 0: no witness, as on a tree; the values after the cut are not present
        for bad in (absent[:3] + [kept[0]], [0] + absent[:3]):
            with pytest.raises(ValueError):
                v.non_membership_witness(ints_to_arr(bad))
            with pytest.raises(ValueError):
                twin.non_membership_witness(ints_to_arr(bad))
        if name == "placed_g5":
            # the partitioned case: a foreign residue is FOREIGN to lookup and refused by the witness call, as on the twin
            m = 5
            r = kept[0] % m
            for x in (t, twin):
                imt.lib.imt_itree_set_value_partition(x.h, m, r)
            probe = kept + absent
            st, leaf = v.lookup(ints_to_arr(probe))
            st2, leaf2 = twin.lookup(ints_to_arr(probe))
            assert (st == st2).all() and (leaf == leaf2).all()
            assert any(a == f.VAL_FOREIGN for a in st) and st[0] == f.VAL_PRESENT
            foreign = next(x for x in absent if x % m != r)
            own = [x for x in absent if x % m == r][:4]
            assert own
            g, w = v.non_membership_witness(ints_to_arr(own)), twin.non_membership_witness(ints_to_arr(own))
            assert all((a == b).all() for a, b in zip(g, w))
            for x in (v, twin):
                with pytest.raises(ValueError):
                    x.non_membership_witness(ints_to_arr(own + [foreign]))
        assert v.stats()[1] == 1 and t.root() == exp["final"]["root"]
    finally:
        t.close()
        twin.close()


# ---------------------------------------------------------------- the view follows the tree
def test_view_follows(imt, forms):
    name = "d32_between"
    sc, exp, trees = ic.BY_NAME[name], ic.expected(name), tr.prefix_trees(name)
    c, f = forms["default"], imt._ffi
    vals, bounds = exp["vals"], ic.batch_bounds(sc)
    idx = tr.query_indices(sc, len(vals))
    s = bounds[2][0] + 1                                           # after two batches
    t = tr.new_tree(imt, c, sc)
    try:
        list(zip(range(2), grow(t, vals, bounds)))
        assert t.size == s
        v = t.view(s)
        assert v.stats()[1] == 0
        check_view(v, sc, trees[s], idx, "at the current size")
        check_view(v, sc, trees[s], idx, "again, nothing changed")
        assert v.stats()[1] == 1
        # pipelined device batches left in flight: the query orders itself behind them
        dv = tr.DeviceBatches(imt, c, t, sc.global_depth)
        for a, b in bounds[2:5]:
            dv.insert(ints_to_arr(vals[a:b]), want_outputs=False)
        check_view(v, sc, trees[s], idx, "behind pipelined batches in flight")
        assert v.stats()[1] == 2
        dv.sync()
        check_view(v, sc, trees[s], idx, "after the sync")
        assert v.stats()[1] == 2
        for a, b in bounds[5:]:
            t.apply_batch(ints_to_arr(vals[a:b]))
        M = len(vals) + 1
        check_view(v, sc, trees[s], idx, "after apply batches")
        assert v.stats()[1] == 3 and v.stats()[0].tolist() == tr.rewind_counts(trees[M], trees[s], idx, M, s, sc.depth)
        # back to a size above the view's: same answers
        mid = bounds[4][0] + 1
        assert t.rewind(mid) == trees[mid]["root"]
        check_view(v, sc, trees[s], idx, "after a rewind above it")
        assert v.stats()[1] == 4 and v.stats()[0].tolist() == tr.rewind_counts(trees[mid], trees[s], idx, mid, s, sc.depth)
        assert t.rewind(mid) == trees[mid]["root"]                # k = 0 changes nothing: no rebuild
        assert v.root() == trees[s]["root"] and v.stats()[1] == 4
        # below the view's size: nothing to answer from, but the view stays
        low = bounds[1][0] + 1
        t.rewind(low)
        for call in (v.root, lambda: v.get_leaves([0]), lambda: v.get_proof_batch([0]), lambda: v.lookup([5]),
                     lambda: v.non_membership_witness([5])):
            with pytest.raises(imt.ImtError) as ei:
                call()
            assert ei.value.code == f.ERR["RANGE"]
        assert v.stats()[1] == 4 and t.size == low and t.root() == trees[low]["root"]
        # another history past s: the view answers for its prefix
        used = set(vals)
        other = [x for x in oracle_lib.synth_values(len(vals) + 8, 0x56574600) if x not in used]
        fork = vals[:low - 1] + other[:len(vals) - (low - 1)]
        t.apply_batch(ints_to_arr(fork[low - 1:s + 20]))
        orc = oracle_lib.load()
        h = orc.sparse_new(sc.depth, sc.cap)
        try:
            for x in fork[:s - 1]:
                assert orc.sparse_insert(h, sc.depth, x)["rc"] == 0
            proofs, pre = ic._snapshot(orc, h, sc.depth, idx)
            want = dict(root=orc.sparse_root(h), proofs=proofs, preimages=pre)
        finally:
            orc.sparse_free(h)
        check_view(v, sc, want, idx, "the new history's prefix")
        assert v.stats()[1] == 5 and want["root"] != trees[s]["root"]
    finally:
        t.close()


# ---------------------------------------------------------------- a size users run
def ceil_div(a, l):
    return -(-a // (1 << l))


def test_view_large(imt, forms):
    """Twins a and b apply the same 2^20 random values, a applies 2^16 more; the view of a at 2^20 + 1 leaves against b.
    About 63 000 kept leaves lose their successor, so on the default context (switch at 16384) the leaf launch and the
    low levels take the thread form k_view_level and the upper ones the quad form; a second context with the switch at
    2^30 runs every launch in the quad form, a third with 0 every one in the thread form.  The queried leaves are chosen
    here on the CPU: every leaf of S_0, its sibling, and 4096 random ones; that their proofs read all three sources at
    every level that has all three is asserted from the sorted order of the values, not from the library."""
    import torch
    depth, cap, M0, n = 32, 1 << 21, 1 << 20, 1 << 16
    allv = oracle_lib.synth_values(M0 + n + 4096, 0x56574C20)
    base_vals, new_vals, probes = allv[:M0], allv[M0:M0 + n], allv[M0 + n:]
    leafvals = [0] + base_vals + new_vals
    order = sorted(range(len(leafvals)), key=leafvals.__getitem__)
    s, M = M0 + 1, M0 + n + 1
    S0 = {s} | {order[j] for j in range(len(order) - 1) if order[j] < s <= order[j + 1]}
    l0 = tr.ceil_log2(M)
    levels, S = [], set(S0)
    for l in range(depth + 1):
        levels.append(S)
        S = {x >> 1 for x in S}
    want_hashes = [len(levels[l]) if l < l0 else 1 for l in range(depth + 1)]
    assert want_hashes[1] > 16384 >= want_hashes[7], "these values must make both forms of k_view_level run"
    rng = np.random.default_rng(0x56574C21)
    S0a = np.array(sorted(S0), np.uint64)
    idx = np.unique(np.concatenate([S0a, S0a ^ np.uint64(1), rng.integers(0, M + 1, 4096).astype(np.uint64)]))
    # the sources of the queried siblings, by the rule: level l < ceil_log2(s) has all three kinds of node when some node
    # is in S_l, some filled node is not, and the level's capacity exceeds what s fills
    for l in range(tr.ceil_log2(s)):
        sib = set(((idx >> np.uint64(l)) ^ np.uint64(1)).tolist())
        fill = ceil_div(s, l)
        have = {"empty": any(x >= fill for x in sib), "side": any(x < fill and x in levels[l] for x in sib),
                "stored": any(x < fill and x not in levels[l] for x in sib)}
        exists = {"empty": (cap >> l) > fill, "side": any(x < fill for x in levels[l]), "stored": fill > len(levels[l])}
        for k in have:
            assert have[k] or not exists[k], f"level {l}: no queried sibling from the {k} source"
    cs = {"default": forms["default"], "quad": forms["quad"]}
    a, b = imt.IndexedTree(cs["default"], depth, cap), imt.IndexedTree(cs["default"], depth, cap)
    a2 = imt.IndexedTree(cs["quad"], depth, cap)
    try:
        pre = ints_to_arr(base_vals)
        assert a.apply_batch(pre) == b.apply_batch(pre) == a2.apply_batch(pre)
        more = ints_to_arr(new_vals)
        assert a.apply_batch(more) == a2.apply_batch(more)
        head = a.root()
        want_pre, want_sib = b.get_leaves(idx), b.get_proof_batch(idx)
        want_wit = b.non_membership_witness(ints_to_arr(probes))
        for t in (a, a2):
            v = t.view(s)
            assert v.root() == b.root()
            hashes, builds = v.stats()
            assert hashes.tolist() == want_hashes and builds == 1
            assert (v.get_leaves(idx) == want_pre).all()
            got = v.get_proof_batch(idx)
            bad = np.argwhere((got != want_sib).any(axis=2))
            assert bad.size == 0, f"proof level {bad[0][0]} of leaf {idx[bad[0][1]]}"
            for g, w, what in zip(v.non_membership_witness(ints_to_arr(probes)), want_wit,
                                  ("low_index", "low_leaf", "low_sib", "is_largest")):
                assert (g == w).all(), what
            assert v.stats()[1] == 1 and t.root() == head and t.size == M
            v.close()
        assert hashes[1] > 16384 >= hashes[7], "both forms of k_view_level must have run on the default context"
    finally:
        a.close()
        a2.close()
        b.close()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- arguments
def test_view_arguments(imt, ctx):
    import torch
    f, lib = imt._ffi, imt.lib
    depth, cap = 32, 64
    vals = oracle_lib.synth_values(60, 0x56574130)
    t = imt.IndexedTree(ctx, depth, cap)
    P_ = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    try:
        t.apply_batch(vals[:20])
        t.insert_batch(vals[20:40])
        idx = np.arange(cap, dtype=np.uint64)
        twin = imt.IndexedTree(ctx, depth, cap)
        twin.apply_batch(vals[:20])

        def state():
            return t.size, t.root(), t.get_leaves(idx).tobytes(), t.get_proof_batch(idx).tobytes()

        def vstate(v):
            return v.root(), v.get_leaves(idx).tobytes(), v.get_proof_batch(idx).tobytes(), v.stats()[1]

        before = state()
        lib.imt_itree_view_free(None)
        assert lib.imt_itree_view_size(None) == 0
        h = ctypes.c_void_p()
        for size in (0, 42, 1 << 40):
            assert lib.imt_itree_view_create(t.h, size, ctypes.byref(h)) == f.ERR["RANGE"] and not h.value
        assert lib.imt_itree_view_create(None, 5, ctypes.byref(h)) == f.ERR["ARG"]
        assert lib.imt_itree_view_create(t.h, 5, None) == f.ERR["ARG"]
        # two views, each the twin of its size; the tree untouched
        v, w = t.view(21), t.view(41)
        assert v.size == 21 and w.size == 41
        assert vstate(v)[:3] == (twin.root(), twin.get_leaves(idx).tobytes(), twin.get_proof_batch(idx).tobytes())
        # the view at the current size: nothing hashed, the tree's answers
        assert vstate(w)[:3] == before[1:] and w.stats()[0].tolist() == [0] * (depth + 1)
        st, leaf = w.lookup(ints_to_arr(vals[:44]))
        st2, leaf2 = t.lookup(ints_to_arr(vals[:44]))
        assert (st == st2).all() and (leaf == leaf2).all()
        vb = vstate(v)
        assert vb[3] == 1 and state() == before
        # refused queries: the pipeline flag, the unknown format, null and misaligned buffers, indices out of range
        out = np.zeros(32, np.uint8)
        host_out = out.ctypes.data_as(ctypes.c_void_p)
        one = ints_to_arr(vals[50:51])
        st8, lf = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
        big = np.zeros((depth, 1, 32), np.uint8)
        pv, ps, pl, pb = (x.ctypes.data_as(ctypes.c_void_p) for x in (one, st8, lf, big))
        for flags in (f.PIPELINE, f.PIPELINE | f.DEVICE_PTRS, 3):
            assert lib.imt_itree_view_root(v.h, host_out, flags) == f.ERR["ARG"]
            assert lib.imt_itree_view_lookup_batch(v.h, pv, 1, ps, pl, flags) == f.ERR["ARG"]
            assert lib.imt_itree_view_get_leaves(v.h, pl, 1, pb, flags) == f.ERR["ARG"]
            assert lib.imt_itree_view_get_proof_batch(v.h, pl, 1, pb, flags) == f.ERR["ARG"]
            assert lib.imt_itree_view_non_membership_witness(v.h, pv, 1, pl, None, None, pb, flags) == f.ERR["ARG"]
        assert lib.imt_itree_view_root(None, host_out, 0) == f.ERR["ARG"]
        assert lib.imt_itree_view_root(v.h, None, 0) == f.ERR["ARG"]
        assert lib.imt_itree_view_stats(None, None, None) == f.ERR["ARG"]
        assert lib.imt_itree_view_get_proof_batch(v.h, None, 1, pb, 0) == f.ERR["ARG"]
        dev_out = torch.zeros(64, dtype=torch.uint8, device="cuda")
        assert lib.imt_itree_view_root(v.h, P_(dev_out, 8), f.DEVICE_PTRS) == f.ERR["ARG"]      # misaligned device root
        for bad in (cap, 1 << 40):
            lf[0] = bad
            assert lib.imt_itree_view_get_proof_batch(v.h, pl, 1, pb, 0) == f.ERR["RANGE"]
            assert lib.imt_itree_view_get_leaves(v.h, pl, 1, pb, 0) == f.ERR["RANGE"]
            assert lib.imt_itree_get_proof_batch(twin.h, pl, 1, pb, 0) == f.ERR["RANGE"]
            assert lib.imt_itree_get_leaves(twin.h, pl, 1, pb, 0) == f.ERR["RANGE"]
        assert vstate(v) == vb and state() == before
        # a sharded batch between begin and end: creation and queries refused
        ev, l0 = ctypes.c_uint32(), ctypes.c_uint32()
        more = ints_to_arr(vals[40:44])
        assert lib.imt_itree_batch_begin(t.h, more.ctypes.data_as(ctypes.c_void_p), 4, 0, ctypes.byref(ev), ctypes.byref(l0)) == 0
        assert lib.imt_itree_view_create(t.h, 5, ctypes.byref(h)) == f.ERR["ARG"] and not h.value
        assert lib.imt_itree_view_root(v.h, host_out, 0) == f.ERR["ARG"]
        assert lib.imt_itree_batch_abort(t.h) == 0
        assert vstate(v) == vb and state() == before
        # an open slice
        dvals = torch.from_numpy(ints_to_arr(vals[40:48])).cuda()
        pay = torch.zeros(int(lib.imt_itree_slice_payload_bytes(8)) + 64, dtype=torch.uint8, device="cuda")
        sl = ctypes.c_int(-1)
        assert lib.imt_itree_slice_prepare(t.h, P_(dvals), 0, 8, 0, None, f.DEVICE_PTRS, ctypes.byref(sl), None) == 0
        assert lib.imt_itree_view_create(t.h, 5, ctypes.byref(h)) == f.ERR["ARG"] and not h.value
        assert lib.imt_itree_view_root(v.h, host_out, 0) == f.ERR["ARG"]
        assert lib.imt_itree_view_get_proof_batch(w.h, idx.ctypes.data_as(ctypes.c_void_p), 1, pb, 0) == f.ERR["ARG"]
        for q in range(depth + 1):
            assert lib.imt_itree_slice_unit(t.h, sl.value, q, P_(pay), None) == 0
        ctx.sync()
        # the slice's 8 values are in: both views answer as before, each after one rebuild
        assert t.size == 49
        assert vstate(v)[:3] == vb[:3] and v.stats()[1] == 2
        assert vstate(w)[:3] == before[1:] and w.stats()[1] == 2 and w.stats()[0][0] > 0
        assert t.rewind(41) == before[1] and state() == before
        # a handle that is not a live view -- the tree's own, a freed view's -- is an argument error, never read through
        stale = ctypes.c_void_p(v.h.value)
        v.close()
        w.close()
        v.close()                                                  # closing twice is harmless
        for bad in (t.h, stale):
            assert lib.imt_itree_view_root(bad, host_out, 0) == f.ERR["ARG"]
            assert lib.imt_itree_view_lookup_batch(bad, pv, 1, ps, pl, 0) == f.ERR["ARG"]
            assert lib.imt_itree_view_get_leaves(bad, pl, 1, pb, 0) == f.ERR["ARG"]
            assert lib.imt_itree_view_get_proof_batch(bad, pl, 1, pb, 0) == f.ERR["ARG"]
            assert lib.imt_itree_view_non_membership_witness(bad, pv, 1, pl, None, None, pb, 0) == f.ERR["ARG"]
            assert lib.imt_itree_view_stats(bad, None, None) == f.ERR["ARG"]
            assert lib.imt_itree_view_size(bad) == 0
            lib.imt_itree_view_free(bad)
        assert state() == before
        twin.close()
    finally:
        t.close()


def test_view_sliced(imt, ctx):
    """world 2 over the local transport: with steps in flight a replica takes no view; after imt_sliced_flush it does, and
    the view at the size after the first step has the sequential oracle's root of that prefix"""
    import torch
    import test_gpu_sliced as ts
    sl = ts.load_sliced()
    depth, cap, world, batch = 32, 1 << 12, 2, 150
    step = world * batch
    vals = oracle_lib.synth_values(2 * step, 0x56575300)
    orc = oracle_lib.load()
    oh = orc.sparse_new(depth, cap)
    for x in vals[:step]:
        assert orc.sparse_insert(oh, depth, x)["rc"] == 0
    want_root = orc.sparse_root(oh)
    orc.sparse_free(oh)
    w = sl.SlicedTree(imt, 0, depth, cap, batch, world, n_local=world, nbuf=8)
    try:
        arr = torch.from_numpy(ints_to_arr(vals)).cuda()
        for r in range(2):
            w.step(arr[r * step:(r + 1) * step])
        h = ctypes.c_void_p()
        for t in w.trees:
            assert imt.lib.imt_itree_view_create(t.h, 1, ctypes.byref(h)) == imt._ffi.ERR["ARG"] and not h.value
        w.flush()
        roots = [t.root() for t in w.trees]
        views = [t.view(step + 1) for t in w.trees]
        assert [v.root() for v in views] == [want_root] * world
        assert [t.root() for t in w.trees] == roots
        for v in views:
            v.close()
    finally:
        w.close()


# ---------------------------------------------------------------- the C example
def test_finalized_reads_example(imt, oracle):
    """examples/finalized_reads_demo.c applies ten blocks while serving witnesses against the root three blocks back; it
    prints the head's and the finalized root after every block, and compares the last finalized root with its argument"""
    exe = os.path.join(ROOT, "examples", "finalized_reads_demo")
    csrc = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "finalized_reads_demo.c"), "-L", csrc, "-limt_hip",
                        "-Wl,-rpath," + csrc, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h, roots = oracle.sparse_new(32, 1024), []
    for j in range(10):
        for i in range(64):
            assert oracle.sparse_insert(h, 32, 1 + 7919023757 * (64 * j + i + 1) % ((1 << 61) - 1))["rc"] == 0
        roots.append(oracle.sparse_root(h))
    oracle.sparse_free(h)
    r = subprocess.run([exe, f"{roots[6]:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for j, want in enumerate(roots):
        assert f"head block {j}: root {want:064x}" in r.stdout, r.stdout
    for j in range(3, 10):
        assert f"finalized block {j - 3} ({1 + 64 * (j - 2)} leaves): root {roots[j - 3]:064x}" in r.stdout, r.stdout
    assert r.stdout.count("64 non-membership witnesses against it, 0 failed") == 7
    assert f"as of 449 leaves: root {roots[6]:064x}" in r.stdout and "equals the expected one" in r.stdout
    r = subprocess.run([exe, f"{roots[9]:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "DIFFERS" in r.stdout
