"""GPU (MI355X): a tree from its value log (imt_itree_load_values / imt_itree_get_values / imt_itree_view_get_values).

The claim under test is an identity: after load_values(vals) a tree cannot be told, through any call, from a fresh tree
of the same depth, capacity, placement and partition that ran apply_batch(vals).  Expected values are the sequential
oracle's (tests/insert_corpus.py) or such a twin's; every comparison is bit-exact.

  test_load_values_scenarios   every scenario of the corpus: at every batch boundary the stream's prefix loaded into a
                               fresh tree, the root against the oracle's new_root of the prefix's last insertion; at the
                               last boundary the stored tree (proof and preimage of every filled leaf, the next empty
                               slot and slot capacity - 1).  d33_top64 / d47_top192 take the comparator fallback, the
                               random streams the radix path, placed_g5 / placed_64 the index base.
  test_load_values_every_size  n = 1 .. 15 at depth 4: every odd and even level length.
  test_loaded_tree_goes_on     insert_batch (device and host prepare), insert_filtered, lookup, non_membership_witness,
                               rewind into the loaded prefix, a view there and its values: all equal to the twin's.
  test_load_values_formats     canonical / MONT256 / DEVICE through host pointers, torch buffers and imt_host_alloc
                               memory, get_values round trips, loading over a tree with IMT_PIPELINE batches in flight,
                               a view created before the load.
  test_load_values_refusals    every class with bad_pos, first offender at 0 and at n - 1; the code with a value >= p and
                               a repeat in both orders against the twin's apply_batch; FULL, NULL, n == 0, format 3, an
                               open slice; get_values out of range leaves the buffer alone.
  test_load_values_sliced_world  a tree with sliced steps in flight refuses both calls.
  test_load_values_large       2^16 + 3 random values at depth 32 against a twin grown by apply_batch.
  test_cold_start_demo_example examples/cold_start_demo.c: its cold-start root against the oracle's.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import insert_corpus as ic
import oracle_lib
import test_gpu_insert_matrix as tm
from oracle_lib import P, arr_ints, ints_to_arr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOPOS = 2 ** 64 - 1
SENT = 0xA5


def P_(x, off=0):
    return ctypes.c_void_p((x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data) + off)


def new_tree(imt, c, sc):
    t = imt.IndexedTree(c, sc.depth, sc.cap)
    if sc.placement:
        t.set_placement(*sc.placement)
    return t


def same_tree(a, b):
    """two trees through every read: size, root, every leaf and proof up to the next empty slot, the last slot"""
    assert a.size == b.size and a.root() == b.root()
    cap = a.capacity
    idx = np.array(sorted(set(range(min(a.size + 1, cap))) | {cap - 1}), np.uint64) + np.uint64(a.index_base)
    assert (a.get_leaves(idx) == b.get_leaves(idx)).all()
    assert (a.get_proof_batch(idx) == b.get_proof_batch(idx)).all()
    assert (a.values() == b.values()).all()


def state(t):
    idx = np.arange(t.index_base, t.index_base + min(t.size + 1, t.capacity), dtype=np.uint64)
    return t.size, t.root(), t.get_leaves(idx).tobytes()


def raw_load(imt, t, arr, n, flags=0, ptr=None):
    """(rc, bad_pos) of the C call; bad_pos keeps NOPOS if the call does not write it"""
    bad = ctypes.c_uint64(NOPOS)
    p = ptr if ptr is not None else (P_(arr) if arr is not None else None)
    rc = imt.lib.imt_itree_load_values(t.h, p, n, ctypes.byref(bad), flags)
    return rc, bad.value


# ---------------------------------------------------------------- the corpus
@pytest.mark.parametrize("name", [s.name for s in ic.SCENARIOS])
def test_load_values_scenarios(imt, ctx, name):
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    vals = ints_to_arr(exp["vals"])
    bounds = ic.batch_bounds(sc)
    for j, (_, b) in enumerate(bounds):
        t = new_tree(imt, ctx, sc)
        try:
            t.load_values(vals[:b])
            assert t.size == b + 1
            assert t.root() == exp["batch_roots"][j + 1] == arr_ints(exp["rec"]["new_root"][b - 1:b])[0], f"prefix of {b}"
            assert (t.values() == vals[:b]).all()
            if j == len(bounds) - 1:
                fin = exp["final"]
                assert t.size == fin["size"] and t.root() == fin["root"]
                assert (t.get_proof_batch(fin["index"], item_major=True) == fin["proofs"]).all()
                assert (t.get_leaves(fin["index"]) == fin["preimages"]).all()
                if exp["full_value"] is not None:       # the tree is full: one value more does not fit
                    more = np.concatenate([vals, ints_to_arr([exp["full_value"]])])
                    before = state(t)
                    assert raw_load(imt, t, more, len(more)) == (imt._ffi.ERR["FULL"], NOPOS) and state(t) == before
        finally:
            t.close()


@pytest.mark.parametrize("n", range(1, 16))
def test_load_values_every_size(imt, ctx, n):
    vals = oracle_lib.synth_values(15, 0x4C560400)[:n]
    a, b = imt.IndexedTree(ctx, 4, 16), imt.IndexedTree(ctx, 4, 16)
    try:
        a.load_values(vals)
        assert b.apply_batch(vals) == a.root()
        same_tree(a, b)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- the loaded tree goes on
@pytest.mark.parametrize("host_prep", [False, True])
def test_loaded_tree_goes_on(imt, ctx, host_prep):
    depth, cap, n0 = 32, 2048, 700
    allv = oracle_lib.synth_values(1200, 0x4C560500)
    a, b = imt.IndexedTree(ctx, depth, cap), imt.IndexedTree(ctx, depth, cap)
    try:
        a.load_values(allv[:n0])
        b.apply_batch(allv[:n0])
        same_tree(a, b)
        ra, rb = a.insert_batch(allv[n0:n0 + 130], host_prep=host_prep), b.insert_batch(allv[n0:n0 + 130], host_prep=host_prep)
        for k in ra:
            assert (ra[k] == rb[k]).all(), k
        mixed = [0, allv[3], allv[900], allv[900], allv[n0 + 5], allv[901], 0, allv[902]]
        fa, fb = a.insert_filtered(mixed, host_prep=host_prep), b.insert_filtered(mixed, host_prep=host_prep)
        assert fa["n_inserted"] == fb["n_inserted"] == 3
        for k in fa:
            assert np.array_equal(fa[k], fb[k]), k
        probe = ints_to_arr([allv[0], allv[n0 - 1], allv[n0 + 1], allv[902], 0, allv[1000], allv[1001], P - 1])
        sa, sb = a.lookup(probe), b.lookup(probe)
        assert (sa[0] == sb[0]).all() and (sa[1] == sb[1]).all()
        assert sa[0].tolist() == [imt._ffi.VAL_PRESENT] * 4 + [imt._ffi.VAL_ZERO] + [imt._ffi.VAL_NEW] * 3
        for x, y in zip(a.non_membership_witness(probe[5:]), b.non_membership_witness(probe[5:])):
            assert (x == y).all()
        # a view inside the loaded prefix, its values, and a rewind to that size
        S = 333
        va, vb = a.view(S), b.view(S)
        assert va.root() == vb.root()
        idx = np.array([0, 1, 150, S - 1, S], np.uint64)
        assert (va.get_leaves(idx) == vb.get_leaves(idx)).all() and (va.get_proof_batch(idx) == vb.get_proof_batch(idx)).all()
        assert (va.values() == ints_to_arr(allv[:S - 1])).all() and (vb.values() == va.values()).all()
        assert (va.values(0, 2) == ints_to_arr([0, allv[0]])).all()
        builds = lambda v: _view_builds(imt, v)
        n_builds = builds(va)
        a.apply_batch(allv[1100:1110])
        b.apply_batch(allv[1100:1110])
        assert (va.values(S - 2, 1) == ints_to_arr(allv[S - 3:S - 2])).all() and builds(va) == n_builds      # no rebuild for values
        buf = np.full((2, 32), SENT, np.uint8)
        assert imt.lib.imt_itree_view_get_values(va.h, S - 1, 2, P_(buf), 0) == imt._ffi.ERR["RANGE"] and (buf == SENT).all()
        assert imt.lib.imt_itree_view_get_values(va.h, S, 1, P_(buf), 0) == imt._ffi.ERR["RANGE"] and (buf == SENT).all()
        assert imt.lib.imt_itree_view_get_values(va.h, 1, 1, P_(buf), imt._ffi.PIPELINE) == imt._ffi.ERR["ARG"]
        assert imt.lib.imt_itree_view_get_values(va.h, 1, 1, P_(buf), 3) == imt._ffi.ERR["ARG"] and (buf == SENT).all()
        va.close()
        vb.close()
        assert a.rewind(S) == b.rewind(S)
        same_tree(a, b)
        assert a.apply_batch(allv[1110:1150]) == b.apply_batch(allv[1110:1150])
        same_tree(a, b)
    finally:
        a.close()
        b.close()


def _view_builds(imt, v):
    h = (ctypes.c_uint64 * (v.depth + 1))()
    builds = ctypes.c_uint64()
    assert imt.lib.imt_itree_view_stats(v.h, h, ctypes.byref(builds)) == 0
    return builds.value


# ---------------------------------------------------------------- formats and pointers
@pytest.mark.parametrize("mem", ["host", "torch", "pinned"])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_load_values_formats(imt, ctx, fmt, mem):
    import torch
    f = imt._ffi
    depth, cap, n = 32, 1024, 300
    ints = oracle_lib.synth_values(n + 200, 0x4C560600 + fmt)
    vals, later = ints[:n], ints[n:]
    src = tm.to_fmt(ints_to_arr(vals), fmt)
    a, twin = imt.IndexedTree(ctx, depth, cap), imt.IndexedTree(ctx, depth, cap)
    pinned = []
    try:
        twin.apply_batch(vals)
        # a non-empty tree, with pipelined batches still in flight when the load arrives
        dv = torch.from_numpy(ints_to_arr(later)).cuda()
        for k in range(3):
            assert imt.lib.imt_itree_insert_batch(a.h, P_(dv, k * 40 * 32), 40, None, f.DEVICE_PTRS | f.PIPELINE) == 0
        old_view = a.view(100)                 # created before the load: answers for the new contents afterwards
        big_view = a.view(121)
        flags = fmt
        if mem == "host":
            rc = imt.lib.imt_itree_load_values(a.h, P_(src), n, None, flags)
        elif mem == "torch":
            buf = torch.from_numpy(src.copy()).cuda()
            rc = imt.lib.imt_itree_load_values(a.h, P_(buf), n, None, flags | f.DEVICE_PTRS)
        else:
            buf = ctx.host_alloc((n, 32))
            pinned.append(buf)
            buf[:] = src
            rc = imt.lib.imt_itree_load_values(a.h, P_(buf), n, None, flags | f.DEVICE_PTRS)
        assert rc == 0, imt.lib.imt_last_error(ctx.h)
        same_tree(a, twin)
        lag = np.empty(32, np.uint8)
        assert imt.lib.imt_itree_root_lagged(a.h, 0, P_(lag), 0) != 0            # no lagged root is kept, as after a load
        tv = twin.view(100)
        assert old_view.root() == tv.root() and (old_view.values() == ints_to_arr(vals[:99])).all()
        tv.close()
        old_view.close()
        # get_values in the same format and memory: the bytes that went in
        if mem == "host":
            out = np.full((n + 1, 32), SENT, np.uint8)
            assert imt.lib.imt_itree_get_values(a.h, 1, n, P_(out), flags) == 0
            got, tail = out[:n], out[n]
        elif mem == "torch":
            out = torch.full((n + 1, 32), SENT, dtype=torch.uint8, device="cuda")
            assert imt.lib.imt_itree_get_values(a.h, 1, n, P_(out), flags | f.DEVICE_PTRS) == 0
            ctx.sync()
            got, tail = out[:n].cpu().numpy(), out[n].cpu().numpy()
        else:
            out = ctx.host_alloc((n + 1, 32))
            pinned.append(out)
            out[:] = SENT
            assert imt.lib.imt_itree_get_values(a.h, 1, n, P_(out), flags | f.DEVICE_PTRS) == 0
            ctx.sync()
            got, tail = out[:n].copy(), out[n].copy()
        assert (got == src).all() and (tail == SENT).all()
        assert (a.values(fmt=fmt) == src).all() and (a.values(0, 1) == 0).all()
        # the round trip: the log read back rebuilds the same tree over itself, and a smaller one makes the view fail
        a.load_values(got, fmt=fmt)
        same_tree(a, twin)
        a.load_values(vals[:50])
        with pytest.raises(imt.ImtError) as ei:
            big_view.root()
        assert ei.value.code == f.ERR["RANGE"]
        with pytest.raises(imt.ImtError) as ei:
            big_view.values()
        assert ei.value.code == f.ERR["RANGE"]
        big_view.close()
        if mem == "torch":                       # values_into / load_values_device
            dbuf = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
            twin.values_into(dbuf.data_ptr(), fmt=fmt)
            a.load_values_device(dbuf.data_ptr(), n, fmt=fmt)
            same_tree(a, twin)
    finally:
        for p in pinned:
            ctx.host_free(p)
        a.close()
        twin.close()


# ---------------------------------------------------------------- refusals
def test_load_values_refusals(imt, ctx):
    import torch
    f = imt._ffi
    depth, cap = 32, 256
    good = oracle_lib.synth_values(120, 0x4C560700)
    t = imt.IndexedTree(ctx, depth, cap)
    part = imt.IndexedTree(ctx, depth, cap)
    try:
        t.apply_batch(good[100:120])
        before = state(t)
        base = good[:40]

        def refused(lst, code, pos, tree=t, was=None):
            was = before if was is None else was
            for flags, arr in ((0, ints_to_arr(lst)), (f.DEVICE_PTRS, torch.from_numpy(ints_to_arr(lst)).cuda())):
                assert raw_load(imt, tree, arr, len(lst), flags) == (f.ERR[code], pos), (lst[:3], code, pos, flags)
                assert state(tree) == was
            twin = imt.IndexedTree(ctx, depth, cap)                 # the code is apply_batch's on a fresh twin
            if tree is part:
                ctx._check(imt.lib.imt_itree_set_value_partition(twin.h, 5, 2))
            root = np.empty(32, np.uint8)
            assert imt.lib.imt_itree_apply_batch(twin.h, P_(ints_to_arr(lst)), len(lst), P_(root), 0) == f.ERR[code]
            twin.close()

        n = len(base) + 1
        for at in (0, n - 1):                                        # the first offender at position 0 and at n - 1
            refused(base[:at] + [0] + base[at:], "VALUE", at)
            refused(base[:at] + [P] + base[at:], "NONCANONICAL", at)
            refused(base[:at] + [(1 << 256) - 1] + base[at:], "NONCANONICAL", at)
        refused([base[0], base[0]] + base[1:], "VALUE", 1)           # a repeat: the second occurrence, as early as it can be
        refused(base + [base[0]], "VALUE", n - 1)
        refused(base + [base[-1]], "VALUE", n - 1)
        refused([0], "VALUE", 0)
        refused([7, 0, 0, 7], "VALUE", 1)
        # a value >= p and a repeat, in both orders: the code is NONCANONICAL, the position the smaller one
        refused(base[:5] + [P + 3] + base[5:20] + [base[2]] + base[20:], "NONCANONICAL", 5)
        refused(base[:5] + [base[2]] + base[5:20] + [P + 3] + base[20:], "NONCANONICAL", 5)
        refused(base[:5] + [P + 3, P + 3] + base[5:], "NONCANONICAL", 5)
        # equal top limbs: the verdict comes from the second attempt
        tied = ic.stream_values(ic.BY_NAME["d47_top192"])[:60]
        refused(tied + [tied[17]], "VALUE", 60)
        refused(tied[:30] + [tied[3]] + tied[30:] + [P], "NONCANONICAL", 30)
        # the other formats: >= p is judged on the bytes as they came
        src = tm.to_fmt(ints_to_arr(base), 1)
        src[11] = ints_to_arr([P + 1])[0]
        assert raw_load(imt, t, src, len(base), f.FMT_MONT256) == (f.ERR["NONCANONICAL"], 11) and state(t) == before
        src = tm.to_fmt(ints_to_arr(base + [base[4]]), 2)
        assert raw_load(imt, t, src, len(base) + 1, f.FMT_DEVICE) == (f.ERR["VALUE"], len(base)) and state(t) == before
        # a foreign residue
        ctx._check(imt.lib.imt_itree_set_value_partition(part.h, 5, 2))
        mine = [v for v in oracle_lib.synth_values(400, 0x4C560701) if v % 5 == 2][:30]
        other = next(v for v in good if v % 5 != 2)
        part.apply_batch(mine[20:])
        pstate = state(part)
        for at in (0, 20):
            refused(mine[:at] + [other] + mine[at:20], "VALUE", at, tree=part, was=pstate)
        part.load_values(mine[:20])
        twin = imt.IndexedTree(ctx, depth, cap)
        ctx._check(imt.lib.imt_itree_set_value_partition(twin.h, 5, 2))
        twin.apply_batch(mine[:20])
        same_tree(part, twin)
        twin.close()
        # what does not depend on the values
        arr = ints_to_arr(good[:100] + oracle_lib.synth_values(156, 0x4C560702))
        assert raw_load(imt, t, arr, cap) == (f.ERR["FULL"], NOPOS) and state(t) == before      # cap values + the sentinel
        assert raw_load(imt, t, None, 5) == (f.ERR["ARG"], NOPOS)
        assert raw_load(imt, t, arr, 0) == (f.ERR["ARG"], NOPOS)
        assert raw_load(imt, t, arr, 5, 3) == (f.ERR["ARG"], NOPOS)
        assert raw_load(imt, t, None, 5, ptr=P_(torch.zeros(256, dtype=torch.uint8, device="cuda"), 8),
                        flags=f.DEVICE_PTRS) == (f.ERR["ARG"], NOPOS)                             # misaligned device values
        assert state(t) == before
        assert imt.lib.imt_itree_load_values(t.h, P_(arr), cap - 1, None, 0) == 0 and t.size == cap     # exactly full
        t.load_values(good[100:120])
        assert state(t) == before
        with pytest.raises(ValueError) as ei:
            t.load_values(base + [base[3]])
        assert ei.value.bad_pos == len(base)
        with pytest.raises(imt.ImtError) as ei:
            t.load_values(base + [P])
        assert ei.value.code == f.ERR["NONCANONICAL"] and ei.value.bad_pos == len(base)
        # get_values out of range: the buffer keeps its fill
        buf = np.full((4, 32), SENT, np.uint8)
        for first, k in ((t.size, 1), (t.size - 1, 2), (1 << 40, 1), (2 ** 64 - 1, 2)):
            assert imt.lib.imt_itree_get_values(t.h, first, k, P_(buf), 0) == f.ERR["RANGE"] and (buf == SENT).all()
        dbuf = torch.full((4, 32), SENT, dtype=torch.uint8, device="cuda")
        assert imt.lib.imt_itree_get_values(t.h, t.size - 1, 2, P_(dbuf), f.DEVICE_PTRS) == f.ERR["RANGE"]
        assert imt.lib.imt_itree_get_values(t.h, 1, 1, P_(dbuf), 3) == f.ERR["ARG"]
        ctx.sync()
        assert (dbuf.cpu().numpy() == SENT).all()
        assert imt.lib.imt_itree_get_values(t.h, 1, 0, None, 0) == 0
        assert imt.lib.imt_itree_get_values(t.h, 1, 1, None, 0) == f.ERR["ARG"]
        placed = imt.IndexedTree(ctx, 8, 256)
        placed.set_placement(12, 5)
        placed.load_values(base)
        assert imt.lib.imt_itree_get_values(placed.h, 1, 1, P_(buf), 0) == f.ERR["RANGE"] and (buf == SENT).all()   # below the base
        assert (placed.values() == ints_to_arr(base)).all()
        placed.close()
        # an open slice
        dvals = torch.from_numpy(ints_to_arr(good[60:68])).cuda()
        pay = torch.zeros(int(imt.lib.imt_itree_slice_payload_bytes(8)) + 64, dtype=torch.uint8, device="cuda")
        sl = ctypes.c_int(-1)
        assert imt.lib.imt_itree_slice_prepare(t.h, P_(dvals), 0, 8, 0, None, f.DEVICE_PTRS, ctypes.byref(sl), None) == 0
        assert raw_load(imt, t, ints_to_arr(base), len(base)) == (f.ERR["ARG"], NOPOS)
        for q in range(depth + 1):
            assert imt.lib.imt_itree_slice_unit(t.h, sl.value, q, P_(pay), None) == 0
        ctx.sync()
        assert t.size == before[0] + 8 and t.rewind(before[0]) == before[1] and state(t) == before
    finally:
        t.close()
        part.close()


def test_load_values_sliced_world(imt, ctx):
    """world 2 over the local transport: with steps in flight only imt_sliced_* calls may touch the trees"""
    import torch
    import test_gpu_sliced as ts
    sl = ts.load_sliced()
    depth, cap, world, batch = 32, 1 << 10, 2, 50
    vals = oracle_lib.synth_values(2 * world * batch, 0x4C560800)
    w = sl.SlicedTree(imt, 0, depth, cap, batch, world, n_local=world, nbuf=8)
    try:
        w.step(torch.from_numpy(ints_to_arr(vals[:world * batch])).cuda())
        log = ints_to_arr(vals[world * batch:])
        buf = np.full((1, 32), SENT, np.uint8)
        for t in w.trees:
            assert raw_load(imt, t, log, len(log)) == (imt._ffi.ERR["ARG"], NOPOS)
            assert imt.lib.imt_itree_get_values(t.h, 0, 1, P_(buf), 0) == imt._ffi.ERR["ARG"] and (buf == SENT).all()
        w.flush()
        assert all(t.size == world * batch + 1 for t in w.trees)
        assert (w.trees[0].values() == ints_to_arr(vals[:world * batch])).all()
    finally:
        w.close()


# ---------------------------------------------------------------- a size users run
def test_load_values_large(imt, ctx):
    """2^16 + 3 values at depth 32: 257 blocks of the check and leaf kernels, and level lengths 65540, 32770, 16385, 8193,
    ... -- odd from level 2 up."""
    import torch
    depth, cap, n = 32, 1 << 17, (1 << 16) + 3
    ints = oracle_lib.synth_values(n + 256, 0x4C560900)
    vals, absent = ints_to_arr(ints[:n]), ints[n:]
    a, b = imt.IndexedTree(ctx, depth, cap), imt.IndexedTree(ctx, depth, cap)
    try:
        a.load_values(vals)
        assert b.apply_batch(vals) == a.root() and a.size == b.size == n + 1
        rng = np.random.default_rng(0x4C560901)
        idx = np.unique(np.concatenate([rng.integers(0, n + 1, 60).astype(np.uint64), np.array([0, 1, n, n + 1], np.uint64)]))
        assert (a.get_proof_batch(idx) == b.get_proof_batch(idx)).all()
        assert (a.get_leaves(idx) == b.get_leaves(idx)).all()
        stored = [ints[int(i)] for i in rng.integers(0, n, 256)]
        sa, sb = a.lookup(ints_to_arr(stored + absent)), b.lookup(ints_to_arr(stored + absent))
        assert (sa[0] == sb[0]).all() and (sa[1] == sb[1]).all()
        assert (sa[0][:256] == imt._ffi.VAL_PRESENT).all() and (sa[0][256:] == imt._ffi.VAL_NEW).all()
        assert (a.values() == vals).all()
    finally:
        a.close()
        b.close()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- the C example
def test_cold_start_demo_example(imt, oracle, tmp_path):
    """examples/cold_start_demo.c grows a tree by ten blocks, writes its value log and starts a second tree from the
    file; given the oracle's root as its argument it compares and fails on a difference."""
    exe = os.path.join(ROOT, "examples", "cold_start_demo")
    csrc = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "cold_start_demo.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    depth, h = 32, oracle.sparse_new(32, 1024)
    for x in range(1, 641):
        assert oracle.sparse_insert(h, depth, 1 + 7919023757 * x % ((1 << 61) - 1))["rc"] == 0
    root = oracle.sparse_root(h)
    oracle.sparse_free(h)
    log = str(tmp_path / "log.values")
    r = subprocess.run([exe, f"{root:064x}", log], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"follower: 641 leaves, root {root:064x}" in r.stdout and f"cold start: 641 leaves, root {root:064x}" in r.stdout
    assert "20480 bytes (a preimage snapshot of the same tree: 61536 bytes)" in r.stdout
    assert "the two roots are equal" in r.stdout and "cold-start root equals the expected one" in r.stdout
    assert "refused at the repeat, the tree as it was" in r.stdout
    r = subprocess.run([exe, f"{root ^ 1:064x}", log], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "DIFFERS" in r.stdout
