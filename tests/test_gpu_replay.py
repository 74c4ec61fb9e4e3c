"""GPU (MI355X): imt_itree_view_insert_witness -- the witnesses of insertions the tree has already made.

The claim under test is an identity: the replay of the n insertions that followed a view's size writes byte for byte what
imt_itree_insert_batch writes on a fresh tree fed the first size - 1 values, and through no call can the tree be told
from one that was never replayed.  Expected values are the sequential oracle's (tests/insert_corpus.py,
test_gpu_rewind.oracle_rows) or a twin tree's; every comparison is bit-exact.

  test_replay_scenarios   every scenario of the corpus on the three hash forms, grown with apply batches only, a view made
                          at every batch boundary.  From the finished tree every view replays the next batch, one
                          insertion, and everything up to the head (which crosses changes of L0): all nine outputs against
                          the oracle's rows; rows [depth, global_depth) of a placed tree's sibling arrays keep the pattern
                          the test wrote.  At the end the tree is the corpus's.
  test_replay_verifies    a replay's witnesses pass imt_insert_witness_batch; with one sibling byte flipped that item fails.
  test_replay_formats     IMT_FMT_MONT256 and IMT_FMT_DEVICE item-major with host pointers, canonical level-major with
                          device pointers.
  test_replay_follows     a replay behind pipelined device batches left in flight, after rewinds above, inside and below
                          the replayed range, and after the tree has grown again along another history.
  test_replay_arguments   every refusal with tree and view untouched, n == 0, the view at the current size, two views.
  test_replay_sliced      refused on a replica with steps in flight, works after the flush.
  test_replay_large       2^16 insertions replayed 2^16 behind the head of a tree of 2^20 + 2^17 + 1 leaves against a twin
                          that made them as a witness batch, both forms of the kernel; that the replayed events read their
                          siblings from all four sources is asserted from the sorted order of the values.
"""
import ctypes

import numpy as np
import pytest

import insert_corpus as ic
import oracle_lib
import test_gpu_insert_matrix as tm
import test_gpu_rewind as tr
from oracle_lib import arr_ints, ints_to_arr
from test_gpu_rewind import forms  # noqa: F401  (the fixture: one context per hash form)

pytestmark = pytest.mark.gpu

FILL = 0xA5
FIELDS = ("low_index", "is_largest", "low_leaf", "new_leaf", "old_root", "interim_root", "new_root", "low_sib", "new_sib")


def buffers(n, G, item):
    """the nine output arrays, every byte the pattern FILL"""
    sib = (n, G, 32) if item else (G, n, 32)
    shapes = dict(low_index=(n, 8), is_largest=(n,), low_leaf=(n, 3, 32), new_leaf=(n, 3, 32), old_root=(n, 32),
                  interim_root=(n, 32), new_root=(n, 32), low_sib=sib, new_sib=sib)
    return {k: np.full(shp, FILL, np.uint8) for k, shp in shapes.items()}


def replay(imt, v, n, G, item=False, fmt=0, fields=FIELDS):
    """the raw call into pattern-filled host arrays: (rc, arrays)"""
    bufs = buffers(n, G, item)
    out = imt._ffi.InsertOut(**{k: bufs[k].ctypes.data for k in fields})
    rc = imt.lib.imt_itree_view_insert_witness(v.h, n, ctypes.byref(out), fmt | (imt._ffi.SIB_ITEM_MAJOR if item else 0))
    return rc, bufs


def compare(bufs, want, lo, depth, item, tag):
    """bufs against rows [lo, lo + n) of `want` (siblings item-major [N, depth, 32]); sibling rows from `depth` up untouched"""
    n = bufs["is_largest"].shape[0]
    for k in tr.OUT_FIELDS:
        g = bufs[k].view(np.uint64).reshape(n) if k == "low_index" else bufs[k]
        bad = np.nonzero((g != want[k][lo:lo + n]).reshape(n, -1).any(axis=1))[0]
        assert bad.size == 0, f"{tag}: {k}, first differing row {lo + bad[0]}"
    for k in ("low_sib", "new_sib"):
        g = bufs[k] if item else bufs[k].transpose(1, 0, 2)
        bad = np.argwhere((g[:, :depth] != want[k][lo:lo + n]).any(axis=2))
        assert bad.size == 0, f"{tag}: {k}, first difference at row {lo + bad[0][0]} level {bad[0][1]}"
        assert (g[:, depth:] == FILL).all(), f"{tag}: {k} rows from {depth} up belong to the caller"


# ---------------------------------------------------------------- every scenario, every boundary
@pytest.mark.parametrize("name,form", tr._scenario_cases())
def test_replay_scenarios(imt, forms, name, form):
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    vals, rec, bounds = exp["vals"], exp["rec"], ic.batch_bounds(sc)
    G, M = sc.global_depth, len(vals) + 1
    t = tr.new_tree(imt, forms[form], sc)
    try:
        views = {1: t.view(1)}
        for a, b in bounds:
            assert t.apply_batch(ints_to_arr(vals[a:b])) == arr_ints(rec["new_root"][b - 1:b])[0]
            views[b + 1] = t.view(b + 1)
        next_batch = {a + 1: b - a for a, b in bounds}
        for s, v in views.items():
            if s == M:                                            # the view at the head: nothing follows it
                rc, bufs = replay(imt, v, 1, G)
                assert rc == imt._ffi.ERR["RANGE"] and all((x == FILL).all() for x in bufs.values())
                rc, bufs = replay(imt, v, 0, G)
                assert rc == 0
                continue
            for n, item in ((next_batch[s], True), (M - s, False)):
                rc, bufs = replay(imt, v, n, G, item=item)
                assert rc == 0, imt.lib.imt_last_error(forms[form].h)
                compare(bufs, rec, s - 1, sc.depth, item, f"{name} view at {s} of {M}, n = {n}")
            one = v.insert_witness(1)                            # the Python method: insert_batch's dict
            one["low_index"] = one["low_index"].view(np.uint8).reshape(1, 8)
            assert (one.pop("new_index") == rec["new_index"][s - 1:s]).all()
            for k in ("low_sib", "new_sib"):                     # np.empty rows the call leaves alone
                one[k][sc.depth:] = FILL
            compare(one, rec, s - 1, sc.depth, False, f"{name} view at {s} of {M}, n = 1")
            assert v.stats()[1] == 1, "one build serves every replay of an unchanged tree"
        fin = exp["final"]
        assert t.size == fin["size"] and t.root() == fin["root"]
        assert (t.get_leaves(fin["index"]) == fin["preimages"]).all()
        assert (t.get_proof_batch(fin["index"], item_major=True) == fin["proofs"]).all()
    finally:
        t.close()


def test_replay_verifies(imt, forms):
    name = "d32_between"
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    c, vals, bounds = forms["default"], exp["vals"], ic.batch_bounds(sc)
    s, d = bounds[len(bounds) // 2][0] + 1, sc.depth
    t = tr.new_tree(imt, c, sc)
    try:
        t.apply_batch(ints_to_arr(vals))
        r = t.view(s).insert_witness(len(vals) + 1 - s)

        def check(low_sib):
            return c.insert_witness(r["old_root"], r["low_leaf"], r["low_index"], low_sib, r["new_root"], r["new_leaf"],
                                    r["new_index"], r["new_sib"], r["is_largest"], d)

        assert not check(r["low_sib"]).any()
        bent = r["low_sib"].copy()
        bent[7, 5, 0] ^= 1                                        # level 7 of item 5
        fail = check(bent)
        assert fail[5] != 0 and not np.delete(fail, 5).any()
    finally:
        t.close()


def test_replay_formats(imt, forms):
    import torch
    name = "d32_between"
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    c, f, lib = forms["default"], imt._ffi, imt.lib
    vals, bounds = exp["vals"], ic.batch_bounds(sc)
    s, d = bounds[len(bounds) // 2][0] + 1, sc.depth
    n = len(vals) + 1 - s
    t = tr.new_tree(imt, c, sc)
    try:
        t.apply_batch(ints_to_arr(vals))
        v = t.view(s)
        for fmt in (f.FMT_MONT256, f.FMT_DEVICE):
            rc, bufs = replay(imt, v, n, d, item=True, fmt=fmt)
            assert rc == 0
            compare(bufs, tm.expected_in(name, fmt)["rec"], s - 1, d, True, f"format {fmt}")
        shapes = {k: a.shape for k, a in buffers(n, d, False).items()}
        dev = {k: torch.full(shp, FILL, dtype=torch.uint8, device="cuda") for k, shp in shapes.items()}
        out = f.InsertOut(**{k: a.data_ptr() for k, a in dev.items()})
        assert lib.imt_itree_view_insert_witness(v.h, n, ctypes.byref(out), f.DEVICE_PTRS) == 0
        c.sync()
        torch.cuda.synchronize()
        compare({k: a.cpu().numpy() for k, a in dev.items()}, exp["rec"], s - 1, d, False, "device pointers")
        assert v.stats()[1] == 1 and t.root() == exp["final"]["root"]
    finally:
        t.close()


# ---------------------------------------------------------------- the replay follows the tree
def test_replay_follows(imt, forms):
    name = "d32_between"
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    c, f = forms["default"], imt._ffi
    vals, rec, bounds = exp["vals"], exp["rec"], ic.batch_bounds(sc)
    d, M = sc.depth, len(vals) + 1
    s = bounds[2][0] + 1
    t = tr.new_tree(imt, c, sc)
    try:
        t.apply_batch(ints_to_arr(vals[:s - 1]))
        v = t.view(s)
        # pipelined device batches left in flight: the replay orders itself behind them
        dv = tr.DeviceBatches(imt, c, t, sc.global_depth)
        for a, b in bounds[2:5]:
            dv.insert(ints_to_arr(vals[a:b]), want_outputs=False)
        n = bounds[4][1] + 1 - s
        rc, bufs = replay(imt, v, n, d)
        assert rc == 0
        compare(bufs, rec, s - 1, d, False, "behind pipelined batches in flight")
        dv.sync()
        assert v.stats()[1] == 1
        t.apply_batch(ints_to_arr(vals[bounds[5][0]:]))
        rc, bufs = replay(imt, v, M - s, d, item=True)
        assert rc == 0
        compare(bufs, rec, s - 1, d, True, "up to the head")
        # back to a size inside the replayed range: that n no longer exists, a shorter one answers as before
        mid = bounds[4][0] + 1
        t.rewind(mid)
        rc, bufs = replay(imt, v, M - s, d)
        assert rc == f.ERR["RANGE"] and all((x == FILL).all() for x in bufs.values())
        rc, bufs = replay(imt, v, mid - s, d)
        assert rc == 0
        compare(bufs, rec, s - 1, d, False, "after a rewind into the range")
        # below the view's size: nothing to replay, but the view stays
        low, builds = bounds[1][0] + 1, v.stats()[1]
        t.rewind(low)
        rc, bufs = replay(imt, v, 1, d)
        assert rc == f.ERR["RANGE"] and all((x == FILL).all() for x in bufs.values())
        assert v.stats()[1] == builds and t.size == low
        # another history past s: the replay gives that history's rows
        used = set(vals)
        other = [x for x in oracle_lib.synth_values(len(vals) + 8, 0x52504600) if x not in used]
        fork = vals[:low - 1] + other[:s + 20 - (low - 1)]
        t.apply_batch(ints_to_arr(fork[low - 1:]))
        assert t.size == s + 21
        want = tr.oracle_rows(sc, fork, s - 1)
        rc, bufs = replay(imt, v, 21, d)
        assert rc == 0
        compare(bufs, want, 0, d, False, "the new history")
        assert not (bufs["new_root"] == rec["new_root"][s - 1:s + 20]).all(axis=1).any()
        assert t.root() == arr_ints(want["new_root"][-1:])[0]
    finally:
        t.close()


# ---------------------------------------------------------------- arguments
def test_replay_arguments(imt, ctx):
    import torch
    f, lib = imt._ffi, imt.lib
    depth, cap = 32, 64
    vals = oracle_lib.synth_values(60, 0x52504130)
    t, twin = imt.IndexedTree(ctx, depth, cap), imt.IndexedTree(ctx, depth, cap)
    P_ = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    try:
        t.apply_batch(vals[:20])
        t.insert_batch(vals[20:40])
        twin.apply_batch(vals[:20])
        want = twin.insert_batch(vals[20:40], item_major=True)       # rows of insertions 20 .. 39: the view at 21 replays them
        idx = np.arange(cap, dtype=np.uint64)

        def state():
            return t.size, t.root(), t.get_leaves(idx).tobytes(), t.get_proof_batch(idx).tobytes(), t.snapshot().tobytes()

        def vstate(v):
            return v.root(), v.get_leaves(idx).tobytes(), v.get_proof_batch(idx).tobytes(), v.stats()[1]

        def refused(v, code, n, flags=0, out="host"):
            bufs = buffers(min(max(n, 1), cap), depth, False)    # a refused n may be far beyond any tree
            o = None if out is None else f.InsertOut(**{k: bufs[k].ctypes.data for k in FIELDS})
            rc = lib.imt_itree_view_insert_witness(v, n, ctypes.byref(o) if o is not None else None, flags)
            assert rc == f.ERR[code], (rc, code, n, flags, lib.imt_last_error(ctx.h))
            assert all((x == FILL).all() for x in bufs.values()), "a refused call writes nothing"

        before = state()
        v, w, head = t.view(21), t.view(31), t.view(41)
        vb, wb = vstate(v), vstate(w)
        # two views replaying in turn, each the twin's rows
        for view, lo, n in ((v, 0, 20), (w, 10, 10), (v, 0, 7), (w, 10, 1)):
            rc, bufs = replay(imt, view, n, depth, item=True)
            assert rc == 0
            compare(bufs, want, lo, depth, True, f"view at {view.size}, n = {n}")
        # NULL fields are skipped; a struct of nothing but NULLs is a call that writes nothing
        rc, bufs = replay(imt, v, 20, depth, fields=("new_root", "low_sib"))
        assert rc == 0 and (bufs["new_root"] == want["new_root"]).all()
        assert (bufs["low_sib"].transpose(1, 0, 2) == want["low_sib"]).all()
        assert all((bufs[k] == FILL).all() for k in FIELDS if k not in ("new_root", "low_sib"))
        assert replay(imt, v, 20, depth, fields=())[0] == 0
        # its own refusals
        refused(v.h, "RANGE", 21)
        refused(v.h, "RANGE", 1 << 40)
        refused(w.h, "RANGE", 11)
        refused(head.h, "RANGE", 1)                               # the view at the current size: nothing follows it
        refused(v.h, "ARG", 5, out=None)
        refused(v.h, "ARG", 0, out=None)
        for view in (v, head):
            rc, bufs = replay(imt, view, 0, depth)
            assert rc == 0 and all((x == FILL).all() for x in bufs.values()), "n == 0 writes nothing"
        # where every view query is refused
        for flags in (f.PIPELINE, f.PIPELINE | f.DEVICE_PTRS, 3):
            refused(v.h, "ARG", 5, flags)
        refused(None, "ARG", 5)
        refused(t.h, "ARG", 5)                                    # a tree's handle is no view
        dev = torch.full((20 * 32 + 64,), FILL, dtype=torch.uint8, device="cuda")
        for field in ("low_leaf", "old_root", "interim_root", "new_root", "new_leaf", "low_sib", "new_sib"):
            o = f.InsertOut(**{field: dev.data_ptr() + 8})       # a misaligned device buffer
            assert lib.imt_itree_view_insert_witness(v.h, 1, ctypes.byref(o), f.DEVICE_PTRS) == f.ERR["ARG"], field
        ctx.sync()
        torch.cuda.synchronize()
        assert (dev.cpu().numpy() == FILL).all()
        assert vstate(v) == vb and vstate(w) == wb and state() == before
        # a sharded batch between begin and end
        ev, l0 = ctypes.c_uint32(), ctypes.c_uint32()
        more = ints_to_arr(vals[40:44])
        assert lib.imt_itree_batch_begin(t.h, more.ctypes.data_as(ctypes.c_void_p), 4, 0, ctypes.byref(ev), ctypes.byref(l0)) == 0
        refused(v.h, "ARG", 5)
        assert lib.imt_itree_batch_abort(t.h) == 0
        assert vstate(v) == vb and state() == before
        # an open slice
        dvals = torch.from_numpy(ints_to_arr(vals[40:48])).cuda()
        pay = torch.zeros(int(lib.imt_itree_slice_payload_bytes(8)) + 64, dtype=torch.uint8, device="cuda")
        sl = ctypes.c_int(-1)
        assert lib.imt_itree_slice_prepare(t.h, P_(dvals), 0, 8, 0, None, f.DEVICE_PTRS, ctypes.byref(sl), None) == 0
        refused(v.h, "ARG", 5)
        refused(head.h, "ARG", 0)
        for q in range(depth + 1):
            assert lib.imt_itree_slice_unit(t.h, sl.value, q, P_(pay), None) == 0
        ctx.sync()
        # the slice's 8 values are in: the replay reaches them, after one rebuild
        assert t.size == 49
        more_want = twin.insert_batch(vals[40:48], item_major=True)
        rc, bufs = replay(imt, head, 8, depth, item=True)
        assert rc == 0
        compare(bufs, more_want, 0, depth, True, "the slice's insertions")
        rc, bufs = replay(imt, v, 20, depth, item=True)
        assert rc == 0
        compare(bufs, want, 0, depth, True, "after the slice")
        assert v.stats()[1] == vb[3] + 1
        assert t.rewind(41) == before[1] and state() == before
        # a handle that is not a live view
        stale = ctypes.c_void_p(v.h.value)
        for view in (v, w, head):
            view.close()
        refused(stale, "ARG", 5)
        assert state() == before
    finally:
        t.close()
        twin.close()


def test_replay_sliced(imt, ctx):
    """world 2 over the local transport: with steps in flight a replica replays nothing; after imt_sliced_flush the view
    made before the steps replays them, the sequential oracle's rows"""
    import torch
    import test_gpu_sliced as ts
    sl = ts.load_sliced()
    depth, cap, world, batch = 32, 1 << 12, 2, 150
    step = world * batch
    vals = oracle_lib.synth_values(2 * step, 0x52505300)
    sc = ic.Scenario("sliced", depth, cap, "random", [2 * step])
    w = sl.SlicedTree(imt, 0, depth, cap, batch, world, n_local=world, nbuf=8)
    try:
        views = [t.view(1) for t in w.trees]
        arr = torch.from_numpy(ints_to_arr(vals)).cuda()
        for r in range(2):
            w.step(arr[r * step:(r + 1) * step])
        for v in views:
            rc, bufs = replay(imt, v, 5, depth)
            assert rc == imt._ffi.ERR["ARG"] and all((x == FILL).all() for x in bufs.values())
        w.flush()
        roots = [t.root() for t in w.trees]
        want = tr.oracle_rows(sc, vals, 0)
        for v in views:
            rc, bufs = replay(imt, v, 2 * step, depth)
            assert rc == 0
            compare(bufs, want, 0, depth, False, "a flushed replica")
            v.close()
        assert [t.root() for t in w.trees] == roots
    finally:
        w.close()


# ---------------------------------------------------------------- a size users run
def replay_coverage(leafvals, s, n, depth, cap):
    """From the sorted order of the values alone: per level l < ceil_log2(s), which of the four sources exist for a view
    at s of this tree, and which of them some event of the replay of n insertions reads its sibling from."""
    total = s + n
    order = sorted(range(len(leafvals)), key=leafvals.__getitem__)
    S0 = {s} | {order[j] for j in range(len(order) - 1) if order[j] < s <= order[j + 1]}
    # the low leaf of leaf x: the nearest leaf to the left in value order with a smaller index
    low, stack = {}, []
    for x in order:
        if x >= total:
            continue
        while stack and stack[-1] > x:
            stack.pop()
        if x >= s:
            low[x] = stack[-1]
        stack.append(x)
    pos = np.empty(2 * n, np.int64)
    pos[0::2] = [low[s + i] for i in range(n)]
    pos[1::2] = np.arange(s, s + n)
    when = np.arange(2 * n)
    S, out = np.array(sorted(S0), np.int64), []
    for l in range(tr.ceil_log2(s)):
        node, y, fill = pos >> l, (pos >> l) ^ 1, -(-s // (1 << l))
        uniq, first = np.unique(node, return_index=True)             # the first event under every touched node
        at = np.minimum(np.searchsorted(uniq, y), len(uniq) - 1)
        batch = (uniq[at] == y) & (first[at] < when)
        empty = ~batch & (y >= fill)
        side = ~batch & ~empty & np.isin(y, S)
        stored = ~batch & ~empty & ~side
        have = dict(batch=batch.any(), empty=empty.any(), side=side.any(), stored=stored.any())
        exists = dict(batch=True, empty=(cap >> l) > fill, side=bool((S < fill).any()), stored=fill > int((S < fill).sum()))
        out.append((exists, have))
        S = np.unique(S >> 1)
    return out


LARGE = dict(depth=32, cap=1 << 21, M0=1 << 20, n=1 << 16, seed=0x52504C20)


def large_values():
    allv = oracle_lib.synth_values(LARGE["M0"] + 2 * LARGE["n"], LARGE["seed"])
    return allv[:LARGE["M0"]], allv[LARGE["M0"]:LARGE["M0"] + LARGE["n"]], allv[LARGE["M0"] + LARGE["n"]:]


def assert_large_coverage(base_vals, new_vals, later):
    depth, cap, M0, n = LARGE["depth"], LARGE["cap"], LARGE["M0"], LARGE["n"]
    cover = replay_coverage([0] + base_vals + new_vals + later, M0 + 1, n, depth, cap)
    full = [l for l, (exists, _) in enumerate(cover) if all(exists.values())]
    # about 6 % of the kept leaves lose their successor, so a node over 2^l leaves stays out of S_l with probability
    # 0.94^(2^l): stored nodes, the scarcest source, are plentiful through level 5 and gone by level 9
    assert set(range(6)) <= set(full), f"only levels {full} have all four sources: these values do not test the replay"
    for l, (exists, have) in enumerate(cover):                      # and at the other levels, every source that exists
        missing = [k for k in exists if exists[k] and not have[k]]
        assert not missing, f"level {l}: no replayed event reads its sibling from {missing}"


def test_replay_large(imt, forms):
    """Twin a applies 2^20 random values, then 2^16, then 2^16 more; twin b applies the same 2^20 and makes the next 2^16 a
    witness batch with all outputs.  The view of a at 2^20 + 1 leaves replays those 2^16: every output equals b's.  On the
    default context the 2^17 events take the thread form k_sweep_view below L0 = 21, on the quad context the quad form."""
    import torch
    depth, cap, M0, n = LARGE["depth"], LARGE["cap"], LARGE["M0"], LARGE["n"]
    base_vals, new_vals, later = large_values()
    assert_large_coverage(base_vals, new_vals, later)
    s = M0 + 1
    a, a2, b = (imt.IndexedTree(forms[k], depth, cap) for k in ("default", "quad", "default"))
    try:
        pre, batch, more = ints_to_arr(base_vals), ints_to_arr(new_vals), ints_to_arr(later)
        assert a.apply_batch(pre) == b.apply_batch(pre) == a2.apply_batch(pre)
        want = b.insert_batch(batch)
        a.apply_batch(batch)
        a2.apply_batch(batch)
        head = a.apply_batch(more)
        assert a2.apply_batch(more) == head
        for t in (a, a2):
            v = t.view(s)
            got = v.insert_witness(n)
            for k in want:
                bad = np.argwhere((got[k] != want[k]).reshape(got[k].shape[0], -1).any(axis=1))
                assert bad.size == 0, f"{k}: first differing row {bad[0][0]}"
            assert v.stats()[1] == 1 and t.root() == head and t.size == s + 2 * n
            v.close()
    finally:
        a.close()
        a2.close()
        b.close()
        torch.cuda.empty_cache()
