"""GPU (MI355X): imt_itree_rewind -- the tree as it was when it held fewer leaves.

The claim under test is an identity: after rewind(s) a tree cannot be told, through any call, from a fresh tree that
received the first s - 1 values -- while only the nodes of S_0 = relinked leaves + {s}, S_(l+1) = {x >> 1} were hashed.
Expected values are the sequential oracle's (Oracle.sparse_insert over a prefix of tests/insert_corpus.py's value
streams) or a twin tree's; every comparison is bit-exact.

  test_rewind_scenarios     every scenario of the corpus on the three hash forms: all batches (apply and witness batches
                            taking turns), then back to every batch boundary from the last to the first and to the empty
                            tree.  After each step: root_out, root(), size, get_leaves and get_proof_batch of every index
                            (of [0, size before] and capacity - 1 when the capacity exceeds 1024), the hashes per level
                            against the definition, lookup of a removed and of a kept value.
  test_rewind_then_fork     back to the middle boundary, then witness batches: the same values again give the corpus's
                            rows, other values the rows of a fresh oracle run of prefix + fork.  Host pointers, device
                            pointers under IMT_PIPELINE with the rewind called while batches are in flight, and
                            IMT_HOST_PREP after the rewind.
  test_rewind_large         2^16 insertions undone in a tree of 2^20 + 2^16 + 1 leaves, against a twin that never made
                            them; both forms of the hash kernel run.
  test_rewind_arguments     every refusal with the tree untouched, k = 0, the never-used tree, the full tree.
  test_rewind_sliced_world  both replicas of a flushed two-GPU world rewound, more steps, against the sequential oracle;
                            refused before the flush.
  test_reorg_demo_example   examples/reorg_demo.c: its last root against the oracle's.
"""
import bisect
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import insert_corpus as ic
import oracle_lib
import test_gpu_insert_matrix as tm
from oracle_lib import arr_ints, ints_to_arr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = tm.FORMS
OUT_FIELDS = ("low_index", "is_largest", "low_leaf", "new_leaf", "old_root", "interim_root", "new_root")


@pytest.fixture(scope="module")
def forms(imt):
    import torch
    torch.cuda.init()
    cs = {}
    for name, coop in FORMS.items():
        c = imt.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        if coop is not None:
            c.set_option(imt._ffi.OPT_COOP_MAX_EVENTS, coop)
        cs[name] = c
    yield cs
    for c in cs.values():
        c.close()


def new_tree(imt, c, sc):
    t = imt.IndexedTree(c, sc.depth, sc.cap)
    if sc.placement:
        t.set_placement(*sc.placement)
    return t


def ceil_log2(x):
    return max(0, (x - 1).bit_length())


# ---------------------------------------------------------------- the oracle's prefix trees
def _lift(orc, depth_from, depth_to, root, proofs):
    """a depth_from tree as the left-most subtree of a depth_to one (ic.extend_depth's rule)"""
    for d in range(depth_from, depth_to):
        z = orc.zero_hashes(d)[d]
        root = arr_ints(orc.hash2_batch(np.stack([ints_to_arr([root])[0], z])[None]))[0]
        proofs = np.concatenate([proofs, np.broadcast_to(z, (proofs.shape[0], 1, 32))], axis=1)
    return root, proofs


def query_indices(sc, n_values):
    """local indices every step of a scenario is checked at"""
    if sc.cap <= 1024:
        return list(range(sc.cap))
    return sorted(set(range(n_values + 2)) | {sc.cap - 1})


@functools.lru_cache(maxsize=None)
def prefix_trees(name):
    """{s: dict(root, proofs, preimages)} of the tree that holds the first s - 1 values of ic.expected(name)["vals"], for
    s = 1 and every batch boundary: one oracle run, snapshots taken on the way (indices: query_indices)."""
    sc, vals = ic.BY_NAME[name], ic.expected(name)["vals"]
    orc = oracle_lib.load()
    d = min(sc.depth, ic.ORACLE_MAX_DEPTH)
    sizes = {1} | {b + 1 for _, b in ic.batch_bounds(sc)}
    idx = query_indices(sc, len(vals))
    h = orc.sparse_new(d, sc.cap)
    orc.sparse_set_index_base(h, sc.index_base)
    out = {}
    try:
        for i in range(len(vals) + 1):
            if i + 1 in sizes:
                proofs, pre = ic._snapshot(orc, h, d, idx)
                root, proofs = _lift(orc, d, sc.depth, orc.sparse_root(h), proofs)
                out[i + 1] = dict(root=root, proofs=proofs, preimages=pre)
            if i < len(vals):
                assert orc.sparse_insert(h, d, vals[i])["rc"] == 0
    finally:
        orc.sparse_free(h)
    return out


def rewind_counts(before, after, idx, M, s, depth):
    """hashes per level by the definition, from the oracle's preimages of the tree of M leaves and of s leaves"""
    if s == M:
        return [0] * (depth + 1)
    pos = {x: r for r, x in enumerate(idx)}
    S = {i for i in range(s) if not (before["preimages"][pos[i]] == after["preimages"][pos[i]]).all()} | {s}
    l0, out = min(ceil_log2(M), depth), []
    for l in range(depth + 1):
        out.append(len(S) if l < l0 else 1)
        S = {x >> 1 for x in S}
    return out


def check_tree(imt, t, sc, want, idx, size, tag):
    """every query of the tree against the oracle's tree of `size` leaves"""
    assert t.size == size and t.root() == want["root"], tag
    gidx = np.array(idx, np.uint64) + np.uint64(sc.index_base)
    pre = t.get_leaves(gidx)
    bad = np.nonzero((pre != want["preimages"]).reshape(len(idx), -1).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: preimage of leaf {idx[bad[0]]}"
    proofs = t.get_proof_batch(gidx, item_major=True)
    bad = np.argwhere((proofs != want["proofs"]).any(axis=2))
    assert bad.size == 0, f"{tag}: proof of leaf {idx[bad[0][0]]} level {bad[0][1]}"


def check_lookup(imt, t, sc, vals, s, M, tag):
    """a removed value is NEW with its low leaf among the kept ones, a kept one PRESENT"""
    f, base = imt._ffi, sc.index_base
    if s < M:
        v = vals[s - 1]                                   # the first removed value
        kept = sorted((x, i + 1) for i, x in enumerate(vals[:s - 1]))
        p = bisect.bisect_left(kept, (v, 0)) - 1
        low = kept[p][1] if p >= 0 else 0
        st, leaf = t.lookup(ints_to_arr([v]))
        assert st[0] == f.VAL_NEW and leaf[0] == base + low, tag
    if s > 1:
        st, leaf = t.lookup(ints_to_arr([vals[s - 2]]))
        assert st[0] == f.VAL_PRESENT and leaf[0] == base + s - 1, tag


def _scenario_cases():
    out = []
    for sc in ic.SCENARIOS:
        for form in ("default", "thread", "quad"):
            if sc.name == "d16_big" and form != "default":
                continue
            out.append(pytest.param(sc.name, form, id=f"{sc.name}-{form}"))
    return out


@pytest.mark.parametrize("name,form", _scenario_cases())
def test_rewind_scenarios(imt, forms, name, form):
    sc, exp, trees = ic.BY_NAME[name], ic.expected(name), prefix_trees(name)
    vals, idx = exp["vals"], query_indices(sc, len(exp["vals"]))
    t = new_tree(imt, forms[form], sc)
    try:
        bounds = ic.batch_bounds(sc)
        for j, (a, b) in enumerate(bounds):
            if j % 2 == 0:
                assert t.apply_batch(ints_to_arr(vals[a:b])) == exp["batch_roots"][j + 1]
            else:
                t.insert_batch(ints_to_arr(vals[a:b]))
        M = len(vals) + 1
        check_tree(imt, t, sc, trees[M], idx, M, f"{name} before any rewind")
        for s in [b + 1 for _, b in reversed(bounds)] + [1]:
            tag = f"{name} rewind {M} -> {s}"
            root = t.rewind(s)
            stats = t.rewind_stats.tolist()
            print(f"{tag}: hashes {stats}")
            assert root == trees[s]["root"], f"{tag}: root_out"
            check_tree(imt, t, sc, trees[s], idx, s, tag)
            assert stats == rewind_counts(trees[M], trees[s], idx, M, s, sc.depth), f"{tag}: hashes per level"
            check_lookup(imt, t, sc, vals, s, M, tag)
            M = s
        assert t.root() == ic.empty_root(oracle_lib.load(), sc.depth)
    finally:
        t.close()


# ---------------------------------------------------------------- rewind, then another branch
def oracle_rows(sc, vals, first):
    """the oracle's imt_insert_out rows of insertions [first, len(vals)) of the sequence `vals` (depth <= 63)"""
    orc, depth, base = oracle_lib.load(), sc.depth, sc.index_base
    h = orc.sparse_new(depth, sc.cap)
    orc.sparse_set_index_base(h, base)
    n = len(vals) - first
    rec = dict(low_index=np.empty(n, np.uint64), is_largest=np.empty(n, np.uint8), low_leaf=np.empty((n, 3, 32), np.uint8),
               new_leaf=np.empty((n, 3, 32), np.uint8), old_root=np.empty((n, 32), np.uint8),
               interim_root=np.empty((n, 32), np.uint8), new_root=np.empty((n, 32), np.uint8),
               low_sib=np.empty((n, depth, 32), np.uint8), new_sib=np.empty((n, depth, 32), np.uint8))
    try:
        for i, v in enumerate(vals):
            old = orc.sparse_root(h)
            r = orc.sparse_insert(h, depth, v)
            assert r["rc"] == 0
            if i < first:
                continue
            k = i - first
            rec["low_index"][k], rec["is_largest"][k], rec["low_leaf"][k] = r["low"] + base, r["largest"], r["low_leaf"]
            nl = r["low_leaf"].copy()
            nl[0] = ints_to_arr([v])[0]
            rec["new_leaf"][k] = nl
            rec["old_root"][k] = ints_to_arr([old])[0]
            rec["interim_root"][k] = ints_to_arr([r["interim_root"]])[0]
            rec["new_root"][k] = ints_to_arr([r["new_root"]])[0]
            rec["low_sib"][k], rec["new_sib"][k] = r["low_proof"], r["new_proof"]
    finally:
        orc.sparse_free(h)
    return rec


def compare_rows(got, want, lo, hi, depth, tag):
    """got: one batch's outputs (numpy; siblings level-major [global_depth, n, 32]); want: rows [lo, hi) of `want`"""
    n = hi - lo
    for k in OUT_FIELDS:
        bad = np.nonzero((np.asarray(got[k]) != want[k][lo:hi]).reshape(n, -1).any(axis=1))[0]
        assert bad.size == 0, f"{tag}: {k}, first differing row {lo + bad[0]}"
    for k in ("low_sib", "new_sib"):
        g = np.asarray(got[k])[:depth].transpose(1, 0, 2)
        bad = np.argwhere((g != want[k][lo:hi]).any(axis=2))
        assert bad.size == 0, f"{tag}: {k}, first difference at row {lo + bad[0][0]} level {bad[0][1]}"


class DeviceBatches:
    """witness batches with device pointers under IMT_PIPELINE: nothing is read before sync()"""

    def __init__(self, imt, c, t, G):
        import torch
        self.imt, self.c, self.t, self.G, self.torch, self.pending = imt, c, t, G, torch, []

    def insert(self, arr, want_outputs=True):
        torch, f, n = self.torch, self.imt._ffi, arr.shape[0]
        v = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        bufs, out = dict(vals=v), None
        if want_outputs:
            shapes = dict(low_index=(n,), is_largest=(n,), low_leaf=(n, 3, 32), new_leaf=(n, 3, 32), old_root=(n, 32),
                          interim_root=(n, 32), new_root=(n, 32), low_sib=(self.G, n, 32), new_sib=(self.G, n, 32))
            for k, shp in shapes.items():
                bufs[k] = torch.zeros(shp, dtype=torch.int64 if k == "low_index" else torch.uint8, device="cuda")
            out = f.InsertOut(**{k: bufs[k].data_ptr() for k in shapes})
        rc = self.imt.lib.imt_itree_insert_batch(self.t.h, ctypes.c_void_p(v.data_ptr()), n,
                                                 ctypes.byref(out) if out is not None else None, f.DEVICE_PTRS | f.PIPELINE)
        assert rc == 0, self.imt.lib.imt_last_error(self.c.h)
        self.pending.append(bufs)
        return bufs

    def sync(self):
        self.c.sync()
        self.torch.cuda.synchronize()

    @staticmethod
    def host(bufs):
        out = {k: v.cpu().numpy() for k, v in bufs.items() if k != "vals"}
        out["low_index"] = out["low_index"].view(np.uint64)
        return out


@pytest.mark.parametrize("mode", ["host", "pipe", "host_prep"])
@pytest.mark.parametrize("name", ["d32_between", "d16_pow2", "placed_g5"])
def test_rewind_then_fork(imt, forms, name, mode):
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    c, vals, bounds = forms["default"], exp["vals"], ic.batch_bounds(sc)
    mid = len(bounds) // 2
    s = bounds[mid][0] + 1                                           # the tree after the batches before `mid`
    used = set(vals)
    other = [v for v in oracle_lib.synth_values(len(vals) + 8, 0x52574600 + sc.seed) if v not in used]
    fork_vals = vals[:s - 1] + other[:len(vals) - (s - 1)]
    branches = (("the same values again", vals, exp["rec"], s - 1),
                ("another branch", fork_vals, oracle_rows(sc, fork_vals, s - 1), 0))
    for what, seq, want, off in branches:
        t = new_tree(imt, c, sc)
        try:
            if mode == "pipe":                                       # every batch enqueued, then the rewind: no sync between
                dv = DeviceBatches(imt, c, t, sc.global_depth)
                for a, b in bounds:
                    dv.insert(ints_to_arr(vals[a:b]), want_outputs=False)
                assert t.rewind(s) == exp["batch_roots"][mid], what
                outs = [dv.insert(ints_to_arr(seq[a:b])) for a, b in bounds[mid:]]
                dv.sync()
                for (a, b), o in zip(bounds[mid:], outs):
                    compare_rows(dv.host(o), want, a - (s - 1) + off, b - (s - 1) + off, sc.depth, f"{name} {what} [{a}, {b})")
            else:
                for j, (a, b) in enumerate(bounds):
                    t.apply_batch(ints_to_arr(vals[a:b])) if j % 2 else t.insert_batch(ints_to_arr(vals[a:b]))
                assert t.rewind(s) == exp["batch_roots"][mid], what
                for a, b in bounds[mid:]:
                    got = t.insert_batch(ints_to_arr(seq[a:b]), host_prep=(mode == "host_prep"))
                    compare_rows(got, want, a - (s - 1) + off, b - (s - 1) + off, sc.depth, f"{name} {what} [{a}, {b})")
                    assert (got["new_index"] == np.arange(a + 1, b + 1, dtype=np.uint64) + np.uint64(sc.index_base)).all()
            assert t.size == len(vals) + 1
            assert t.root() == arr_ints(want["new_root"][-1:])[0], what
        finally:
            t.close()


# ---------------------------------------------------------------- a size users run
def test_rewind_large(imt, forms):
    """Twins a and b apply the same 2^20 random values; a applies 2^16 more and goes back to 2^20 + 1 leaves.  Computed on
    the CPU first (the sorted order of all values): about 63 000 kept leaves lose their successor, so with l0 = 21 (of the
    size before the call) the leaf launch and levels 1..6 take the thread form k_apply_level, levels 7..20 (launch bounds
    2^14 .. 2) the quad form under the default switch of 16384, levels 21..32 are the single chain.  The assertion
    hashes[1] > 16384 >= hashes[7] holds for these values and is checked on the CPU's counts before it is asked of the
    GPU's."""
    import torch
    depth, cap, M0, n = 32, 1 << 21, 1 << 20, 1 << 16
    c = forms["default"]
    allv = oracle_lib.synth_values(M0 + n + 1024, 0x52574C20)
    base_vals, new_vals, more = allv[:M0], allv[M0:M0 + n], allv[M0 + n:]
    # on the CPU: the leaves (sentinel = leaf 0) in value order, the kept ones whose successor is removed
    leafvals = [0] + base_vals + new_vals
    order = sorted(range(len(leafvals)), key=leafvals.__getitem__)
    s, M = M0 + 1, M0 + n + 1
    S = {s} | {order[j] for j in range(len(order) - 1) if order[j] < s <= order[j + 1]}
    want = []
    for l in range(depth + 1):
        want.append(len(S) if l < ceil_log2(M) else 1)
        S = {x >> 1 for x in S}
    assert want[1] > 16384 >= want[7], "these values must make both forms of k_apply_level run"
    a, b = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    try:
        pre = ints_to_arr(base_vals)
        assert a.apply_batch(pre) == b.apply_batch(pre)
        a.apply_batch(ints_to_arr(new_vals))
        assert a.size == M and a.root() != b.root()
        root = a.rewind(s)
        stats = a.rewind_stats.tolist()
        print(f"large: hashes per level {stats}, {sum(stats) / n:.2f} per insertion undone")
        assert root == a.root() == b.root() and a.size == b.size == s
        assert stats == want
        assert stats[1] > 16384 >= stats[7], "both forms of k_apply_level must have run"
        rng = np.random.default_rng(0x52574C21)
        idx = np.unique(np.concatenate([rng.integers(0, M + 1, 4096).astype(np.uint64),
                                        np.arange(M0 - 64, M0 + n + 2, dtype=np.uint64)]))
        assert (a.get_leaves(idx) == b.get_leaves(idx)).all()
        assert (a.get_proof_batch(idx) == b.get_proof_batch(idx)).all()
        ra, rb = a.insert_batch(ints_to_arr(more)), b.insert_batch(ints_to_arr(more))
        for k in ra:
            assert (ra[k] == rb[k]).all(), k
    finally:
        a.close()
        b.close()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- arguments
def test_rewind_arguments(imt, ctx):
    import torch
    f, lib = imt._ffi, imt.lib
    depth, cap = 32, 64
    vals = oracle_lib.synth_values(100, 0x52574130)
    t = imt.IndexedTree(ctx, depth, cap)
    P_ = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    try:
        root0 = t.root()
        assert t.rewind(1) == root0 and t.size == 1 and t.rewind_stats.tolist() == [0] * (depth + 1)   # never used
        t.apply_batch(vals[:20])
        t.insert_batch(vals[20:40])
        idx = np.arange(cap, dtype=np.uint64)

        def state():
            return t.size, t.root(), t.get_leaves(idx).tobytes(), t.get_proof_batch(idx).tobytes()

        def refused(code, size, root_out=None, flags=0):
            before = state()
            h = (ctypes.c_uint64 * (depth + 1))()
            rc = lib.imt_itree_rewind(t.h, size, root_out, h, flags)
            assert rc == f.ERR[code], (rc, lib.imt_last_error(ctx.h))
            return before

        out = np.zeros(32, np.uint8)
        host_out = out.ctypes.data_as(ctypes.c_void_p)
        for code, size, ro, flags in (("RANGE", 0, host_out, 0), ("RANGE", 42, host_out, 0), ("RANGE", 1 << 40, None, 0),
                                      ("ARG", 30, host_out, f.PIPELINE), ("ARG", 30, None, f.PIPELINE | f.DEVICE_PTRS),
                                      ("ARG", 30, host_out, 3)):
            assert refused(code, size, ro, flags) == state(), (code, size, flags)
        dev_out = torch.zeros(64, dtype=torch.uint8, device="cuda")
        assert refused("ARG", 30, P_(dev_out, 8), f.DEVICE_PTRS) == state()             # misaligned device root_out
        # a sharded batch between begin and end
        ev, l0 = ctypes.c_uint32(), ctypes.c_uint32()
        more = ints_to_arr(vals[40:44])
        assert lib.imt_itree_batch_begin(t.h, more.ctypes.data_as(ctypes.c_void_p), 4, 0, ctypes.byref(ev), ctypes.byref(l0)) == 0
        before = refused("ARG", 30, host_out)
        assert lib.imt_itree_batch_abort(t.h) == 0
        assert before == state()
        # an open slice
        dvals = torch.from_numpy(ints_to_arr(vals[40:48])).cuda()
        pay = torch.zeros(int(lib.imt_itree_slice_payload_bytes(8)) + 64, dtype=torch.uint8, device="cuda")
        sl = ctypes.c_int(-1)
        before = state()
        assert lib.imt_itree_slice_prepare(t.h, P_(dvals), 0, 8, 0, None, f.DEVICE_PTRS, ctypes.byref(sl), None) == 0
        h = (ctypes.c_uint64 * (depth + 1))()
        assert lib.imt_itree_rewind(t.h, 30, host_out, h, 0) == f.ERR["ARG"]
        assert lib.imt_itree_rewind(t.h, 49, host_out, h, 0) == f.ERR["ARG"]            # k = 0 is refused there too
        for q in range(depth + 1):
            assert lib.imt_itree_slice_unit(t.h, sl.value, q, P_(pay), None) == 0
        ctx.sync()
        assert t.size == 49 and t.rewind(41) == before[1] and state() == before         # the slice's 8 values undone
        # k = 0: nothing runs, the current root, hashes all zero; root_out on the device in another format
        h = (ctypes.c_uint64 * (depth + 1))(*([7] * (depth + 1)))
        assert lib.imt_itree_rewind(t.h, 41, host_out, h, 0) == 0
        assert arr_ints(out)[0] == before[1] and list(h) == [0] * (depth + 1) and state() == before
        assert lib.imt_itree_rewind(t.h, 41, None, None, 0) == 0
        dev_root = torch.zeros(32, dtype=torch.uint8, device="cuda")
        assert lib.imt_itree_rewind(t.h, 31, P_(dev_root), None, f.DEVICE_PTRS | f.FMT_MONT256) == 0
        ctx.sync()
        assert arr_ints(dev_root.cpu().numpy())[0] == t.root() * tm.R_OF[1] % oracle_lib.P and t.size == 31
        # apply_stats keeps the last apply call's counts
        stats = t.apply_stats().tolist()
        t.rewind(21)
        assert t.apply_stats().tolist() == stats
        # root_lagged has no root to give until the next batch, as after a load
        buf = np.empty(32, np.uint8)
        assert lib.imt_itree_root_lagged(t.h, 0, buf.ctypes.data_as(ctypes.c_void_p), 0) != 0
        # rewind, fill to capacity, IMT_ERR_FULL, rewind again
        twin = imt.IndexedTree(ctx, depth, cap)
        twin.apply_batch(vals[:20])
        assert twin.root() == t.root()
        fill = vals[40:40 + cap - 21]
        assert t.apply_batch(fill) == twin.apply_batch(fill) and t.size == cap
        assert lib.imt_itree_root_lagged(t.h, 0, buf.ctypes.data_as(ctypes.c_void_p), 0) == 0 and arr_ints(buf)[0] == t.root()
        with pytest.raises(imt.ImtError) as ei:
            t.apply_batch([12345])
        assert ei.value.code == f.ERR["FULL"] and t.size == cap and t.root() == twin.root()
        assert t.rewind(cap - 1) != twin.root()
        last = t.insert_batch(fill[-1:])
        assert t.root() == twin.root() and (t.snapshot() == twin.snapshot()).all()
        assert (t.get_proof_batch(idx) == twin.get_proof_batch(idx)).all()
        assert int(last["new_index"][0]) == cap - 1
        assert t.rewind(1) == root0 and t.size == 1
        fresh = imt.IndexedTree(ctx, depth, cap)
        assert (t.get_proof_batch(idx) == fresh.get_proof_batch(idx)).all()
        fresh.close()
        twin.close()
    finally:
        t.close()


# ---------------------------------------------------------------- the multi-GPU mode
def test_rewind_sliced_world(imt, ctx):
    """world 2 over the local transport: three steps, a rewind before the flush is refused, imt_sliced_flush, both
    replicas back to the size after the first step, three other steps in the same world: every witness of every rank
    against the sequential oracle over first step + the new steps."""
    import torch
    import test_gpu_sliced as ts
    sl = ts.load_sliced()
    depth, cap, world, batch = 32, 1 << 12, 2, 150
    step = world * batch
    vals = oracle_lib.synth_values(7 * step, 0x52575300)
    dropped, fork = vals[:3 * step], vals[:step] + vals[3 * step:6 * step]
    orc = oracle_lib.load()
    oh = orc.sparse_new(depth, cap)
    rows = [orc.sparse_insert(oh, depth, v) for v in fork]
    assert all(r["rc"] == 0 for r in rows)
    want_root = orc.sparse_root(oh)
    orc.sparse_free(oh)
    w = sl.SlicedTree(imt, 0, depth, cap, batch, world, n_local=world, nbuf=8)
    try:
        arr = torch.from_numpy(ints_to_arr(dropped)).cuda()
        for r in range(3):
            w.step(arr[r * step:(r + 1) * step])
        h = (ctypes.c_uint64 * (depth + 1))()
        for t in w.trees:                                    # steps in flight: only imt_sliced_* calls may touch the trees
            assert imt.lib.imt_itree_rewind(t.h, step + 1, None, h, 0) == imt._ffi.ERR["ARG"]
        w.flush()
        assert all(t.size == 3 * step + 1 for t in w.trees)
        roots = [t.rewind(step + 1) for t in w.trees]
        assert roots[0] == roots[1] == rows[step - 1]["new_root"]
        assert (w.trees[0].snapshot() == w.trees[1].snapshot()).all()
        arr2 = torch.from_numpy(ints_to_arr(fork[step:])).cuda()
        rounds = [w.step(arr2[r * step:(r + 1) * step]) for r in range(3)]
        w.flush()
        for r, R in enumerate(rounds):
            for k in range(world):
                o = {f: v.cpu().numpy() for f, v in w.outputs(R, k).items() if torch.is_tensor(v)}
                first = (r + 1) * step + k * batch
                assert w.outputs(R, k)["first_insertion"] == 1 + first
                for j in range(batch):
                    e = rows[first + j]
                    assert imt.to_int(o["new_root"][j]) == e["new_root"] and imt.to_int(o["interim_root"][j]) == e["interim_root"]
                    assert imt.to_int(o["old_root"][j]) == rows[first + j - 1]["new_root"], (r, k, j)
                    assert int(o["low_index"][j]) == e["low"] and int(o["is_largest"][j]) == e["largest"], (r, k, j)
                    assert (o["low_sib"][:, j] == e["low_proof"]).all() and (o["new_sib"][:, j] == e["new_proof"]).all()
                    assert (o["low_leaf"][j] == e["low_leaf"]).all(), (r, k, j)
        assert all(t.root() == want_root and t.size == 4 * step + 1 for t in w.trees)
    finally:
        w.close()


# ---------------------------------------------------------------- the C example
def test_reorg_demo_example(imt, oracle):
    """examples/reorg_demo.c applies ten blocks, rewinds three and applies three others, printing each root; given the
    oracle's last root as its argument it compares and fails on a difference."""
    exe = os.path.join(ROOT, "examples", "reorg_demo")
    csrc = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "reorg_demo.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def value(branch, j, i):       # the example's values
        return 1 + 7919023757 * (64 * j + i + 1 + (1000000 if branch else 0)) % ((1 << 61) - 1)

    def run(blocks):
        h, roots = oracle.sparse_new(32, 1024), []
        for branch, j in blocks:
            for i in range(64):
                assert oracle.sparse_insert(h, 32, value(branch, j, i))["rc"] == 0
            roots.append(oracle.sparse_root(h))
        oracle.sparse_free(h)
        return roots

    first = run([(0, j) for j in range(10)])
    second = run([(0, j) for j in range(7)] + [(1, j) for j in range(7, 10)])
    r = subprocess.run([exe, f"{second[-1]:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for j, want in enumerate(first):
        assert f"block {j}: root {want:064x}" in r.stdout, r.stdout
    assert f"rewind to 449 leaves: root {first[6]:064x}" in r.stdout, r.stdout
    for j in range(7, 10):
        assert f"fork block {j}: root {second[j]:064x}" in r.stdout, r.stdout
    assert "final root equals the expected one" in r.stdout
    r = subprocess.run([exe, f"{first[-1]:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "DIFFERS" in r.stdout
