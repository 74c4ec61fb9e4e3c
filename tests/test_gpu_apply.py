"""GPU (MI355X): witness-free batch insertion (imt_itree_apply_batch / _apply_filtered / _apply_stats).

The claim under test is an identity: after apply_batch(vals) a tree cannot be told, through any call, from a twin that
ran insert_batch(vals) -- while every node the batch touches was hashed exactly once.  Expected values are the
sequential oracle's (tests/insert_corpus.py); every comparison is bit-exact.

  test_apply_scenarios     every scenario of the corpus, GPU and host prepare, the three hash forms: per batch the
                           root (root_out and root()) and the hashes per level (apply_stats against the definition:
                           S_0 = low leaves + new leaves, S_(l+1) = {x >> 1}); the tree's queries at the scenario's
                           checkpoint; the stored tree after the last batch; refused batches and the full tree.
  test_apply_alternation   apply and witness batches taking turns on one tree, either parity: every output of every
                           witness batch against the oracle -- a stale inner node that no final proof crosses is a
                           sibling of a later witness.  Once with host pointers, once with the witness batches under
                           IMT_DEVICE_PTRS | IMT_PIPELINE, so an apply call lands behind batches still in flight.
  test_apply_formats       IMT_FMT_MONT256 with host pointers; IMT_DEVICE_PTRS with root_out on the device.
  test_apply_filtered      mixed batches against the Python model of the reference's loop, with and without a value
                           partition; the tree against a twin fed insert_batch(accepted).
  test_apply_large         2^16 values into a depth-32 tree of 2^20, against a twin through insert_batch(out = NULL).
  test_apply_arguments     IMT_PIPELINE, the empty batch, apply_stats before any apply call.
  test_follow_chain_example  examples/follow_chain.c: its last root against the oracle's.
"""
import bisect
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import insert_corpus as ic
import oracle_lib
import test_gpu_insert_matrix as tm
from oracle_lib import P, arr_ints, ints_to_arr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = tm.FORMS


def touched(low_local, M, n, depth):
    """hashes per level by the definition: |S_l| for l = 0 .. depth"""
    s = set(int(x) for x in low_local) | set(range(M, M + n))
    out = [len(s)]
    for _ in range(depth):
        s = {x >> 1 for x in s}
        out.append(len(s))
    return out


def scenario_counts(sc, exp, a, b):
    low = exp["rec"]["low_index"][a:b].astype(np.uint64) - np.uint64(sc.index_base)
    return touched(low, a + 1, b - a, sc.depth)


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


def checkpoint(imt, t, chk):
    buf = np.empty(32, np.uint8)
    for lag, want in ((1, chk["prev_root"]), (0, chk["root"])):
        assert imt.lib.imt_itree_root_lagged(t.h, lag, buf.ctypes.data_as(ctypes.c_void_p), 0) == 0
        assert arr_ints(buf)[0] == want, f"root_lagged({lag})"
    assert t.root() == chk["root"]
    assert (t.get_proof_batch(chk["present_index"], item_major=True) == chk["present_proofs"]).all()
    status, leaf = t.lookup(ints_to_arr(chk["present_vals"] + chk["absent_vals"]))
    k = len(chk["present_vals"])
    assert (status[:k] == imt._ffi.VAL_PRESENT).all() and (leaf[:k] == chk["present_index"]).all()
    assert (status[k:] == imt._ffi.VAL_NEW).all() and (leaf[k:] == chk["low_index"]).all()
    absent = ints_to_arr(chk["absent_vals"])
    assert (t.find_low(absent) == chk["low_index"]).all()
    low, leaves, sib, largest = t.non_membership_witness(absent)
    assert (low == chk["low_index"]).all() and (leaves == chk["low_preimages"]).all()
    assert (largest == chk["low_largest"]).all()
    assert (sib.transpose(1, 0, 2) == chk["low_proofs"]).all()


def final_state(t, fin):
    assert t.size == fin["size"] and t.root() == fin["root"]
    assert (t.get_proof_batch(fin["index"], item_major=True) == fin["proofs"]).all()
    assert (t.get_leaves(fin["index"]) == fin["preimages"]).all()


def refused(imt, t, cap, bad, code, host_prep=False):
    """apply_batch(bad) fails with `code` and changes neither root, size nor leaves"""
    size, root = t.size, t.root()
    idx = np.arange(t.index_base, t.index_base + min(size + 1, cap), dtype=np.uint64)
    leaves = t.get_leaves(idx)
    with pytest.raises((ValueError, imt.ImtError)) as ei:
        t.apply_batch(ints_to_arr(bad), host_prep=host_prep)
    if code != "VALUE":
        assert ei.value.code == imt._ffi.ERR[code]
    else:
        assert isinstance(ei.value, ValueError)
    assert t.size == size and t.root() == root and (t.get_leaves(idx) == leaves).all()


def _scenario_cases():
    out = []
    for sc in ic.SCENARIOS:
        for form, host_prep in (("default", False), ("default", True), ("thread", False), ("quad", False)):
            if sc.name == "d16_big" and form != "default":
                continue
            out.append(pytest.param(sc.name, form, host_prep, id=f"{sc.name}-{form}-{'host' if host_prep else 'gpu'}prep"))
    return out


@pytest.mark.parametrize("name,form,host_prep", _scenario_cases())
def test_apply_scenarios(imt, forms, oracle, name, form, host_prep):
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    t = new_tree(imt, forms[form], sc)
    try:
        assert t.root() == ic.empty_root(oracle, sc.depth)
        for j, (a, b) in enumerate(ic.batch_bounds(sc)):
            for bad in exp["refused"].get(j, ()):
                refused(imt, t, sc.cap, bad, "VALUE", host_prep)
            root = t.apply_batch(ints_to_arr(exp["vals"][a:b]), host_prep=host_prep)
            print(f"{name} batch {j}: hashes {t.apply_stats().tolist()}")
            assert root == exp["batch_roots"][j + 1], f"root_out after batch {j}"
            assert t.root() == exp["batch_roots"][j + 1] and t.size == b + 1
            assert t.apply_stats().tolist() == scenario_counts(sc, exp, a, b), f"hashes per level, batch {j}"
            if j == sc.check:
                checkpoint(imt, t, exp["check"])
        final_state(t, exp["final"])
        if exp["full_value"] is not None:
            refused(imt, t, sc.cap, [exp["full_value"]], "FULL", host_prep)
    finally:
        t.close()


# ---------------------------------------------------------------- alternation with witness batches
class Alternating(tm.Runner):
    """tests/test_gpu_insert_matrix.py's runner with every batch of one parity sent through imt_itree_apply_batch"""

    def __init__(self, imt, c, sc, path, apply_parity):
        super().__init__(imt, c, sc, path)
        self.apply_parity, self.roots = apply_parity, []

    def batch(self, j, a, b):
        if j % 2 != self.apply_parity:
            return super().batch(j, a, b)
        imt, f, n = self.imt, self.imt._ffi, b - a
        want = self.exp["batch_roots"][j + 1]
        if self.path == "py":
            assert self.t.apply_batch(ints_to_arr(self.exp["vals"][a:b])) == want, f"apply root, batch {j}"
        else:                      # device pointers, the path's format; the root is read after the last batch
            flags = self.cfg["flags"] & ~(f.PIPELINE | f.SIB_ITEM_MAJOR)
            out = self.torch.zeros(32, dtype=self.torch.uint8, device="cuda")
            rc = imt.lib.imt_itree_apply_batch(self.t.h, ctypes.c_void_p(self.vaddr + a * 32), n,
                                               ctypes.c_void_p(out.data_ptr()), flags)
            assert rc == 0, imt.lib.imt_last_error(self.c.h)
            self.roots.append((j, out, want))
        assert self.t.size == b + 1

    def finish(self):
        super().finish()
        for j, out, want in self.roots:
            got = arr_ints(out.cpu().numpy())[0]
            assert got == want * tm.R_OF.get(self.cfg["fmt"], 1) % P, f"apply root_out, batch {j}"


@pytest.mark.parametrize("path", ["py", "pipe"])
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("name", [s.name for s in ic.SCENARIOS])
def test_apply_alternation(imt, forms, name, parity, path):
    sc = ic.BY_NAME[name]
    r = Alternating(imt, forms["default"], sc, path, parity)
    try:
        for j, (a, b) in enumerate(ic.batch_bounds(sc)):
            r.batch(j, a, b)
            if path == "pipe" and j == sc.check:
                r.checkpoint()
        r.finish()
    finally:
        r.close()


# ---------------------------------------------------------------- formats
@pytest.mark.parametrize("mode", ["mont256_host", "device_ptrs", "inputs_ready"])
def test_apply_formats(imt, forms, mode):
    """inputs_ready: IMT_DEVICE_PTRS | IMT_INPUTS_READY, every batch enqueued before the one synchronisation -- the
    preparation of a batch then runs on the side stream beside the hashing of the batch before."""
    import torch
    sc, exp = ic.BY_NAME["d32_between"], ic.expected("d32_between")
    c, f = forms["default"], imt._ffi
    t = new_tree(imt, c, sc)
    pending = []
    try:
        for j, (a, b) in enumerate(ic.batch_bounds(sc)):
            vals = ints_to_arr(exp["vals"][a:b])
            want = exp["batch_roots"][j + 1]
            if mode == "mont256_host":
                v = tm.to_fmt(vals, 1)
                out = np.zeros(32, np.uint8)
                rc = imt.lib.imt_itree_apply_batch(t.h, v.ctypes.data_as(ctypes.c_void_p), b - a,
                                                   out.ctypes.data_as(ctypes.c_void_p), f.FMT_MONT256)
                assert rc == 0, imt.lib.imt_last_error(c.h)
                assert arr_ints(out)[0] == want * tm.R_OF[1] % P, f"batch {j}"
            elif mode == "inputs_ready":
                v = torch.from_numpy(vals.copy()).cuda()
                out = torch.zeros(32, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()               # the caller's side of IMT_INPUTS_READY: the buffers are idle
                rc = imt.lib.imt_itree_apply_batch(t.h, ctypes.c_void_p(v.data_ptr()), b - a, ctypes.c_void_p(out.data_ptr()),
                                                   f.DEVICE_PTRS | f.INPUTS_READY)
                assert rc == 0, imt.lib.imt_last_error(c.h)
                pending.append((j, v, out, want))
                continue
            else:
                v = torch.from_numpy(vals.copy()).cuda()
                out = torch.zeros(32, dtype=torch.uint8, device="cuda")
                rc = imt.lib.imt_itree_apply_batch(t.h, ctypes.c_void_p(v.data_ptr()), b - a, ctypes.c_void_p(out.data_ptr()),
                                                   f.DEVICE_PTRS)
                assert rc == 0, imt.lib.imt_last_error(c.h)
                c.sync()
                assert arr_ints(out.cpu().numpy())[0] == want, f"batch {j}"
            assert t.apply_stats().tolist() == scenario_counts(sc, exp, a, b)
        c.sync()
        for j, _, out, want in pending:
            assert arr_ints(out.cpu().numpy())[0] == want, f"batch {j}"
        final_state(t, exp["final"])
    finally:
        t.close()


# ---------------------------------------------------------------- filtered
ZERO, PRESENT, REPEATED, NEW, FOREIGN = 1, 2, 3, 0, 4
NONE = (1 << 64) - 1


class Model:
    """The stored values of a tree (leaf order) and the reference's loop with the rejected values skipped
    (restated from tests/test_gpu_filtered.py)."""

    def __init__(self, base=0, pm=0, pr=0):
        self.vals, self.where, self.base, self.pm, self.pr = [0], {0: 0}, base, pm, pr

    def classify(self, batch):
        M, first, acc, status, leaf = len(self.vals), {}, [], [], []
        for v in batch:
            if v == 0:
                s, l = ZERO, self.base
            elif self.pm > 1 and v % self.pm != self.pr:
                s, l = FOREIGN, NONE
            elif v in self.where:
                s, l = PRESENT, self.base + self.where[v]
            elif v in first:
                s, l = REPEATED, self.base + M + first[v]
            else:
                first[v] = len(acc)
                acc.append(v)
                s, l = NEW, self.base + M + first[v]
            status.append(s)
            leaf.append(l)
        return status, leaf, acc

    def commit(self, acc):
        for v in acc:
            self.where[v] = len(self.vals)
            self.vals.append(v)


def mixed_batch(rng, model, fresh, n, p_zero=0.08, p_stored=0.15, p_repeat=0.15):
    out = []
    for _ in range(n):
        r = rng.random()
        if r < p_zero:
            out.append(0)
        elif r < p_zero + p_stored and len(model.vals) > 1:
            out.append(rng.choice(model.vals[1:]))
        elif r < p_zero + p_stored + p_repeat and out:
            out.append(rng.choice(out))
        elif fresh:
            out.append(fresh.pop())
        else:
            out.append(0)
    return out


@pytest.mark.parametrize("partition", [None, (3, 1)])
@pytest.mark.parametrize("host_prep", [False, True])
def test_apply_filtered(imt, ctx, partition, host_prep):
    depth, cap = 32, 1024
    rng = random.Random(0x41504C00 + 2 * bool(partition) + host_prep)
    fresh = oracle_lib.synth_values(cap, 0x41504C10)
    a, b = imt.IndexedTree(ctx, depth, cap), imt.IndexedTree(ctx, depth, cap)
    pm, pr = partition or (0, 0)
    try:
        if partition:
            ctx._check(imt.lib.imt_itree_set_value_partition(a.h, pm, pr))
            ctx._check(imt.lib.imt_itree_set_value_partition(b.h, pm, pr))
        m = Model(0, pm, pr)
        # an all-rejected batch on the empty tree: IMT_OK, nothing inserted, the root stays
        root0 = a.root()
        st, leaf, k, root = a.apply_filtered([0, 0, 0], host_prep=host_prep)
        assert k == 0 and root == root0 and st.tolist() == [ZERO] * 3 and a.size == 1
        for n in (4, 9, 3, 1, 40, 120, 200):
            batch = mixed_batch(rng, m, fresh, n)
            status, leaf, acc = m.classify(batch)
            st, lf, k, root = a.apply_filtered(batch, host_prep=host_prep)
            assert k == len(acc) and st.tolist() == status and lf.tolist() == leaf, batch
            if acc:
                b.insert_batch(acc)
                assert a.apply_stats()[0] >= len(acc)
            m.commit(acc)
            assert root == a.root() == b.root() and a.size == b.size == len(m.vals)
        assert (a.snapshot() == b.snapshot()).all()
        idx = np.arange(a.size, dtype=np.uint64)
        assert (a.get_proof_batch(idx) == b.get_proof_batch(idx)).all()
        # all rejected on a filled tree
        before = a.root()
        st, lf, k, root = a.apply_filtered([0, m.vals[1], m.vals[2]], host_prep=host_prep)
        assert k == 0 and root == before == a.root() and st.tolist() == [ZERO, PRESENT, PRESENT]
        # the next witness batch on the applied tree is the twin's, row for row
        more = [v for v in fresh[:40] if not partition or v % pm == pr]
        ra, rb = a.insert_batch(more), b.insert_batch(more)
        for key in ra:
            assert (ra[key] == rb[key]).all(), key
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- a size users run
def test_apply_large(imt, forms):
    """2^16 random values into a depth-32 tree that holds 2^20 + 1 leaves, against a twin through
    imt_itree_insert_batch(out = NULL).  E = 2^17 events and l0 = 21 (2^20 < size after the batch <= 2^21), so the
    launches are bounded by min(2^17, 2^(21 - l)) nodes: the leaf launch and levels 1..6 (bounds 2^17 .. 2^15) take the
    thread form k_apply_level, levels 7..20 (bounds 2^14 .. 2) the quad form k_apply_level_coop under the default
    switch of 16384, and levels 21..32 are the single chain of k_apply_top.  The counts asserted below straddle the
    switch: more than 16384 nodes at level 1, at most 16384 at level 7."""
    import torch
    depth, cap, M0, n = 32, 1 << 21, 1 << 20, 1 << 16
    c, f = forms["default"], imt._ffi
    allv = oracle_lib.synth_values(M0 + n, 0x41504C20)
    base_vals, new_vals = allv[:M0], allv[M0:]
    a, b = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    try:
        pre = ints_to_arr(base_vals)
        ra, rb = a.apply_batch(pre), b.apply_batch(pre)
        assert ra == rb and a.size == b.size == M0 + 1
        nv = ints_to_arr(new_vals)
        root = a.apply_batch(nv)
        stats = a.apply_stats().tolist()
        rc = imt.lib.imt_itree_insert_batch(b.h, nv.ctypes.data_as(ctypes.c_void_p), n, None, 0)
        assert rc == 0, imt.lib.imt_last_error(c.h)
        assert root == a.root() == b.root() and a.size == b.size == M0 + n + 1
        # low leaves on the CPU: the nearest smaller value among the stored ones and the batch values inserted earlier
        order = sorted(range(M0), key=base_vals.__getitem__)
        skeys = [0] + [base_vals[i] for i in order]
        sleaf = [0] + [i + 1 for i in order]
        seen, seen_leaf, low = [], {}, []
        for i, v in enumerate(new_vals):
            p = bisect.bisect_left(skeys, v) - 1
            q = bisect.bisect_left(seen, v) - 1
            low.append(seen_leaf[seen[q]] if q >= 0 and seen[q] > skeys[p] else sleaf[p])
            bisect.insort(seen, v)
            seen_leaf[v] = M0 + 1 + i
        want = touched(low, M0 + 1, n, depth)
        print(f"large: hashes per level {stats}, {sum(stats) / n:.2f} per insertion (witness sweep: {2 + 2 * depth})")
        assert stats == want and sum(stats) == sum(want)
        assert stats[1] > 16384 >= stats[7], "both forms of k_apply_level must have run"
        rng = np.random.default_rng(0x41504C21)
        idx = np.unique(np.concatenate([rng.integers(0, M0 + n + 1, 4096).astype(np.uint64), np.array(low, np.uint64),
                                        np.arange(M0 + 1, M0 + n + 1, dtype=np.uint64)]))
        assert (a.get_proof_batch(idx) == b.get_proof_batch(idx)).all()
        assert (a.get_leaves(idx) == b.get_leaves(idx)).all()
    finally:
        a.close()
        b.close()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- arguments
def test_apply_arguments(imt, ctx):
    f = imt._ffi
    t = imt.IndexedTree(ctx, 8, 64)
    try:
        stats = (ctypes.c_uint64 * 9)()
        assert imt.lib.imt_itree_apply_stats(t.h, stats) == f.ERR["ARG"]           # no apply call yet
        v = ints_to_arr([5, 6])
        out = np.zeros(32, np.uint8)
        root0 = t.root()
        rc = imt.lib.imt_itree_apply_batch(t.h, v.ctypes.data_as(ctypes.c_void_p), 2, out.ctypes.data_as(ctypes.c_void_p),
                                           f.PIPELINE | f.DEVICE_PTRS)
        assert rc == f.ERR["ARG"] and t.size == 1 and t.root() == root0
        rc = imt.lib.imt_itree_apply_batch(t.h, None, 0, out.ctypes.data_as(ctypes.c_void_p), 0)   # n == 0: the current root
        assert rc == 0 and arr_ints(out)[0] == root0
        assert t.apply_batch([5, 6]) == t.root() != root0
        assert imt.lib.imt_itree_apply_batch(t.h, None, 0, None, 0) == 0
        with pytest.raises(ValueError):
            t.apply_batch([7, 5])                                                   # 5 is stored
        with pytest.raises(ValueError):
            t.apply_batch([7, 7])
        with pytest.raises(imt.ImtError) as ei:
            t.apply_batch([P])
        assert ei.value.code == f.ERR["NONCANONICAL"]
        assert t.size == 3
    finally:
        t.close()


# ---------------------------------------------------------------- the C example
def test_follow_chain_example(imt, oracle):
    """examples/follow_chain.c applies ten batches and prints each root; given the oracle's last root as its argument it
    compares and fails on a difference."""
    exe = os.path.join(ROOT, "examples", "follow_chain")
    csrc = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "follow_chain.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the example's values: item i of block j -> 1 + 7919023757 (64 j + i + 1) mod (2^61 - 1)
    depth, h = 32, oracle.sparse_new(32, 1024)
    roots = []
    for j in range(10):
        for i in range(64):
            assert oracle.sparse_insert(h, depth, 1 + 7919023757 * (64 * j + i + 1) % ((1 << 61) - 1))["rc"] == 0
        roots.append(oracle.sparse_root(h))
    oracle.sparse_free(h)
    r = subprocess.run([exe, f"{roots[-1]:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for j, want in enumerate(roots):
        assert f"block {j}: root {want:064x}" in r.stdout, r.stdout
    assert "final root equals the expected one" in r.stdout
    r = subprocess.run([exe, f"{roots[-2]:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "DIFFERS" in r.stdout
