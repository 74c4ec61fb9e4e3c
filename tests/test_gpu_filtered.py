"""GPU: imt_itree_insert_filtered and imt_itree_lookup_batch (include/imt.h).

The spec of insert_filtered is an identity: with A = the values whose status is NEW, in input order, the call is
insert_batch(A) -- the same tree, byte for byte the same witness rows.  Every test here checks that identity against a
twin tree fed the model's accepted values, the statuses and leaf indices against a plain sequential model (the
reference's insert_leaf loop with the rejected values skipped), and the witness rows against the sequential oracle."""
import ctypes
import random

import numpy as np
import pytest

import oracle_lib
from oracle_lib import P, ints_to_arr

NEW, ZERO, PRESENT, REPEATED, FOREIGN = 0, 1, 2, 3, 4
NONE = (1 << 64) - 1
KEYS = ("low_index", "is_largest", "low_leaf", "new_leaf", "old_root", "interim_root", "new_root", "low_sib", "new_sib",
        "new_index")


def ints(a):
    return [int.from_bytes(bytes(r), "little") for r in np.asarray(a, dtype=np.uint8).reshape(-1, 32)]


class Model:
    """The stored values of a tree (leaf order) and the reference's loop with the rejected values skipped."""

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
    """n values: fresh ones (popped from `fresh`), zeros, stored values and repeats of earlier ones in the batch"""
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


def same_rows(rf, rb, sib_rows=None):
    for k in KEYS:
        if k not in rb:
            continue
        a, b = rf[k], rb[k]
        if sib_rows is not None and k.endswith("_sib"):
            a, b = sib_rows(a), sib_rows(b)
        assert a.shape == b.shape and (a == b).all(), k


# ---------------------------------------------------------------- 1. the identity, both layouts, against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [3, 8, 32])
@pytest.mark.parametrize("item_major", [False, True])
def test_filtered_is_insert_batch_of_the_accepted_values(imt, ctx, oracle, depth, item_major):
    cap = min(512, 1 << depth)
    rng = random.Random(0x46494C00 + depth * 2 + item_major)
    fresh = oracle_lib.synth_values(cap, 0x46494C10 + depth)
    a, b = imt.IndexedTree(ctx, depth, cap), imt.IndexedTree(ctx, depth, cap)
    m = Model()
    oh = oracle.sparse_new(depth, cap)
    prev_root = a.root()
    sizes = [4, 9, 3, 1, 40, 120, 200] if depth > 3 else [4, 3, 5, 2, 6]
    for n in sizes:
        batch = mixed_batch(rng, m, fresh, n)
        status, leaf, acc = m.classify(batch)
        room = cap - len(m.vals)
        if len(acc) > room:                       # keep inside the capacity (the FULL case has a test of its own)
            break
        rf = a.insert_filtered(batch, item_major=item_major)
        assert rf["n_inserted"] == len(acc)
        assert rf["status"].tolist() == status and rf["leaf_index"].tolist() == leaf, batch
        if acc:
            rb = b.insert_batch(acc, item_major=item_major)
            same_rows(rf, rb)
            for i, v in enumerate(acc):           # the witness rows are the sequential oracle's
                o = oracle.sparse_insert(oh, depth, v)
                assert o["rc"] == 0
                assert int(rf["low_index"][i]) == o["low"] and int(rf["is_largest"][i]) == o["largest"]
                assert (rf["low_leaf"][i] == o["low_leaf"]).all()
                assert ints(rf["old_root"][i]) == [prev_root]
                assert ints(rf["interim_root"][i]) == [o["interim_root"]] and ints(rf["new_root"][i]) == [o["new_root"]]
                ls = rf["low_sib"][i] if item_major else rf["low_sib"][:, i]
                ns = rf["new_sib"][i] if item_major else rf["new_sib"][:, i]
                assert (ls == o["low_proof"]).all() and (ns == o["new_proof"]).all()
                prev_root = o["new_root"]
        else:
            assert all(rf[k].shape[0 if (item_major or not k.endswith("_sib")) else 1] == 0 for k in KEYS)
        m.commit(acc)
        assert a.root() == b.root() == prev_root == oracle.sparse_root(oh) and a.size == b.size == len(m.vals)
    assert (a.snapshot() == b.snapshot()).all()
    oracle.sparse_free(oh)


@pytest.mark.gpu
def test_level_major_rows_keep_the_callers_stride(imt, ctx):
    """Sibling rows of accepted value r sit at [level][r] of a [depth][n] array; rows [n_inserted, n) are not written."""
    depth, n = 8, 12
    t = imt.IndexedTree(ctx, depth, 64)
    t.insert_batch([100, 200])
    vals = [5, 100, 0, 7, 5, 300, 7, 200, 9, 0, 11, 9]
    res = {k: np.full(s, 0xAB, np.uint8) for k, s in (("low_sib", (depth, n, 32)), ("new_sib", (depth, n, 32)),
                                                       ("new_root", (n, 32)))}
    out = imt._ffi.InsertOut(**{k: a.ctypes.data for k, a in res.items()})
    status, leaf, k_ins = np.empty(n, np.uint8), np.empty(n, np.uint64), ctypes.c_uint64()
    v = imt.to_bytes(vals)
    rc = imt.lib.imt_itree_insert_filtered(t.h, v.ctypes.data_as(ctypes.c_void_p), n, status.ctypes.data_as(ctypes.c_void_p),
                                           leaf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(k_ins), ctypes.byref(out), 0)
    assert rc == 0, imt.lib.imt_last_error(ctx.h)
    acc = [5, 7, 300, 9, 11]
    assert k_ins.value == len(acc)
    assert status.tolist() == [NEW, PRESENT, ZERO, NEW, REPEATED, NEW, REPEATED, PRESENT, NEW, ZERO, NEW, REPEATED]
    assert leaf.tolist() == [3, 1, 0, 4, 3, 5, 4, 2, 6, 0, 7, 6]
    twin = imt.IndexedTree(ctx, depth, 64)
    twin.insert_batch([100, 200])
    want = twin.insert_batch(acc)
    m = len(acc)
    assert (res["low_sib"][:, :m] == want["low_sib"]).all() and (res["new_sib"][:, :m] == want["new_sib"]).all()
    assert (res["new_root"][:m] == want["new_root"]).all()
    assert (res["low_sib"][:, m:] == 0xAB).all() and (res["new_sib"][:, m:] == 0xAB).all()
    assert (res["new_root"][m:] == 0xAB).all()
    assert t.root() == twin.root()


# ---------------------------------------------------------------- 2. GPU classification against the host one
@pytest.mark.gpu
def test_gpu_filter_equals_host_filter(imt, ctx):
    rng = random.Random(0x46494C20)
    depth, cap = 32, 4096
    fresh = oracle_lib.synth_values(3000, 0x46494C21)
    a, b, m = imt.IndexedTree(ctx, depth, cap), imt.IndexedTree(ctx, depth, cap), imt.IndexedTree(ctx, depth, cap)
    model = Model()
    for k, n in enumerate([1, 2, 7, 64, 300, 33, 900, 5, 1000]):
        batch = mixed_batch(rng, model, fresh, n, p_zero=0.05, p_stored=0.2, p_repeat=0.2)
        ra = a.insert_filtered(batch, host_prep=True)
        rb = b.insert_filtered(batch)
        rm = m.insert_filtered(batch, host_prep=(k % 2 == 1), item_major=False)
        for key in KEYS + ("status", "leaf_index"):
            assert (ra[key] == rb[key]).all() and (ra[key] == rm[key]).all(), (key, k)
        assert ra["n_inserted"] == rb["n_inserted"] == rm["n_inserted"]
        model.commit(model.classify(batch)[2])
    assert a.root() == b.root() == m.root()
    assert (a.snapshot() == b.snapshot()).all() and (a.snapshot() == m.snapshot()).all()


# ---------------------------------------------------------------- 3. pipelined device-pointer batches
@pytest.mark.gpu
def test_pipelined_filtered_batches_see_the_batches_still_in_flight(imt, ctx):
    """Depth 32, 2^16 values per batch, about 10 % rejected, IMT_DEVICE_PTRS | IMT_PIPELINE on torch buffers, interleaved
    with plain insert_batch calls.  Every filtered batch repeats values of the batch right before it, which is still
    hashing when it is classified: those must come out PRESENT."""
    import torch
    depth, n = 32, 1 << 16
    dev = torch.device("cuda", 0)
    rng = random.Random(0x46494C30)
    c2 = imt.Context(0)
    c2.set_stream(torch.cuda.current_stream().cuda_stream)
    t = imt.IndexedTree(c2, depth, 1 << 19)
    model = Model()
    fresh = list({rng.randrange(1, P) for _ in range(7 * n)})
    rng.shuffle(fresh)
    flags = imt._ffi.DEVICE_PTRS | imt._ffi.PIPELINE
    plan, keep, prev = [], [], []
    for step in range(6):
        if step in (2, 4):                        # a plain batch in between
            batch = [fresh.pop() for _ in range(n // 2)]
            vt = torch.from_numpy(imt.to_bytes(batch)).to(dev)
            root = torch.empty((len(batch), 32), dtype=torch.uint8, device=dev)
            o = imt._ffi.InsertOut(new_root=root.data_ptr())
            rc = imt.lib.imt_itree_insert_batch(t.h, ctypes.c_void_p(vt.data_ptr()), len(batch), ctypes.byref(o), flags)
            assert rc == 0, imt.lib.imt_last_error(c2.h)
            keep += [vt, root, o]
            model.commit(batch)
            plan.append(("plain", batch, None))
            prev = batch
            continue
        batch = []
        for _ in range(n):
            r = rng.random()
            if r < 0.05 and prev:
                batch.append(rng.choice(prev))    # in flight
            elif r < 0.08:
                batch.append(batch[rng.randrange(len(batch))] if batch else 0)
            elif r < 0.09:
                batch.append(0)
            elif r < 0.10 and len(model.vals) > 1:
                batch.append(rng.choice(model.vals[1:]))
            else:
                batch.append(fresh.pop())
        status, leaf, acc = model.classify(batch)
        assert 0.07 < 1 - len(acc) / n < 0.13
        vt = torch.from_numpy(imt.to_bytes(batch)).to(dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        lf = torch.empty(n, dtype=torch.int64, device=dev)
        root = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        sib = torch.empty((depth, n, 32), dtype=torch.uint8, device=dev)
        o = imt._ffi.InsertOut(new_root=root.data_ptr(), new_sib=sib.data_ptr())
        k_ins = ctypes.c_uint64()
        rc = imt.lib.imt_itree_insert_filtered(t.h, ctypes.c_void_p(vt.data_ptr()), n, ctypes.c_void_p(st.data_ptr()),
                                               ctypes.c_void_p(lf.data_ptr()), ctypes.byref(k_ins), ctypes.byref(o), flags)
        assert rc == 0, imt.lib.imt_last_error(c2.h)
        assert k_ins.value == len(acc)
        keep += [vt, root, sib, o]
        plan.append(("filtered", acc, (st, lf, status, leaf)))
        model.commit(acc)
        prev = batch
    c2.sync()
    torch.cuda.synchronize()
    for kind, vals, chk in plan:
        if chk:
            st, lf, status, leaf = chk
            assert st.cpu().numpy().tolist() == status
            assert lf.cpu().numpy().astype(np.uint64).tolist() == leaf
    ref = imt.IndexedTree(ctx, depth, 1 << 19)
    for kind, vals, _ in plan:
        ref.insert_batch(vals, proofs=False)
    assert t.size == ref.size == len(model.vals)
    assert t.root() == ref.root()
    assert (t.snapshot() == ref.snapshot()).all()
    t.close(); ref.close(); c2.close()


# ---------------------------------------------------------------- 4. edge cases
@pytest.mark.gpu
@pytest.mark.parametrize("host_prep", [False, True])
def test_nothing_accepted_capacity_and_noncanonical(imt, ctx, host_prep):
    t = imt.IndexedTree(ctx, 16, 16)
    t.insert_batch(list(range(1, 11)))            # size 11: room for 5
    root, size = t.root(), t.size
    r = t.insert_filtered([0, 3, 3, 0, 10], host_prep=host_prep)
    assert r["n_inserted"] == 0 and r["status"].tolist() == [ZERO, PRESENT, PRESENT, ZERO, PRESENT]
    assert r["leaf_index"].tolist() == [0, 3, 3, 0, 10] and r["new_root"].shape == (0, 32)
    assert t.root() == root and t.size == size
    # 16 values, 5 of them new: size + n > capacity, size + n_inserted == capacity
    batch = [20, 1, 21, 20, 0, 22, 5, 23, 23, 7, 24, 2, 0, 21, 9, 10]
    r = t.insert_filtered(batch, host_prep=host_prep)
    assert r["n_inserted"] == 5 and t.size == 16
    twin = imt.IndexedTree(ctx, 16, 16)
    twin.insert_batch(list(range(1, 11)))
    same_rows(r, twin.insert_batch([20, 21, 22, 23, 24]))
    assert t.root() == twin.root()
    root = t.root()
    with pytest.raises(imt.ImtError) as ei:        # one accepted value past full
        t.insert_filtered([1, 25, 2], host_prep=host_prep)
    assert ei.value.code == imt._ffi.ERR["FULL"]
    assert t.root() == root and t.size == 16
    r = t.insert_filtered([1, 24, 0], host_prep=host_prep)     # a full tree still classifies
    assert r["n_inserted"] == 0 and r["status"].tolist() == [PRESENT, PRESENT, ZERO]
    t2 = imt.IndexedTree(ctx, 16, 64)
    t2.insert_batch([4, 8])
    root, size = t2.root(), t2.size
    with pytest.raises(imt.ImtError) as ei:
        t2.insert_filtered([5, P + 1, 4], host_prep=host_prep)
    assert ei.value.code == imt._ffi.ERR["NONCANONICAL"]
    assert t2.root() == root and t2.size == size
    assert t2.insert_filtered([5, 6, 4], host_prep=host_prep)["n_inserted"] == 2    # and it works afterwards


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,R", [(1, 1 << 256), (2, 1 << 261)])
@pytest.mark.parametrize("host_prep", [False, True])
def test_montgomery_and_device_format_inputs(imt, ctx, fmt, R, host_prep):
    rng = random.Random(0x46494C40 + fmt)
    depth = 32
    fresh = oracle_lib.synth_values(400, 0x46494C41 + fmt)
    model = Model()
    a, b = imt.IndexedTree(ctx, depth, 1024), imt.IndexedTree(ctx, depth, 1024)
    for n in (50, 200, 120):
        batch = mixed_batch(rng, model, fresh, n)
        status, leaf, acc = model.classify(batch)
        v = ints_to_arr([x * R % P for x in batch])
        res = dict(new_root=np.empty((n, 32), np.uint8), low_leaf=np.empty((n, 3, 32), np.uint8),
                   low_sib=np.empty((depth, n, 32), np.uint8))
        out = imt._ffi.InsertOut(**{k: x.ctypes.data for k, x in res.items()})
        st, lf, k_ins = np.empty(n, np.uint8), np.empty(n, np.uint64), ctypes.c_uint64()
        rc = imt.lib.imt_itree_insert_filtered(a.h, v.ctypes.data_as(ctypes.c_void_p), n, st.ctypes.data_as(ctypes.c_void_p),
                                               lf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(k_ins), ctypes.byref(out),
                                               fmt | (imt._ffi.HOST_PREP if host_prep else 0))
        assert rc == 0, imt.lib.imt_last_error(ctx.h)
        assert st.tolist() == status and lf.tolist() == leaf and k_ins.value == len(acc)
        want = b.insert_batch(acc)
        m = len(acc)
        assert ints(res["new_root"][:m]) == [x * R % P for x in ints(want["new_root"])]
        assert ints(res["low_leaf"][:m]) == [x * R % P for x in ints(want["low_leaf"])]
        assert ints(res["low_sib"][:, :m]) == [x * R % P for x in ints(want["low_sib"])]
        model.commit(acc)
    assert a.root() == b.root()


# ---------------------------------------------------------------- 5. placed and partitioned tree
@pytest.mark.gpu
@pytest.mark.parametrize("item_major", [False, True])
def test_placed_and_partitioned_tree(imt, ctx, item_major):
    depth, gd, sub, world = 10, 13, 5, 8
    base = sub << depth
    rng = random.Random(0x46494C50 + item_major)
    trees = []
    for _ in range(2):
        t = imt.IndexedTree(ctx, depth, 512)
        t.set_placement(gd, sub)
        ctx._check(imt.lib.imt_itree_set_value_partition(t.h, world, sub))
        trees.append(t)
    a, b = trees
    model = Model(base, world, sub)
    mine = [v for v in oracle_lib.synth_values(3000, 0x46494C51) if v % world == sub][:300]
    for n in (20, 90, 150):
        batch = []
        for _ in range(n):
            r = rng.random()
            if r < 0.2:
                batch.append(rng.randrange(1, P) * world % P)       # mostly another residue
            elif r < 0.3 and batch:
                batch.append(rng.choice(batch))
            elif r < 0.4 and len(model.vals) > 1:
                batch.append(rng.choice(model.vals[1:]))
            elif r < 0.45:
                batch.append(0)
            else:
                batch.append(mine.pop())
        status, leaf, acc = model.classify(batch)
        assert FOREIGN in status
        rf = a.insert_filtered(batch, item_major=item_major)
        assert rf["status"].tolist() == status and rf["leaf_index"].tolist() == leaf
        rb = b.insert_batch(acc, item_major=item_major)
        # a placed tree writes sibling rows [0, depth) of arrays dimensioned for global_depth
        same_rows(rf, rb, sib_rows=(lambda x: x[:, :depth]) if item_major else (lambda x: x[:depth]))
        assert rf["new_index"].tolist() == [base + len(model.vals) + i for i in range(len(acc))]
        model.commit(acc)
    assert a.root() == b.root() and (a.snapshot() == b.snapshot()).all()
    st, lf = a.lookup([0, model.vals[3], rng.randrange(1, P) * world % P or 1])
    assert st.tolist()[:2] == [ZERO, PRESENT] and lf.tolist()[:2] == [base, base + 3]


# ---------------------------------------------------------------- 6. lookup
@pytest.mark.gpu
def test_lookup_2pow20_against_the_model(imt, ctx):
    import torch
    depth, N = 32, 1 << 20
    rng = random.Random(0x46494C60)
    vals = list({rng.randrange(1, P) for _ in range(N + 4096)})[:N]
    t = imt.IndexedTree(ctx, depth, 1 << 21)
    for s in range(0, N, 1 << 16):
        t.insert_batch(vals[s:s + (1 << 16)], proofs=False)
    leaf_of = {v: i + 1 for i, v in enumerate(vals)}
    stored_pick = rng.sample(vals, N // 2)
    absent = []
    while len(absent) < N // 2 - 2:
        x = rng.randrange(1, P)
        if x not in leaf_of:
            absent.append(x)
    cand = stored_pick + absent + [0, 0]
    rng.shuffle(cand)
    cb = imt.to_bytes(cand)
    st, lf = t.lookup(cb)
    want_st = np.array([ZERO if v == 0 else PRESENT if v in leaf_of else NEW for v in cand], np.uint8)
    assert (st == want_st).all()
    pres = np.nonzero(st == PRESENT)[0]
    new = np.nonzero(st == NEW)[0]
    assert (lf[pres] == np.array([leaf_of[cand[i]] for i in pres], np.uint64)).all()
    assert (lf[st == ZERO] == 0).all()
    assert (lf[new] == t.find_low(cb[new])).all()
    # PRESENT indices round-trip through get_leaves, and their proofs verify against the root
    got = t.get_leaves(lf[pres])
    assert (got[:, 0] == cb[pres]).all()
    sub = pres[:4096]
    pre = t.get_leaves(lf[sub])
    sib = t.get_proof_batch(lf[sub])
    root = np.tile(imt.to_bytes(t.root()), (sub.size, 1))
    assert ctx.verify_proof_batch(ctx.hash3(pre), lf[sub], root, sib, depth).all()
    # device pointers
    dev = torch.device("cuda", 0)
    vt = torch.from_numpy(cb).to(dev)
    st_d = torch.empty(len(cand), dtype=torch.uint8, device=dev)
    lf_d = torch.empty(len(cand), dtype=torch.int64, device=dev)
    rc = imt.lib.imt_itree_lookup_batch(t.h, ctypes.c_void_p(vt.data_ptr()), len(cand), ctypes.c_void_p(st_d.data_ptr()),
                                        ctypes.c_void_p(lf_d.data_ptr()), imt._ffi.DEVICE_PTRS)
    assert rc == 0, imt.lib.imt_last_error(ctx.h)
    torch.cuda.synchronize()
    assert (st_d.cpu().numpy() == st).all() and (lf_d.cpu().numpy().astype(np.uint64) == lf).all()
    with pytest.raises(imt.ImtError) as ei:
        t.lookup([5, P])
    assert ei.value.code == imt._ffi.ERR["NONCANONICAL"]
    t.close()
