"""GPU (MI355X): views and replays watching an indexed tree under mixed sequences of its writers.

A view (imt_itree_view_*) is a cache keyed by (size, the tree's count of content-changing calls), and a replay
(imt_itree_view_insert_witness) reads the values and the index where the writers left them.  Every writer has to bump
that count, nothing else may, and a build has to read the copy of the list the last writer left current -- a mistake in
either raises no error, it serves wrong proofs against a finalized root.  test_gpu_view.py and test_gpu_replay.py grow
their trees with apply and witness batches; this file plays the committed scripts of tests/tree_model.py (the twelve ways
into the tree in every adjacent order, refused calls between them; a mixed batch with an INSERT makes every view stale,
one of READs only and a refused one make none stale) exactly as test_gpu_tree_sequences.Player plays them,
the tree's own checks included, with views alive beside the tree (tree_model.view_schedule; tests/test_tree_model.py
asserts what that schedule covers).  Expected answers are the plain-Python model's and the CPU oracle's for the prefix
vals[:size] of whatever the model then holds; every comparison is bit-exact.

  after every step, every live view, in one round (raw calls; device and host pointers take turns between rounds)
      root, get_leaves and get_proof_batch (item-major) of every slot
      lookup of probes, kept values, values stored after the cut (NEW, the low leaf a kept one), 0, foreign residues
      non_membership_witness of the prefix's probes, the witness accepted by imt_non_membership_batch against the view's
      root, a stored value and 0 refused
      insert_witness of the next min(size of the tree - size of the view, 16) insertions: all nine fields and new_index;
      sibling rows [depth, global_depth) keep the caller's pattern; one insertion more than the tree holds is refused;
      where the replayed range holds a whole mixed batch that has just run, its rows there are that batch's INSERT rows;
      where it is exactly one insert_bulk batch that has just run, imt_itree_view_bulk_witness of it equals that step's
      rows; where it is exactly one mixed_filtered / mixed_pipelined block, imt_itree_view_mixed_witness of the operations
      carried out equals that step's INSERT and READ rows
      behind a step with no check (third pass) there is no round and no view is made: the next step follows at once
      stats: the hashes per level by imt_itree_rewind's definition, and one rebuild exactly where tree_model.view_rounds
      says: the first answered round, and every answered round behind a step that changed the contents
      while the tree is smaller than the view: every query IMT_ERR_RANGE, no rebuild
  On the thread and quad forms of the hash kernels a round costs several times what it costs on the default context (every
  launch of a build and a replay is a latency-bound kernel of a few events), so there the views are queried after every
  second step; the default context, which plays every script, keeps every round.
  test_view_across_batch_end     imt_itree_batch_begin .. _end with views alive
  test_views_across_sliced_steps imt_sliced_step with views made before the steps

Every failure message names the script, the step, the step's writer kind and the view's size.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib
import test_gpu_bulk as tgb
import test_gpu_replay as trp
import test_gpu_rewind as tr
import tree_model as tmod
from oracle_lib import arr_ints, ints_to_arr
from test_gpu_tree_sequences import FOREIGN_PROBES, KIND_NAMES, N_PROBES, SCRIPTS, Player, _cases
from test_gpu_tree_sequences import forms  # noqa: F401  (the fixture: one context per hash form, on torch's stream)

pytestmark = pytest.mark.gpu

FILL = trp.FILL


class Bufs:
    """The arrays of the raw calls of one round: numpy for host pointers, torch tensors on the GPU for IMT_DEVICE_PTRS.
    It keeps every array it hands out alive, so a pointer taken from one stays good for the call it is passed to."""

    def __init__(self, imt, c, device):
        import torch
        self.imt, self.c, self.device, self.torch = imt, c, device, torch
        self.flags = imt._ffi.DEVICE_PTRS if device else 0
        self.keep = []

    def inp(self, arr):
        a = np.ascontiguousarray(arr)
        if self.device:
            a = self.torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
        self.keep.append(a)
        return a

    def out(self, shape, dtype=np.uint8, fill=0):
        if self.device:
            a = self.torch.full(shape, fill, dtype=self.torch.int64 if dtype == np.uint64 else self.torch.uint8, device="cuda")
        else:
            a = np.full(shape, fill, dtype)
        self.keep.append(a)
        return a

    def p(self, x):
        return ctypes.c_void_p(x.data_ptr() if self.device else x.ctypes.data)

    def get(self, x):
        if not self.device:
            return x
        self.c.sync()
        self.torch.cuda.synchronize()
        a = x.cpu().numpy()
        return a.view(np.uint64) if a.dtype == np.int64 else a


def raw_replay(imt, B, v, n, G):
    """imt_itree_view_insert_witness, level-major, into arrays filled with FILL: (rc, the nine arrays as numpy)"""
    bufs = {k: B.out(a.shape, fill=FILL) for k, a in trp.buffers(n, G, False).items()}
    out = imt._ffi.InsertOut(**{k: B.p(a).value for k, a in bufs.items()})
    rc = imt.lib.imt_itree_view_insert_witness(v.h, n, ctypes.byref(out), B.flags)
    return rc, {k: B.get(a) for k, a in bufs.items()}


def check_view(imt, c, v, sh, vals, device, tag):
    """Every query of view `v` of a tree that holds `vals` (the model's list, sentinel first), device or host pointers.
    Returns the hashes per level its cache must have cost."""
    f, lib = imt._ffi, imt.lib
    s, M, cap, depth, base = v.size, len(vals), sh.cap, sh.depth, tmod.index_base(sh)
    G = depth if not sh.placement else sh.placement[0]
    B = Bufs(imt, c, device)
    ok = lambda rc, what: _ok(imt, c, rc, f"{tag}: {what}")
    if M < s:
        # the tree is smaller than the view: nothing to answer from
        one, idx1 = B.inp(ints_to_arr([5 if sh.partition[0] == 0 else 4])), B.inp(np.array([base], np.uint64))
        big = B.out((depth, 1, 32))
        st, lf = B.out((1, )), B.out((1, ), np.uint64)
        want = f.ERR["RANGE"]
        assert lib.imt_itree_view_root(v.h, B.p(big), B.flags) == want, f"{tag}: root of a tree smaller than the view"
        assert lib.imt_itree_view_get_leaves(v.h, B.p(idx1), 1, B.p(big), B.flags) == want, f"{tag}: get_leaves"
        assert lib.imt_itree_view_get_proof_batch(v.h, B.p(idx1), 1, B.p(big), B.flags) == want, f"{tag}: get_proof_batch"
        assert lib.imt_itree_view_lookup_batch(v.h, B.p(one), 1, B.p(st), B.p(lf), B.flags) == want, f"{tag}: lookup"
        assert lib.imt_itree_view_non_membership_witness(v.h, B.p(one), 1, B.p(lf), B.p(B.out((1, 3, 32))), B.p(st), B.p(big),
                                                         B.flags) == want, f"{tag}: non_membership_witness"
        rc, bufs = raw_replay(imt, B, v, 1, G)
        assert rc == want and all((x == FILL).all() for x in bufs.values()), f"{tag}: a replay of one insertion: {rc}"
        out = f.InsertOut()
        assert lib.imt_itree_view_insert_witness(v.h, 0, ctypes.byref(out), B.flags) == want, f"{tag}: a replay of nothing"
        return None
    prefix = tuple(vals[:s])
    pm = tmod.new_model(sh, prefix)
    want_root, proofs = tmod.oracle_root(sh, prefix), tmod.oracle_proofs(sh, prefix)
    want_pre = tmod.pre_arr(pm.preimages(range(cap)))
    idx = np.arange(cap, dtype=np.uint64) + np.uint64(base)
    d_idx = B.inp(idx)
    # root, preimages and proofs of every slot
    root = B.out((32, ))
    ok(lib.imt_itree_view_root(v.h, B.p(root), B.flags), "root")
    got_root = arr_ints(B.get(root).reshape(1, 32))[0]
    assert got_root == want_root, f"{tag}: root {got_root:#x}, the oracle's tree of {s} leaves has {want_root:#x}"
    pre = B.out((cap, 3, 32))
    ok(lib.imt_itree_view_get_leaves(v.h, B.p(d_idx), cap, B.p(pre), B.flags), "get_leaves")
    bad = np.nonzero((B.get(pre) != want_pre).reshape(cap, -1).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: get_leaves: preimage of leaf {bad[:1]} is {arr_ints(B.get(pre)[bad[:1]])}"
    sib = B.out((cap, depth, 32))
    ok(lib.imt_itree_view_get_proof_batch(v.h, B.p(d_idx), cap, B.p(sib), B.flags | f.SIB_ITEM_MAJOR), "get_proof_batch")
    bad = np.argwhere((B.get(sib) != proofs).any(axis=2))
    assert bad.size == 0, f"{tag}: get_proof_batch: leaf {bad[:1, 0]} level {bad[:1, 1]}"
    # lookup: probes, kept values, values stored after the cut, 0, another subtree's values
    probes = pm.probes()[:N_PROBES]
    later = list(dict.fromkeys(list(vals[s:s + 3]) + list(vals[s:][-2:])))
    foreign = [x for x in FOREIGN_PROBES if not pm.mine(x)]
    mix = probes[:8] + list(prefix[1:4]) + list(prefix[-3:]) + later + [0] + foreign
    st, lf = B.out((len(mix), )), B.out((len(mix), ), np.uint64)
    ok(lib.imt_itree_view_lookup_batch(v.h, B.p(B.inp(ints_to_arr(mix))), len(mix), B.p(st), B.p(lf), B.flags), "lookup")
    got = list(zip(B.get(st).tolist(), B.get(lf).tolist()))
    assert got == [pm.lookup(x) for x in mix], f"{tag}: lookup"
    a = len(probes[:8]) + len(prefix[1:4]) + len(prefix[-3:])
    assert all(g[0] == f.VAL_NEW and g[1] - base < s for g in got[a:a + len(later)]), \
        f"{tag}: a value stored after the cut is NEW, its low leaf a kept one"
    # the non-membership witness of the prefix's probes: all four outputs, and the checker accepts them
    n = len(probes)
    pv = ints_to_arr(probes)
    want = [pm.nm_witness(x) for x in probes]
    low, leaves = B.out((n, ), np.uint64), B.out((n, 3, 32))
    largest, nsib = B.out((n, )), B.out((depth, n, 32))
    ok(lib.imt_itree_view_non_membership_witness(v.h, B.p(B.inp(pv)), n, B.p(low), B.p(leaves), B.p(largest), B.p(nsib),
                                                 B.flags), "non_membership_witness")
    low, leaves, largest, nsib = (np.ascontiguousarray(B.get(x)) for x in (low, leaves, largest, nsib))
    assert low.tolist() == [w[0] for w in want], f"{tag}: non_membership_witness: low index"
    assert (leaves == tmod.pre_arr([w[1] for w in want])).all(), f"{tag}: non_membership_witness: low leaf"
    assert largest.tolist() == [w[2] for w in want], f"{tag}: non_membership_witness: is_largest"
    assert (nsib == proofs[[w[0] - base for w in want]].transpose(1, 0, 2)).all(), f"{tag}: non_membership_witness: siblings"
    fail = c.non_membership(imt.to_bytes(got_root), leaves, low, nsib, depth, pv, largest)
    assert not fail.any(), f"{tag}: imt_non_membership_batch rejects the view's witness: {fail.tolist()}"
    for x in [0] + ([prefix[-1]] if s > 1 else []):
        bad_vals = B.inp(ints_to_arr(probes[:2] + [x]))
        rc = lib.imt_itree_view_non_membership_witness(v.h, B.p(bad_vals), 3, B.p(B.out((3, ), np.uint64)),
                                                       B.p(B.out((3, 3, 32))), B.p(B.out((3, ))), B.p(B.out((depth, 3, 32))),
                                                       B.flags)
        assert rc == f.ERR["VALUE"], f"{tag}: non_membership_witness of {x:#x}: {rc}"
    # the replay of the insertions that follow the view's size
    n = min(M - s, tmod.REPLAY_MAX)
    if n:
        rows = tmod.oracle_rows(sh, prefix, tuple(vals[s:s + n]))
        rc, bufs = raw_replay(imt, B, v, n, G)
        ok(rc, f"insert_witness({n})")
        bufs["low_index"] = np.ascontiguousarray(bufs["low_index"]).view(np.uint64).reshape(n)
        tr.compare_rows(bufs, rows, 0, n, depth, f"{tag}: insert_witness({n})")
        for k in ("low_sib", "new_sib"):
            assert (bufs[k][depth:] == FILL).all(), f"{tag}: insert_witness({n}): {k} rows from {depth} up belong to the caller"
        if not device:                                            # the Python method: insert_batch's dict, with new_index
            res = v.insert_witness(n)
            tr.compare_rows(res, rows, 0, n, depth, f"{tag}: IndexedTreeView.insert_witness({n})")
            new_index = np.arange(s, s + n, dtype=np.uint64) + np.uint64(base)
            assert (res["new_index"] == new_index).all(), f"{tag}: insert_witness({n}): new_index"
    rc, bufs = raw_replay(imt, B, v, M - s + 1, G)
    assert rc == f.ERR["RANGE"] and all((x == FILL).all() for x in bufs.values()), \
        f"{tag}: a replay one past the head returned {rc}"
    now = dict(preimages=tmod.pre_arr(tmod.new_model(sh, vals).preimages(range(cap))))
    return tr.rewind_counts(now, dict(preimages=want_pre), list(range(cap)), M, s, depth)


def _ok(imt, c, rc, what):
    assert rc == 0, f"{what}: refused with {rc}: {imt.lib.imt_last_error(c.h)}"


class ViewPlayer(Player):
    """Player, with the views of tree_model.view_schedule alive beside the tree"""

    def __init__(self, imt, c, script, every=1):
        super().__init__(imt, c, script)
        self.schedule, self.rounds = tmod.view_schedule(script), tmod.view_rounds(script, every)
        self.every, self.n_rounds = every, 0
        self.views = {}                                           # size -> [view, rebuilds expected so far]
        self.n_whole_mixed = 0                                    # replays compared with a mixed batch's own INSERT rows
        self.n_whole_bulk = self.n_whole_block = 0                # and with a bulk batch's / a witness block's own rows
        self.open(1)

    def open(self, s):
        self.views[s] = [self.t.view(s), 0]
        assert self.views[s][0].stats()[1] == 0, f"{self.script.name}: a new view at {s} has built nothing"

    def close(self):
        for v, _ in self.views.values():                          # views before the tree
            v.close()
        super().close()

    def step(self, i, st):
        super().step(i, st)
        closed, created = self.schedule[i]
        for s in closed:
            self.views.pop(s)[0].close()
        for s in created:
            self.open(s)
        if i % self.every or st.check == tmod.NO_CHECK:             # NO_CHECK: nothing is called before the next step
            assert not self.rounds[i] and (st.check != tmod.NO_CHECK or not (closed or created))
            return
        device = bool(self.n_rounds & 1)
        self.n_rounds += 1
        assert [r.size for r in self.rounds[i]] == list(self.views)
        for r in self.rounds[i]:
            ent = self.views[r.size]
            what = f"refused {st.refusal}: {KIND_NAMES[st.kind]}" if st.refusal else KIND_NAMES[st.kind]
            tag = (f"{self.script.name} step {i} kind {tmod.writer_kind(st)} ({what}), view at {r.size} of {self.m.size} "
                   f"({r.state}), {'device' if device else 'host'} pointers, content changed by kinds {list(r.since)} since it "
                   f"last answered")
            try:
                hashes = check_view(self.imt, self.c, ent[0], self.shape, self.m.vals, device, tag)
            except AssertionError as e:                           # a wrong answer: say whether the view had rebuilt for it
                raise AssertionError(f"{e}\n{tag}: {ent[0].stats()[1]} rebuilds so far, {ent[1] + r.build} expected") from None
            assert (hashes is None) == (r.state == tmod.SMALLER), tag
            ent[1] += r.build
            got_hashes, builds = ent[0].stats()
            assert builds == ent[1], f"{tag}: {builds} rebuilds so far, {ent[1]} expected ({'one' if r.build else 'none'} in this round)"
            if hashes is not None:
                assert got_hashes.tolist() == hashes, f"{tag}: hashes per level {got_hashes.tolist()}, by the definition {hashes}"
            if st.kind == tmod.MIXED and not st.refusal and r.size <= self.last_mixed[0] and r.size + r.n_replay >= self.m.size:
                # the replay reaches across the whole mixed batch: its rows there are the batch's own INSERT rows
                M0, ins = self.last_mixed
                res = ent[0].insert_witness(r.n_replay)
                a, b = M0 - r.size, self.m.size - r.size
                for k in trp.FIELDS + ("new_index", ):
                    got = res[k][:, a:b] if k.endswith("_sib") else res[k][a:b]
                    assert got.shape == ins[k].shape and (got == ins[k]).all(), f"{tag}: the replay of the mixed batch's INSERTs: {k}"
                self.n_whole_mixed += 1
            n_new = self.m.size - r.size
            if st.kind == tmod.BULK and not st.refusal and self.last_bulk[3] is st and r.size == self.last_bulk[0]:
                # the replayed range is exactly the bulk batch that has just run: its bulk witness is that step's rows
                _, rows, im, _ = self.last_bulk
                res = ent[0].bulk_witness(n_new, item_major=im)
                for k in tgb.FIELDS:
                    assert res[k].shape == rows[k].shape and (res[k] == rows[k]).all(), f"{tag}: the bulk witness of the batch: {k}"
                self.n_whole_bulk += 1
            blk = self.last_block
            if st.kind in (tmod.MIXED_FILT, tmod.MIXED_PIPE) and not st.refusal and blk is not None and blk[4] is st and \
                    r.size == blk[0] and n_new == len(blk[3]["acc"]) > 0:
                # exactly one witness block: the replay of the operations it carried out gives its INSERT and READ rows
                _, ins, rd, out, _ = blk
                carried = out["carried"]
                res = ent[0].mixed_witness(ints_to_arr([st.vals[p] for p in carried]), [st.arg["ops"][p] for p in carried],
                                           members=st.arg["members"])
                for got, want, what in ((res[0], ins, "INSERT"), (res[1], rd, "READ")):
                    for k, a in want.items():
                        assert got[k].shape == a.shape and (got[k] == a).all(), f"{tag}: the replay of the block's {what} rows: {k}"
                self.n_whole_block += 1


@pytest.mark.parametrize("name,form", _cases())
def test_view_sequence(imt, forms, name, form):
    script = SCRIPTS[name]
    p = ViewPlayer(imt, forms[form], script, 1 if form == "default" else tmod.VIEW_ROUNDS_OTHER_FORMS)
    try:
        for i, st in enumerate(script.steps):
            p.step(i, st)
        assert not p.in_flight and not p.piped
        # the comparisons with a step's own rows ran wherever the model says a view's replayed range was that step
        played = list(zip(tmod.trace(script), p.rounds))
        exact = [st for (st, before, after, res), rnd in played for r in rnd
                 if not st.refusal and r.prefix is not None and r.size == len(before) < len(after)]
        assert p.n_whole_bulk == sum(st.kind == tmod.BULK for st in exact), name
        assert p.n_whole_block == sum(st.kind == tmod.MIXED_FILT or (st.kind == tmod.MIXED_PIPE and not st.arg["apply"]) for st in exact), name
        assert p.n_whole_mixed == sum(1 for (st, before, after, res), rnd in played for r in rnd
                                      if st.kind == tmod.MIXED and not st.refusal and r.size <= len(before) and
                                      r.size + r.n_replay >= len(after)), name
    finally:
        p.close()


# ---------------------------------------------------------------- two writers the scripts do not have
SMALL = tmod.Shape("d32_small", 32, 256, None, (0, 0))


def answers(imt, c, v, vals, builds, tag):
    """host-pointer queries of a view of a tree of shape SMALL that holds [0] + vals, and its count of rebuilds"""
    check_view(imt, c, v, SMALL, [0] + list(vals), False, tag)
    assert v.stats()[1] == builds, f"{tag}: {v.stats()[1]} rebuilds, {builds} expected"


def test_view_across_batch_end(imt, forms):
    """One sharded single-list batch (imt_itree_batch_begin .. _end) driven by one process in two slot ranges, with views
    alive at size 1 and at the head: refused between begin and end, each rebuilt once afterwards, and the head view's
    replay of the batch is what imt_itree_insert_batch writes on a twin."""
    import torch
    c, f, lib = forms["default"], imt._ffi, imt.lib
    depth, cap, n0, n, parts = SMALL.depth, SMALL.cap, 37, 16, 2
    vals = oracle_lib.synth_values(n0 + n, 0x56535142)
    t, twin = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    P_ = lambda x: ctypes.c_void_p(x.data_ptr())
    try:
        t.apply_batch(ints_to_arr(vals[:n0]))
        twin.apply_batch(ints_to_arr(vals[:n0]))
        one, head = t.view(1), t.view(n0 + 1)
        answers(imt, c, one, vals[:n0], 1, "the view at 1 before the batch")
        answers(imt, c, head, vals[:n0], 1, "the view at the head before the batch")
        chunk = torch.from_numpy(ints_to_arr(vals[n0:])).cuda()
        ev, l0 = ctypes.c_uint32(), ctypes.c_uint32()
        assert lib.imt_itree_batch_begin(t.h, P_(chunk), n, f.DEVICE_PTRS, ctypes.byref(ev), ctypes.byref(l0)) == 0, \
            lib.imt_last_error(c.h)
        E, L0 = ev.value, l0.value
        out = np.zeros((depth, 1, 32), np.uint8)
        zero = np.zeros(1, np.uint64)
        po, pi = out.ctypes.data_as(ctypes.c_void_p), zero.ctypes.data_as(ctypes.c_void_p)
        val = torch.empty((L0 + 1, E, 32), dtype=torch.uint8, device="cuda")
        kc = E // parts

        def refused(where):
            for v in (one, head):
                assert lib.imt_itree_view_root(v.h, po, 0) == f.ERR["ARG"], where
                assert lib.imt_itree_view_get_proof_batch(v.h, pi, 1, po, 0) == f.ERR["ARG"], where
                rc, bufs = trp.replay(imt, v, 1, depth)
                assert rc == f.ERR["ARG"] and all((x == FILL).all() for x in bufs.values()), where
                assert v.stats()[1] == 1, where

        refused("after imt_itree_batch_begin")
        for q in range(parts):
            assert lib.imt_itree_batch_leaves(t.h, P_(val[0]), q * kc, kc) == 0
        for l in range(L0):
            for q in range(parts):
                assert lib.imt_itree_batch_level(t.h, l, P_(val[l]), P_(val[l + 1]), q * kc, kc) == 0
        refused("after the levels")
        roots = torch.empty((E, 32), dtype=torch.uint8, device="cuda")
        tops = [torch.zeros((depth - L0 + 1, 32), dtype=torch.uint8, device="cuda") for _ in range(parts)]
        for q in range(parts):
            assert lib.imt_itree_batch_top(t.h, P_(val[L0]), q * kc, kc, P_(roots), P_(tops[q])) == 0
        ptrs = (ctypes.c_void_p * (L0 + 1))(*[val[l].data_ptr() for l in range(L0 + 1)])
        refused("before imt_itree_batch_end")
        assert lib.imt_itree_batch_end(t.h, ptrs, P_(tops[parts - 1])) == 0, lib.imt_last_error(c.h)
        c.sync()
        want = twin.insert_batch(ints_to_arr(vals[n0:]))
        assert t.size == n0 + n + 1 and t.root() == twin.root()
        answers(imt, c, one, vals, 2, "the view at 1 after imt_itree_batch_end")
        answers(imt, c, head, vals, 2, "the view at the former head after imt_itree_batch_end")
        rc, bufs = trp.replay(imt, head, n, depth)
        assert rc == 0, lib.imt_last_error(c.h)
        want["low_index"] = want["low_index"].view(np.uint8).reshape(n, 8)
        for k in trp.FIELDS:
            assert (bufs[k] == want[k]).all(), f"the replay of the sharded batch: {k}"
        assert one.stats()[1] == head.stats()[1] == 2 and t.root() == twin.root()
    finally:
        t.close()
        twin.close()


def test_views_across_sliced_steps(imt, ctx):
    """World 2 over the local transport.  On every replica a view at size 1 and one at the size after a first flushed step
    exist before two more steps and a flush: each then answers the oracle's prefix after one rebuild, and the replay from
    the second reaches through the last step's values with the oracle's rows."""
    import torch
    import test_gpu_sliced as ts
    sl = ts.load_sliced()
    depth, cap, world, batch = SMALL.depth, SMALL.cap, 2, 24
    step = world * batch
    vals = oracle_lib.synth_values(3 * step, 0x56535153)
    w = sl.SlicedTree(imt, 0, depth, cap, batch, world, n_local=world, nbuf=8)
    try:
        arr = torch.from_numpy(ints_to_arr(vals)).cuda()
        w.step(arr[:step])
        w.flush()
        views = [(t.view(1), t.view(step + 1)) for t in w.trees]
        for r in (1, 2):
            w.step(arr[r * step:(r + 1) * step])
        w.flush()
        assert [t.size for t in w.trees] == [3 * step + 1] * world
        rows = tmod.oracle_rows(SMALL, tuple([0] + vals[:step]), tuple(vals[step:]))
        for k, (t, (one, mid)) in enumerate(zip(w.trees, views)):
            assert t.root() == tmod.oracle_root(SMALL, tuple([0] + vals)), f"replica {k}: the head"
            answers(imt, t.ctx, one, vals, 1, f"replica {k}: the view at 1 after two sliced steps")
            answers(imt, t.ctx, mid, vals, 1, f"replica {k}: the view at {step + 1} after two sliced steps")
            res = mid.insert_witness(2 * step)                    # both steps; rows [step, 2 * step) are the last step's
            tr.compare_rows(res, rows, 0, 2 * step, depth, f"replica {k}: the replay of the sliced steps")
            assert mid.stats()[1] == 1 and t.root() == tmod.oracle_root(SMALL, tuple([0] + vals))
            one.close()
            mid.close()
    finally:
        w.close()
