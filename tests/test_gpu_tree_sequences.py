"""GPU (MI355X): an indexed tree under mixed sequences of its writers and readers.

imt_itree keeps its sorted list twice -- the host mirror and the device index -- and synchronises the copies lazily:
every call that changes the tree leaves another combination of mirror_valid / dev_index_valid / sorted_cur / batches in
flight behind, and every call that reads the list picks its path from those and from the pointer mode.  The other GPU
tests follow one writer each; this one walks the transitions.  test_sequence plays the committed scripts of
tests/tree_model.py (every ordered pair of the twelve writer kinds adjacent with a light and with a full check between
them, every kind right after a refused call; tests/test_tree_model.py asserts that coverage) on an IndexedTree beside
the plain-Python model.  Expected lists come from the model, expected roots, proofs and witness rows from the CPU oracle
loaded with the model's preimages; every comparison is bit-exact.

  after an accepted step   the call's own outputs (root_out, rewind's root, status / leaf_index / n_inserted, the witness
                           rows, new_index); a pipelined device-pointer batch is left in flight, its rows are compared at
                           the next full check
  after a mixed batch      (kinds 12 and 13; host pointers through IndexedTree.mixed_batch, device pointers through
                           test_gpu_mixed.Raw with every buffer pre-filled) n_inserted, new_index, the INSERT rows = the
                           oracle's rows of inserting the INSERTs alone, every field of every READ row = one walk of the
                           oracle over the operations (tree_model.oracle_read_rows), rows beyond the counts untouched;
                           imt_itree_root_lagged(0) is the new root after kind 12; after kind 13 it returns what it returned
                           right before (code and bytes) and size, root() and snapshot() are what they were
  after a refused step     the error code; size, root() and the whole snapshot unchanged; of a mixed batch also *bad_op and,
                           with device pointers, that no output byte was written
  the third pass           (kinds 14 to 20, tree_model._ThirdGenerator; the model is MemberModel)
      14 insert_bulk       every field of imt_bulk_out = tests/bulk_model.py over the oracle's hashes, orc_verify_non_inclusion
                           == 0 per row
      16 / 17 / 18         n_inserted, n_read, status, leaf_index, bad_op from the model; INSERT rows = the oracle's rows of
                           the accepted INSERTs alone, READ and MEMBER rows = one walk of the oracle over the operations
                           carried out, rows beyond the counts and the outputs a call does not have untouched; root_out
      15 / 18 pipelined    the verdict and the INSERT count at once; root_out and the rows of every batch left in flight are
                           compared behind the next light or full check, each batch's own; a refused one leaves its
                           buffers and the batches in flight alone
      19 load_values       bad_pos on refusal; afterwards imt_itree_root_lagged has no root to give
      20 reserve           imt_itree_capacity; imt_itree_root_lagged answers what it answered; the full check runs over
                           the capacity the tree has now, the empty slots included
  no check                 (third pass only, behind a pipelined call) nothing is called before the next step, not even
                           size: that step enters with the batches before it still in flight
  light check              size and root(): neither touches the two copies of the list
  full check               size, root(), get_leaves of every slot (host and device pointers), snapshot(), the proof of
                           every slot, find_low of the probe set (host and device pointers) and its refusals, lookup,
                           non_membership_witness through the device index and through the host calls, and the witness
                           against imt_non_membership_batch

Every failure message names the script, the step and the step's kind, so it names the transition.
"""
import ctypes

import numpy as np
import pytest

import bulk_model as bm
import oracle_lib
import test_gpu_bulk as tgb
import test_gpu_insert_matrix as tm
import test_gpu_member_reads as tgr
import test_gpu_mixed as tgm
import tree_model as tmod
from oracle_lib import arr_ints, ints_to_arr
from test_gpu_rewind import DeviceBatches, compare_rows

pytestmark = pytest.mark.gpu

SCRIPTS = {s.name: s for s in tmod.scripts()}
KIND_NAMES = {1: "insert_batch", 2: "insert_batch host_prep", 3: "insert_batch device pipelined", 4: "insert_filtered",
              5: "insert_filtered host_prep", 6: "apply_batch", 7: "apply_batch host_prep", 8: "apply_filtered", 9: "rewind",
              10: "load", 12: "mixed_batch", 13: "mixed_batch READs only", 14: "insert_bulk", 15: "apply_pipelined",
              16: "mixed_filtered", 17: "apply_mixed / apply_mixed_filtered", 18: "mixed_pipelined / apply_mixed_pipelined",
              19: "load_values", 20: "reserve"}
N_PROBES = 24
FOREIGN_PROBES = (5, 6, 8, 9)          # of another residue on the partitioned tree (v % 3 != 1)
SENT = tgm.SENTINEL


def _cases():
    out = [pytest.param(name, "default", id=name) for name in SCRIPTS]
    for shape_name in ("d32", "part3"):          # two of the scripts on the other two forms of the hash kernels as well
        name = next(s.name for s in tmod.scripts() if s.shape.name == shape_name)
        out += [pytest.param(name, form, id=f"{name}-{form}") for form in ("thread", "quad")]
    name = tmod.third_pass_d32().name            # and one of the third pass: all seven newer kinds at depth 32
    out += [pytest.param(name, form, id=f"{name}-{form}") for form in ("thread", "quad")]
    return out


@pytest.fixture(scope="module")
def forms(imt):
    """one context per hash form, all on torch's current stream (the device-pointer calls' buffers are torch's)"""
    import torch
    torch.cuda.init()
    cs = {}
    for name, coop in tm.FORMS.items():
        c = imt.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        if coop is not None:
            c.set_option(imt._ffi.OPT_COOP_MAX_EVENTS, coop)
        cs[name] = c
    yield cs
    for c in cs.values():
        c.close()


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr())


class Player:
    """one script on one tree, the model beside it"""

    def __init__(self, imt, c, script):
        import torch
        self.imt, self.c, self.script, self.torch = imt, c, script, torch
        sh = script.shape
        self.t = t = imt.IndexedTree(c, sh.depth, sh.cap)
        if sh.placement:
            t.set_placement(*sh.placement)
        if sh.partition[0]:
            c._check(imt.lib.imt_itree_set_value_partition(t.h, *sh.partition))
        self.m = tmod.new_model(sh)
        self.base = tmod.index_base(sh)
        self.dv = DeviceBatches(imt, c, t, t.global_depth)
        self.in_flight = []                       # (device buffers, the oracle's rows, tag) of pipelined batches
        self.grew, self.entered = False, (1, False)
        self.piped = []                           # the comparisons owed for kinds 15 and 18 in flight: run behind the next check
        self.last_mixed = None                    # (size before, the INSERT rows, level-major) of the last kind-12 step
        self.last_bulk = self.last_block = None   # the same of the last kind-14 step and of the last kind-16 / 18 witness block
        self.err_name = {v: k for k, v in imt._ffi.ERR.items()}

    @property
    def shape(self):
        """the script's shape at the capacity the tree has now (a reserve step changes it): what the oracle is loaded at"""
        return self.script.shape._replace(cap=self.m.cap)

    def close(self):
        self.dv.sync()
        self.t.close()

    def code_of(self, call):
        """(IMT_ERR_* name or None, the call's result)"""
        try:
            return None, call()
        except ValueError:                        # the Python layer's IMT_ERR_VALUE of insert / apply / load / find_low
            return "VALUE", None
        except self.imt.ImtError as e:
            return self.err_name[e.code], None

    def dev(self, arr):
        a = np.ascontiguousarray(arr)
        return self.torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()

    # ---- the step ----
    def call(self, st):
        t, k = self.t, st.kind
        arr = ints_to_arr(st.vals) if st.vals is not None else None
        if k in (1, 2):
            return t.insert_batch(arr, host_prep=(k == 2))
        if k == 3:
            return self.dv.insert(arr)
        if k in (4, 5):
            return t.insert_filtered(arr, host_prep=(k == 5))
        if k in (6, 7):
            return t.apply_batch(arr, host_prep=(k == 7))
        if k == 8:
            return t.apply_filtered(arr, host_prep=bool(st.arg))
        if k == 9:
            return t.rewind(st.arg)
        pre = tm.to_fmt(tmod.pre_arr(st.arg["pre"]), st.arg["fmt"])
        if st.arg["device"]:
            d = self.dev(pre)
            return t.load_device(d.data_ptr(), pre.shape[0], st.arg["fmt"])
        return t.load(pre, st.arg["fmt"])

    # ---- the mixed batch ----
    def root_lagged(self):
        """(return code, the 32 bytes) of imt_itree_root_lagged(t, 0), host pointers"""
        out = np.zeros(32, np.uint8)
        rc = self.imt.lib.imt_itree_root_lagged(self.t.h, 0, out.ctypes.data_as(ctypes.c_void_p), 0)
        return rc, out.tobytes()

    def mixed_call(self, st):
        """(IMT_ERR_* name or None, bad_op or None, n_inserted, ins, rd, untouched): ins / rd cut to their rows, siblings
        item-major [rows, depth, 32]; untouched: on the device-pointer path, whether no output byte was written"""
        t, f, depth = self.t, self.imt._ffi, self.shape.depth
        arr, ops, im = ints_to_arr(st.vals), list(st.arg["ops"]), st.arg["item_major"]
        n = len(ops)
        rows_first = lambda a: a if im else a.transpose(1, 0, 2)
        if not st.arg["device"]:
            try:
                ins, rd = t.mixed_batch(arr, ops, item_major=im)
            except ValueError as e:
                return "VALUE", e.bad_op, None, None, None, None
            except self.imt.ImtError as e:
                return self.err_name[e.code], None, None, None, None, None
            n_ins = ins["low_index"].shape[0]
        else:
            r = tgm.Raw(self.imt, depth, n, im, dev=True)
            rc = r.call(t, arr, ops, f.SIB_ITEM_MAJOR if im else 0)          # returns behind a synchronisation of both streams
            if rc:
                assert r.n_ins.value == 0xDEAD, "n_inserted written by a refused call"
                bad = None if r.bad.value == 0xDEAD else r.bad.value
                return self.err_name[rc], bad, None, None, None, r.untouched()
            assert r.bad.value == 0xDEAD, "bad_op written by an accepted call"
            n_ins = r.n_ins.value
            assert n_ins <= n, f"n_inserted {n_ins} of {n} operations"
            ins, rd = tgm.cut(r.host(r.ins), n_ins, n, im), tgm.cut(r.host(r.rd), n - n_ins, n, im)      # beyond: the sentinel
            ins["new_index"] = np.arange(t.size - n_ins, t.size, dtype=np.uint64)
        for d in (ins, rd):
            for k in d:
                if k.endswith("_sib"):
                    d[k] = rows_first(d[k])
        return None, None, n_ins, ins, rd, None

    def check_mixed(self, st, before, out, n_ins, ins, rd, tag):
        sh, ops = self.shape, st.arg["ops"]
        acc, n_rd = out["acc"], ops.count(tmod.OP_READ)
        assert n_ins == len(acc), f"{tag}: n_inserted {n_ins}"
        assert all(a.shape[0] == n_ins for a in ins.values()) and all(a.shape[0] == n_rd for a in rd.values()), f"{tag}: row counts"
        ins = {k: (a.transpose(1, 0, 2) if k.endswith("_sib") else a) for k, a in ins.items()}      # compare_rows: level-major
        self.check_rows(ins, before, acc, tag)
        self.last_mixed = (len(before), ins)      # for tests/test_gpu_view_sequences.py: a replay across this step gives these rows
        want = tmod.oracle_read_rows(sh, before, st)
        assert [int(x) for x in want["low_index"]] == [r[1] for r in out["reads"]]
        assert set(rd) == set(tgm.RD_FIELDS)
        for k in tgm.RD_FIELDS:
            bad = np.nonzero((np.asarray(rd[k]) != want[k]).reshape(n_rd, -1).any(axis=1))[0]
            first = out["reads"][bad[0]] if bad.size else None
            assert bad.size == 0, f"{tag}: READ row {bad[:1]} (operation {first[0]}, {first[4]} INSERTs before it): {k}"

    def check_rows(self, got, before, acc, tag):
        n = len(acc)
        if n == 0:                                # a filtered batch that accepted nothing wrote no row
            return
        want = tmod.oracle_rows(self.shape, before, acc)
        compare_rows(got, want, 0, n, self.shape.depth, tag)
        new_index = np.arange(len(before), len(before) + n, dtype=np.uint64) + np.uint64(self.base)
        assert (got["new_index"] == new_index).all(), f"{tag}: new_index"

    def step(self, i, st):
        t, m, sh = self.t, self.m, self.shape
        what = f"refused {st.refusal}: {KIND_NAMES[st.kind]}" if st.refusal else KIND_NAMES[st.kind]
        prev = self.script.steps[i - 1] if i else None
        came = f" after kind {tmod.writer_kind(prev)} and a {prev.check} check" if prev else ""
        tag = f"{self.script.name} step {i} kind {tmod.writer_kind(st)} ({what}, size {m.size}){came}"
        before = tuple(m.vals)
        quiet = prev is None or prev.check != tmod.NO_CHECK        # nothing in flight: calls before the step are allowed
        self.entered = (len(before), self.grew)                    # for check(): did this step insert; did the one before
        if st.kind in tmod.NEW_KINDS:
            self.new_kind(i, st, before, tag)
            return self.check(st, tag)
        mixed = st.kind in (tmod.MIXED, tmod.MIXED_READS)
        if mixed:
            if st.kind == tmod.MIXED_READS:               # behind a step with no check nothing is called before this one
                lagged = self.root_lagged() if quiet else None
            code, bad_op, n_ins, ins, rd, untouched = self.mixed_call(st)
            tag += f", {'device' if st.arg['device'] else 'host'} pointers, {'item' if st.arg['item_major'] else 'level'}-major"
        else:
            code, res = self.code_of(lambda: self.call(st))
        if st.refusal:
            assert code == tmod.REFUSAL_CODE[st.refusal], f"{tag}: returned {code}"
            if mixed:
                with pytest.raises(tmod.Refused) as e:
                    tmod.play(m, st)
                assert bad_op == e.value.bad_op, f"{tag}: bad_op {bad_op}, the walk is refused at {e.value.bad_op}"
                assert untouched in (None, True), f"{tag}: a refused call wrote into an output buffer"
            assert t.size == len(before) and t.root() == tmod.oracle_root(sh, before), f"{tag}: size or root changed"
            assert (t.snapshot() == tmod.pre_arr(m.preimages(range(m.size)))).all(), f"{tag}: snapshot changed"
        else:
            assert code is None, f"{tag}: refused with {code}: {self.imt.lib.imt_last_error(self.c.h)}"
            out = tmod.play(m, st)
            after, k = tuple(m.vals), st.kind
            if k in (1, 2):
                self.check_rows(res, before, out["acc"], tag)
            elif k == 3:
                self.in_flight.append((res, before, out["acc"], tag))
            elif k in (4, 5):
                assert res["n_inserted"] == len(out["acc"]), f"{tag}: n_inserted {res['n_inserted']}"
                assert res["status"].tolist() == out["status"], f"{tag}: status"
                assert res["leaf_index"].tolist() == out["leaf"], f"{tag}: leaf_index"
                self.check_rows(res, before, out["acc"], tag)
            elif k in (6, 7):
                assert res == tmod.oracle_root(sh, after), f"{tag}: root_out"
            elif k == 8:
                status, leaf, n_ins, root = res
                assert n_ins == len(out["acc"]), f"{tag}: n_inserted {n_ins}"
                assert status.tolist() == out["status"] and leaf.tolist() == out["leaf"], f"{tag}: status / leaf_index"
                assert root == tmod.oracle_root(sh, after), f"{tag}: root_out"
            elif k == 9:
                assert res == tmod.oracle_root(sh, after), f"{tag}: rewind's root"
            elif mixed:
                self.check_mixed(st, before, out, n_ins, ins, rd, tag)
                if k == tmod.MIXED:
                    rc, root = self.root_lagged()
                    assert rc == 0 and arr_ints(np.frombuffer(root, np.uint8)) == [tmod.oracle_root(sh, after)], \
                        f"{tag}: imt_itree_root_lagged(0) returned {rc}, not the root after the batch"
                else:                                     # READs only: a writer that changes nothing
                    if lagged is None:
                        lagged = self.lagged_behind_flight()
                    assert lagged is None or self.root_lagged() == lagged, f"{tag}: imt_itree_root_lagged(0) sees a batch of READs only"
                    assert t.size == len(before) and t.root() == tmod.oracle_root(sh, before), f"{tag}: size or root changed"
                    assert (t.snapshot() == tmod.pre_arr(m.preimages(range(m.size)))).all(), f"{tag}: snapshot changed"
        self.check(st, tag)

    def check(self, st, tag):
        """the check behind a step; the device outputs of the pipelined calls of kinds 15 and 18 are compared behind the
        synchronisation it makes.  NO_CHECK: nothing is called, not even size"""
        t, m = self.t, self.m
        self.grew = not st.refusal and st.kind not in (9, 10, tmod.LOAD_VALUES, tmod.RESERVE) and m.size > self.entered[0]
        if st.check == tmod.NO_CHECK:
            return
        if st.check == tmod.FULL:
            self.full_check(tag)
        else:
            assert t.size == m.size, f"{tag}: size {t.size}, the model has {m.size}"
            assert t.root() == tmod.oracle_root(self.shape, m.vals), f"{tag}: root()"
        if self.piped:
            self.dv.sync()
            for settle in self.piped:
                settle(tag)
            self.piped = []

    def lagged_behind_flight(self):
        """what imt_itree_root_lagged(0) must answer in a step that entered behind batches in flight and changes nothing,
        where the model knows it: the step before was a batch that inserted, so its root is the root of the list as it
        is.  (code, bytes), or None where the step before inserted nothing."""
        if not self.entered[1]:
            return None
        return 0, self.imt.to_bytes(tmod.oracle_root(self.shape, self.m.vals)).tobytes()

    # ---- the kinds of the third pass ----
    def unchanged(self, before, tag):
        t, m = self.t, self.m
        assert t.size == len(before) and t.root() == tmod.oracle_root(self.shape, before), f"{tag}: size or root changed"
        assert (t.snapshot() == tmod.pre_arr(m.preimages(range(m.size)))).all(), f"{tag}: snapshot changed"
        assert t.capacity == m.cap, f"{tag}: capacity {t.capacity}, the model has {m.cap}"

    def refused_as(self, st, code, bad, tag):
        """the model refuses the step as the library did: the code and bad_op / bad_pos"""
        assert code == tmod.REFUSAL_CODE[st.refusal], f"{tag}: returned {code}"
        with pytest.raises(tmod.Refused) as e:
            tmod.play(self.m, st)
        assert e.value.code == code and bad == e.value.bad_op, f"{tag}: bad position {bad}, the model stops at {e.value.bad_op}"

    def block_rows(self, st, before, out, h, n_ins, n_rd, im, tag):
        """INSERT rows = the oracle's rows of the accepted INSERTs alone, READ and MEMBER rows = one walk of the oracle over
        the operations carried out, nothing written beyond the counts; returns the INSERT rows level-major"""
        sh, n = self.shape, len(st.vals)
        assert (n_ins, n_rd) == (len(out["acc"]), len(out["reads"])), f"{tag}: {n_ins} INSERTs, {n_rd} READs / MEMBERs"
        tgr.same_rows(h["ins"], tmod.oracle_rows(sh, before, out["acc"]), n_ins, n, im, 0, f"{tag}: INSERT rows")
        want = tmod.oracle_read_rows(sh, before, st, out["carried"])
        assert [int(x) for x in want["low_index"]] == [r[1] for r in out["reads"]], tag
        tgr.same_rows(h["rd"], want, n_rd, n, im, 0, f"{tag}: READ / MEMBER rows")
        level_major = lambda d: {k: (a.transpose(1, 0, 2) if k.endswith("_sib") and im else a) for k, a in d.items()}
        ins, rd = level_major(tgm.cut(h["ins"], n_ins, n, im)), level_major(tgm.cut(h["rd"], n_rd, n, im))
        ins["new_index"] = np.arange(len(before), len(before) + n_ins, dtype=np.uint64)
        return ins, rd

    def new_kind(self, i, st, before, tag):
        imt, t, m, k, torch = self.imt, self.t, self.m, st.kind, self.torch
        f, lib, depth = imt._ffi, imt.lib, self.script.shape.depth
        prev = self.script.steps[i - 1] if i else None
        quiet = prev is None or prev.check != tmod.NO_CHECK        # nothing in flight: calls before the step are allowed
        now = st.check != tmod.NO_CHECK
        arr = ints_to_arr(st.vals) if st.vals is not None else None
        if k == tmod.BULK:
            n, im = len(st.vals), st.arg["item_major"]
            tag += f", {'device' if st.arg['device'] else 'host'} pointers, {'item' if im else 'level'}-major"
            r = tgb.Raw(imt, depth, n, im, st.arg["device"])
            rc = r.call(t, arr, f.SIB_ITEM_MAJOR if im else 0)
            if st.refusal:
                self.refused_as(st, self.err_name[rc], None, tag)
                assert r.untouched(), f"{tag}: a refused call wrote into an output buffer"
                return self.unchanged(before, tag)
            assert rc == 0, f"{tag}: refused with {rc}: {lib.imt_last_error(self.c.h)}"
            tmod.play(m, st)
            orc, res = oracle_lib.load(), r.host()
            tgb.check_model(res, bm.bulk_witness(orc, depth, list(before), list(st.vals)), n, im, tag)
            for j in range(n):                                    # the reference's relation on every row
                helper = np.zeros((depth, 32), np.uint8)
                helper[:, 0] = [1 - ((int(res["low_index"][j]) >> l) & 1) for l in range(depth)]
                sib = res["low_sib"][j] if im else res["low_sib"][:, j]
                fail, _ = orc.verify_non_inclusion(arr_ints(res["root_before"][j])[0], arr_ints(res["low_leaf"][j]), sib, helper,
                                                   st.vals[int(res["order"][j])], int(res["is_largest"][j]))
                assert fail == 0, f"{tag}: orc_verify_non_inclusion rejects row {j}: {fail}"
            self.last_bulk = (len(before), res, im, st)
        elif k == tmod.APPLY_PIPE:
            d, root = self.dev(arr), torch.zeros(32, dtype=torch.uint8, device="cuda")
            if st.arg["inputs_ready"]:
                torch.cuda.current_stream().synchronize()         # the copy of the values is done; the batches in flight go on
            flags = f.DEVICE_PTRS | (f.HOST_PREP if st.arg["host_prep"] else 0) | (f.INPUTS_READY if st.arg["inputs_ready"] else 0)
            tag += f", {'IMT_HOST_PREP' if st.arg['host_prep'] else 'GPU prepare'}{', IMT_INPUTS_READY' if st.arg['inputs_ready'] else ''}"
            rc = lib.imt_itree_apply_pipelined(t.h, _ptr(d), len(st.vals), _ptr(root), flags)
            if st.refusal:
                self.refused_as(st, self.err_name[rc], None, tag)
                self.piped.append(lambda at, keep=d: self.same_bytes(root, bytes(32), f"{tag}, read at {at}: root_out of a refused batch"))
                return self.unchanged(before, tag) if now else None
            assert rc == 0, f"{tag}: refused with {rc}: {lib.imt_last_error(self.c.h)}"
            tmod.play(m, st)
            want = imt.to_bytes(tmod.oracle_root(self.shape, m.vals)).tobytes()
            self.piped.append(lambda at, keep=d: self.same_bytes(root, want, f"{tag}, read at {at}: the batch's own root_out"))
        elif k in (tmod.MIXED_FILT, tmod.APPLY_MIXED, tmod.MIXED_PIPE):
            ops, n, members = list(st.arg["ops"]), len(st.vals), st.arg["members"]
            if k == tmod.MIXED_FILT:
                which, dev, im = "mixed_filtered", st.arg["device"], st.arg["item_major"]
            elif k == tmod.APPLY_MIXED:
                which, dev, im = ("apply_mixed_filtered" if st.arg["filtered"] else "apply_mixed"), False, False
            else:
                which, dev, im = ("apply_mixed_pipelined" if st.arg["apply"] else "mixed_pipelined"), True, False
            tag += f", {which}, {'device' if dev else 'host'} pointers, {'item' if im else 'level'}-major{', IMT_MEMBER_OPS' if members else ''}"
            lagged = self.root_lagged() if quiet and k != tmod.MIXED_PIPE else None
            call = tgr.Call(imt, depth, n, dev, im)
            rc = call.run(which, t.h, arr, ops, (f.SIB_ITEM_MAJOR if im else 0) | (f.MEMBER_OPS if members else 0), wait=k != tmod.MIXED_PIPE)
            witness, filtered = which in ("mixed_filtered", "mixed_pipelined"), which.endswith("filtered")
            if st.refusal:
                bad = None if filtered or call.bad == tgr.UNSET else call.bad
                self.refused_as(st, self.err_name[rc], bad, tag)
                if filtered:                                      # the filtered twins: both counts 0 on every error
                    assert (call.n_ins, call.n_rd) == (0, 0), f"{tag}: counts {call.n_ins}, {call.n_rd} of a refused call"
                    assert self.err_name[rc] == "ARG", f"{tag}: only IMT_ERR_ARG leaves status and leaf_index untouched"
                else:
                    assert call.n_ins == tgr.UNSET, f"{tag}: n_inserted written by a refused call"
                if k == tmod.MIXED_PIPE:
                    self.piped.append(lambda at: self.all_untouched(call, f"{tag}, read at {at}"))
                    return self.unchanged(before, tag) if now else None
                self.all_untouched(call, tag)
                return self.unchanged(before, tag)
            assert rc == 0, f"{tag}: refused with {rc}: {lib.imt_last_error(self.c.h)}"
            out = tmod.play(m, st)
            after = tuple(m.vals)
            assert call.n_ins == len(out["acc"]), f"{tag}: n_inserted {call.n_ins}"
            assert filtered or call.bad == tgr.UNSET, f"{tag}: bad_op written by an accepted call"
            want_root = imt.to_bytes(tmod.oracle_root(self.shape, after)).tobytes()

            def outputs(at=None):
                where = tag if at is None else f"{tag}, read at {at}"
                h = call.host()
                if filtered:
                    assert call.n_rd == len(out["reads"]), f"{where}: n_read {call.n_rd}"
                    assert h["extra"]["status"][:n].tolist() == out["status"], f"{where}: status"
                    assert h["extra"]["leaf_index"][:n].tolist() == out["leaf"], f"{where}: leaf_index"
                else:
                    assert all((h["extra"][x].view(np.uint8) == SENT).all() for x in ("status", "leaf_index")), f"{where}: status written"
                if witness:
                    n_rd = call.n_rd if filtered else n - call.n_ins
                    ins, rd = self.block_rows(st, before, out, h, call.n_ins, n_rd, im, where)
                    assert (h["extra"]["root_out"] == SENT).all(), f"{where}: root_out written"
                    self.last_block = (len(before), ins, rd, out, st)
                else:
                    assert h["extra"]["root_out"].tobytes() == want_root, f"{where}: root_out"
                    assert all((a.view(np.uint8) == SENT).all() for x in ("ins", "rd") for a in h[x].values()), f"{where}: a witness row written"

            if k == tmod.MIXED_PIPE:
                self.piped.append(outputs)
            else:
                outputs()
                if out["acc"]:
                    assert self.root_lagged() == (0, want_root), f"{tag}: imt_itree_root_lagged(0) is not the root after the block"
                elif lagged is not None:                          # nothing inserted: a writer that changes nothing
                    assert self.root_lagged() == lagged, f"{tag}: imt_itree_root_lagged(0) sees a block without an INSERT"
                    self.unchanged(before, tag)
        elif k == tmod.LOAD_VALUES:
            vals = tm.to_fmt(ints_to_arr(st.arg["vals"]), st.arg["fmt"])
            tag += f", {'device' if st.arg['device'] else 'host'} pointers, format {st.arg['fmt']}, {len(vals)} values ({st.arg['source']})"
            code, bad = None, None
            try:
                if st.arg["device"]:
                    d = self.dev(vals)
                    t.load_values_device(d.data_ptr(), vals.shape[0], st.arg["fmt"])
                else:
                    t.load_values(vals, st.arg["fmt"])
            except ValueError as e:
                code, bad = "VALUE", e.bad_pos
            except imt.ImtError as e:
                code, bad = self.err_name[e.code], e.bad_pos
            if st.refusal:
                self.refused_as(st, code, bad, tag)
                return self.unchanged(before, tag)
            assert code is None, f"{tag}: refused with {code}: {lib.imt_last_error(self.c.h)}"
            tmod.play(m, st)
            assert self.root_lagged()[0] != 0, f"{tag}: imt_itree_root_lagged has a root to give right after load_values"
        else:
            lagged = self.root_lagged() if quiet else None
            code, _ = self.code_of(lambda: t.reserve(st.arg))
            if st.refusal:
                self.refused_as(st, code, None, tag)
                return self.unchanged(before, tag)
            assert code is None, f"{tag}: refused with {code}: {lib.imt_last_error(self.c.h)}"
            tmod.play(m, st)
            assert t.capacity == m.cap == st.arg, f"{tag}: capacity {t.capacity}"
            if lagged is None:                                    # behind batches in flight there was no call to ask before:
                lagged = self.lagged_behind_flight()              # the root of the batch before, where that batch inserted
            if lagged is not None:
                assert self.root_lagged() == lagged, f"{tag}: imt_itree_root_lagged answers something else behind reserve"

    def same_bytes(self, dev_buf, want, what):
        got = dev_buf.cpu().numpy().tobytes()
        assert got == want, f"{what}: {got.hex()}, expected {want.hex()}"

    def all_untouched(self, call, tag):
        assert call.untouched(), f"{tag}: a refused call wrote into an output buffer"

    # ---- every reader ----
    def full_check(self, tag):
        imt, c, t, m, sh, torch = self.imt, self.c, self.t, self.m, self.shape, self.torch
        f, lib, base, cap, depth = imt._ffi, imt.lib, self.base, sh.cap, sh.depth
        tag = f"{tag}, full check"
        assert t.size == m.size, f"{tag}: size {t.size}, the model has {m.size}"
        assert t.root() == tmod.oracle_root(sh, m.vals), f"{tag}: root()"
        idx = np.arange(cap, dtype=np.uint64) + np.uint64(base)
        want_pre = tmod.pre_arr(m.preimages(range(cap)))

        def same_leaves(got, n, how):
            bad = np.nonzero((got != want_pre[:n]).reshape(n, -1).any(axis=1))[0]
            assert bad.size == 0, f"{tag}: {how}: preimage of leaf {bad[:1]} is {arr_ints(got[bad[:1]])}"

        same_leaves(t.get_leaves(idx), cap, "get_leaves, host pointers")
        d_idx, d_pre = self.dev(idx), torch.zeros((cap, 3, 32), dtype=torch.uint8, device="cuda")
        assert lib.imt_itree_get_leaves(t.h, _ptr(d_idx), cap, _ptr(d_pre), f.DEVICE_PTRS) == 0, lib.imt_last_error(c.h)
        torch.cuda.synchronize()
        same_leaves(d_pre.cpu().numpy(), cap, "get_leaves, device pointers")
        same_leaves(t.snapshot(), m.size, "snapshot()")
        proofs = tmod.oracle_proofs(sh, m.vals)
        got = t.get_proof_batch(idx, item_major=True)
        bad = np.argwhere((got != proofs).any(axis=2))
        assert bad.size == 0, f"{tag}: get_proof_batch: leaf {bad[:1, 0]} level {bad[:1, 1]}"
        # find_low: host pointers (the mirror when it is valid), device pointers (always the device index)
        probes = m.probes()[:N_PROBES]
        pv = ints_to_arr(probes)
        want_low = [m.find_low(v) for v in probes]
        assert t.find_low(pv).tolist() == want_low, f"{tag}: find_low, host pointers"
        d_vals, d_low = self.dev(pv), torch.zeros(len(probes), dtype=torch.int64, device="cuda")
        assert lib.imt_itree_find_low_batch(t.h, _ptr(d_vals), len(probes), _ptr(d_low), f.DEVICE_PTRS) == 0, lib.imt_last_error(c.h)
        torch.cuda.synchronize()
        assert d_low.cpu().numpy().view(np.uint64).tolist() == want_low, f"{tag}: find_low, device pointers"
        refused = [0] + ([m.vals[-1], m.order[len(m.order) // 2]] if m.size > 1 else []) + \
            [v for v in FOREIGN_PROBES if not m.mine(v)]
        for v in refused:
            bad_vals = ints_to_arr(probes[:2] + [v])
            assert self.code_of(lambda: t.find_low(bad_vals))[0] == "VALUE", f"{tag}: find_low of {v:#x}, host pointers"
            d_bad = self.dev(bad_vals)
            rc = lib.imt_itree_find_low_batch(t.h, _ptr(d_bad), 3, _ptr(d_low), f.DEVICE_PTRS)
            assert rc == f.ERR["VALUE"], f"{tag}: find_low of {v:#x}, device pointers: {rc}"
        # lookup: stored, absent, zero and (on a partitioned tree) another subtree's values
        mix = probes[:8] + m.vals[1:4] + m.vals[-3:] + [0] + [v for v in FOREIGN_PROBES if not m.mine(v)]
        status, leaf = t.lookup(ints_to_arr(mix))
        assert list(zip(status.tolist(), leaf.tolist())) == [m.lookup(v) for v in mix], f"{tag}: lookup"
        # the non-membership witness, through the device index and through the host calls
        want = [m.nm_witness(v) for v in probes]
        want_leaves = tmod.pre_arr([w[1] for w in want])
        want_sib = proofs[[w[0] - base for w in want]].transpose(1, 0, 2)
        root = imt.to_bytes(t.root())
        for host in (False, True):
            how = f"non_membership_witness(host={host})"
            low, leaves, sib, largest = t.non_membership_witness(pv, host=host)
            assert low.tolist() == [w[0] for w in want], f"{tag}: {how}: low index"
            assert (leaves == want_leaves).all(), f"{tag}: {how}: low leaf"
            assert largest.tolist() == [w[2] for w in want], f"{tag}: {how}: is_largest"
            assert (sib == want_sib).all(), f"{tag}: {how}: siblings"
            fail = c.non_membership(root, leaves, low, sib, depth, pv, largest)
            assert not fail.any(), f"{tag}: {how}: imt_non_membership_batch rejects the witness: {fail.tolist()}"
        # the pipelined batches left in flight: their outputs are complete after a synchronisation
        if self.in_flight:
            self.dv.sync()
            for bufs, before, acc, its_tag in self.in_flight:
                got = DeviceBatches.host(bufs)
                got["new_index"] = np.arange(len(before), len(before) + len(acc), dtype=np.uint64) + np.uint64(base)
                self.check_rows(got, before, acc, f"{its_tag}, read at {tag}")
            self.in_flight = []
            self.dv.pending = []


@pytest.mark.parametrize("name,form", _cases())
def test_sequence(imt, forms, name, form):
    script = SCRIPTS[name]
    p = Player(imt, forms[form], script)
    try:
        for i, st in enumerate(script.steps):
            p.step(i, st)
        assert not p.in_flight and not p.piped
    finally:
        p.close()
