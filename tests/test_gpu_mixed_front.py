"""GPU: the refusals the five mixed entry points make through one shared front (imt_itree.cpp: check_mixed_mode,
check_mixed_ptrs, check_host_ops, and the rank kernel for a device-pointer caller's op bytes).

imt_itree_mixed_batch, imt_itree_apply_mixed, imt_itree_mixed_filtered, imt_itree_apply_mixed_filtered and
imt_itree_view_mixed_witness each have a test_refusals of their own, written with the entry point; this is the same
matrix for all five, row by row, so that a refusal one of them loses shows here whichever it is:

  each of IMT_PIPELINE, IMT_HOST_PREP, IMT_INPUTS_READY (host and device pointers), in the entry point's own words
  a placed tree, a partitioned tree, in the entry point's own words
  a misaligned device pointer to field elements: vals for all five, an INSERT output and a READ output where there are any
  a misaligned device low_index array: the INSERTs', the READs'
  an op byte that is neither INSERT nor READ, with host pointers and with device pointers

Every row asserts the result, that every array of the caller's still holds its sentinel bytes, that the counts were left
alone (or zeroed, for the filtered calls) and that the tree's size and root -- and the view's root -- are what they were.
The shapes are the smallest that have every position: a depth-4 tree holding 3 values and a list of 3 operations, INSERT
x READ with the offender, where there is one, in the middle.  The calls themselves are checked against the oracle in the
entry points' own suites; here a well-formed call must merely succeed, so that no row passes for the wrong reason.
"""
import ctypes

import numpy as np
import pytest

from oracle_lib import ints_to_arr
from test_gpu_rewind import forms  # noqa: F401  (the fixture: one context per hash form, on torch's stream)

pytestmark = pytest.mark.gpu

DEPTH, CAP, N = 4, 16, 3
STORED = [10, 13, 16]                   # all 1 mod 3: the partitioned tree takes them too
VALS, OPS = [4, 7, 19], [0, 1, 1]       # INSERT 4, READ 7, READ 19
SENTINEL = 0xA5
ENTRIES = ("mixed_batch", "apply_mixed", "mixed_filtered", "apply_mixed_filtered", "view_mixed_witness")
INS = dict(low_index=N * 8, low_leaf=N * 96, is_largest=N, old_root=N * 32, interim_root=N * 32, new_root=N * 32,
           new_leaf=N * 96, low_sib=DEPTH * N * 32, new_sib=DEPTH * N * 32)
RD = dict(low_index=N * 8, low_leaf=N * 96, is_largest=N, root=N * 32, low_sib=DEPTH * N * 32)
HAS_ROWS = ("mixed_batch", "mixed_filtered", "view_mixed_witness")      # the entry points with INSERT and READ outputs
FILTERED = ("mixed_filtered", "apply_mixed_filtered")


class Call:
    """one call of one entry point: every array the caller owns pre-filled with the sentinel byte, 16 bytes longer than
    the call needs so that a pointer moved off its alignment still points into it"""

    def __init__(self, imt, entry, dev):
        self.imt, self.entry, self.dev = imt, entry, dev
        sizes = {}
        if entry in HAS_ROWS:
            sizes.update({f"ins.{k}": b for k, b in INS.items()})
            sizes.update({f"rd.{k}": b for k, b in RD.items()})
        if entry in FILTERED:
            sizes.update(status=N, leaf=N * 8)
        if entry.startswith("apply"):
            sizes.update(root=32)
        self.buf = {k: self._buf(np.full(b + 16, SENTINEL, np.uint8)) for k, b in sizes.items()}

    def _buf(self, a):
        if not self.dev:
            return a
        import torch
        return torch.from_numpy(a).cuda()

    def _at(self, x, off=0):
        return (x.data_ptr() if self.dev else x.ctypes.data) + off

    def run(self, handle, ops=OPS, flags=0, off=None):
        """off: {array name or "vals": bytes its pointer is moved by}"""
        f, lib, off = self.imt._ffi, self.imt.lib, off or {}
        self.keep = (self._buf(np.concatenate([ints_to_arr(VALS).reshape(-1), np.zeros(16, np.uint8)])),
                     self._buf(np.asarray(ops, np.uint8)))
        pv, po = ctypes.c_void_p(self._at(self.keep[0], off.get("vals", 0))), ctypes.c_void_p(self._at(self.keep[1]))
        p = {k: ctypes.c_void_p(self._at(x, off.get(k, 0))) for k, x in self.buf.items()}
        ins = rd = None
        if self.entry in HAS_ROWS:
            ins = ctypes.byref(f.InsertOut(**{k: p[f"ins.{k}"] for k in INS}))
            rd = ctypes.byref(f.ReadOut(**{k: p[f"rd.{k}"] for k in RD}))
        self.k1, self.k2 = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
        n1, n2 = ctypes.byref(self.k1), ctypes.byref(self.k2)
        flags |= f.DEVICE_PTRS if self.dev else 0
        if self.entry == "mixed_batch":
            rc = lib.imt_itree_mixed_batch(handle, pv, po, N, ins, rd, n1, n2, flags)
        elif self.entry == "apply_mixed":
            rc = lib.imt_itree_apply_mixed(handle, pv, po, N, p["root"], n1, n2, flags)
        elif self.entry == "mixed_filtered":
            rc = lib.imt_itree_mixed_filtered(handle, pv, po, N, p["status"], p["leaf"], ins, rd, n1, n2, flags)
        elif self.entry == "apply_mixed_filtered":
            rc = lib.imt_itree_apply_mixed_filtered(handle, pv, po, N, p["status"], p["leaf"], n1, n2, p["root"], flags)
        else:
            rc = lib.imt_itree_view_mixed_witness(handle, pv, po, N, ins, rd, n1, n2, flags)
        return rc

    def untouched(self):
        return all(((x.cpu().numpy() if self.dev else x) == SENTINEL).all() for x in self.buf.values())

    def counts(self):
        return self.k1.value, self.k2.value


def make_tree(imt, c, entry, kind):
    """(tree, handle the entry point takes, state()): 3 values stored; a replay's tree has applied the list's INSERT as
    well and is watched through a view at the size before it"""
    t = imt.IndexedTree(c, DEPTH, CAP)
    if kind == "placed":
        t.set_placement(6, 1)
    if kind == "partitioned":
        c._check(imt.lib.imt_itree_set_value_partition(t.h, 3, 1))
    t.apply_batch(STORED)
    if entry != "view_mixed_witness":
        return t, None, t.h, lambda: (t.root(), t.size)
    t.apply_batch([v for v, op in zip(VALS, OPS) if op == 0])
    v = t.view(1 + len(STORED))
    if kind == "plain":
        v.root()                                        # built: a refusal must not rebuild it either
        return t, v, v.h, lambda: (t.root(), t.size, v.root(), v.stats()[1])
    return t, v, v.h, lambda: (t.root(), t.size, v.stats()[1])


@pytest.mark.parametrize("entry", ENTRIES)
def test_shared_refusals(imt, forms, entry):
    import torch
    f, lib, c = imt._ffi, imt.lib, forms["default"]
    ARG = f.ERR["ARG"]
    left_alone = (0, 0) if entry in FILTERED else (0xDEAD, 0xDEAD)
    replay = entry == "view_mixed_witness"
    t, v, h, state = make_tree(imt, c, entry, "plain")
    try:
        before = state()

        def refused(tag, dev=False, handle=h, says=None, **kw):
            r = Call(imt, entry, dev)
            rc = r.run(handle, **kw)
            if dev:
                c.sync()
                torch.cuda.synchronize()
            msg = lib.imt_last_error(c.h)
            assert rc == ARG, (entry, tag, rc, msg)
            assert says is None or says in msg, (entry, tag, msg)
            assert r.untouched() and r.counts() == left_alone, (entry, tag)

        # the three flags, in the entry point's words
        takes = b"a mixed replay takes neither" if replay else b"mixed batches take neither"
        for flag in (f.PIPELINE, f.HOST_PREP, f.INPUTS_READY):
            for dev in (False, True):
                refused(f"flag {flag:#x} dev {dev}", dev=dev, flags=flag, says=takes)
        # misaligned device pointers: field elements in, field elements out (an INSERT's, a READ's), the low_index arrays
        refused("vals", dev=True, off={"vals": 8}, says=b"not 16-byte aligned")
        if entry in HAS_ROWS:
            for name in ("ins.new_root", "ins.low_sib", "rd.root", "rd.low_leaf", "rd.low_sib"):
                refused(name, dev=True, off={name: 8}, says=b"not 16-byte aligned")
            for name in ("ins.low_index", "rd.low_index"):
                refused(name, dev=True, off={name: 4}, says=b"low_index array is not 8-byte aligned")
        # a bad op byte between an INSERT and a READ, through both kinds of pointer
        for dev in (False, True):
            for bad in (2, 255):
                refused(f"op byte {bad} dev {dev}", dev=dev, ops=[0, bad, 1], says=b"neither IMT_OP_INSERT nor IMT_OP_READ")
        assert state() == before
        # a placed tree, a partitioned tree
        no = b"mixed replays are not available" if replay else b"mixed batches are not available"
        for kind in ("placed", "partitioned"):
            t2, v2, h2, state2 = make_tree(imt, c, entry, kind)
            try:
                was = state2()
                for dev in (False, True):
                    refused(f"{kind} dev {dev}", dev=dev, handle=h2, says=no)
                assert state2() == was
            finally:
                if v2 is not None:
                    v2.close()
                t2.close()
        # and the same call with nothing wrong with it is carried out
        for dev in (False, True):
            t3, v3, h3, state3 = make_tree(imt, c, entry, "plain")
            try:
                r = Call(imt, entry, dev)
                assert r.run(h3) == 0, (entry, dev, lib.imt_last_error(c.h))
                c.sync()
                assert r.k1.value == 1 and not r.untouched()
                assert t3.size == 1 + len(STORED) + 1
            finally:
                if v3 is not None:
                    v3.close()
                t3.close()
    finally:
        if v is not None:
            v.close()
        t.close()
