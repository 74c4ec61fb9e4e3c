#!/usr/bin/env python3
"""What imt_itree_mixed_batch costs and what it replaces, in one process on twin depth-32 trees grown to 2^20 leaves, with
random values, IMT_DEVICE_PTRS, every output requested and a READ at every fourth operation.

  (a) one mixed batch of 2^16 operations against imt_itree_insert_batch (un-pipelined, `out` given) of its 49 152 INSERTs
      alone: what the reads add.  Per repeat both trees receive the same INSERTs, so they stay twins: their roots must be
      equal afterwards, otherwise the row says "verified": false and its figures mean nothing.
  (b) one mixed batch of 2^12 operations against the only way without it: the same sequence cut at every READ --
      imt_itree_insert_batch of the INSERTs up to the READ, then imt_itree_non_membership_witness of the one value and
      imt_itree_root.  What the call replaces.

Each arm is warmed once, then timed `--repeats` times with the host clock, closed by imt_ctx_sync; reported: the median,
every repeat and the min-max spread relative to the median, as tools/bench_apply.py does.  imt_version() says which build
was measured.

  python tools/bench_mixed.py [--repeats 3] [--preload 20] [--out profiles/mixed.txt]"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import imt_amd  # noqa: E402

F, lib = imt_amd._ffi, imt_amd.lib
spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)
DEPTH = 32
INS = ("low_index", "low_leaf", "is_largest", "old_root", "interim_root", "new_root", "new_leaf", "low_sib", "new_sib")
RD = ("low_index", "low_leaf", "is_largest", "root", "low_sib")


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def ptr(x, row=0):
    return ctypes.c_void_p(x[row].data_ptr() if row else x.data_ptr())


class Buffers:
    """device outputs for n operations: both structs, level-major siblings with stride n"""

    def __init__(self, dev, n):
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)
        shapes = dict(low_leaf=(n, 3, 32), new_leaf=(n, 3, 32), is_largest=(n,), old_root=(n, 32), interim_root=(n, 32),
                      new_root=(n, 32), root=(n, 32), low_sib=(DEPTH, n, 32), new_sib=(DEPTH, n, 32))
        self.ins = {k: z(n, dt=torch.int64) if k == "low_index" else z(*shapes[k]) for k in INS}
        self.rd = {k: z(n, dt=torch.int64) if k == "low_index" else z(*shapes[k]) for k in RD}
        self.ins_out = F.InsertOut(**{k: v.data_ptr() for k, v in self.ins.items()})
        self.rd_out = F.ReadOut(**{k: v.data_ptr() for k, v in self.rd.items()})


def mixed(ctx, tree, vals, ops, buf):
    k = ctypes.c_uint64()
    check(ctx, lib.imt_itree_mixed_batch(tree.h, ptr(vals), ptr(ops), vals.shape[0], ctypes.byref(buf.ins_out),
                                         ctypes.byref(buf.rd_out), ctypes.byref(k), None, F.DEVICE_PTRS))
    ctx.sync()


def inserts_alone(ctx, tree, ins_vals, buf):
    check(ctx, lib.imt_itree_insert_batch(tree.h, ptr(ins_vals), ins_vals.shape[0], ctypes.byref(buf.ins_out), F.DEVICE_PTRS))
    ctx.sync()


def cut_at_every_read(ctx, tree, vals, ops_host, buf):
    """the same sequence without the call: runs of INSERTs as insert_batch, each READ as a witness call and a root call"""
    p, n = 0, vals.shape[0]
    b = buf.rd
    while p < n:
        q = p
        while q < n and ops_host[q] == F.OP_INSERT:
            q += 1
        if q > p:
            check(ctx, lib.imt_itree_insert_batch(tree.h, ptr(vals, p), q - p, ctypes.byref(buf.ins_out), F.DEVICE_PTRS))
        if q < n:
            check(ctx, lib.imt_itree_non_membership_witness(tree.h, ptr(vals, q), 1, ptr(b["low_index"]), ptr(b["low_leaf"]),
                                                            ptr(b["is_largest"]), ptr(b["low_sib"]), F.DEVICE_PTRS))
            check(ctx, lib.imt_itree_root(tree.h, ptr(b["root"]), F.DEVICE_PTRS))
        p = q + 1
    ctx.sync()


def timed(fn, *a):
    t0 = time.perf_counter()
    fn(*a)
    return time.perf_counter() - t0


def summary(name, secs, n_ops):
    med = float(np.median(secs))
    return {f"{name}_ms": round(1e3 * med, 3), f"{name}_ops_per_s": round(n_ops / med),
            f"{name}_all_ms": [round(1e3 * s, 3) for s in secs], f"{name}_spread": round((max(secs) - min(secs)) / med, 4)}


def measure(ctx, dev, preload, logn, repeats, seed, other):
    n = 1 << logn
    pre = torch.from_numpy(bench.synth_values(1 << preload, 0, 1, seed)).to(dev)
    cap = 1 << (preload + 1)
    A, B = imt_amd.IndexedTree(ctx, DEPTH, cap), imt_amd.IndexedTree(ctx, DEPTH, cap)
    for t in (A, B):
        check(ctx, lib.imt_itree_apply_batch(t.h, ptr(pre), 1 << preload, None, F.DEVICE_PTRS))
    ops_host = np.array([F.OP_READ if p % 4 == 3 else F.OP_INSERT for p in range(n)], np.uint8)
    ops = torch.from_numpy(ops_host).to(dev)
    keep = torch.from_numpy(ops_host == F.OP_INSERT).to(dev)
    buf = Buffers(dev, n)
    secs = dict(mixed=[], other=[])
    for r in range(repeats + 1):                                  # the first round warms both arms
        vals = torch.from_numpy(bench.synth_values(n, 0, 1, seed + 1 + r)).to(dev)
        ins_vals = vals[keep].contiguous()
        torch.cuda.synchronize()
        tm_ = timed(mixed, ctx, A, vals, ops, buf)
        to_ = timed(inserts_alone, ctx, B, ins_vals, buf) if other == "inserts_alone" else timed(cut_at_every_read, ctx, B, vals, ops_host, buf)
        if r:
            secs["mixed"].append(tm_)
            secs["other"].append(to_)
    verified = A.root() == B.root() and A.size == B.size
    n_ins = int((ops_host == F.OP_INSERT).sum())
    row = dict(operations=n, inserts=n_ins, reads=n - n_ins, leaves_before=(1 << preload) + 1, leaves_after=int(A.size),
               repeats=repeats, verified=bool(verified), against=other)
    row.update(summary("mixed", secs["mixed"], n))
    row.update(summary(other, secs["other"], n_ins if other == "inserts_alone" else n))
    row["mixed_over_other"] = round(float(np.median(secs["mixed"])) / float(np.median(secs["other"])), 4)
    for t in (A, B):
        t.close()
    del pre, buf
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--preload", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lines = [json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                             preload=1 << args.preload, read_every=4, flags="IMT_DEVICE_PTRS, every output requested"))]
    print(lines[0], flush=True)
    a = measure(ctx, dev, args.preload, 16, args.repeats, 0x4D495800, "inserts_alone")
    lines.append(json.dumps(dict(case="a", **a)))
    print(lines[-1], flush=True)
    b = measure(ctx, dev, args.preload, 12, args.repeats, 0x4D495810, "cut_at_every_read")
    lines.append(json.dumps(dict(case="b", **b)))
    print(lines[-1], flush=True)
    lines.append(f"# (a) 2^16 operations: mixed {a['mixed_ms']} ms ({100 * a['mixed_spread']:.2f} % spread) against its "
                 f"{a['inserts']} INSERTs alone {a['inserts_alone_ms']} ms ({100 * a['inserts_alone_spread']:.2f} %): "
                 f"x{a['mixed_over_other']}; {a['mixed_ops_per_s'] / 1e6:.3f} M operations/s; verified {a['verified']}")
    lines.append(f"# (b) 2^12 operations: mixed {b['mixed_ms']} ms ({100 * b['mixed_spread']:.2f} % spread) against the sequence "
                 f"cut at every READ {b['cut_at_every_read_ms']} ms ({100 * b['cut_at_every_read_spread']:.2f} %): "
                 f"x{b['mixed_over_other']}; verified {b['verified']}")
    print("\n".join(lines[-2:]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
