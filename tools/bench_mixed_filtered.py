#!/usr/bin/env python3
"""What the classification of imt_itree_mixed_filtered costs and what the call replaces, in one process on twin depth-32
trees grown to 2^20 leaves, with random values, IMT_DEVICE_PTRS, every output requested and a READ at every fourth
operation -- the conventions, the seeds and the blocks of tools/bench_mixed.py, so the imt_itree_mixed_batch arm of (a)
is that tool's case (a) again.

  (a) a clean block of 2^16 operations through imt_itree_mixed_filtered on one tree and through imt_itree_mixed_batch on
      its twin: the difference is the price of the classification (a sort of the positions, two scans, four short kernels, one
      more host wait).  Both trees receive the same block, so their roots must be equal afterwards ("verified").
  (b) a block of 2^12 operations with 16 offenders (double spends, READs of values spent earlier in the block, READs and
      INSERTs of stored values, zeros): one imt_itree_mixed_filtered call against the only way without it -- call
      imt_itree_mixed_batch, drop the operation *bad_op names, call again: 17 calls.  The loop's time includes gathering
      the remaining operations on the device each round.

Each arm is warmed once, then timed `--repeats` times with the host clock, closed by imt_ctx_sync; reported: the median,
every repeat and the min-max spread relative to the median.  imt_version() says which build was measured.

  python tools/bench_mixed_filtered.py [--repeats 3] [--preload 20] [--out profiles/mixed_filtered.txt]"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import imt_amd  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_mixed", os.path.join(ROOT, "tools", "bench_mixed.py"))
bm = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bm)
F, lib, DEPTH, bench = bm.F, bm.lib, bm.DEPTH, bm.bench
check, ptr, timed, summary = bm.check, bm.ptr, bm.timed, bm.summary


class Status:
    """device status / leaf_index for n operations"""

    def __init__(self, dev, n):
        self.status = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.leaf = torch.zeros(n, dtype=torch.int64, device=dev)


def filtered(ctx, tree, vals, ops, buf, st, counts):
    k, m = ctypes.c_uint64(), ctypes.c_uint64()
    check(ctx, lib.imt_itree_mixed_filtered(tree.h, ptr(vals), ptr(ops), vals.shape[0], ptr(st.status), ptr(st.leaf),
                                            ctypes.byref(buf.ins_out), ctypes.byref(buf.rd_out), ctypes.byref(k), ctypes.byref(m),
                                            F.DEVICE_PTRS))
    ctx.sync()
    counts[:] = [k.value, m.value]


def drop_one_per_round(ctx, tree, vals, ops, buf, rounds):
    """imt_itree_mixed_batch until it is accepted, the operation it names removed each time"""
    keep = torch.ones(vals.shape[0], dtype=torch.bool, device=vals.device)
    pos = torch.arange(vals.shape[0], device=vals.device)
    k, bad = ctypes.c_uint64(), ctypes.c_uint64()
    calls = 0
    while True:
        v, o, at = vals[keep].contiguous(), ops[keep].contiguous(), pos[keep]
        rc = lib.imt_itree_mixed_batch(tree.h, ptr(v), ptr(o), v.shape[0], ctypes.byref(buf.ins_out), ctypes.byref(buf.rd_out),
                                       ctypes.byref(k), ctypes.byref(bad), F.DEVICE_PTRS)
        calls += 1
        if rc == 0:
            break
        if rc != F.ERR["VALUE"]:
            check(ctx, rc)
        keep[at[bad.value]] = False
    ctx.sync()
    rounds[:] = [calls]


def clean_block(ctx, dev, preload, logn, repeats, seed):
    n = 1 << logn
    pre = torch.from_numpy(bench.synth_values(1 << preload, 0, 1, seed)).to(dev)
    cap = 1 << (preload + 1)
    A, B = imt_amd.IndexedTree(ctx, DEPTH, cap), imt_amd.IndexedTree(ctx, DEPTH, cap)
    for t in (A, B):
        check(ctx, lib.imt_itree_apply_batch(t.h, ptr(pre), 1 << preload, None, F.DEVICE_PTRS))
    ops_host = np.array([F.OP_READ if p % 4 == 3 else F.OP_INSERT for p in range(n)], np.uint8)
    ops = torch.from_numpy(ops_host).to(dev)
    buf, st, counts = bm.Buffers(dev, n), Status(dev, n), [0, 0]
    secs = dict(filtered=[], mixed=[])
    all_new = True
    for r in range(repeats + 1):                                  # the first round warms both arms
        vals = torch.from_numpy(bench.synth_values(n, 0, 1, seed + 1 + r)).to(dev)
        torch.cuda.synchronize()
        tf = timed(filtered, ctx, A, vals, ops, buf, st, counts)
        tm_ = timed(bm.mixed, ctx, B, vals, ops, buf)
        all_new = all_new and counts[0] + counts[1] == n and not bool(st.status.any())
        if r:
            secs["filtered"].append(tf)
            secs["mixed"].append(tm_)
    verified = A.root() == B.root() and A.size == B.size and all_new
    row = dict(operations=n, inserts=int((ops_host == F.OP_INSERT).sum()), reads=int((ops_host == F.OP_READ).sum()),
               leaves_before=(1 << preload) + 1, leaves_after=int(A.size), repeats=repeats, verified=bool(verified))
    row.update(summary("filtered", secs["filtered"], n))
    row.update(summary("mixed_batch", secs["mixed"], n))
    row["classification_ms"] = round(1e3 * (float(np.median(secs["filtered"])) - float(np.median(secs["mixed"]))), 3)
    row["filtered_over_mixed_batch"] = round(float(np.median(secs["filtered"])) / float(np.median(secs["mixed"])), 4)
    for t in (A, B):
        t.close()
    del pre, buf
    torch.cuda.empty_cache()
    return row


def block_with_offenders(ctx, dev, preload, logn, offenders, repeats, seed):
    n = 1 << logn
    pre_host = bench.synth_values(1 << preload, 0, 1, seed)
    pre = torch.from_numpy(pre_host).to(dev)
    cap = 1 << (preload + 1)
    A, B = imt_amd.IndexedTree(ctx, DEPTH, cap), imt_amd.IndexedTree(ctx, DEPTH, cap)
    for t in (A, B):
        check(ctx, lib.imt_itree_apply_batch(t.h, ptr(pre), 1 << preload, None, F.DEVICE_PTRS))
    ops_host = np.array([F.OP_READ if p % 4 == 3 else F.OP_INSERT for p in range(n)], np.uint8)
    at = [(j + 1) * n // (offenders + 1) for j in range(offenders)]         # spread over the block
    buf, st, counts, rounds = bm.Buffers(dev, n), Status(dev, n), [0, 0], [0]
    secs = dict(filtered=[], loop=[])
    ok = True
    for r in range(repeats + 1):
        host = bench.synth_values(n, 0, 1, seed + 1 + r).copy()
        ops_r = ops_host.copy()
        for j, p in enumerate(at):                                # the kinds in turn, as INSERT and as READ
            first_insert = 4 * (j + 1)                            # an INSERT position well before p
            host[p] = (host[first_insert], pre_host[1000 + j], np.zeros(32, np.uint8))[j % 3]
            ops_r[p] = F.OP_READ if j & 1 else F.OP_INSERT
        vals, ops = torch.from_numpy(host).to(dev), torch.from_numpy(ops_r).to(dev)
        torch.cuda.synchronize()
        tf = timed(filtered, ctx, A, vals, ops, buf, st, counts)
        tl = timed(drop_one_per_round, ctx, B, vals, ops, buf, rounds)
        ok = ok and counts[0] + counts[1] == n - offenders and rounds[0] == offenders + 1
        if r:
            secs["filtered"].append(tf)
            secs["loop"].append(tl)
    verified = ok and A.root() == B.root() and A.size == B.size
    row = dict(operations=n, offenders=offenders, loop_calls=rounds[0], leaves_before=(1 << preload) + 1, leaves_after=int(A.size),
               repeats=repeats, verified=bool(verified))
    row.update(summary("filtered", secs["filtered"], n))
    row.update(summary("drop_one_per_round", secs["loop"], n))
    row["filtered_over_loop"] = round(float(np.median(secs["filtered"])) / float(np.median(secs["loop"])), 4)
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
    a = clean_block(ctx, dev, args.preload, 16, args.repeats, 0x4D495800)
    lines.append(json.dumps(dict(case="a", **a)))
    print(lines[-1], flush=True)
    b = block_with_offenders(ctx, dev, args.preload, 12, 16, args.repeats, 0x4D495810)
    lines.append(json.dumps(dict(case="b", **b)))
    print(lines[-1], flush=True)
    lines.append(f"# (a) clean block of 2^16 operations: mixed_filtered {a['filtered_ms']} ms ({100 * a['filtered_spread']:.2f} % spread) "
                 f"against mixed_batch {a['mixed_batch_ms']} ms ({100 * a['mixed_batch_spread']:.2f} %): the classification costs "
                 f"{a['classification_ms']} ms, x{a['filtered_over_mixed_batch']}; verified {a['verified']}")
    lines.append(f"# (b) 2^12 operations, 16 offenders: one mixed_filtered call {b['filtered_ms']} ms ({100 * b['filtered_spread']:.2f} % "
                 f"spread) against {b['loop_calls']} mixed_batch calls dropping one operation per round "
                 f"{b['drop_one_per_round_ms']} ms ({100 * b['drop_one_per_round_spread']:.2f} %): x{b['filtered_over_loop']}; "
                 f"verified {b['verified']}")
    print("\n".join(lines[-2:]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
