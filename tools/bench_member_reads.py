#!/usr/bin/env python3
"""What a presence read (IMT_OP_MEMBER under IMT_MEMBER_OPS) costs and what it replaces, in one process on depth-32 trees
grown to 2^20 leaves, with random values, IMT_DEVICE_PTRS and every output requested.

  (a) one mixed block of 2^16 operations with a MEMBER at every fourth operation -- half of them of a value stored before
      the block, half of the value the INSERT two operations earlier put in -- against the block of the same INSERTs and as
      many READs (of random absent values) through imt_itree_mixed_batch without the flag.  Both kinds of read cost 1 + depth
      hashes.  Both trees receive the same INSERTs, so they stay twins: their roots must be equal afterwards, otherwise the row
      says "verified": false and its figures mean nothing.
      --reads-only measures the READ arm alone: with IMT_LIB_PATH naming another build of the library (the commit before
      this one, which has no flag to pass) it gives the figure of that build on the same blocks.
  (b) one block of 2^12 operations against the only way without the call: the same sequence cut at every MEMBER --
      imt_itree_insert_batch of the INSERTs up to it, then imt_itree_lookup_batch, imt_itree_get_leaves and
      imt_itree_get_proof_batch of the one value and imt_itree_root.  What the call replaces.

Each arm is warmed once, then timed `--repeats` times with the host clock, closed by imt_ctx_sync; reported: the median,
every repeat and the min-max of the repeats, as tools/bench_mixed.py does.  imt_version() says which build was measured.

  python tools/bench_member_reads.py [--repeats 3] [--preload 20] [--reads-only] [--out profiles/member_reads.txt]"""
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
spec = importlib.util.spec_from_file_location("bench_mixed", os.path.join(ROOT, "tools", "bench_mixed.py"))
bm = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bm)
bench, check, ptr, Buffers, timed, DEPTH = bm.bench, bm.check, bm.ptr, bm.Buffers, bm.timed, bm.DEPTH
OP_MEMBER, MEMBER_OPS = 2, 0x400          # include/imt.h; spelled out so that --reads-only runs on a build without them


def block(ctx, tree, vals, ops, buf, flags):
    k = ctypes.c_uint64()
    check(ctx, lib.imt_itree_mixed_batch(tree.h, ptr(vals), ptr(ops), vals.shape[0], ctypes.byref(buf.ins_out),
                                         ctypes.byref(buf.rd_out), ctypes.byref(k), None, F.DEVICE_PTRS | flags))
    ctx.sync()


def cut_at_every_member(ctx, tree, vals, ops_host, buf, status):
    """the same sequence without the call: runs of INSERTs as insert_batch, each MEMBER as lookup, leaf, proof and root"""
    p, n = 0, vals.shape[0]
    b = buf.rd
    while p < n:
        q = p
        while q < n and ops_host[q] == F.OP_INSERT:
            q += 1
        if q > p:
            check(ctx, lib.imt_itree_insert_batch(tree.h, ptr(vals, p), q - p, ctypes.byref(buf.ins_out), F.DEVICE_PTRS))
        if q < n:
            check(ctx, lib.imt_itree_lookup_batch(tree.h, ptr(vals, q), 1, ptr(status), ptr(b["low_index"]), F.DEVICE_PTRS))
            check(ctx, lib.imt_itree_get_leaves(tree.h, ptr(b["low_index"]), 1, ptr(b["low_leaf"]), F.DEVICE_PTRS))
            check(ctx, lib.imt_itree_get_proof_batch(tree.h, ptr(b["low_index"]), 1, ptr(b["low_sib"]), F.DEVICE_PTRS))
            check(ctx, lib.imt_itree_root(tree.h, ptr(b["root"]), F.DEVICE_PTRS))
        p = q + 1
    ctx.sync()


def summary(name, secs, n_ops):
    med = float(np.median(secs))
    return {f"{name}_ms": round(1e3 * med, 3), f"{name}_ops_per_s": round(n_ops / med),
            f"{name}_all_ms": [round(1e3 * s, 3) for s in secs], f"{name}_min_ms": round(1e3 * min(secs), 3),
            f"{name}_max_ms": round(1e3 * max(secs), 3)}


def member_values(vals, pre, ops_host, rng):
    """the block's values with every MEMBER's put in: of a stored value at every other MEMBER, of the value the INSERT two
    operations earlier put in at the rest"""
    out = vals.clone()
    where = torch.from_numpy(np.flatnonzero(ops_host != F.OP_INSERT)).to(vals.device)
    even, odd = where[0::2], where[1::2]
    out[even] = pre[torch.from_numpy(rng.integers(0, pre.shape[0], size=even.shape[0])).to(vals.device)]
    out[odd] = vals[odd - 2]                       # operation p - 2 of a block with a MEMBER at every fourth is an INSERT
    return out


def measure(ctx, dev, preload, logn, repeats, seed, case, reads_only):
    n = 1 << logn
    pre = torch.from_numpy(bench.synth_values(1 << preload, 0, 1, seed)).to(dev)
    cap = 1 << (preload + 1)
    arms = ["reads"] if reads_only else ["members", "reads" if case == "a" else "cut"]
    trees = {a: imt_amd.IndexedTree(ctx, DEPTH, cap) for a in arms}
    for t in trees.values():
        check(ctx, lib.imt_itree_apply_batch(t.h, ptr(pre), 1 << preload, None, F.DEVICE_PTRS))
    kinds = np.array([1 if p % 4 == 3 else 0 for p in range(n)], np.uint8)          # 1: the read of either kind
    ops_rd = torch.from_numpy(np.where(kinds == 1, F.OP_READ, F.OP_INSERT).astype(np.uint8)).to(dev)
    ops_mb_host = np.where(kinds == 1, OP_MEMBER, F.OP_INSERT).astype(np.uint8)
    ops_mb = torch.from_numpy(ops_mb_host).to(dev)
    buf = Buffers(dev, n)
    status = torch.zeros(8, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(seed)
    secs = {a: [] for a in arms}
    for r in range(repeats + 1):                                  # the first round warms every arm
        vals = torch.from_numpy(bench.synth_values(n, 0, 1, seed + 1 + r)).to(dev)
        mvals = member_values(vals, pre, ops_mb_host, rng)
        torch.cuda.synchronize()
        took = {}
        if "members" in arms:
            took["members"] = timed(block, ctx, trees["members"], mvals, ops_mb, buf, MEMBER_OPS)
        if "reads" in arms:
            took["reads"] = timed(block, ctx, trees["reads"], vals, ops_rd, buf, 0)
        if "cut" in arms:
            took["cut"] = timed(cut_at_every_member, ctx, trees["cut"], mvals, ops_mb_host, buf, status)
        if r:
            for a in arms:
                secs[a].append(took[a])
    sizes, roots = {t.size for t in trees.values()}, {t.root() for t in trees.values()}
    n_ins = int((kinds == 0).sum())
    row = dict(operations=n, inserts=n_ins, reads_or_members=n - n_ins, leaves_before=(1 << preload) + 1, leaves_after=int(sizes.pop()),
               repeats=repeats, verified=bool(len(roots) == 1 and not sizes), arms=arms)
    for a in arms:
        row.update(summary(a, secs[a], n))
    if len(arms) == 2:
        row[f"members_over_{arms[1]}"] = round(float(np.median(secs["members"])) / float(np.median(secs[arms[1]])), 4)
    for t in trees.values():
        t.close()
    del pre, buf
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--preload", type=int, default=20)
    ap.add_argument("--reads-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lines = [json.dumps(dict(version=lib.imt_version().decode(), library=os.path.relpath(F.LIB_PATH, ROOT),
                             device=torch.cuda.get_device_name(0), depth=DEPTH, preload=1 << args.preload, read_every=4,
                             flags="IMT_DEVICE_PTRS, every output requested"))]
    print(lines[0], flush=True)
    a = measure(ctx, dev, args.preload, 16, args.repeats, 0x4D454D00, "a", args.reads_only)
    lines.append(json.dumps(dict(case="a", **a)))
    print(lines[-1], flush=True)
    if args.reads_only:
        lines.append(f"# (a, READ arm alone) 2^16 operations: {a['reads_ms']} ms, {a['reads_min_ms']} .. {a['reads_max_ms']} ms")
    else:
        b = measure(ctx, dev, args.preload, 12, args.repeats, 0x4D454D10, "b", False)
        lines.append(json.dumps(dict(case="b", **b)))
        print(lines[-1], flush=True)
        lines.append(f"# (a) 2^16 operations, every fourth a MEMBER: {a['members_ms']} ms ({a['members_min_ms']} .. {a['members_max_ms']}) "
                     f"against the same INSERTs and as many READs {a['reads_ms']} ms ({a['reads_min_ms']} .. {a['reads_max_ms']}): "
                     f"x{a['members_over_reads']}; {a['members_ops_per_s'] / 1e6:.3f} M operations/s; verified {a['verified']}")
        lines.append(f"# (b) 2^12 operations: one call {b['members_ms']} ms ({b['members_min_ms']} .. {b['members_max_ms']}) against the "
                     f"sequence cut at every MEMBER {b['cut_ms']} ms ({b['cut_min_ms']} .. {b['cut_max_ms']}): "
                     f"x{b['members_over_cut']}; verified {b['verified']}")
    print("\n".join(l for l in lines if l.startswith("#")))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
