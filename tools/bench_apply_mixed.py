#!/usr/bin/env python3
"""What applying a mixed block without witnesses costs, in one process on three depth-32 trees grown to 2^20 leaves, with
random values and IMT_DEVICE_PTRS -- the conventions and seeds of tools/bench_mixed_filtered.py.  The block is a
sequencer's: 2^16 operations, a READ at every odd position, and 256 offenders spread over it (double spends, READs of
values spent earlier in the block, stored values, zeros).  Every round the same block goes into all three trees:

  apply_mixed_filtered   imt_itree_apply_mixed_filtered: the classification, the checks, one hash per touched node
  mixed_filtered_null    imt_itree_mixed_filtered with ins == rd == NULL: what a caller had to use before -- the same
                         classification and checks, then the witness sweep (2 + 2*depth hashes per INSERT, 1 + depth per READ)
  apply_filtered_inserts imt_itree_apply_filtered of the block's INSERT values alone: the floor -- the same hashing with
                         no READ looked at (and so with no say on whether the READs hold)

The three trees must have equal roots and sizes afterwards, and the hash counts of the first and the third call must be
equal level by level ("verified").  The arms alternate within a round; the first round warms all three, then `--repeats`
rounds are timed with the host clock, each call closed by imt_ctx_sync; reported: the median, every repeat and the
min-max spread relative to the median.  imt_version() says which build was measured.

  python tools/bench_apply_mixed.py [--repeats 7] [--preload 20] [--out profiles/apply_mixed.txt]"""
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


class Out:
    """device status / leaf_index / root for n operations, and the counts of the last call"""

    def __init__(self, dev, n):
        self.status = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.leaf = torch.zeros(n, dtype=torch.int64, device=dev)
        self.root = torch.zeros(32, dtype=torch.uint8, device=dev)
        self.counts = (0, 0)


def apply_mixed_filtered(ctx, tree, vals, ops, out):
    k, m = ctypes.c_uint64(), ctypes.c_uint64()
    check(ctx, lib.imt_itree_apply_mixed_filtered(tree.h, ptr(vals), ptr(ops), vals.shape[0], ptr(out.status), ptr(out.leaf),
                                                  ctypes.byref(k), ctypes.byref(m), ptr(out.root), F.DEVICE_PTRS))
    ctx.sync()
    out.counts = (k.value, m.value)


def mixed_filtered_null(ctx, tree, vals, ops, out):
    k, m = ctypes.c_uint64(), ctypes.c_uint64()
    check(ctx, lib.imt_itree_mixed_filtered(tree.h, ptr(vals), ptr(ops), vals.shape[0], ptr(out.status), ptr(out.leaf), None, None,
                                            ctypes.byref(k), ctypes.byref(m), F.DEVICE_PTRS))
    ctx.sync()
    out.counts = (k.value, m.value)


def apply_filtered_inserts(ctx, tree, ins_vals, out):
    k = ctypes.c_uint64()
    check(ctx, lib.imt_itree_apply_filtered(tree.h, ptr(ins_vals), ins_vals.shape[0], ptr(out.status), ptr(out.leaf),
                                            ctypes.byref(k), ptr(out.root), F.DEVICE_PTRS))
    ctx.sync()
    out.counts = (k.value, 0)


def measure(ctx, dev, preload, logn, offenders, repeats, seed):
    n = 1 << logn
    pre_host = bench.synth_values(1 << preload, 0, 1, seed)
    pre = torch.from_numpy(pre_host).to(dev)
    cap = 1 << (preload + 1)
    trees = [imt_amd.IndexedTree(ctx, DEPTH, cap) for _ in range(3)]
    A, B, C = trees
    for t in trees:
        check(ctx, lib.imt_itree_apply_batch(t.h, ptr(pre), 1 << preload, None, F.DEVICE_PTRS))
    ops_host = np.array([F.OP_READ if p & 1 else F.OP_INSERT for p in range(n)], np.uint8)
    at = [(j + 1) * n // (offenders + 1) for j in range(offenders)]         # spread over the block
    outs = [Out(dev, n) for _ in range(3)]
    names = ("apply_mixed_filtered", "mixed_filtered_null", "apply_filtered_inserts")
    secs = {k: [] for k in names}
    ok, accepted = True, (0, 0)
    for r in range(repeats + 1):                                  # the first round warms all three arms
        host = bench.synth_values(n, 0, 1, seed + 1 + r).copy()
        ops_r = ops_host.copy()
        for j, p in enumerate(at):                                # the kinds in turn, as INSERT and as READ
            host[p] = (host[2 * (j + 1)], pre_host[1000 + j], np.zeros(32, np.uint8))[j % 3]      # 2 (j + 1): an INSERT well before p
            ops_r[p] = F.OP_READ if j & 1 else F.OP_INSERT
        vals, ops = torch.from_numpy(host).to(dev), torch.from_numpy(ops_r).to(dev)
        ins_vals = vals[torch.from_numpy(ops_r == F.OP_INSERT).to(dev)].contiguous()
        torch.cuda.synchronize()
        t = (timed(apply_mixed_filtered, ctx, A, vals, ops, outs[0]), timed(mixed_filtered_null, ctx, B, vals, ops, outs[1]),
             timed(apply_filtered_inserts, ctx, C, ins_vals, outs[2]))
        accepted = outs[0].counts
        ok = ok and outs[0].counts == outs[1].counts and outs[2].counts[0] == accepted[0] and sum(accepted) == n - offenders
        ok = ok and bool((outs[0].status == outs[1].status).all()) and bool((outs[0].leaf == outs[1].leaf).all())
        ok = ok and bool((outs[0].root == outs[2].root).all()) and bool((A.apply_stats() == C.apply_stats()).all())
        if r:
            for k, s in zip(names, t):
                secs[k].append(s)
    verified = ok and A.root() == B.root() == C.root() and A.size == B.size == C.size
    hashes = [int(x) for x in A.apply_stats()]
    row = dict(operations=n, inserts=int((ops_r == F.OP_INSERT).sum()), reads=int((ops_r == F.OP_READ).sum()), offenders=offenders,
               accepted_inserts=accepted[0], accepted_reads=accepted[1], leaves_before=(1 << preload) + 1, leaves_after=int(A.size),
               repeats=repeats, verified=bool(verified), apply_hashes_last_round=sum(hashes),
               sweep_hashes_last_round=accepted[0] * (2 + 2 * DEPTH) + accepted[1] * (1 + DEPTH))
    for k in names:
        row.update(summary(k, secs[k], n))
    med = {k: float(np.median(secs[k])) for k in names}
    row["apply_mixed_over_mixed_filtered_null"] = round(med[names[0]] / med[names[1]], 4)
    row["apply_mixed_over_apply_filtered_inserts"] = round(med[names[0]] / med[names[2]], 4)
    for t in trees:
        t.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--preload", type=int, default=20)
    ap.add_argument("--logn", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lines = [json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                             preload=1 << args.preload, read_every=2, flags="IMT_DEVICE_PTRS, status / leaf_index / root requested"))]
    print(lines[0], flush=True)
    a = measure(ctx, dev, args.preload, args.logn, 256, args.repeats, 0x41504D00)
    lines.append(json.dumps(dict(case="a", **a)))
    print(lines[-1], flush=True)
    rng = lambda k: f"{min(a[k + '_all_ms'])} .. {max(a[k + '_all_ms'])}"
    lines.append(f"# 2^{args.logn} operations ({a['inserts']} INSERTs, {a['reads']} READs, {a['offenders']} offenders) behind "
                 f"{a['leaves_before']} leaves, medians of {a['repeats']} with min .. max: apply_mixed_filtered "
                 f"{a['apply_mixed_filtered_ms']} ms ({rng('apply_mixed_filtered')}); mixed_filtered with ins == rd == NULL "
                 f"{a['mixed_filtered_null_ms']} ms ({rng('mixed_filtered_null')}): x{a['apply_mixed_over_mixed_filtered_null']}; "
                 f"apply_filtered of the INSERT values alone {a['apply_filtered_inserts_ms']} ms ({rng('apply_filtered_inserts')}): "
                 f"x{a['apply_mixed_over_apply_filtered_inserts']}; hashes {a['apply_hashes_last_round']} against "
                 f"{a['sweep_hashes_last_round']} of the sweep; verified {a['verified']}")
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
