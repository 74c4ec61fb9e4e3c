#!/usr/bin/env python3
"""What the bulk witness of a block applied earlier costs: imt_itree_view_bulk_witness against the other ways to the same
or a comparable witness, in one process on depth-32 trees.

A tree is preloaded with 2^`--preload` values (S = leaves before the block), then for every block size n (default 2^10,
2^13, 2^16) the block goes in with imt_itree_apply_batch and the tree moves 2^`--ahead` leaves past it.  Four arms produce
witnesses of that block, every output written to device memory (IMT_DEVICE_PTRS), timed with the host clock from the call
to the return of the closing imt_ctx_sync, `--repeats` times after six warm-up rounds (a tree rotates over five plan sets
and allocates each at its first use; the warm-up takes every arm past that):
  (a) replay      imt_itree_view_bulk_witness(n) through a view at S (built before the clock starts)
  (b) live        imt_itree_insert_bulk of the same block on a twin of S leaves (rewound to S between the repeats, untimed)
  (c) load+bulk   imt_itree_load of a device-resident snapshot of the S leaves into a second tree, then
                  imt_itree_insert_bulk there: the only route to a late bulk witness before the replay existed
  (d) other form  imt_itree_view_insert_witness(n) through the same view: the two-paths-per-insertion witness
and the view's one-off build (the first query of a fresh view at S) is timed beside them.  Reported per n: milliseconds
per block of each arm (median, min and max of the repeats), the ratios of the medians, and whether the min-max ranges are
disjoint -- the project's rule for calling a difference a gain or a loss.  The hash counts are stated, not measured:
n * (1 + depth) for the sweep of (a), (b), (c); n leaves plus one hash per distinct node of the range at every level until
one node is left plus that node's path for the append of (a).
Verification: (a) and (b) write the same bytes in all ten arrays, and the replayed root is the root the tree reported for
the block; otherwise the row says "verified": false and its figures mean nothing.

  python tools/bench_replay_bulk.py [--sizes 10,13,16] [--repeats 3] [--preload 20] [--ahead 16]"""
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
ARMS = ("replay", "live", "load_bulk", "other_form")
WARM = 6


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def buffers(dev, n):
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)                     # noqa: E731
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)                             # noqa: E731
    bulk = dict(order=i64(n), low_index=i64(n), low_leaf=u8(n, 3, 32), is_largest=u8(n), root_before=u8(n, 32),
                root_after=u8(n, 32), low_sib=u8(DEPTH, n, 32), new_leaf=u8(n, 3, 32), append_sib=u8(DEPTH, 32), root=u8(32))
    ins = dict(low_index=i64(n), low_leaf=u8(n, 3, 32), is_largest=u8(n), old_root=u8(n, 32), interim_root=u8(n, 32),
               new_root=u8(n, 32), new_leaf=u8(n, 3, 32), low_sib=u8(DEPTH, n, 32), new_sib=u8(DEPTH, n, 32))
    return (bulk, F.BulkOut(**{k: t.data_ptr() for k, t in bulk.items()})), (ins, F.InsertOut(**{k: t.data_ptr() for k, t in ins.items()}))


def timed(ctx, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0)


def disjoint(x, y):
    return bool(min(x) > max(y) or min(y) > max(x))


def append_hashes(S, n):
    total, l = n, 0                                         # the leaves, then every distinct node of the range per level
    while ((S + n - 1) >> l) != (S >> l):
        l += 1
        total += ((S + n - 1) >> l) - (S >> l) + 1
    return total + (DEPTH - l)                              # and the path of the one node that is left


def one_size(ctx, dev, pre, snap, logn, ahead, repeats, seed):
    n, S = 1 << logn, pre.shape[0] + 1
    cap = 1 << (S + n + (1 << ahead)).bit_length()
    block = torch.from_numpy(bench.synth_values(n, 0, 1, seed)).to(dev)
    more = torch.from_numpy(bench.synth_values(1 << ahead, 0, 1, seed + 1)).to(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                                # noqa: E731
    tree, twin, second = (imt_amd.IndexedTree(ctx, DEPTH, cap) for _ in range(3))
    root_of_block = torch.zeros(32, dtype=torch.uint8, device=dev)
    for t in (tree, twin):
        check(ctx, lib.imt_itree_apply_batch(t.h, P(pre), pre.shape[0], None, F.DEVICE_PTRS))
    check(ctx, lib.imt_itree_apply_batch(tree.h, P(block), n, P(root_of_block), F.DEVICE_PTRS))
    check(ctx, lib.imt_itree_apply_batch(tree.h, P(more), more.shape[0], None, F.DEVICE_PTRS))
    ctx.sync()
    (bulk, bulk_out), (ins, ins_out) = buffers(dev, n)
    (bulk2, bulk_out2), _ = buffers(dev, n)
    view = tree.view(S)
    build_ms = timed(ctx, view.root)                        # the first query builds the side table
    probe = tree.view(S)
    build_ms = min(build_ms, timed(ctx, probe.root))
    probe.close()

    def replay():
        check(ctx, lib.imt_itree_view_bulk_witness(view.h, n, ctypes.byref(bulk_out), F.DEVICE_PTRS))

    def live():
        check(ctx, lib.imt_itree_insert_bulk(twin.h, P(block), n, ctypes.byref(bulk_out2), F.DEVICE_PTRS))

    def load_bulk():
        check(ctx, lib.imt_itree_load(second.h, P(snap), S, F.DEVICE_PTRS))
        check(ctx, lib.imt_itree_insert_bulk(second.h, P(block), n, ctypes.byref(bulk_out2), F.DEVICE_PTRS))

    def other_form():
        check(ctx, lib.imt_itree_view_insert_witness(view.h, n, ctypes.byref(ins_out), F.DEVICE_PTRS))

    arms = dict(replay=replay, live=live, load_bulk=load_bulk, other_form=other_form)
    ms = {a: [] for a in ARMS}
    verified = True
    for r in range(WARM + repeats):
        for a in ARMS:
            t = timed(ctx, arms[a])
            if r >= WARM:
                ms[a].append(t)
            if a == "live":
                verified = verified and all(bool((bulk[k] == bulk2[k]).all()) for k in bulk)
                twin.rewind(S)
        verified = verified and bool((bulk["root"] == root_of_block).all())
    med = {a: float(np.median(v)) for a, v in ms.items()}
    row = dict(n=n, log2_n=logn, S=S, tree_size=tree.size, repeats=repeats, verified=bool(verified),
               view_build_ms=round(build_ms, 3))
    for a in ARMS:
        row[a + "_ms"] = dict(median=round(med[a], 3), min=round(min(ms[a]), 3), max=round(max(ms[a]), 3))
    for a in ARMS[1:]:
        row["replay_over_" + a] = round(med["replay"] / med[a], 3)
        row["ranges_disjoint_replay_" + a] = disjoint(ms["replay"], ms[a])
    row["replay_M_per_s"] = round(n / med["replay"] / 1e3, 3)
    row["hashes_per_block"] = dict(sweep=n * (1 + DEPTH), replay_append=append_hashes(S, n), other_form=n * (2 + 2 * DEPTH))
    view.close()
    for t in (tree, twin, second):
        t.close()
    del block, more, bulk, bulk2, ins
    torch.cuda.empty_cache()
    return row


def table(rows):
    yield ("#  log2 n        S   view build ms   (a) replay ms [min-max]   (b) live ms [min-max]   (c) load+bulk ms [min-max]"
           "   (d) other form ms [min-max]   a/b   a/c   a/d   verified")
    for r in rows:
        cell = lambda a: f"{r[a + '_ms']['median']:8.3f} [{r[a + '_ms']['min']:.3f}-{r[a + '_ms']['max']:.3f}]"               # noqa: E731
        ratio = lambda a: f"{r['replay_over_' + a]:>4.2f}{'' if r['ranges_disjoint_replay_' + a] else '~'}"                    # noqa: E731
        yield (f"#  {r['log2_n']:>6} {r['S']:>8}   {r['view_build_ms']:>13.3f}   {cell('replay'):>23}   {cell('live'):>21}   "
               f"{cell('load_bulk'):>26}   {cell('other_form'):>27}  {ratio('live')}  {ratio('load_bulk')}  {ratio('other_form')}"
               f"   {r['verified']}")
    yield "#  (~ behind a ratio: the min-max ranges of the two arms overlap, so the difference is not called a gain or a loss)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,13,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--preload", type=int, default=20)
    ap.add_argument("--ahead", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                          preload=1 << args.preload, ahead=1 << args.ahead,
                          replay="imt_itree_view_bulk_witness(all outputs, IMT_DEVICE_PTRS)",
                          live="imt_itree_insert_bulk(all outputs, IMT_DEVICE_PTRS) on a twin",
                          load_bulk="imt_itree_load(device snapshot) + imt_itree_insert_bulk on a second tree",
                          other_form="imt_itree_view_insert_witness(all outputs, IMT_DEVICE_PTRS)")), flush=True)
    pre = torch.from_numpy(bench.synth_values(1 << args.preload, 0, 1, 0x52424C4B)).to(dev)
    # the snapshot of the tree as of S, device-resident: what route (c) starts from
    t0 = imt_amd.IndexedTree(ctx, DEPTH, 1 << (pre.shape[0] + 1).bit_length())
    check(ctx, lib.imt_itree_apply_batch(t0.h, ctypes.c_void_p(pre.data_ptr()), pre.shape[0], None, F.DEVICE_PTRS))
    snap = torch.zeros((t0.size, 3, 32), dtype=torch.uint8, device=dev)
    t0.snapshot_into(snap.data_ptr())
    ctx.sync()
    t0.close()
    rows = []
    for k, logn in enumerate(int(x) for x in args.sizes.split(",")):
        rows.append(one_size(ctx, dev, pre, snap, logn, args.ahead, args.repeats, 0x52424C50 + 16 * k))
        print(json.dumps(rows[-1]), flush=True)
    for line in table(rows):
        print(line)
    ctx.close()


if __name__ == "__main__":
    main()
