#!/usr/bin/env python3
"""What overlapping witness-free batches buys a follower that applies block after block and wants every block's root:
imt_itree_apply_pipelined against the two ways there were, in one process on twin depth-32 trees.

For every block size n (default 2^10, 2^13, 2^16) three fresh trees are preloaded with the same 2^20 values and grow
through the run as a follower's does (M = leaves before the first timed block, M_end = after the last); each arm inserts
the same 2^19 values in blocks of n, `--repeats` times, timed with the host clock from the first call to the return of
the closing imt_ctx_sync:
  (a) apply       imt_itree_apply_batch(IMT_DEVICE_PTRS) per block, root_out per block
  (b) pipelined   imt_itree_apply_pipelined(IMT_DEVICE_PTRS) per block, root_out per block, one sync at the end
  (c) witness     imt_itree_insert_batch(out = NULL, IMT_DEVICE_PTRS | IMT_PIPELINE) per block -- no per-block root
Every arm is warmed with two blocks first.  Reported per n: insertions/s of each arm (median of the repeats, with min and
max), the ratios of the medians, whether the min-max ranges of (b) and (a), and of (b) and (c), are disjoint -- the
project's rule for calling a difference a gain -- the host milliseconds per block spent inside the calls of each arm, and,
from a separate pass of eight blocks with the event profiler on, milliseconds per block per profile class of (b).
Verification: the per-block roots of (b) equal those of (a), row for row, in every repeat, and the three final roots are
equal; otherwise the row says "verified": false and its figures mean nothing.  imt_version() is printed so the line says
which build was measured.

  python tools/bench_apply_pipelined.py [--sizes 10,13,16] [--repeats 3] [--preload 20] [--values 19]"""
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
WARM, PROF = 2, 8
ARMS = ("apply", "pipelined", "witness")


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def run_arm(arm, ctx, tree, vals, n, roots):
    """every block of `vals` through one arm, then one sync; returns (seconds in all, seconds inside the calls)"""
    blocks = vals.shape[0] // n
    inside = 0.0
    t0 = time.perf_counter()
    for k in range(blocks):
        v = ctypes.c_void_p(vals[k * n].data_ptr())
        r = ctypes.c_void_p(roots[k].data_ptr()) if roots is not None else None
        c0 = time.perf_counter()
        if arm == "apply":
            rc = lib.imt_itree_apply_batch(tree.h, v, n, r, F.DEVICE_PTRS)
        elif arm == "pipelined":
            rc = lib.imt_itree_apply_pipelined(tree.h, v, n, r, F.DEVICE_PTRS)
        else:
            rc = lib.imt_itree_insert_batch(tree.h, v, n, None, F.DEVICE_PTRS | F.PIPELINE)
        inside += time.perf_counter() - c0
        check(ctx, rc)
    ctx.sync()
    return time.perf_counter() - t0, inside


def profile(ctx, arm, tree, vals, n):
    prof = (ctypes.c_double * (2 * len(F.PROF_NAMES)))()
    check(ctx, lib.imt_profile_read_all(ctx.h, prof))                 # reset
    check(ctx, lib.imt_profile_enable(ctx.h, 1))
    run_arm(arm, ctx, tree, vals, n, None)
    check(ctx, lib.imt_profile_read_all(ctx.h, prof))
    check(ctx, lib.imt_profile_enable(ctx.h, 0))
    k = vals.shape[0] // n
    return {name: round(prof[2 * c] / k, 3) for c, name in enumerate(F.PROF_NAMES) if prof[2 * c + 1]}


def disjoint(x, y):
    return bool(min(x) > max(y) or min(y) > max(x))


def one_size(ctx, dev, pre, logn, values, repeats, seed):
    n, total = 1 << logn, 1 << values
    blocks = total // n
    need = pre.shape[0] + 1 + repeats * total + (WARM + PROF) * n
    trees = {arm: imt_amd.IndexedTree(ctx, DEPTH, 1 << (need - 1).bit_length()) for arm in ARMS}
    for arm in ARMS:
        check(ctx, lib.imt_itree_apply_batch(trees[arm].h, ctypes.c_void_p(pre.data_ptr()), pre.shape[0], None, F.DEVICE_PTRS))
    ctx.sync()
    warm = torch.from_numpy(bench.synth_values(WARM * n, 0, 1, seed + 1)).to(dev)
    for arm in ARMS:
        run_arm(arm, ctx, trees[arm], warm, n, None)
    M = trees["apply"].size
    rates = {arm: [] for arm in ARMS}
    host_ms = {arm: [] for arm in ARMS}
    roots = {arm: torch.zeros((blocks, 32), dtype=torch.uint8, device=dev) for arm in ("apply", "pipelined")}
    verified = True
    for r in range(repeats):
        vals = torch.from_numpy(bench.synth_values(total, 0, 1, seed + 2 + r)).to(dev)
        torch.cuda.synchronize()
        for arm in ARMS:
            secs, inside = run_arm(arm, ctx, trees[arm], vals, n, roots.get(arm))
            rates[arm].append(total / secs)
            host_ms[arm].append(1e3 * inside / blocks)
        torch.cuda.synchronize()
        verified = verified and bool((roots["apply"] == roots["pipelined"]).all().item()) and bool(roots["apply"].any().item())
        verified = verified and trees["apply"].root() == trees["pipelined"].root() == trees["witness"].root()
        del vals
    M_end = trees["apply"].size
    vals = torch.from_numpy(bench.synth_values(PROF * n, 0, 1, seed + 2 + repeats)).to(dev)
    torch.cuda.synchronize()
    classes = profile(ctx, "pipelined", trees["pipelined"], vals, n)
    for arm in ("apply", "witness"):
        run_arm(arm, ctx, trees[arm], vals, n, None)                  # the trees stay twins to the end
    verified = verified and trees["apply"].root() == trees["pipelined"].root() == trees["witness"].root()
    verified = verified and trees["apply"].size == trees["pipelined"].size == trees["witness"].size
    med = {k: float(np.median(v)) for k, v in rates.items()}
    row = dict(n=n, log2_n=logn, blocks_per_arm=blocks, M=int(M), M_end=int(M_end), repeats=repeats, verified=bool(verified))
    for arm in ARMS:
        row[arm + "_ins_per_s"] = dict(median=round(med[arm]), min=round(min(rates[arm])), max=round(max(rates[arm])))
        row[arm + "_host_ms_per_block_in_calls"] = round(float(np.median(host_ms[arm])), 4)
        row[arm + "_ms_per_block"] = round(1e3 * n / med[arm], 4)
    row["pipelined_over_apply"] = round(med["pipelined"] / med["apply"], 3)
    row["pipelined_over_witness"] = round(med["pipelined"] / med["witness"], 3)
    row["ranges_disjoint_pipelined_apply"] = disjoint(rates["pipelined"], rates["apply"])
    row["ranges_disjoint_pipelined_witness"] = disjoint(rates["pipelined"], rates["witness"])
    row["pipelined_profile_ms_per_block"] = classes
    for t in trees.values():
        t.close()
    del warm, vals, roots
    torch.cuda.empty_cache()
    return row


def table(rows):
    yield ("#  log2 n  blocks         M   (a) apply M/s [min-max]   (b) pipelined M/s [min-max]   (c) witness M/s [min-max]"
           "   b/a   b/c   host ms/block a, b, c   verified")
    for r in rows:
        cell = lambda arm: (f"{r[arm + '_ins_per_s']['median'] / 1e6:7.3f} [{r[arm + '_ins_per_s']['min'] / 1e6:.3f}-"  # noqa: E731
                            f"{r[arm + '_ins_per_s']['max'] / 1e6:.3f}]")
        mark = lambda d: "" if d else "~"                                                                                     # noqa: E731
        yield (f"#  {r['log2_n']:>6} {r['blocks_per_arm']:>7} {r['M']:>9}   {cell('apply'):>24}   {cell('pipelined'):>27}   {cell('witness'):>24}"
               f"  {r['pipelined_over_apply']:>4.2f}{mark(r['ranges_disjoint_pipelined_apply'])}"
               f"  {r['pipelined_over_witness']:>4.2f}{mark(r['ranges_disjoint_pipelined_witness'])}"
               f"   {r['apply_host_ms_per_block_in_calls']:.3f}, {r['pipelined_host_ms_per_block_in_calls']:.3f},"
               f" {r['witness_host_ms_per_block_in_calls']:.3f}   {r['verified']}")
    yield "#  (~ behind a ratio: the min-max ranges of the two arms overlap, so the difference is not called a gain or a loss)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,13,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--preload", type=int, default=20)
    ap.add_argument("--values", type=int, default=19)
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                          preload=1 << args.preload, values_per_arm=1 << args.values,
                          apply="imt_itree_apply_batch(IMT_DEVICE_PTRS), root_out per block",
                          pipelined="imt_itree_apply_pipelined(IMT_DEVICE_PTRS), root_out per block, one sync",
                          witness="imt_itree_insert_batch(out=NULL, IMT_DEVICE_PTRS | IMT_PIPELINE)")), flush=True)
    pre = torch.from_numpy(bench.synth_values(1 << args.preload, 0, 1, 0x41505000)).to(dev)
    rows = []
    for k, logn in enumerate(sizes):
        rows.append(one_size(ctx, dev, pre, logn, args.values, args.repeats, 0x41505010 + 16 * k))
        print(json.dumps(rows[-1]), flush=True)
    for line in table(rows):
        print(line)
    ctx.close()


if __name__ == "__main__":
    main()
