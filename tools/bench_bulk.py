#!/usr/bin/env python3
"""What the bulk witness form costs against the sequential one: imt_itree_insert_bulk against imt_itree_insert_batch, in
one process on twin depth-32 trees.

For every batch size n (default 2^10, 2^13, 2^16) three fresh trees are preloaded with the same 2^20 values and grow
through the run (M = leaves before the first timed batch); each arm inserts the same 2^`--values` values in batches of n,
`--repeats` times, every output of the call written to device memory, timed with the host clock from the first call to
the return of the closing imt_ctx_sync:
  (a) bulk        imt_itree_insert_bulk(all ten outputs, IMT_DEVICE_PTRS)
  (b) witness     imt_itree_insert_batch(all nine outputs, IMT_DEVICE_PTRS)
  (c) pipelined   imt_itree_insert_batch(all nine outputs, IMT_DEVICE_PTRS | IMT_PIPELINE): the rate a caller has today
Every arm is warmed with two batches first.  Reported per n: insertions/s of each arm (median of the repeats, min and
max), the ratios of the medians, whether the min-max ranges are disjoint -- the project's rule for calling a difference a
gain or a loss --, the host milliseconds per batch inside the calls, and, from a separate pass with the event profiler on,
milliseconds per batch per profile class of (a): the APPLY_* classes are the append stage alone.  The hash counts are
stated, not measured: n * (1 + depth) for the sweep, imt_itree_apply_stats for the append of the last batch.
Verification: the three final roots and sizes are equal after every repeat; otherwise the row says "verified": false and
its figures mean nothing.

  python tools/bench_bulk.py [--sizes 10,13,16] [--repeats 3] [--preload 20] [--values 19]"""
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
WARM, PROF = 2, 4
ARMS = ("bulk", "witness", "pipelined")


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def buffers(dev, n):
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)                     # noqa: E731
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)                             # noqa: E731
    bulk = dict(order=i64(n), low_index=i64(n), low_leaf=u8(n, 3, 32), is_largest=u8(n), root_before=u8(n, 32),
                root_after=u8(n, 32), low_sib=u8(DEPTH, n, 32), new_leaf=u8(n, 3, 32), append_sib=u8(DEPTH, 32), root=u8(32))
    ins = dict(low_index=i64(n), low_leaf=u8(n, 3, 32), is_largest=u8(n), old_root=u8(n, 32), interim_root=u8(n, 32),
               new_root=u8(n, 32), new_leaf=u8(n, 3, 32), low_sib=u8(DEPTH, n, 32), new_sib=u8(DEPTH, n, 32))
    return (bulk, F.BulkOut(**{k: t.data_ptr() for k, t in bulk.items()})), (ins, F.InsertOut(**{k: t.data_ptr() for k, t in ins.items()}))


def run_arm(arm, ctx, tree, vals, n, outs):
    """every batch of `vals` through one arm, then one sync; returns (seconds in all, seconds inside the calls)"""
    (_, bulk_out), (_, ins_out) = outs
    inside = 0.0
    t0 = time.perf_counter()
    for k in range(vals.shape[0] // n):
        v = ctypes.c_void_p(vals[k * n].data_ptr())
        c0 = time.perf_counter()
        if arm == "bulk":
            rc = lib.imt_itree_insert_bulk(tree.h, v, n, ctypes.byref(bulk_out), F.DEVICE_PTRS)
        else:
            rc = lib.imt_itree_insert_batch(tree.h, v, n, ctypes.byref(ins_out),
                                            F.DEVICE_PTRS | (F.PIPELINE if arm == "pipelined" else 0))
        inside += time.perf_counter() - c0
        check(ctx, rc)
    ctx.sync()
    return time.perf_counter() - t0, inside


def profile(ctx, arm, tree, vals, n, outs):
    prof = (ctypes.c_double * (2 * len(F.PROF_NAMES)))()
    check(ctx, lib.imt_profile_read_all(ctx.h, prof))                 # reset
    check(ctx, lib.imt_profile_enable(ctx.h, 1))
    run_arm(arm, ctx, tree, vals, n, outs)
    check(ctx, lib.imt_profile_read_all(ctx.h, prof))
    check(ctx, lib.imt_profile_enable(ctx.h, 0))
    k = vals.shape[0] // n
    return {name: round(prof[2 * c] / k, 3) for c, name in enumerate(F.PROF_NAMES) if prof[2 * c + 1]}


def disjoint(x, y):
    return bool(min(x) > max(y) or min(y) > max(x))


def one_size(ctx, dev, pre, logn, values, repeats, seed):
    n = 1 << logn
    total = max(1 << values, 4 * n)
    batches = total // n
    need = pre.shape[0] + 1 + repeats * total + (WARM + PROF) * n
    trees = {arm: imt_amd.IndexedTree(ctx, DEPTH, 1 << (need - 1).bit_length()) for arm in ARMS}
    for arm in ARMS:
        check(ctx, lib.imt_itree_apply_batch(trees[arm].h, ctypes.c_void_p(pre.data_ptr()), pre.shape[0], None, F.DEVICE_PTRS))
    ctx.sync()
    outs = buffers(dev, n)
    warm = torch.from_numpy(bench.synth_values(WARM * n, 0, 1, seed + 1)).to(dev)
    for arm in ARMS:
        run_arm(arm, ctx, trees[arm], warm, n, outs)
    M = trees["bulk"].size
    rates = {arm: [] for arm in ARMS}
    host_ms = {arm: [] for arm in ARMS}
    same = lambda: (trees["bulk"].root() == trees["witness"].root() == trees["pipelined"].root() and                # noqa: E731
                    trees["bulk"].size == trees["witness"].size == trees["pipelined"].size)
    verified = same()
    for r in range(repeats):
        vals = torch.from_numpy(bench.synth_values(total, 0, 1, seed + 2 + r)).to(dev)
        torch.cuda.synchronize()
        for arm in ARMS:
            secs, inside = run_arm(arm, ctx, trees[arm], vals, n, outs)
            rates[arm].append(total / secs)
            host_ms[arm].append(1e3 * inside / batches)
        torch.cuda.synchronize()
        verified = verified and same()
        del vals
    vals = torch.from_numpy(bench.synth_values(PROF * n, 0, 1, seed + 2 + repeats)).to(dev)
    torch.cuda.synchronize()
    classes = profile(ctx, "bulk", trees["bulk"], vals, n, outs)
    append_hashes = int(trees["bulk"].apply_stats().sum())
    for arm in ("witness", "pipelined"):
        run_arm(arm, ctx, trees[arm], vals, n, outs)
    verified = verified and same()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    row = dict(n=n, log2_n=logn, batches_per_arm=batches, M=int(M), repeats=repeats, verified=bool(verified))
    for arm in ARMS:
        row[arm + "_ins_per_s"] = dict(median=round(med[arm]), min=round(min(rates[arm])), max=round(max(rates[arm])))
        row[arm + "_host_ms_per_batch_in_calls"] = round(float(np.median(host_ms[arm])), 4)
        row[arm + "_ms_per_batch"] = round(1e3 * n / med[arm], 4)
    row["bulk_over_witness"] = round(med["bulk"] / med["witness"], 3)
    row["bulk_over_pipelined"] = round(med["bulk"] / med["pipelined"], 3)
    row["ranges_disjoint_bulk_witness"] = disjoint(rates["bulk"], rates["witness"])
    row["ranges_disjoint_bulk_pipelined"] = disjoint(rates["bulk"], rates["pipelined"])
    row["bulk_profile_ms_per_batch"] = classes
    row["bulk_append_stage_ms_per_batch"] = round(sum(v for k, v in classes.items() if k.startswith("apply_")), 3)
    row["hashes_per_batch"] = dict(bulk_sweep=n * (1 + DEPTH), bulk_append_last_batch=append_hashes, witness=n * (2 + 2 * DEPTH))
    for t in trees.values():
        t.close()
    del warm, vals, outs
    torch.cuda.empty_cache()
    return row


def table(rows):
    yield ("#  log2 n  batches         M   (a) bulk M/s [min-max]   (b) witness M/s [min-max]   (c) pipelined M/s [min-max]"
           "   a/b   a/c   host ms/batch a, b, c   append ms/batch   verified")
    for r in rows:
        cell = lambda arm: (f"{r[arm + '_ins_per_s']['median'] / 1e6:7.3f} [{r[arm + '_ins_per_s']['min'] / 1e6:.3f}-"  # noqa: E731
                            f"{r[arm + '_ins_per_s']['max'] / 1e6:.3f}]")
        mark = lambda d: "" if d else "~"                                                                                     # noqa: E731
        yield (f"#  {r['log2_n']:>6} {r['batches_per_arm']:>8} {r['M']:>9}   {cell('bulk'):>22}   {cell('witness'):>25}   {cell('pipelined'):>27}"
               f"  {r['bulk_over_witness']:>4.2f}{mark(r['ranges_disjoint_bulk_witness'])}"
               f"  {r['bulk_over_pipelined']:>4.2f}{mark(r['ranges_disjoint_bulk_pipelined'])}"
               f"   {r['bulk_host_ms_per_batch_in_calls']:.3f}, {r['witness_host_ms_per_batch_in_calls']:.3f},"
               f" {r['pipelined_host_ms_per_batch_in_calls']:.3f}   {r['bulk_append_stage_ms_per_batch']:>15.3f}   {r['verified']}")
    yield "#  (~ behind a ratio: the min-max ranges of the two arms overlap, so the difference is not called a gain or a loss)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,13,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--preload", type=int, default=20)
    ap.add_argument("--values", type=int, default=19)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                          preload=1 << args.preload, values_per_arm=1 << args.values,
                          bulk="imt_itree_insert_bulk(all outputs, IMT_DEVICE_PTRS)",
                          witness="imt_itree_insert_batch(all outputs, IMT_DEVICE_PTRS)",
                          pipelined="imt_itree_insert_batch(all outputs, IMT_DEVICE_PTRS | IMT_PIPELINE)")), flush=True)
    pre = torch.from_numpy(bench.synth_values(1 << args.preload, 0, 1, 0x42554C4B)).to(dev)
    rows = []
    for k, logn in enumerate(int(x) for x in args.sizes.split(",")):
        rows.append(one_size(ctx, dev, pre, logn, args.values, args.repeats, 0x42554C50 + 16 * k))
        print(json.dumps(rows[-1]), flush=True)
    for line in table(rows):
        print(line)
    ctx.close()


if __name__ == "__main__":
    main()
