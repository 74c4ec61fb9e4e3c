#!/usr/bin/env python3
"""What witness-free insertion buys: imt_itree_apply_batch against the fastest way to the same tree without it,
imt_itree_insert_batch(out = NULL, IMT_DEVICE_PTRS | IMT_PIPELINE), in one process on twin depth-32 trees.

For every batch size n (default 2^13, 2^16, 2^18, 2^20): two fresh trees preloaded with the same 2^20 values, with the
capacity the whole run of that size needs, so the trees grow through the run as a follower's does (M = leaves before
the first timed batch and M_end = leaves after the last one are printed per row; the hashes per insertion are
the last batch's, at M_end).  Both arms are warmed with two batches; the second apply batch sizes the
arms: B = max(10, what fills 1.1 s of the faster arm).  Then `--repeats` times: B baseline batches on tree A closed by
imt_ctx_sync, timed with the host clock; the same B batches through apply on tree T, the same way; and once more on a
third twin with IMT_INPUTS_READY added (apply_inputs_ready: the next batch's preparation beside this batch's hashing
instead of behind it -- reported, not part of the comparison).  The trees stay
twins, so after the timed loop their roots must be equal: otherwise the row says "verified": false and its figures
mean nothing.  Reported per n: insertions/s of both arms (median of the repeats), their ratio, the min-max spread of
each arm over the repeats relative to its median, whether apply is faster by more than twice the larger spread,
hashes per insertion (sum(apply_stats()) / n of the last batch) beside the witness sweep's 2 + 2 * depth, and -- from a
separate pass of three batches per arm with the event profiler on -- milliseconds per batch per profile class.
The baseline is this library's own unchanged witness path, timed in the same process; imt_version() is printed so the
line says which build was measured.

  python tools/bench_apply.py [--sizes 13,16,18,20] [--repeats 3] [--preload 20]"""
import argparse
import ctypes
import importlib.util
import json
import math
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
WARM, PROF = 2, 3


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def baseline(ctx, tree, vals, n):
    for k in range(vals.shape[0] // n):
        check(ctx, lib.imt_itree_insert_batch(tree.h, ctypes.c_void_p(vals[k * n].data_ptr()), n, None,
                                              F.DEVICE_PTRS | F.PIPELINE))
    ctx.sync()


def apply(ctx, tree, vals, n, flags=F.DEVICE_PTRS):
    for k in range(vals.shape[0] // n):
        check(ctx, lib.imt_itree_apply_batch(tree.h, ctypes.c_void_p(vals[k * n].data_ptr()), n, None, flags))
    ctx.sync()


def apply_ready(ctx, tree, vals, n):
    """the caller vouches that the value buffers are idle: the next batch's preparation then runs on the side stream
    beside this batch's hashing instead of behind it (an apply batch hashes on the context's stream)"""
    apply(ctx, tree, vals, n, F.DEVICE_PTRS | F.INPUTS_READY)


def timed(fn, *a):
    t0 = time.perf_counter()
    fn(*a)
    return time.perf_counter() - t0


def profile(ctx, fn, tree, vals, n):
    prof = (ctypes.c_double * (2 * len(F.PROF_NAMES)))()
    check(ctx, lib.imt_profile_read_all(ctx.h, prof))                 # reset
    check(ctx, lib.imt_profile_enable(ctx.h, 1))
    fn(ctx, tree, vals, n)
    check(ctx, lib.imt_profile_read_all(ctx.h, prof))
    check(ctx, lib.imt_profile_enable(ctx.h, 0))
    k = vals.shape[0] // n
    return {name: round(prof[2 * c] / k, 3) for c, name in enumerate(F.PROF_NAMES) if prof[2 * c + 1]}


def one_size(ctx, dev, preload, logn, repeats, seed):
    n = 1 << logn
    pre = torch.from_numpy(bench.synth_values(1 << preload, 0, 1, seed)).to(dev)
    # a generous capacity first (the arms are sized after the warm-up): 2^26 leaves, more only if the run needs it
    warm = torch.from_numpy(bench.synth_values(WARM * n, 0, 1, seed + 1)).to(dev)
    probe = imt_amd.IndexedTree(ctx, DEPTH, 1 << max(preload + 1, logn + 2))
    apply(ctx, probe, pre, 1 << preload)
    apply(ctx, probe, warm[:n], n)
    t_apply = timed(apply, ctx, probe, warm[n:], n)
    probe.close()
    B = max(10, math.ceil(1.1 / t_apply))
    total = (1 << preload) + 1 + (WARM + repeats * B + PROF) * n
    cap = 1 << max(26, (total - 1).bit_length())
    A, T, R = (imt_amd.IndexedTree(ctx, DEPTH, cap) for _ in range(3))
    for t in (A, T, R):
        apply(ctx, t, pre, 1 << preload)
    baseline(ctx, A, warm, n)
    apply(ctx, T, warm, n)
    apply_ready(ctx, R, warm, n)
    M = A.size
    rates = dict(baseline=[], apply=[], apply_inputs_ready=[])
    for r in range(repeats):
        vals = torch.from_numpy(bench.synth_values(B * n, 0, 1, seed + 2 + r)).to(dev)
        torch.cuda.synchronize()
        rates["baseline"].append(B * n / timed(baseline, ctx, A, vals, n))
        rates["apply"].append(B * n / timed(apply, ctx, T, vals, n))
        rates["apply_inputs_ready"].append(B * n / timed(apply_ready, ctx, R, vals, n))
        del vals
    stats, M_end = T.apply_stats(), T.size
    verified = A.root() == T.root() == R.root() and A.size == T.size == R.size
    vals = torch.from_numpy(bench.synth_values(PROF * n, 0, 1, seed + 2 + repeats)).to(dev)
    classes = dict(baseline=profile(ctx, baseline, A, vals, n), apply=profile(ctx, apply, T, vals, n))
    verified = verified and A.root() == T.root()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in rates.items()}
    ratio = med["apply"] / med["baseline"]
    spread_gate = max(spread["baseline"], spread["apply"])
    row = dict(n=n, log2_n=logn, M=int(M), M_end=int(M_end), batches_per_arm=B, repeats=repeats, verified=bool(verified),
               baseline_ins_per_s=round(med["baseline"]), apply_ins_per_s=round(med["apply"]), ratio=round(ratio, 3),
               baseline_spread=round(spread["baseline"], 4), apply_spread=round(spread["apply"], 4),
               faster_beyond_twice_spread=bool(ratio - 1 > 2 * spread_gate),
               apply_inputs_ready_ins_per_s=round(med["apply_inputs_ready"]),
               ratio_inputs_ready=round(med["apply_inputs_ready"] / med["baseline"], 3),
               apply_inputs_ready_spread=round(spread["apply_inputs_ready"], 4),
               baseline_ms_per_batch=round(1e3 * n / med["baseline"], 3), apply_ms_per_batch=round(1e3 * n / med["apply"], 3),
               hashes_per_insertion=round(float(stats.sum()) / n, 3), witness_hashes_per_insertion=2 + 2 * DEPTH,
               hash_ratio=round((2 + 2 * DEPTH) * n / float(stats.sum()), 2),
               all_rates=dict((k, [round(x) for x in v]) for k, v in rates.items()), profile_ms_per_batch=classes)
    for t in (A, T, R):
        t.close()
    del pre, warm, vals
    torch.cuda.empty_cache()
    return row


def table(rows):
    yield ("#  log2 n         M     M_end   baseline M/s  (spread)   apply M/s  (spread)   ratio   +INPUTS_READY M/s  ratio"
           "   hashes/ins  hash ratio  verified")
    for r in rows:
        yield (f"#  {r['log2_n']:>6} {r['M']:>9} {r['M_end']:>9} {r['baseline_ins_per_s'] / 1e6:>12.3f}  ({100 * r['baseline_spread']:.2f} %)"
               f" {r['apply_ins_per_s'] / 1e6:>10.3f}  ({100 * r['apply_spread']:.2f} %) {r['ratio']:>7.2f}"
               f" {r['apply_inputs_ready_ins_per_s'] / 1e6:>17.3f} {r['ratio_inputs_ready']:>7.2f} {r['hashes_per_insertion']:>11.2f}"
               f" {r['hash_ratio']:>10.2f}  {r['verified']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="13,16,18,20")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--preload", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                          preload=1 << args.preload,
                          baseline="imt_itree_insert_batch(out=NULL, IMT_DEVICE_PTRS | IMT_PIPELINE)",
                          apply="imt_itree_apply_batch(IMT_DEVICE_PTRS)")), flush=True)
    rows = []
    for k, logn in enumerate(int(x) for x in args.sizes.split(",")):
        rows.append(one_size(ctx, dev, args.preload, logn, args.repeats, 0x41504C00 + 16 * k))
        print(json.dumps(rows[-1]), flush=True)
    for line in table(rows):
        print(line)
    ctx.close()


if __name__ == "__main__":
    main()
