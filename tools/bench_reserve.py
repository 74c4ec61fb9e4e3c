#!/usr/bin/env python3
"""What a larger capacity costs: imt_itree_reserve against the only other route to the same tree, in one process on
depth-32 trees.

For every size (default 2^20 and 2^24 leaves; --sizes 20,24) a tree holds S leaves at capacity S -- it is full -- and two
arms double its room, `--repeats` times after one dropped warm-up round, swapping places from round to round:

  (a) reserve      imt_itree_reserve(T, 2 S, 0);
  (b) move         imt_itree_get_values(T) into a device buffer, imt_itree_new at 2 S, imt_itree_load_values of the
                   buffer (IMT_DEVICE_PTRS), imt_itree_free(T): the route without (a).  The buffer exists before the
                   clock starts.

Each arm is timed with the host clock from its first call to the point where the tree of capacity 2 S is complete on the
device; both arms return to capacity S outside the timed region (imt_itree_reserve(T, S, 0)), and the roots of the two
trees must be equal after every round: otherwise the row says "verified": false and its figures mean nothing.

For (a) the library reports where the call spent its time (imt_itree_reserve_stats): the kernel that moves the nodes
(device time) and hipMalloc + hipFree (host time).  The kernel's traffic is 32 bytes written per node of the new layout
plus 32 bytes read per node the old layout has; it is set beside the 6.29 TB/s a float4 copy reaches on this GPU
(MI355X_MICROARCH.md's figure, not measured here).

The shrink is reported too: a tree of 2^hi leaves rewound to 2^lo (--shrink 24,20; outside the clock) gives its memory
back with imt_itree_reserve(T, 2^lo, 0).

  python tools/bench_reserve.py [--sizes 20,24] [--repeats 3] [--shrink 24,20]"""
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
COPY_TBS = 6.29


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def P_(t):
    return ctypes.c_void_p(t.data_ptr())


def level_len(cap, l):
    return max(1, cap >> l)


def kernel_bytes(old_cap, new_cap):
    """32 bytes written per node of the new layout, 32 read per node that comes from the old one"""
    written = sum(level_len(new_cap, l) for l in range(DEPTH + 1))
    read = sum(min(level_len(old_cap, l), level_len(new_cap, l)) for l in range(DEPTH + 1))
    return 32 * (written + read)


def full_tree(ctx, dev, S, seed):
    vals = torch.from_numpy(bench.synth_values(S - 1, 0, 1, seed)).to(dev)
    t = imt_amd.IndexedTree(ctx, DEPTH, S)
    check(ctx, lib.imt_itree_load_values(t.h, P_(vals), S - 1, None, F.DEVICE_PTRS))
    ctx.sync()
    return t, vals


def summary(ms):
    return round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)


def one_size(ctx, dev, logs, repeats, seed):
    S = 1 << logs
    A, vals = full_tree(ctx, dev, S, seed)
    B, _ = full_tree(ctx, dev, S, seed)
    del vals
    buf = torch.empty((S - 1, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    root = A.root()
    ms = dict(a=[], b=[], kernel=[], mem=[])
    verified = B.root() == root
    for r in range(repeats + 1):                         # the first round warms both arms and is dropped
        t = {}

        def arm_a():
            t0 = time.perf_counter()
            check(ctx, lib.imt_itree_reserve(A.h, 2 * S, 0))
            t["a"] = 1e3 * (time.perf_counter() - t0)
            t["stats"] = A.reserve_stats()

        def arm_b():
            nonlocal B
            t0 = time.perf_counter()
            check(ctx, lib.imt_itree_get_values(B.h, 1, S - 1, P_(buf), F.DEVICE_PTRS))
            new = imt_amd.IndexedTree(ctx, DEPTH, 2 * S)
            check(ctx, lib.imt_itree_load_values(new.h, P_(buf), S - 1, None, F.DEVICE_PTRS))
            B.close()
            ctx.sync()
            t["b"] = 1e3 * (time.perf_counter() - t0)
            B = new

        for arm in ((arm_a, arm_b) if r % 2 else (arm_b, arm_a)):
            arm()
        verified = (verified and A.root() == B.root() == root and A.size == B.size == S
                    and A.capacity == B.capacity == 2 * S)
        A.reserve(S)                                     # back to the full tree, outside the clock
        B.reserve(S)
        verified = verified and A.root() == B.root() == root and A.capacity == B.capacity == S
        if r:
            ms["a"].append(t["a"])
            ms["b"].append(t["b"])
            ms["kernel"].append(t["stats"][1])
            ms["mem"].append(t["stats"][2])
    nbytes = kernel_bytes(S, 2 * S)
    row = dict(log2_size=logs, leaves=S, repeats=repeats, verified=bool(verified))
    for k, name in (("a", "reserve"), ("b", "move"), ("kernel", "reserve_kernel"), ("mem", "reserve_malloc_free")):
        med, lo, hi = summary(ms[k])
        row.update({f"{name}_ms": med, f"{name}_min_ms": lo, f"{name}_max_ms": hi, f"{name}_all_ms": [round(x, 3) for x in ms[k]]})
    kmed = float(np.median(ms["kernel"]))
    row.update(move_over_reserve=round(row["move_ms"] / row["reserve_ms"], 2),
               move_over_reserve_range=[round(min(ms["b"]) / max(ms["a"]), 2), round(max(ms["b"]) / min(ms["a"]), 2)],
               reserve_faster_spreads_disjoint=bool(max(ms["a"]) < min(ms["b"])),
               kernel_bytes=nbytes, kernel_TBs=round(nbytes / (kmed * 1e-3) / 1e12, 3) if kmed > 0 else None,
               copy_TBs_guide=COPY_TBS,
               malloc_free_share=round(float(np.median(ms["mem"])) / row["reserve_ms"], 3))
    print(json.dumps(row), flush=True)
    A.close()
    B.close()
    del buf
    torch.cuda.empty_cache()
    return row


def shrink(ctx, dev, hi, lo, repeats, seed):
    """2^hi leaves at capacity 2^hi, rewound to 2^lo: the capacity follows"""
    H, L = 1 << hi, 1 << lo
    T, vals = full_tree(ctx, dev, H, seed)
    ms, kernel, mem = [], [], []
    verified = True
    for r in range(repeats + 1):
        root = T.rewind(L)
        t0 = time.perf_counter()
        check(ctx, lib.imt_itree_reserve(T.h, L, 0))
        dt = 1e3 * (time.perf_counter() - t0)
        st = T.reserve_stats()
        verified = verified and T.root() == root and T.capacity == L and T.size == L
        T.reserve(H)                                     # and up again with the dropped values, outside the clock
        check(ctx, lib.imt_itree_load_values(T.h, P_(vals), H - 1, None, F.DEVICE_PTRS))
        ctx.sync()
        if r:
            ms.append(dt)
            kernel.append(st[1])
            mem.append(st[2])
    med, mn, mx = summary(ms)
    row = dict(shrink_from_log2=hi, shrink_to_log2=lo, repeats=repeats, verified=bool(verified), shrink_ms=med, shrink_min_ms=mn,
               shrink_max_ms=mx, shrink_all_ms=[round(x, 3) for x in ms], shrink_kernel_ms=summary(kernel)[0],
               shrink_malloc_free_ms=summary(mem)[0], kernel_bytes=kernel_bytes(H, L))
    print(json.dumps(row), flush=True)
    T.close()
    del vals
    torch.cuda.empty_cache()
    return row


def table(rows, srow):
    yield ("#  log2 size   (a) reserve ms (min - max)      (b) move ms (min - max)      b / a (range)        a<b disjoint"
           "   kernel ms   kernel TB/s (copy: 6.29)   malloc+free ms (share of a)  verified")
    for r in rows:
        yield (f"#  {r['log2_size']:>9}   {r['reserve_ms']:>10.3f} ({r['reserve_min_ms']:.3f} - {r['reserve_max_ms']:.3f})"
               f"   {r['move_ms']:>10.3f} ({r['move_min_ms']:.3f} - {r['move_max_ms']:.3f})"
               f"   {r['move_over_reserve']:>6.2f} ({r['move_over_reserve_range'][0]:.2f} - {r['move_over_reserve_range'][1]:.2f})"
               f"   {str(r['reserve_faster_spreads_disjoint']):>10}   {r['reserve_kernel_ms']:>9.3f}   {str(r['kernel_TBs']):>12}"
               f"   {r['reserve_malloc_free_ms']:>18.3f} ({r['malloc_free_share']:.2f})  {r['verified']}")
    if srow:
        yield (f"#  shrink 2^{srow['shrink_from_log2']} -> 2^{srow['shrink_to_log2']} after a rewind: {srow['shrink_ms']:.3f} ms"
               f" ({srow['shrink_min_ms']:.3f} - {srow['shrink_max_ms']:.3f}), kernel {srow['shrink_kernel_ms']:.3f} ms,"
               f" malloc + free {srow['shrink_malloc_free_ms']:.3f} ms, verified {srow['verified']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shrink", default="24,20")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                          a="imt_itree_reserve(T, 2 S, 0) on a full tree of S leaves",
                          b="imt_itree_get_values + imt_itree_new(2 S) + imt_itree_load_values + imt_itree_free, device pointers")),
          flush=True)
    rows = [one_size(ctx, dev, logs, args.repeats, 0x52530000 + 64 * i) for i, logs in enumerate(int(x) for x in args.sizes.split(","))]
    srow = None
    if args.shrink:
        hi, lo = (int(x) for x in args.shrink.split(","))
        srow = shrink(ctx, dev, hi, lo, args.repeats, 0x52531000)
    for line in table(rows, srow):
        print(line)
    ok = all(r["verified"] for r in rows) and (srow is None or srow["verified"])
    print("# every root equal across the arms and after every return to the old capacity: " + ("yes" if ok else "NO"))
    ctx.close()


if __name__ == "__main__":
    main()
