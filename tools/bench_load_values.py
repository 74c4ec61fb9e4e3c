#!/usr/bin/env python3
"""What a cold start from values costs: imt_itree_load_values against the two other ways to the same tree, in one process
on depth-32 trees.

For every size (default 2^20 and 2^24 leaves; --sizes 20,24,26) the same n = size - 1 values lie in device memory and
three arms take turns, `--repeats` times after one dropped warm-up round ((a) and (b) swap places from round to round):

  (a) load_values  imt_itree_load_values(A, values, n, IMT_DEVICE_PTRS): canonical values, 32 bytes per leaf;
  (b) load         imt_itree_load(B, preimages, n + 1, IMT_DEVICE_PTRS): the canonical preimages of the same tree
                   (imt_itree_get_leaves of A, taken once, not charged), 96 bytes per leaf;
  (c) apply        imt_itree_apply_batch in chunks of 2^20 with IMT_DEVICE_PTRS | IMT_INPUTS_READY onto a FRESH tree (made
                   outside the timed region), then one synchronisation: the only route from values without (a).

Every arm is timed with the host clock from the first call to the point where the tree is complete on the device.  The
roots of the three trees must be equal after every round: otherwise the row says "verified": false and its figures mean
nothing.  Reported per size: milliseconds per arm (median and min - max), leaves per second, the ratios c / a and b / a,
whether a's and c's spreads are disjoint, whether a is slower than b by more than the larger of the two spreads.

Memory: while (a) and (b) run, a thread samples the free device memory (hipMemGetInfo through torch); the largest drop
below the level before the call is the scratch the call took from the context and gave back (the sort workspace, plus a
staging copy only for inputs that are not canonical device memory -- there is none here).  The input the caller must
hold is 32 n bytes for (a) and 96 (n + 1) for (b).

  python tools/bench_load_values.py [--sizes 20,24] [--repeats 3]"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys
import threading
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
CHUNK = 1 << 20


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def P_(t, row=0):
    return ctypes.c_void_p(t.data_ptr() + row * t.stride(0) * t.element_size())


class FreeMemory:
    """the smallest amount of free device memory seen while the block runs, sampled by a thread"""

    def __enter__(self):
        self.before = self.low = torch.cuda.mem_get_info()[0]
        self.stop = False
        self.th = threading.Thread(target=self.run)
        self.th.start()
        return self

    def run(self):
        while not self.stop:
            self.low = min(self.low, torch.cuda.mem_get_info()[0])
            time.sleep(0.0005)

    def __exit__(self, *a):
        self.stop = True
        self.th.join()

    @property
    def drop(self):
        return self.before - self.low


def one_size(ctx, dev, logs, repeats, seed):
    S = 1 << logs
    n = S - 1
    cap = 1 << (logs + 1)
    vals = torch.from_numpy(bench.synth_values(n, 0, 1, seed)).to(dev)
    A, B = imt_amd.IndexedTree(ctx, DEPTH, cap), imt_amd.IndexedTree(ctx, DEPTH, cap)
    check(ctx, lib.imt_itree_load_values(A.h, P_(vals), n, None, F.DEVICE_PTRS))
    pre = torch.empty((S, 3, 32), dtype=torch.uint8, device=dev)
    check(ctx, lib.imt_itree_get_leaves(A.h, None, S, P_(pre), F.DEVICE_PTRS))
    ctx.sync()
    ms = dict(a=[], b=[], c=[])
    drop = dict(a=0, b=0)
    verified = True
    for r in range(repeats + 1):                         # the first round warms every arm (allocations) and is dropped
        C = imt_amd.IndexedTree(ctx, DEPTH, cap)
        torch.cuda.synchronize()
        t = {}

        def arm_a():
            with FreeMemory() as f:
                t0 = time.perf_counter()
                check(ctx, lib.imt_itree_load_values(A.h, P_(vals), n, None, F.DEVICE_PTRS))
                t["a"] = 1e3 * (time.perf_counter() - t0)
            return f

        def arm_b():
            with FreeMemory() as f:
                t0 = time.perf_counter()
                check(ctx, lib.imt_itree_load(B.h, P_(pre), S, F.DEVICE_PTRS))
                t["b"] = 1e3 * (time.perf_counter() - t0)
            return f

        if r % 2:                                        # (a) and (b) swap places from round to round
            fa = arm_a()
            fb = arm_b()
        else:
            fb = arm_b()
            fa = arm_a()
        t4 = time.perf_counter()
        for at in range(0, n, CHUNK):
            check(ctx, lib.imt_itree_apply_batch(C.h, P_(vals, at), min(CHUNK, n - at), None, F.DEVICE_PTRS | F.INPUTS_READY))
        ctx.sync()
        t5 = time.perf_counter()
        verified = verified and A.root() == B.root() == C.root() and A.size == B.size == C.size == S
        C.close()
        if r:
            ms["a"].append(t["a"])
            ms["b"].append(t["b"])
            ms["c"].append(1e3 * (t5 - t4))
            drop["a"], drop["b"] = max(drop["a"], fa.drop), max(drop["b"], fb.drop)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    row = dict(log2_size=logs, leaves=S, repeats=repeats, verified=bool(verified))
    for k, name in (("a", "load_values"), ("b", "load"), ("c", "apply")):
        row.update({f"{name}_ms": round(med[k], 3), f"{name}_min_ms": round(min(ms[k]), 3), f"{name}_max_ms": round(max(ms[k]), 3),
                    f"{name}_Mleaves_s": round(S / med[k] / 1e3, 1), f"{name}_all_ms": [round(x, 3) for x in ms[k]]})
    row.update(apply_over_load_values=round(med["c"] / med["a"], 2),
               apply_over_load_values_range=[round(min(ms["c"]) / max(ms["a"]), 2), round(max(ms["c"]) / min(ms["a"]), 2)],
               load_over_load_values=round(med["b"] / med["a"], 3),
               load_values_faster_than_apply_spreads_disjoint=bool(max(ms["a"]) < min(ms["c"])),
               load_values_slower_than_load_beyond_spread=bool(med["a"] - med["b"] > max(spread["a"], spread["b"])),
               load_values_input_bytes=32 * n, load_input_bytes=96 * S,
               load_values_scratch_bytes_seen=int(drop["a"]), load_scratch_bytes_seen=int(drop["b"]))
    print(json.dumps(row), flush=True)
    A.close()
    B.close()
    del vals, pre
    torch.cuda.empty_cache()
    return row


def table(rows):
    yield ("#  log2 size   (a) load_values ms (min - max)     (b) load ms (min - max)        (c) apply ms (min - max)      c / a   b / a"
           "   a<c disjoint   scratch seen a / b (MiB)   input a / b (MiB)  verified")
    for r in rows:
        yield (f"#  {r['log2_size']:>9}   {r['load_values_ms']:>10.2f} ({r['load_values_min_ms']:.2f} - {r['load_values_max_ms']:.2f})"
               f"   {r['load_ms']:>10.2f} ({r['load_min_ms']:.2f} - {r['load_max_ms']:.2f})"
               f"   {r['apply_ms']:>10.2f} ({r['apply_min_ms']:.2f} - {r['apply_max_ms']:.2f})"
               f"   {r['apply_over_load_values']:>6.2f}  {r['load_over_load_values']:>6.3f}"
               f"   {str(r['load_values_faster_than_apply_spreads_disjoint']):>12}"
               f"   {r['load_values_scratch_bytes_seen'] / 2**20:>10.1f} / {r['load_scratch_bytes_seen'] / 2**20:.1f}"
               f"   {r['load_values_input_bytes'] / 2**20:>10.1f} / {r['load_input_bytes'] / 2**20:.1f}  {r['verified']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                          a="imt_itree_load_values(device-resident canonical values, IMT_DEVICE_PTRS)",
                          b="imt_itree_load(device-resident canonical preimages of the same tree, IMT_DEVICE_PTRS)",
                          c="imt_itree_apply_batch in chunks of 2^20, IMT_DEVICE_PTRS | IMT_INPUTS_READY, onto a fresh tree")),
          flush=True)
    rows = [one_size(ctx, dev, logs, args.repeats, 0x4C560000 + 64 * i) for i, logs in enumerate(int(x) for x in args.sizes.split(","))]
    for line in table(rows):
        print(line)
    print("# every root equal across the three arms: " + ("yes" if all(r["verified"] for r in rows) else "NO"))
    ctx.close()


if __name__ == "__main__":
    main()
