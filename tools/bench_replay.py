#!/usr/bin/env python3
"""What proving a block later costs: imt_itree_view_insert_witness against the only other route to the same witnesses --
a second tree loaded with a snapshot as of the block's first leaf, then imt_itree_insert_batch -- and against the
insertion alone, in one process on depth-32 trees.  A measurement, not a gate: nothing here passes or fails on a time.

For every base size S (default 2^20 and 2^24 leaves) trees A and B are filled with the same S - 1 values by
imt_itree_apply_batch and a snapshot of that state is taken into device memory (the load arm's best case: no PCIe).  For
every n (default 2^10, 2^13, 2^16) A applies n values (M = S + n leaves) and carries a view at S.  `--repeats` times, after
one warm-up round that is dropped, timed with the host clock around synchronous calls, all outputs requested, device
pointers, level-major:
  (a) build    A gets one more value and is rewound to M again, then imt_itree_view_root: the view's rebuild, warm;
      replay   imt_itree_view_insert_witness(view, n) on the view just rebuilt: preparation, sweep and outputs;
  (b) load     imt_itree_load(B, snapshot of S leaves, IMT_DEVICE_PTRS),
      + insert imt_itree_insert_batch(B, the same n values), not pipelined: load + insert is the route without this call;
  (c) insert   imt_itree_insert_batch of the same n values on B rewound to S, not pipelined: the floor for the sweep.
The replay's nine outputs must equal the insertion's byte for byte, and A's root must not move: otherwise the row says
"verified": false and its figures mean nothing.  imt_version() is printed so the file says which build was measured.

  python tools/bench_replay.py [--bases 20,24] [--ns 10,13,16] [--repeats 3]"""
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
CHUNK = 1 << 20
P_ = lambda x: ctypes.c_void_p(x.data_ptr())


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def apply(ctx, tree, vals):
    for a in range(0, vals.shape[0], CHUNK):
        n = min(CHUNK, vals.shape[0] - a)
        check(ctx, lib.imt_itree_apply_batch(tree.h, P_(vals[a]), n, None, F.DEVICE_PTRS))
    ctx.sync()


def timed(ctx, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def outputs(n, dev):
    shapes = dict(low_index=(n, 8), is_largest=(n,), low_leaf=(n, 3, 32), new_leaf=(n, 3, 32), old_root=(n, 32),
                  interim_root=(n, 32), new_root=(n, 32), low_sib=(DEPTH, n, 32), new_sib=(DEPTH, n, 32))
    bufs = {k: torch.zeros(shp, dtype=torch.uint8, device=dev) for k, shp in shapes.items()}
    return bufs, F.InsertOut(**{k: b.data_ptr() for k, b in bufs.items()})


def one_base(ctx, dev, logs, ns, repeats, seed):
    S = 1 << logs
    ns = [n for n in ns if (1 << n) < S]
    cap = 1 << (logs + 1)
    A, B = imt_amd.IndexedTree(ctx, DEPTH, cap), imt_amd.IndexedTree(ctx, DEPTH, cap)
    base = torch.from_numpy(bench.synth_values(S - 1, 0, 1, seed)).to(dev)
    for t in (A, B):
        apply(ctx, t, base)
    del base
    snap = torch.empty((S, 3, 32), dtype=torch.uint8, device=dev)
    check(ctx, lib.imt_itree_get_leaves(A.h, None, S, P_(snap), F.DEVICE_PTRS))
    ctx.sync()
    rows = []
    for j, logn in enumerate(ns):
        n = 1 << logn
        extra = torch.from_numpy(bench.synth_values(n + 1, 0, 1, seed + 1 + j)).to(dev)
        spare, extra = extra[n:], extra[:n]
        apply(ctx, A, extra)
        M, head = S + n, A.root()
        view = A.view(S)
        got, got_out = outputs(n, dev)
        want, want_out = outputs(n, dev)
        ms = dict(build=[], replay=[], load=[], load_insert=[], insert=[])
        verified = True
        for r in range(repeats + 1):                     # the first round warms every arm (allocations) and is dropped
            apply(ctx, A, spare)
            check(ctx, lib.imt_itree_rewind(A.h, M, None, None, 0))
            t = dict(build=timed(ctx, view.root))
            t["replay"] = timed(ctx, lambda: check(ctx, lib.imt_itree_view_insert_witness(
                view.h, n, ctypes.byref(got_out), F.DEVICE_PTRS)))
            t["load"] = timed(ctx, lambda: check(ctx, lib.imt_itree_load(B.h, P_(snap), S, F.DEVICE_PTRS)))
            t["load_insert"] = timed(ctx, lambda: check(ctx, lib.imt_itree_insert_batch(
                B.h, P_(extra), n, ctypes.byref(want_out), F.DEVICE_PTRS)))
            verified = verified and all(bool(torch.equal(got[k], want[k])) for k in got) and A.root() == head and A.size == M
            check(ctx, lib.imt_itree_rewind(B.h, S, None, None, 0))
            for b in want.values():
                b.zero_()
            t["insert"] = timed(ctx, lambda: check(ctx, lib.imt_itree_insert_batch(
                B.h, P_(extra), n, ctypes.byref(want_out), F.DEVICE_PTRS)))
            verified = verified and all(bool(torch.equal(got[k], want[k])) for k in got)
            check(ctx, lib.imt_itree_rewind(B.h, S, None, None, 0))
            if r:
                for a, x in t.items():
                    ms[a].append(x)
        view.close()
        row = dict(S=S, log2_S=logs, n=n, log2_n=logn, repeats=repeats, verified=bool(verified))
        for a, v in ms.items():
            row[a + "_ms"] = round(float(np.median(v)), 3)
            row[a + "_min_ms"] = round(min(v), 3)
            row[a + "_max_ms"] = round(max(v), 3)
        row["route_b_ms"] = round(row["load_ms"] + row["load_insert_ms"], 3)
        row["route_a_ms"] = round(row["build_ms"] + row["replay_ms"], 3)
        row["b_over_a"] = round(row["route_b_ms"] / row["route_a_ms"], 2)
        row["replay_over_insert"] = round(row["replay_ms"] / row["insert_ms"], 2)
        row["replay_within_insert_spread"] = bool(row["insert_min_ms"] <= row["replay_ms"] <= row["insert_max_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        check(ctx, lib.imt_itree_rewind(A.h, S, None, None, 0))
        del extra, spare, got, want
    A.close()
    B.close()
    del snap
    torch.cuda.empty_cache()
    return rows


def table(rows):
    spread = lambda r, a: f"{r[a + '_ms']:>9.3f} ({r[a + '_min_ms']:.3f} - {r[a + '_max_ms']:.3f})"
    yield ("#  log2 S  log2 n | (a) view build ms (min - max) | (a) replay ms | (b) load ms | (b) insert after load ms |"
           " (c) insert ms | (b) / (a)  replay / (c)")
    for r in rows:
        yield (f"#  {r['log2_S']:>6}  {r['log2_n']:>6} | {spread(r, 'build')} | {spread(r, 'replay')} | {spread(r, 'load')} |"
               f" {spread(r, 'load_insert')} | {spread(r, 'insert')} | {r['b_over_a']:>8.2f} {r['replay_over_insert']:>8.2f}"
               f"  verified={r['verified']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", default="20,24")
    ap.add_argument("--ns", default="10,13,16")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                          a="imt_itree_view_root after the tree changed (build) + imt_itree_view_insert_witness (replay)",
                          b="imt_itree_load(twin, device-resident snapshot of S leaves) + imt_itree_insert_batch",
                          c="imt_itree_insert_batch on a tree of S leaves, not pipelined")), flush=True)
    rows = []
    ns = [int(x) for x in args.ns.split(",")]
    for i, logs in enumerate(int(x) for x in args.bases.split(",")):
        rows += one_base(ctx, dev, logs, ns, args.repeats, 0x52500000 + 64 * i)
    for line in table(rows):
        print(line)
    print("# every row verified: " + ("yes" if all(r["verified"] for r in rows) else "NO"))
    ctx.close()


if __name__ == "__main__":
    main()
