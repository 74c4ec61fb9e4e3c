#!/usr/bin/env python3
"""What reading at an earlier size costs: a view of the tree (imt_itree_view_*) against the two other ways to the same
answers -- imt_itree_rewind of a twin, and imt_itree_load of a snapshot into a second tree -- and a view's proof gather
against the tree's own, in one process on twin depth-32 trees.  A measurement, not a gate: nothing here passes or fails
on a time.

For every base size S (default 2^20 and 2^24 leaves) trees A and B are filled with the same S - 1 values by
imt_itree_apply_batch and a snapshot of that state is taken into device memory (the load arm's best case: no PCIe, the
snapshot already there).  For every k (default 2^10, 2^13, 2^16) both apply the same k values (M = S + k leaves); A stays
there and carries a view at S.  `--repeats` times, after one warm-up round that is dropped, timed with the host clock
around synchronous calls:
  build    A gets one more value and is rewound to M again (two changes of its contents), then imt_itree_view_root: the
           query finds the tree changed and rebuilds the view first -- buffers warm, the same (M, S) every time;
  fresh    imt_itree_view_create + the first imt_itree_view_root of a new view: the same build with its allocations;
  rewind   imt_itree_rewind(B, S), after which B applies the k values again;
  load     imt_itree_load(B, snapshot of S leaves, IMT_DEVICE_PTRS), after which B applies the k values again;
  proofs   imt_itree_view_get_proof_batch of 2^16 random indices below S (device pointers, level-major) against
           imt_itree_get_proof_batch of the same indices on A itself: what the per-sibling list search costs.
Every root involved must equal the root noted at S, and the view's proofs must equal those of B rewound to S: otherwise
the row says "verified": false and its figures mean nothing.  imt_version() is printed so the file says which build was
measured.

  python tools/bench_view.py [--bases 20,24] [--ks 10,13,16] [--repeats 3]"""
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
N_PROOFS = 1 << 16


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def apply(ctx, tree, vals):
    for a in range(0, vals.shape[0], CHUNK):
        n = min(CHUNK, vals.shape[0] - a)
        check(ctx, lib.imt_itree_apply_batch(tree.h, ctypes.c_void_p(vals[a].data_ptr()), n, None, F.DEVICE_PTRS))
    ctx.sync()


def timed(ctx, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def one_base(ctx, dev, logs, ks, repeats, seed):
    S = 1 << logs
    ks = [k for k in ks if (1 << k) < S]
    cap = 1 << (logs + 1)
    A, B = imt_amd.IndexedTree(ctx, DEPTH, cap), imt_amd.IndexedTree(ctx, DEPTH, cap)
    base = torch.from_numpy(bench.synth_values(S - 1, 0, 1, seed)).to(dev)
    for t in (A, B):
        apply(ctx, t, base)
    del base
    root_S = A.root()
    assert A.size == B.size == S and B.root() == root_S
    snap = torch.empty((S, 3, 32), dtype=torch.uint8, device=dev)
    check(ctx, lib.imt_itree_get_leaves(A.h, None, S, ctypes.c_void_p(snap.data_ptr()), F.DEVICE_PTRS))
    ctx.sync()
    rng = np.random.default_rng(seed)
    idx = torch.from_numpy(rng.integers(0, S, N_PROOFS).astype(np.int64)).to(dev)
    sib_v = torch.empty((DEPTH, N_PROOFS, 32), dtype=torch.uint8, device=dev)
    sib_t = torch.empty((DEPTH, N_PROOFS, 32), dtype=torch.uint8, device=dev)
    P_ = lambda x: ctypes.c_void_p(x.data_ptr())
    rows = []
    for j, logk in enumerate(ks):
        k = 1 << logk
        extra = torch.from_numpy(bench.synth_values(k + 1, 0, 1, seed + 1 + j)).to(dev)
        spare, extra = extra[k:], extra[:k]
        for t in (A, B):
            apply(ctx, t, extra)
        M = S + k
        view = A.view(S)
        ms = dict(build=[], fresh=[], rewind=[], load=[], view_proofs=[], tree_proofs=[])
        verified, roots_ok = True, []
        hashes = None
        for r in range(repeats + 1):                     # the first round warms every arm (allocations) and is dropped
            apply(ctx, A, spare)
            check(ctx, lib.imt_itree_rewind(A.h, M, None, None, 0))
            t = dict(build=timed(ctx, lambda: roots_ok.append(view.root() == root_S)))
            hashes, _ = view.stats()
            box = []
            t["fresh"] = timed(ctx, lambda: box.append(fresh_view(A, S)))
            roots_ok.append(box[0].root() == root_S)
            box[0].close()
            t["view_proofs"] = timed(ctx, lambda: check(ctx, lib.imt_itree_view_get_proof_batch(
                view.h, P_(idx), N_PROOFS, P_(sib_v), F.DEVICE_PTRS)))
            t["tree_proofs"] = timed(ctx, lambda: check(ctx, lib.imt_itree_get_proof_batch(
                A.h, P_(idx), N_PROOFS, P_(sib_t), F.DEVICE_PTRS)))
            t["rewind"] = timed(ctx, lambda: check(ctx, lib.imt_itree_rewind(B.h, S, None, None, 0)))
            check(ctx, lib.imt_itree_get_proof_batch(B.h, P_(idx), N_PROOFS, P_(sib_t), F.DEVICE_PTRS))
            ctx.sync()
            verified = verified and B.root() == root_S and bool(torch.equal(sib_v, sib_t)) and A.size == M
            apply(ctx, B, extra)
            t["load"] = timed(ctx, lambda: check(ctx, lib.imt_itree_load(B.h, P_(snap), S, F.DEVICE_PTRS)))
            verified = verified and B.root() == root_S and B.size == S
            apply(ctx, B, extra)
            if r:
                for a, x in t.items():
                    ms[a].append(x)
        view.close()
        med = {a: float(np.median(v)) for a, v in ms.items()}
        row = dict(S=S, log2_S=logs, k=k, log2_k=logk, M=M, repeats=repeats, verified=bool(verified and all(roots_ok)),
                   view_hashes=int(hashes.sum()), relinked=int(hashes[0]) - 1, n_proofs=N_PROOFS)
        for a in ms:
            row[a + "_ms"] = round(med[a], 3)
            row[a + "_min_ms"] = round(min(ms[a]), 3)
            row[a + "_max_ms"] = round(max(ms[a]), 3)
        row["rewind_over_build"] = round(med["rewind"] / med["build"], 2)
        row["load_over_build"] = round(med["load"] / med["build"], 2)
        row["view_over_tree_proofs"] = round(med["view_proofs"] / med["tree_proofs"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        check(ctx, lib.imt_itree_rewind(A.h, S, None, None, 0))
        check(ctx, lib.imt_itree_rewind(B.h, S, None, None, 0))
        del extra, spare
    A.close()
    B.close()
    del snap
    torch.cuda.empty_cache()
    return rows


def fresh_view(tree, size):
    v = tree.view(size)
    v.root()
    return v


def table(rows):
    spread = lambda r, a: f"{r[a + '_ms']:>9.3f} ({r[a + '_min_ms']:.3f} - {r[a + '_max_ms']:.3f})"
    yield "#  log2 S  log2 k  relinked |  view build ms (min - max) |  fresh view ms |  rewind ms |  load ms | rewind / build  load / build"
    for r in rows:
        yield (f"#  {r['log2_S']:>6}  {r['log2_k']:>6}  {r['relinked']:>8} | {spread(r, 'build')} | {spread(r, 'fresh')} |"
               f" {spread(r, 'rewind')} | {spread(r, 'load')} | {r['rewind_over_build']:>8.2f} {r['load_over_build']:>10.2f}"
               f"  verified={r['verified']}")
    yield f"#  log2 S  log2 k |  {N_PROOFS} proofs: view ms (min - max) |  tree ms (min - max) |  view / tree"
    for r in rows:
        yield (f"#  {r['log2_S']:>6}  {r['log2_k']:>6} | {spread(r, 'view_proofs')} | {spread(r, 'tree_proofs')} |"
               f" {r['view_over_tree_proofs']:>6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", default="20,24")
    ap.add_argument("--ks", default="10,13,16")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                          build="imt_itree_view_root of a view at S after the tree of M = S + k leaves changed",
                          rewind="imt_itree_rewind(twin, S)",
                          load="imt_itree_load(twin, device-resident snapshot of S leaves, IMT_DEVICE_PTRS)")), flush=True)
    rows = []
    ks = [int(x) for x in args.ks.split(",")]
    for i, logs in enumerate(int(x) for x in args.bases.split(",")):
        rows += one_base(ctx, dev, logs, ks, args.repeats, 0x56570000 + 64 * i)
    for line in table(rows):
        print(line)
    print("# every row verified: " + ("yes" if all(r["verified"] for r in rows) else "NO"))
    ctx.close()


if __name__ == "__main__":
    main()
