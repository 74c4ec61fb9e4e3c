#!/usr/bin/env python3
"""What going back costs: imt_itree_rewind against the only other way back, imt_itree_load of a snapshot of the same
state, in one process on twin depth-32 trees.

For every base size S (default 2^20 and 2^24 leaves) two trees are filled with the same S - 1 values by
imt_itree_apply_batch, and a snapshot of that state is taken into device memory (imt_itree_get_leaves with
IMT_DEVICE_PTRS): the load arm's best case -- no PCIe, the snapshot already there, nothing charged for taking or keeping
it.  For every k (default 2^10, 2^13, 2^16, 2^20; only k < S) and `--repeats` times: both trees apply the same k values
(M = S + k leaves), then tree A goes back with imt_itree_rewind(S) and tree B with
imt_itree_load(snapshot, S, IMT_DEVICE_PTRS); both calls are synchronous and are timed with the host clock around the
call.  Afterwards the roots of A, B and the root noted before the k values must be equal: otherwise the row says
"verified": false and its figures mean nothing.  Reported per (S, k): milliseconds of both arms (median and min - max
over the repeats), their ratio, whether the spreads are disjoint with the rewind below, and what the rewind hashed
(the `hashes` output of the call) beside the load's about 2 S.  imt_version() is printed so the file says which build was
measured.

  python tools/bench_rewind.py [--bases 20,24] [--ks 10,13,16,20] [--repeats 3]"""
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


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def apply(ctx, tree, vals):
    for a in range(0, vals.shape[0], CHUNK):
        n = min(CHUNK, vals.shape[0] - a)
        check(ctx, lib.imt_itree_apply_batch(tree.h, ctypes.c_void_p(vals[a].data_ptr()), n, None, F.DEVICE_PTRS))
    ctx.sync()


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
    hashes = (ctypes.c_uint64 * (DEPTH + 1))()
    rows = []
    for j, logk in enumerate(ks):
        k = 1 << logk
        extra = torch.from_numpy(bench.synth_values(k, 0, 1, seed + 1 + j)).to(dev)
        ms = dict(rewind=[], load=[])
        verified = True
        for r in range(repeats + 1):                     # the first round warms both arms (allocations) and is dropped
            for t in (A, B):
                apply(ctx, t, extra)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            check(ctx, lib.imt_itree_rewind(A.h, S, None, hashes, 0))
            t1 = time.perf_counter()
            check(ctx, lib.imt_itree_load(B.h, ctypes.c_void_p(snap.data_ptr()), S, F.DEVICE_PTRS))
            t2 = time.perf_counter()
            verified = verified and A.root() == B.root() == root_S and A.size == B.size == S
            if r:
                ms["rewind"].append(1e3 * (t1 - t0))
                ms["load"].append(1e3 * (t2 - t1))
        med = {a: float(np.median(v)) for a, v in ms.items()}
        n_hash = int(sum(hashes))
        rows.append(dict(S=S, log2_S=logs, k=k, log2_k=logk, M=S + k, repeats=repeats, verified=bool(verified),
                         rewind_ms=round(med["rewind"], 3), rewind_min_ms=round(min(ms["rewind"]), 3),
                         rewind_max_ms=round(max(ms["rewind"]), 3), load_ms=round(med["load"], 3),
                         load_min_ms=round(min(ms["load"]), 3), load_max_ms=round(max(ms["load"]), 3),
                         ratio=round(med["load"] / med["rewind"], 2),
                         rewind_faster_spreads_disjoint=bool(max(ms["rewind"]) < min(ms["load"])),
                         k_at_most_S_over_16=bool(16 * k <= S), rewind_hashes=n_hash, rewind_relinked=int(hashes[0]) - 1,
                         load_hashes_about=2 * S, hash_ratio=round(2 * S / n_hash, 1)))
        print(json.dumps(rows[-1]), flush=True)
        del extra
    A.close()
    B.close()
    del snap
    torch.cuda.empty_cache()
    return rows


def table(rows):
    yield ("#  log2 S  log2 k   rewind ms  (min - max)           load ms  (min - max)            load / rewind   rewind hashes"
           "   2 S / hashes  disjoint  verified")
    for r in rows:
        yield (f"#  {r['log2_S']:>6}  {r['log2_k']:>6} {r['rewind_ms']:>11.3f}  ({r['rewind_min_ms']:.3f} - {r['rewind_max_ms']:.3f})"
               f" {r['load_ms']:>14.3f}  ({r['load_min_ms']:.3f} - {r['load_max_ms']:.3f}) {r['ratio']:>16.2f}"
               f" {r['rewind_hashes']:>15} {r['hash_ratio']:>14.1f}  {str(r['rewind_faster_spreads_disjoint']):>8}  {r['verified']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", default="20,24")
    ap.add_argument("--ks", default="10,13,16,20")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH,
                          rewind="imt_itree_rewind(S)",
                          load="imt_itree_load(device-resident snapshot of S leaves, IMT_DEVICE_PTRS)")), flush=True)
    rows = []
    ks = [int(x) for x in args.ks.split(",")]
    for i, logs in enumerate(int(x) for x in args.bases.split(",")):
        rows += one_base(ctx, dev, logs, ks, args.repeats, 0x52570000 + 64 * i)
    for line in table(rows):
        print(line)
    ok = all(r["verified"] and (r["rewind_faster_spreads_disjoint"] or not r["k_at_most_S_over_16"]) for r in rows)
    print("# direction (rewind faster than load, spreads disjoint) at every k <= S / 16: " + ("yes" if ok else "NO"))
    ctx.close()


if __name__ == "__main__":
    main()
