#!/usr/bin/env python3
"""What overlapping consecutive mixed blocks buys the follower and the prover of a chain whose blocks hold
verify_non_inclusion transactions: imt_itree_apply_mixed_pipelined and imt_itree_mixed_pipelined against the calls they are
defined by, in one process on twin depth-32 trees.

For every block size n (default 2^10, 2^13, 2^16 operations) five fresh trees are preloaded with the same 2^20 values and
grow through the run as a follower's does (M = leaves before the first timed block).  Every fourth operation of a block is
a READ of a value nobody inserts, the others are INSERTs.  Each arm plays the same 2^19 operations in blocks of n,
`--repeats` times, timed with the host clock from the first call to the return of the closing imt_ctx_sync:
  (a) apply_mixed    imt_itree_apply_mixed(IMT_DEVICE_PTRS) per block, root_out per block
  (b) apply_mixed_p  imt_itree_apply_mixed_pipelined per block, root_out per block, one sync at the end
  (c) mixed          imt_itree_mixed_batch(IMT_DEVICE_PTRS) per block, all nine + five witness arrays written to HBM
  (d) mixed_p        imt_itree_mixed_pipelined per block, the same arrays, one sync at the end
  (e) apply_p        imt_itree_apply_pipelined of the block's INSERT values alone: the floor, no READ is checked
The witness arms write into a ring of five sets of arrays, block k into set k mod 5, so no two blocks in flight share one.
Every arm is warmed with two blocks first.  Reported per n: operations/s of each arm (median of the repeats, with min and
max), the ratios b/a, d/c and b/e of the medians, whether the min-max ranges of the two arms of a ratio are disjoint -- the
project's rule for calling a difference a gain or a loss -- and the host milliseconds per block spent inside the calls.
Verification: the per-block roots of (b) equal those of (a) row for row and the ring of (d) equals the ring of (c) byte for
byte in every repeat, the INSERT counts agree, and the five final roots are equal; otherwise the row says
"verified": false and its figures mean nothing.

  python tools/bench_mixed_pipelined.py [--sizes 10,13,16] [--repeats 3] [--preload 20] [--values 19]"""
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
WARM, RING = 2, 5
ARMS = ("apply_mixed", "apply_mixed_p", "mixed", "mixed_p", "apply_p")
INS_FIELDS = dict(low_index=8, low_leaf=96, is_largest=1, old_root=32, interim_root=32, new_root=32, new_leaf=96,
                  low_sib=32 * DEPTH, new_sib=32 * DEPTH)
RD_FIELDS = dict(low_index=8, low_leaf=96, is_largest=1, root=32, low_sib=32 * DEPTH)


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


class Ring:
    """RING sets of witness arrays for blocks of n operations, in device memory"""

    def __init__(self, n, dev):
        mk = lambda per_row: torch.zeros(n * per_row, dtype=torch.uint8, device=dev)        # noqa: E731
        self.sets = [({k: mk(b) for k, b in INS_FIELDS.items()}, {k: mk(b) for k, b in RD_FIELDS.items()}) for _ in range(RING)]
        self.structs = [(F.InsertOut(**{k: x.data_ptr() for k, x in i.items()}), F.ReadOut(**{k: x.data_ptr() for k, x in r.items()}))
                        for i, r in self.sets]

    def equals(self, other):
        return all(bool((x == y[k]).all().item()) for a, b in zip(self.sets, other.sets) for d, y in zip(a, b) for k, x in d.items())


def run_arm(arm, ctx, tree, ops_vals, ops, ins_vals, n, roots, ring):
    """every block through one arm, then one sync; returns (seconds in all, seconds inside the calls, INSERTs carried out)"""
    blocks = ops_vals.shape[0] // n
    k_ins = ins_vals.shape[0] // blocks
    inside, inserted = 0.0, 0
    n_ins, bad = ctypes.c_uint64(), ctypes.c_uint64()
    t0 = time.perf_counter()
    for k in range(blocks):
        v, o = ctypes.c_void_p(ops_vals[k * n].data_ptr()), ctypes.c_void_p(ops[k * n:].data_ptr())
        r = ctypes.c_void_p(roots[k].data_ptr()) if roots is not None else None
        c0 = time.perf_counter()
        if arm == "apply_mixed":
            rc = lib.imt_itree_apply_mixed(tree.h, v, o, n, r, ctypes.byref(n_ins), ctypes.byref(bad), F.DEVICE_PTRS)
        elif arm == "apply_mixed_p":
            rc = lib.imt_itree_apply_mixed_pipelined(tree.h, v, o, n, r, ctypes.byref(n_ins), ctypes.byref(bad), F.DEVICE_PTRS)
        elif arm in ("mixed", "mixed_p"):
            fn = lib.imt_itree_mixed_batch if arm == "mixed" else lib.imt_itree_mixed_pipelined
            i, d = ring.structs[k % RING]
            rc = fn(tree.h, v, o, n, ctypes.byref(i), ctypes.byref(d), ctypes.byref(n_ins), ctypes.byref(bad), F.DEVICE_PTRS)
        else:
            rc = lib.imt_itree_apply_pipelined(tree.h, ctypes.c_void_p(ins_vals[k * k_ins].data_ptr()), k_ins, r, F.DEVICE_PTRS)
            n_ins.value = k_ins
        inside += time.perf_counter() - c0
        check(ctx, rc)
        inserted += n_ins.value
    ctx.sync()
    return time.perf_counter() - t0, inside, inserted


def disjoint(x, y):
    return bool(min(x) > max(y) or min(y) > max(x))


def block_stream(dev, count, seed):
    """`count` operations, every fourth a READ: (values [count][32], op bytes [count], the INSERT values in order)"""
    vals = torch.from_numpy(bench.synth_values(count, 0, 1, seed)).to(dev)
    ops = torch.zeros(count, dtype=torch.uint8, device=dev)
    ops[3::4] = 1
    return vals, ops, vals[ops == 0].contiguous()


def one_size(ctx, dev, pre, logn, values, repeats, seed):
    n, total = 1 << logn, 1 << values
    blocks = total // n
    need = pre.shape[0] + 1 + (repeats * total + WARM * n) * 3 // 4
    trees = {arm: imt_amd.IndexedTree(ctx, DEPTH, 1 << (need - 1).bit_length()) for arm in ARMS}
    for arm in ARMS:
        check(ctx, lib.imt_itree_apply_batch(trees[arm].h, ctypes.c_void_p(pre.data_ptr()), pre.shape[0], None, F.DEVICE_PTRS))
    ctx.sync()
    rings = {arm: Ring(n, dev) for arm in ("mixed", "mixed_p")}
    warm = block_stream(dev, WARM * n, seed + 1)
    for arm in ARMS:
        run_arm(arm, ctx, trees[arm], *warm, n, None, rings.get(arm))
    M = trees["apply_mixed"].size
    rates = {arm: [] for arm in ARMS}
    host_ms = {arm: [] for arm in ARMS}
    roots = {arm: torch.zeros((blocks, 32), dtype=torch.uint8, device=dev) for arm in ("apply_mixed", "apply_mixed_p", "apply_p")}
    verified = True
    for r in range(repeats):
        stream = block_stream(dev, total, seed + 2 + r)
        torch.cuda.synchronize()
        counts = set()
        for arm in ARMS:
            secs, inside, inserted = run_arm(arm, ctx, trees[arm], *stream, n, roots.get(arm), rings.get(arm))
            rates[arm].append(total / secs)
            host_ms[arm].append(1e3 * inside / blocks)
            counts.add(inserted)
        torch.cuda.synchronize()
        verified = verified and counts == {total * 3 // 4}
        verified = verified and all(bool((roots["apply_mixed"] == roots[a]).all().item()) for a in ("apply_mixed_p", "apply_p"))
        verified = verified and bool(roots["apply_mixed"].any().item()) and rings["mixed"].equals(rings["mixed_p"])
        verified = verified and len({trees[a].root() for a in ARMS}) == 1 and len({trees[a].size for a in ARMS}) == 1
        del stream
    med = {k: float(np.median(v)) for k, v in rates.items()}
    row = dict(n=n, log2_n=logn, blocks_per_arm=blocks, M=int(M), M_end=int(trees["apply_mixed"].size), repeats=repeats,
               reads_per_block=n // 4, verified=bool(verified))
    for arm in ARMS:
        row[arm + "_ops_per_s"] = dict(median=round(med[arm]), min=round(min(rates[arm])), max=round(max(rates[arm])))
        row[arm + "_host_ms_per_block_in_calls"] = round(float(np.median(host_ms[arm])), 4)
        row[arm + "_ms_per_block"] = round(1e3 * n / med[arm], 4)
    for name, x, y in (("apply_mixed_p_over_apply_mixed", "apply_mixed_p", "apply_mixed"), ("mixed_p_over_mixed", "mixed_p", "mixed"),
                       ("apply_mixed_p_over_apply_p", "apply_mixed_p", "apply_p")):
        row[name] = round(med[x] / med[y], 3)
        row["ranges_disjoint_" + name] = disjoint(rates[x], rates[y])
    for t in trees.values():
        t.close()
    del warm, roots, rings
    torch.cuda.empty_cache()
    return row


def table(rows):
    yield ("#  log2 n  blocks        M   (a) apply_mixed [min-max]  (b) apply_mixed_pipelined   (c) mixed_batch [min-max]"
           "  (d) mixed_pipelined [min-max]  (e) apply_pipelined, INSERTs only   b/a    d/c    b/e"
           "   host ms/block a, b, c, d, e   verified      (M operations/s)")
    for r in rows:
        cell = lambda arm: (f"{r[arm + '_ops_per_s']['median'] / 1e6:7.3f} [{r[arm + '_ops_per_s']['min'] / 1e6:.3f}-"    # noqa: E731
                            f"{r[arm + '_ops_per_s']['max'] / 1e6:.3f}]")
        ratio = lambda k: f"{r[k]:>5.2f}" + ("" if r["ranges_disjoint_" + k] else "~")                                       # noqa: E731
        yield (f"#  {r['log2_n']:>6} {r['blocks_per_arm']:>7} {r['M']:>8}   {cell('apply_mixed'):>25}  {cell('apply_mixed_p'):>25}"
               f"   {cell('mixed'):>25}  {cell('mixed_p'):>29}  {cell('apply_p'):>34}"
               f"  {ratio('apply_mixed_p_over_apply_mixed')}  {ratio('mixed_p_over_mixed')}  {ratio('apply_mixed_p_over_apply_p')}   "
               + ", ".join(f"{r[a + '_host_ms_per_block_in_calls']:.3f}" for a in ARMS) + f"   {r['verified']}")
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
                          preload=1 << args.preload, operations_per_arm=1 << args.values, reads="every fourth operation",
                          apply_mixed="imt_itree_apply_mixed(IMT_DEVICE_PTRS), root_out per block",
                          apply_mixed_p="imt_itree_apply_mixed_pipelined, root_out per block, one sync",
                          mixed="imt_itree_mixed_batch(IMT_DEVICE_PTRS), every witness array to HBM",
                          mixed_p="imt_itree_mixed_pipelined, every witness array to HBM, one sync",
                          apply_p="imt_itree_apply_pipelined of the INSERT values alone, root_out per block, one sync")), flush=True)
    pre = torch.from_numpy(bench.synth_values(1 << args.preload, 0, 1, 0x4D505000)).to(dev)
    rows = []
    for k, logn in enumerate(sizes):
        rows.append(one_size(ctx, dev, pre, logn, args.values, args.repeats, 0x4D505010 + 16 * k))
        print(json.dumps(rows[-1]), flush=True)
    for line in table(rows):
        print(line)
    ctx.close()


if __name__ == "__main__":
    main()
