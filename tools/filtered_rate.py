#!/usr/bin/env python3
"""What the classification of imt_itree_insert_filtered costs: bench.py's workload (depth 32, 2^16 values per batch,
bench.py's synthetic values, IMT_DEVICE_PTRS | IMT_PIPELINE | IMT_INPUTS_READY, every witness written to HBM in two
rotating output sets) through imt_itree_insert_batch on clean values, against imt_itree_insert_filtered with 0 / 1 /
10 / 50 % of the values rejected (half of them stored values of the batch before, still hashing; 40 % repeats inside
the batch; 10 % zeros).  Each leg runs on a fresh tree: warm-up batches, then timed batches closed by a device
synchronise; the legs alternate, `rounds` times in one process.  Reported per leg: accepted insertions/s and the host
time of one call.  Then the lookup rate at 2^20 candidates (half stored) against a 2^20-leaf tree, beside
imt_itree_find_low_batch on 2^20 absent candidates.

  python tools/filtered_rate.py [--steps 20] [--warmup 3] [--rounds 3] [--no-lookup]"""
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
DEPTH, N = 32, 1 << 16
FLAGS = F.DEVICE_PTRS | F.PIPELINE | F.INPUTS_READY


def batches(total, reject, seed):
    """`total` batches of N values with a fraction `reject` rejected; returns (uint8 [total, N, 32], accepted per batch)"""
    rng = np.random.default_rng(seed)
    k = int(round(N * reject))
    fresh = bench.synth_values(total * (N - k), 0, 1, seed)
    out = np.empty((total, N, 32), np.uint8)
    for b in range(total):
        f = fresh[b * (N - k):(b + 1) * (N - k)]
        n_prev = k // 2 if b > 0 else 0
        n_zero = k // 10
        n_rep = k - n_prev - n_zero
        parts = [f]
        if n_prev:
            parts.append(out[b - 1][rng.choice(N, n_prev, replace=False)])
            parts[-1] = parts[-1][(parts[-1] != 0).any(axis=1)]              # a rejected zero of the batch before
            n_zero += n_prev - parts[-1].shape[0]
        parts.append(f[rng.integers(0, N - k, n_rep)])
        parts.append(np.zeros((n_zero, 32), np.uint8))
        out[b] = np.concatenate(parts)[rng.permutation(N)]
    return out


def outputs(dev):
    u8 = dict(dtype=torch.uint8, device=dev)
    sets = [dict(low_index=torch.empty(N, dtype=torch.int64, device=dev), low_leaf=torch.empty((N, 3, 32), **u8),
                 is_largest=torch.empty(N, **u8), old_root=torch.empty((N, 32), **u8),
                 interim_root=torch.empty((N, 32), **u8), new_root=torch.empty((N, 32), **u8),
                 new_leaf=torch.empty((N, 3, 32), **u8), low_sib=torch.empty((DEPTH, N, 32), **u8),
                 new_sib=torch.empty((DEPTH, N, 32), **u8)) for _ in range(2)]
    return sets, [F.InsertOut(**{k: t.data_ptr() for k, t in s.items()}) for s in sets]


def leg(ctx, dev, vals, filtered, warmup, steps, outs):
    total = warmup + steps
    tree = imt_amd.IndexedTree(ctx, DEPTH, 1 << (total * N).bit_length())
    st = torch.empty(N, dtype=torch.uint8, device=dev)
    lf = torch.empty(N, dtype=torch.int64, device=dev)
    k_ins = ctypes.c_uint64()
    accepted, host = 0, 0.0
    for i in range(total):
        if i == warmup:
            torch.cuda.synchronize()
            accepted, host, t0 = 0, 0.0, time.perf_counter()
        v = ctypes.c_void_p(vals[i].data_ptr())
        th = time.perf_counter()
        if filtered:
            rc = lib.imt_itree_insert_filtered(tree.h, v, N, ctypes.c_void_p(st.data_ptr()), ctypes.c_void_p(lf.data_ptr()),
                                               ctypes.byref(k_ins), ctypes.byref(outs[i % 2]), FLAGS)
            accepted += k_ins.value
        else:
            rc = lib.imt_itree_insert_batch(tree.h, v, N, ctypes.byref(outs[i % 2]), FLAGS)
            accepted += N
        host += time.perf_counter() - th
        if rc != 0:
            raise RuntimeError(lib.imt_last_error(ctx.h).decode())
    torch.cuda.synchronize()
    ctx.sync()
    dt = time.perf_counter() - t0
    tree.close()
    return dict(accepted_per_s=accepted / dt, host_ms_per_call=1e3 * host / steps, ms_per_batch=1e3 * dt / steps,
                accepted_per_batch=accepted / steps)


def lookup_rate(ctx, dev, reps=10):
    M = 1 << 20
    vals = bench.synth_values(M + M // 2, 0, 1, 0x46494C52)
    tree = imt_amd.IndexedTree(ctx, DEPTH, 1 << 21)
    vt = torch.from_numpy(vals).to(dev)
    for s in range(0, M, N):
        rc = lib.imt_itree_insert_batch(tree.h, ctypes.c_void_p(vt[s].data_ptr()), N, None, F.DEVICE_PTRS | F.PIPELINE)
        assert rc == 0, lib.imt_last_error(ctx.h)
    ctx.sync()
    rng = np.random.default_rng(7)
    mixed = torch.from_numpy(np.concatenate([vals[rng.choice(M, M // 2, replace=False)], vals[M:]])[rng.permutation(M)]).to(dev)
    absent = torch.from_numpy(np.concatenate([vals[M:], vals[M:]])).to(dev)     # find_low refuses stored values
    st = torch.empty(M, dtype=torch.uint8, device=dev)
    lf = torch.empty(M, dtype=torch.int64, device=dev)

    def timed(call):
        call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    def lk():
        assert lib.imt_itree_lookup_batch(tree.h, ctypes.c_void_p(mixed.data_ptr()), M, ctypes.c_void_p(st.data_ptr()),
                                          ctypes.c_void_p(lf.data_ptr()), F.DEVICE_PTRS) == 0

    def fl():
        assert lib.imt_itree_find_low_batch(tree.h, ctypes.c_void_p(absent.data_ptr()), M, ctypes.c_void_p(lf.data_ptr()),
                                            F.DEVICE_PTRS) == 0

    a, b = timed(lk), timed(fl)
    tree.close()
    return dict(candidates=M, tree_leaves=M + 1, lookup_ms=1e3 * a, lookup_per_s=M / a, find_low_ms=1e3 * b,
                find_low_per_s=M / b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-lookup", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    total = args.warmup + args.steps
    legs = [("insert_batch", 0.0, False), ("filtered_0", 0.0, True), ("filtered_1", 0.01, True),
            ("filtered_10", 0.10, True), ("filtered_50", 0.50, True)]
    data = {name: torch.from_numpy(batches(total, r, 0x46494C70 + int(r * 100))).to(dev) for name, r, _ in legs}
    _, outs = outputs(dev)
    res = {name: [] for name, _, _ in legs}
    for rnd in range(args.rounds):
        for name, r, filtered in legs:
            x = leg(ctx, dev, data[name], filtered, args.warmup, args.steps, outs)
            res[name].append(x)
            print(json.dumps(dict(round=rnd, leg=name, rejected=r, **{k: round(v, 4) for k, v in x.items()})), flush=True)
    base = [x["accepted_per_s"] for x in res["insert_batch"]]
    print("# leg              accepted M/s (median of rounds)  host ms/call  vs insert_batch (same round, median)")
    for name, _, _ in legs:
        rates = [x["accepted_per_s"] for x in res[name]]
        rel = [a / b for a, b in zip(rates, base)]
        print(f"  {name:<16} {np.median(rates) / 1e6:8.3f}   [{' '.join(f'{v / 1e6:.3f}' for v in rates)}]"
              f"   {np.median([x['host_ms_per_call'] for x in res[name]]):7.2f}   {np.median(rel):.4f}", flush=True)
    if not args.no_lookup:
        print(json.dumps(dict(leg="lookup", **{k: round(v, 4) if isinstance(v, float) else v
                                              for k, v in lookup_rate(ctx, dev).items()})), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
