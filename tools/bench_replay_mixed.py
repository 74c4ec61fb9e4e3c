#!/usr/bin/env python3
"""What proving a mixed block later costs: imt_itree_view_mixed_witness against its floor and against what a caller does
without it, in one process on depth-32 trees of 2^20 leaves, random values, IMT_DEVICE_PTRS, every output requested,
level-major, a READ at every fourth operation.  A measurement, not a gate: nothing here passes or fails on a time.

Trees A, B and C receive the same 2^20 - 1 values; a snapshot of that state is taken into device memory.  The block has
2^16 operations: of its READs a half ask for values nobody inserts, a quarter for values a later INSERT of the block puts
in, a quarter for values of the tail.  A applies the block's INSERTs and 2^16 later values witness-free and carries a view
at the block's start.  `--repeats` times, after one warm-up round that is dropped, host clock around calls closed by
imt_ctx_sync:
  (a) replay      imt_itree_view_mixed_witness(view, the block) on A; the view's one-off build is reported beside it;
  (b) live        imt_itree_mixed_batch of the same block on B (then B is rewound, untimed): the floor -- the same hashes,
                  no searches in the view's lists;
  (c) load+live   imt_itree_load(C, device-resident snapshot of the first S leaves) + imt_itree_mixed_batch there: the
                  route without the call that keeps A where it is;
  (d) cut         a block of 2^12 operations (B has applied it and 2^12 later values) cut at every READ with view calls:
                  per READ one imt_itree_view_create at the size as of the READ, imt_itree_view_non_membership_witness and
                  imt_itree_view_root of the one value, imt_itree_view_insert_witness of the INSERTs up to the next READ,
                  imt_itree_view_free; against one imt_itree_view_mixed_witness of that block (d_replay).
The outputs of (a) and (c) must equal (b)'s byte for byte and A's root must not move, otherwise "verified" is false and
the figures mean nothing.  Reported per arm: the median, every repeat, min and max.  imt_version() says which build was
measured.

  python tools/bench_replay_mixed.py [--repeats 3] [--preload 20] [--log-n 16] [--log-cut 12] [--out profiles/replay_mixed.txt]"""
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
INS = ("low_index", "low_leaf", "is_largest", "old_root", "interim_root", "new_root", "new_leaf", "low_sib", "new_sib")
RD = ("low_index", "low_leaf", "is_largest", "root", "low_sib")


def check(ctx, rc):
    if rc != 0:
        raise RuntimeError(lib.imt_last_error(ctx.h).decode())


def ptr(x, row=0):
    return ctypes.c_void_p(x[row].data_ptr() if row else x.data_ptr())


class Buffers:
    """device outputs for n operations: both structs, level-major siblings with stride n"""

    def __init__(self, dev, n):
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)
        shapes = dict(low_leaf=(n, 3, 32), new_leaf=(n, 3, 32), is_largest=(n,), old_root=(n, 32), interim_root=(n, 32),
                      new_root=(n, 32), root=(n, 32), low_sib=(DEPTH, n, 32), new_sib=(DEPTH, n, 32))
        self.ins = {k: z(n, dt=torch.int64) if k == "low_index" else z(*shapes[k]) for k in INS}
        self.rd = {k: z(n, dt=torch.int64) if k == "low_index" else z(*shapes[k]) for k in RD}
        self.ins_out = F.InsertOut(**{k: v.data_ptr() for k, v in self.ins.items()})
        self.rd_out = F.ReadOut(**{k: v.data_ptr() for k, v in self.rd.items()})

    def equal(self, other):
        return all(bool(torch.equal(self.ins[k], other.ins[k])) for k in INS) and \
            all(bool(torch.equal(self.rd[k], other.rd[k])) for k in RD)


def apply(ctx, tree, vals):
    for a in range(0, vals.shape[0], CHUNK):
        n = min(CHUNK, vals.shape[0] - a)
        check(ctx, lib.imt_itree_apply_batch(tree.h, ptr(vals, a), n, None, F.DEVICE_PTRS))
    ctx.sync()


def timed(ctx, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def make_block(n, seed, dev):
    """(vals [n][32], ops [n], INSERT values, tail values) on the device, and the op bytes on the host"""
    ops_host = np.array([F.OP_READ if p % 4 == 3 else F.OP_INSERT for p in range(n)], np.uint8)
    n_rd = n // 4
    n_ins = n - n_rd
    pool = bench.synth_values(n_ins + n + n_rd, 0, 1, seed)               # INSERTs, the tail, values nobody inserts
    ins_vals, tail, never = pool[:n_ins], pool[n_ins:n_ins + n], pool[n_ins + n:]
    vals = np.empty((n, 32), np.uint8)
    vals[ops_host == F.OP_INSERT] = ins_vals
    rank = np.cumsum(ops_host == F.OP_INSERT)
    for q, p in enumerate(np.nonzero(ops_host == F.OP_READ)[0]):
        r = int(rank[p])
        if q % 2 == 0:
            vals[p] = never[q]
        elif q % 4 == 1 and r + 7 < n_ins:
            vals[p] = ins_vals[r + 7]                                       # inserted a few operations later
        else:
            vals[p] = tail[(q * 37) % n]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(vals), t(ops_host), t(ins_vals), t(tail), ops_host


def replay(ctx, view, vals, ops, buf):
    k = ctypes.c_uint64()
    check(ctx, lib.imt_itree_view_mixed_witness(view.h, ptr(vals), ptr(ops), vals.shape[0], ctypes.byref(buf.ins_out),
                                                ctypes.byref(buf.rd_out), ctypes.byref(k), None, F.DEVICE_PTRS))


def live(ctx, tree, vals, ops, buf):
    k = ctypes.c_uint64()
    check(ctx, lib.imt_itree_mixed_batch(tree.h, ptr(vals), ptr(ops), vals.shape[0], ctypes.byref(buf.ins_out),
                                         ctypes.byref(buf.rd_out), ctypes.byref(k), None, F.DEVICE_PTRS))


def cut_with_views(ctx, tree, S, vals, ops_host, buf):
    """the block without the call: per READ a view at the size as of the READ, its witness and root, and the witnesses of
    the INSERTs up to the next READ through the same view"""
    n, p, size = vals.shape[0], 0, S
    b = buf.rd
    while p < n:
        v = ctypes.c_void_p()
        check(ctx, lib.imt_itree_view_create(tree.h, size, ctypes.byref(v)))
        if ops_host[p] == F.OP_READ:
            check(ctx, lib.imt_itree_view_non_membership_witness(v, ptr(vals, p), 1, ptr(b["low_index"]), ptr(b["low_leaf"]),
                                                                 ptr(b["is_largest"]), ptr(b["low_sib"]), F.DEVICE_PTRS))
            check(ctx, lib.imt_itree_view_root(v, ptr(b["root"]), F.DEVICE_PTRS))
            p += 1
        q = p
        while q < n and ops_host[q] == F.OP_INSERT:
            q += 1
        if q > p:
            check(ctx, lib.imt_itree_view_insert_witness(v, q - p, ctypes.byref(buf.ins_out), F.DEVICE_PTRS))
            size += q - p
        p = q
        ctx.sync()
        lib.imt_itree_view_free(v)


def stats(name, ms):
    return {f"{name}_ms": round(float(np.median(ms)), 3), f"{name}_min_ms": round(min(ms), 3), f"{name}_max_ms": round(max(ms), 3),
            f"{name}_all_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--preload", type=int, default=20)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--log-cut", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_mixed.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    S, n, n_cut = 1 << args.preload, 1 << args.log_n, 1 << args.log_cut
    lines = [json.dumps(dict(version=lib.imt_version().decode(), device=torch.cuda.get_device_name(0), depth=DEPTH, leaves_before=S,
                             read_every=4, flags="IMT_DEVICE_PTRS, every output requested, level-major"))]
    print(lines[0], flush=True)
    cap = 1 << (args.preload + 1)
    A, B, C = (imt_amd.IndexedTree(ctx, DEPTH, cap) for _ in range(3))
    base = torch.from_numpy(bench.synth_values(S - 1, 0, 1, 0x564D4200)).to(dev)
    for t in (A, B, C):
        apply(ctx, t, base)
    del base
    snap = torch.empty((S, 3, 32), dtype=torch.uint8, device=dev)
    check(ctx, lib.imt_itree_get_leaves(A.h, None, S, ptr(snap), F.DEVICE_PTRS))
    ctx.sync()

    # ---- (a) (b) (c): the block of 2^log-n operations ----
    vals, ops, ins_vals, tail, ops_host = make_block(n, 0x564D4210, dev)
    n_ins = int((ops_host == F.OP_INSERT).sum())
    apply(ctx, A, ins_vals)
    apply(ctx, A, tail)
    head, size = A.root(), A.size
    view = A.view(S)
    build_ms = timed(ctx, view.root)
    got, want, other = Buffers(dev, n), Buffers(dev, n), Buffers(dev, n)
    ms = dict(replay=[], live=[], load=[], load_live=[])
    verified = True
    for r in range(args.repeats + 1):                    # the first round warms every arm (allocations) and is dropped
        t = dict(replay=timed(ctx, lambda: replay(ctx, view, vals, ops, got)))
        t["live"] = timed(ctx, lambda: live(ctx, B, vals, ops, want))
        check(ctx, lib.imt_itree_rewind(B.h, S, None, None, 0))
        t["load"] = timed(ctx, lambda: check(ctx, lib.imt_itree_load(C.h, ptr(snap), S, F.DEVICE_PTRS)))
        t["load_live"] = timed(ctx, lambda: live(ctx, C, vals, ops, other))
        check(ctx, lib.imt_itree_rewind(C.h, S, None, None, 0))            # the next load finds the tree tools/bench_replay.py's finds
        verified = verified and got.equal(want) and other.equal(want) and A.root() == head and A.size == size
        if r:
            for k, x in t.items():
                ms[k].append(x)
    row = dict(case="block", operations=n, inserts=n_ins, reads=n - n_ins, leaves_view=S, leaves_tree=int(size),
               repeats=args.repeats, verified=bool(verified), view_build_once_ms=round(build_ms, 3), view_builds=int(view.stats()[1]))
    for k, v in ms.items():
        row.update(stats(k, v))
    route_c = [a + b for a, b in zip(ms["load"], ms["load_live"])]
    row.update(stats("route_c", route_c))
    row["a_over_b"] = round(row["replay_ms"] / row["live_ms"], 3)
    row["a_over_b_range"] = [round(min(ms["replay"]) / max(ms["live"]), 3), round(max(ms["replay"]) / min(ms["live"]), 3)]
    row["c_over_a"] = round(row["route_c_ms"] / row["replay_ms"], 3)
    row["c_over_a_range"] = [round(min(route_c) / max(ms["replay"]), 3), round(max(route_c) / min(ms["replay"]), 3)]
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)
    view.close()
    del got, want, other, vals, ops, ins_vals, tail
    torch.cuda.empty_cache()

    # ---- (d): a block of 2^log-cut operations cut at every READ with view calls ----
    vals, ops, ins_vals, tail, ops_host = make_block(n_cut, 0x564D4220, dev)
    apply(ctx, B, ins_vals)
    apply(ctx, B, tail)
    view = B.view(S)
    buf = Buffers(dev, n_cut)
    ms = dict(d_replay=[], cut=[])
    for r in range(args.repeats + 1):
        t = dict(d_replay=timed(ctx, lambda: replay(ctx, view, vals, ops, buf)))
        t["cut"] = timed(ctx, lambda: cut_with_views(ctx, B, S, vals, ops_host, buf))
        if r:
            for k, x in t.items():
                ms[k].append(x)
    row_d = dict(case="cut", operations=n_cut, reads=n_cut // 4, leaves_view=S, leaves_tree=int(B.size), repeats=args.repeats)
    for k, v in ms.items():
        row_d.update(stats(k, v))
    row_d["cut_over_replay"] = round(row_d["cut_ms"] / row_d["d_replay_ms"], 1)
    lines.append(json.dumps(row_d))
    print(lines[-1], flush=True)
    view.close()
    sp = lambda r, k: f"{r[k + '_ms']} ms ({r[k + '_min_ms']} - {r[k + '_max_ms']})"
    lines.append(f"# 2^{args.log_n} operations behind 2^{args.preload} leaves: (a) replay {sp(row, 'replay')}, (b) live {sp(row, 'live')}, "
                 f"(c) load {sp(row, 'load')} + live {sp(row, 'load_live')} = {sp(row, 'route_c')}; (a)/(b) x{row['a_over_b']} "
                 f"{row['a_over_b_range']}, (c)/(a) x{row['c_over_a']} {row['c_over_a_range']}; view build once {row['view_build_once_ms']} ms; "
                 f"verified {row['verified']}")
    lines.append(f"# 2^{args.log_cut} operations: (d) cut at every READ with view calls {sp(row_d, 'cut')} against one replay "
                 f"{sp(row_d, 'd_replay')}: x{row_d['cut_over_replay']}")
    print("\n".join(lines[-2:]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    for t in (A, B, C):
        t.close()
    ctx.close()


if __name__ == "__main__":
    main()
