#!/usr/bin/env python3
"""Rate of imt_hash_n_batch (1..16 inputs) beside imt_hash2_batch / imt_hash3_batch, and of imt_hash_n_trace_batch beside
imt_hash_trace_batch.  One process, device pointers, HIP events on the context's stream; per arm one warm-up and three
timed repeats: median with min-max.  The model the value arms are compared with: time per hash proportional to its
floor(len / 2) + 1 permutations at the permutation rate of imt_hash2_batch (2 permutations per hash).
Writes profiles/hash_n.txt."""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import imt_amd  # noqa: E402

N_VALUES = 1 << 20          # hashes per value arm
N_TRACES = 1 << 14          # hashes per trace arm: 2^14 x 5443 rows x 32 bytes = 2.9 GB at 16 inputs
REPEATS = 3
F = imt_amd._ffi
lib = imt_amd.lib


def inputs(n, length):
    rng = np.random.default_rng(length)
    a = rng.integers(0, 256, size=(n, length, 32), dtype=np.uint8)
    a[:, :, 31] &= 0x0f                                   # below 2^252 < p
    return torch.from_numpy(a).cuda()


def timed(ctx, call):
    """[ms] of REPEATS runs of call() after one warm-up"""
    call()
    ctx.sync()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        ctx.sync()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def spread(xs):
    return f"{statistics.median(xs):9.3f} ({min(xs):.3f}-{max(xs):.3f})"


def main():
    ctx = imt_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lines = [f"{torch.cuda.get_device_name(0)}; {imt_amd.lib.imt_version().decode()}; one process, device pointers, format 0",
             f"values: {N_VALUES} hashes per arm, {REPEATS} repeats after one warm-up: median (min-max)", ""]
    out = torch.empty((N_VALUES, 32), dtype=torch.uint8, device="cuda")

    def check(rc):
        assert rc == 0, (rc, lib.imt_last_error(ctx.h).decode())

    fixed = {}
    for arity, fn in ((2, lib.imt_hash2_batch), (3, lib.imt_hash3_batch)):
        x = inputs(N_VALUES, arity)
        fixed[arity] = timed(ctx, lambda: check(fn(ctx.h, p(x), p(out), N_VALUES, F.DEVICE_PTRS)))
    per_perm = statistics.median(fixed[2]) / 2            # ms per 2^20 permutations, existing kernel
    lines.append(f"{'call':<24}{'ms per call':>30}{'M hashes/s':>12}{'perms':>7}{'ms per perm-batch':>32}{'vs hash2':>10}")
    for arity in (2, 3):
        t = fixed[arity]
        lines.append(f"{'imt_hash%d_batch' % arity:<24}{spread(t):>30}{N_VALUES / statistics.median(t) / 1e3:>12.2f}{2:>7}"
                     f"{spread([v / 2 for v in t]):>32}{statistics.median(t) / 2 / per_perm:>10.3f}")
    for length in (1, 2, 3, 4, 8, 16):
        x = inputs(N_VALUES, length)
        t = timed(ctx, lambda: check(lib.imt_hash_n_batch(ctx.h, p(x), length, p(out), N_VALUES, F.DEVICE_PTRS)))
        perms = length // 2 + 1
        lines.append(f"{'imt_hash_n_batch len %d' % length:<24}{spread(t):>30}{N_VALUES / statistics.median(t) / 1e3:>12.2f}{perms:>7}"
                     f"{spread([v / perms for v in t]):>32}{statistics.median(t) / perms / per_perm:>10.3f}")
        del x
    lines += ["", "  perms = floor(len / 2) + 1; 'vs hash2' = time per permutation over imt_hash2_batch's (the model says 1.000)", "",
              f"traces: {N_TRACES} hashes per arm, row-major", ""]
    del out
    lines.append(f"{'call':<32}{'ms per call':>30}{'rows':>6}{'M rows/s':>10}{'GB/s written':>14}")
    arms = [("imt_hash_trace_batch(2)", 2, lib.imt_hash_trace_batch), ("imt_hash_n_trace_batch len 2", 2, lib.imt_hash_n_trace_batch),
            ("imt_hash_n_trace_batch len 16", 16, lib.imt_hash_n_trace_batch)]
    for name, length, fn in arms:
        rows = lib.imt_hash_n_trace_rows(length)
        x = inputs(N_TRACES, length)
        tr = torch.empty((rows, N_TRACES, 32), dtype=torch.uint8, device="cuda")
        t = timed(ctx, lambda: check(fn(ctx.h, p(x), length, N_TRACES, p(tr), F.DEVICE_PTRS)))
        m = statistics.median(t)
        lines.append(f"{name:<32}{spread(t):>30}{rows:>6}{rows * N_TRACES / m / 1e3:>10.1f}{rows * N_TRACES * 32 / m / 1e6:>14.1f}")
        del x, tr
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "hash_n.txt"), "w") as f:
        f.write(text)
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
