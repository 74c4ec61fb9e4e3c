"""CPU: the frontier behind a bulk replay (csrc/imt_replay.hpp frontier_*, the code k_bulk_frontier_base,
k_bulk_frontier_level and the replay's host driver run for imt_itree_view_bulk_witness).

append_sib[l] of a bulk witness is row l of the proof of the first free slot S after the rewrites of the stored low leaves.
The live call reads it from the stored tree behind its write-back; a replay writes nothing back and picks the rows up
between the level launches.  tests/native/bulk_frontier.cpp composes that on the host over the header's functions and the
sweep's own tables, with versions that are labels (level, event) instead of hashes.

The definition is tests/bulk_model.py's SparseModel: the tree as of S, the walk's rewrites played on it in the walk's
order, then proof(S).  Here its hashes are labels too -- ("view", level, node) for what the tree held at S, ("version",
event) for whatever a rewrite made, ("Z", level) for the empty subtree -- so row l of proof(S) says which node it is and
which row last wrote it.

  test_small_sizes_exhaustive      S = 1 .. 9, batches of 1 .. 4 values in every order, at the smallest depth and a deeper one
  test_random_scripts              300 scripts with S, n < 40
  test_named_edges                 S a power of two, odd, even; all of the batch in one gap; a batch that touches no leaf
                                   under a frontier node (the class must be the view's)
  test_standalone_under_sanitizers the driver as a program of its own with -fsanitize=address,undefined against a linear
                                   walk written in C++
"""
import ctypes
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import bulk_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "bulk_frontier.cpp")
ZERO, VIEW, VERSION = 0, 1, 2
NO_EVENT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("frontier") / "libbulkfrontier.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so, SRC],
                   check=True)
    lib = ctypes.CDLL(so)
    P = ctypes.POINTER
    lib.bulk_frontier_host.argtypes = [ctypes.c_uint64, ctypes.c_uint, P(ctypes.c_uint32), ctypes.c_uint32, P(ctypes.c_int),
                                       P(ctypes.c_uint64), P(ctypes.c_uint32), P(ctypes.c_uint32)]
    lib.bulk_frontier_host.restype = ctypes.c_int
    return lib


def run(lib, S, depth, lows):
    """[(class, node, event)] per level, as the device composes it"""
    low = np.asarray(lows, np.uint32)
    cls, node = np.zeros(depth, np.int32), np.zeros(depth, np.uint64)
    event, hits = np.zeros(depth, np.uint32), np.zeros(depth, np.uint32)
    P = ctypes.POINTER
    rc = lib.bulk_frontier_host(S, depth, low.ctypes.data_as(P(ctypes.c_uint32)), len(low), cls.ctypes.data_as(P(ctypes.c_int)),
                                node.ctypes.data_as(P(ctypes.c_uint64)), event.ctypes.data_as(P(ctypes.c_uint32)),
                                hits.ctypes.data_as(P(ctypes.c_uint32)))
    assert rc == 0, (S, depth, lows)
    for l in range(depth):                                  # one slot per level stores: no two may claim the version
        assert hits[l] == (1 if cls[l] == VERSION else 0), (S, depth, lows, l, int(hits[l]))
    return list(zip(cls.tolist(), node.tolist(), event.tolist()))


class LabelModel(bm.SparseModel):
    """bulk_model.SparseModel with labels for hashes: set_leaves, get and proof are the model's own"""

    def __init__(self, depth, S):
        self.depth, self.nodes, self.event = depth, {}, None
        self.Z = [("Z", l) for l in range(depth + 1)]
        for l in range(depth + 1):                          # the tree as of S: every node that has a leaf under it
            for i in range(((S - 1) >> l) + 1):
                self.nodes[(l, i)] = ("view", l, i)

    def h3(self, triples):
        return [("version", self.event)] * len(triples)

    def h2(self, pairs):
        return [("version", self.event)] * len(pairs)


def model(S, depth, lows):
    """the same list from the definition: the rewrites played on the tree as of S, then proof(S)"""
    tree = LabelModel(depth, S)
    for k, low in enumerate(lows):
        tree.event = k
        tree.set_leaves({low: None})
    out = []
    for l, label in enumerate(tree.proof(S)):
        if label[0] == "Z":
            assert label == ("Z", l) and not (S >> l) & 1
            out.append((ZERO, 0, NO_EVENT))
        elif label[0] == "view":
            assert label == ("view", l, (S >> l) - 1) and (S >> l) & 1
            out.append((VIEW, (S >> l) - 1, NO_EVENT))
        else:
            assert (S >> l) & 1
            out.append((VERSION, (S >> l) - 1, label[1]))
    return out


def lows_of(stored, vals):
    """the low leaf of every row, in the walk's order"""
    return [r["low_index"] for r in bm.bulk_walk(stored, vals)[0]]


def depths_for(S, n):
    least = max(1, (S + n - 1).bit_length())                # the shallowest tree that holds S + n leaves
    return (least, least + 3)


def test_small_sizes_exhaustive(driver):
    rng = random.Random(0xF407)
    cache, scripts = {}, 0
    for S in range(1, 10):
        leaf_vals = [10 * (i + 1) for i in range(S - 1)]
        rng.shuffle(leaf_vals)                              # leaf order is not value order
        stored = [0] + leaf_vals
        # one candidate in every gap, a second one in the lowest and in the highest gap
        cands = sorted({10 * g + 3 for g in range(S)} | {6, 10 * (S - 1) + 6})
        for n in range(1, 5):
            for batch in itertools.permutations(cands, n):
                lows = tuple(lows_of(stored, list(batch)))
                for depth in depths_for(S, n):
                    key = (S, depth, lows)
                    if key not in cache:
                        cache[key] = model(S, depth, lows)
                    assert run(driver, S, depth, lows) == cache[key], (S, depth, batch, lows)
                    scripts += 1
    assert scripts > 20000 and len(cache) > 1000, (scripts, len(cache))


def test_random_scripts(driver):
    rng = random.Random(0xF408)
    classes = set()
    for case in range(300):
        S, n = rng.randrange(1, 40), rng.randrange(1, 40)
        pool = rng.sample(range(1, 400), S - 1 + n)
        stored, vals = [0] + pool[:S - 1], pool[S - 1:]
        if case % 4 == 1:                                   # crowded: the whole batch above everything stored
            vals = rng.sample(range(1000, 2000), n)
        lows = lows_of(stored, vals)
        for depth in depths_for(S, n):
            got = run(driver, S, depth, lows)
            assert got == model(S, depth, lows), (S, depth, stored, vals)
            classes |= {c for c, _, _ in got}
    assert classes == {ZERO, VIEW, VERSION}


def test_named_edges(driver):
    def both(S, depth, lows):
        got = run(driver, S, depth, lows)
        assert got == model(S, depth, lows), (S, depth, lows)
        return got

    # S a power of two: the only left-hand sibling is node 0 of level log2 S, made by the last event whatever it touched
    for S, top in ((1, 0), (2, 1), (8, 3), (16, 4)):
        for lows in ([0], [S - 1, 0, S // 2], [S - 1] * 3):
            got = both(S, top + 2, lows)
            assert got[top] == (VERSION, 0, len(lows) - 1), (S, lows)
            assert all(g == (ZERO, 0, NO_EVENT) for l, g in enumerate(got) if l != top), (S, lows)
    # S odd: leaf S - 1 is the level-0 row; S even: level 0 is the empty leaf
    assert both(7, 5, [2, 6, 1])[0] == (VERSION, 6, 1)
    assert both(7, 5, [2, 5, 1])[0] == (VIEW, 6, NO_EVENT)
    assert both(6, 5, [2, 5, 1])[0] == (ZERO, 0, NO_EVENT)
    # all of the batch in one gap: every event rewrites the same leaf, the last one made every version above it
    got = both(13, 6, [4] * 5)
    assert got[0] == (VIEW, 12, NO_EVENT) and got[2] == (VIEW, 2, NO_EVENT) and got[3] == (VERSION, 0, 4)
    # a batch that touches no leaf under a frontier node: that row is the view's node, nothing else
    got = both(6, 5, [4, 5, 4])                             # frontier nodes (1, 2) over leaves 4 .. 5 and (2, 0) over 0 .. 3
    assert got[1] == (VERSION, 2, 2) and got[2] == (VIEW, 0, NO_EVENT)
    got = both(6, 5, [0, 3, 1])
    assert got[1] == (VIEW, 2, NO_EVENT) and got[2] == (VERSION, 0, 2)
    got = both(21, 7, [16, 17, 18, 19])                     # 10101: leaf 20, node (2, 4) over 16 .. 19, node (4, 0) over 0 .. 15
    assert got[0] == (VIEW, 20, NO_EVENT) and got[2] == (VERSION, 4, 3) and got[4] == (VIEW, 0, NO_EVENT)


def test_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bulk_frontier_main")
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DBULK_FRONTIER_MAIN", "-I", CSRC, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scripts agree with the linear walk" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
