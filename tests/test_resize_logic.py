"""CPU: the layout arithmetic of imt_itree_reserve (csrc/imt_resize.hpp, the code k_restride_levels runs).

The claim: the stored nodes of a tree are a filled prefix per level and every node outside the prefix reads as Z[l], so
the tree of another capacity is a re-layout of bytes the tree holds.  tests/native/resize_levels.cpp runs the header's
functions in a sequential loop; every expectation is imt_itree_new's formula -- level l holds max(1, capacity >> l)
nodes, levels lie one after the other -- written out here.

For depths 1, 2, 5, 32, 33, 63, 64 and every pair of power-of-two capacities up to 2^12 (2^30 and 2^31 as numbers only):
  * lengths, offsets and totals are the formula's;
  * the flat-index lookup inverts the offsets at the first and the last node of every level;
  * a tagged node array (node i of level l carries (l, i)) lands, in both directions, exactly where the formula says:
    node i of level l of the new layout is the old node i if i < old length, Z[l] otherwise."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
DEPTHS = (1, 2, 5, 32, 33, 63, 64)
CAPS = tuple(1 << k for k in range(1, 13))
BIG = (1 << 30, 1 << 31)
ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def rs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("resize") / "libresizelevels.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "native", "resize_levels.cpp")], check=True)
    lib = ctypes.CDLL(so)
    for name in ("resize_level_len", "resize_level_off", "resize_total_nodes"):
        getattr(lib, name).argtypes = [ctypes.c_uint64, ctypes.c_uint]
        getattr(lib, name).restype = ctypes.c_uint64
    lib.resize_locate.argtypes = [ctypes.c_uint64, ctypes.c_uint, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint), u64p]
    lib.resize_locate.restype = ctypes.c_int
    lib.resize_host.argtypes = [u8p, ctypes.c_uint64, u8p, ctypes.c_uint64, ctypes.c_uint, u8p]
    lib.resize_host.restype = ctypes.c_uint64
    return lib


def lens(cap, depth):
    """imt_itree_new: level l stores max(1, capacity >> l) nodes"""
    return [max(1, cap >> l) for l in range(depth + 1)]


def offs(cap, depth):
    out, at = [], 0
    for n in lens(cap, depth):
        out.append(at)
        at += n
    return out, at


def tagged(cap, depth, old_cap=None):
    """[total, 4] uint64: node i of level l is (l, i, ~l, ~i); with old_cap, nodes the old layout lacks are Z[l] = (l, ~0, ~l, 0)"""
    rows = []
    for l, n in enumerate(lens(cap, depth)):
        i = np.arange(n, dtype=np.uint64)
        if old_cap is not None:
            i[max(1, old_cap >> l):] = ONES
        lv = np.full(n, l, np.uint64)
        rows.append(np.stack([lv, i, ~lv, ~i], axis=1))
    return np.ascontiguousarray(np.concatenate(rows))


@pytest.mark.parametrize("depth", DEPTHS)
def test_lengths_and_offsets(rs, depth):
    for cap in CAPS + BIG:
        want_len = lens(cap, depth)
        want_off, total = offs(cap, depth)
        assert [rs.resize_level_len(cap, l) for l in range(depth + 1)] == want_len, (depth, cap)
        assert [rs.resize_level_off(cap, l) for l in range(depth + 1)] == want_off, (depth, cap)
        assert rs.resize_level_off(cap, depth + 1) == total == rs.resize_total_nodes(cap, depth)
        assert total < 2 * cap + depth + 1


@pytest.mark.parametrize("depth", DEPTHS)
def test_locate_inverts_the_offsets(rs, depth):
    lv, pos = ctypes.c_uint(), ctypes.c_uint64()
    for cap in CAPS + BIG:
        off, total = offs(cap, depth)
        for l, n in enumerate(lens(cap, depth)):
            for i in {0, n - 1}:
                assert rs.resize_locate(cap, depth, off[l] + i, ctypes.byref(lv), ctypes.byref(pos)) == 0
                assert (lv.value, pos.value) == (l, i), (depth, cap, l, i)
        assert rs.resize_locate(cap, depth, total, ctypes.byref(lv), ctypes.byref(pos)) == -1


@pytest.mark.parametrize("depth", DEPTHS)
def test_relayout_of_a_tagged_array(rs, depth):
    lv = np.arange(depth + 1, dtype=np.uint64)
    zero = np.ascontiguousarray(np.stack([lv, np.full(depth + 1, ONES, np.uint64), ~lv, np.zeros(depth + 1, np.uint64)], axis=1))
    src = {cap: tagged(cap, depth) for cap in CAPS}
    for a in CAPS:                 # every ordered pair: growing, shrinking and a == b
        for b in CAPS:
            want = tagged(b, depth, old_cap=a)
            got = np.full_like(want, 0xEE)
            zeros = rs.resize_host(src[a].ctypes.data_as(u8p), a, got.ctypes.data_as(u8p), b, depth, zero.ctypes.data_as(u8p))
            assert (got == want).all(), (depth, a, b)
            assert zeros == int((want[:, 1] == ONES).sum()), (depth, a, b)
            if b <= a:
                assert zeros == 0      # a shrink only drops nodes
