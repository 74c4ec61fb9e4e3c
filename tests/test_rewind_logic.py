"""CPU: the index work of imt_itree_rewind (csrc/imt_rewind.hpp, the code the kernels run).

The claim: the tree of s leaves is a function of the first s values, which the tree of M >= s leaves still holds, so
going back needs no journal.  tests/native/rewind_lists.cpp composes the header's functions the way the device does
(one scan, one compaction, one relink pass, a sort, then the list building of imt_apply.hpp); every expectation is the
sequential oracle's (Oracle.sparse_insert / sparse_preimage) or set arithmetic written out here.

For the stream orders random / ascending / descending / sawtooth, tree sizes up to 1 025 and cuts at 1, 2, every
power of two +- 1 below M, M - 1 and M:
  * the compacted index is the index of the prefix;
  * the relinked leaves are exactly the kept leaves whose oracle preimage differs between the full and the prefix run,
    and their new preimages are the prefix run's (global next_idx on a placed tree);
  * the table is S_0 = relinked + {s} ascending with one preimage row each, slot s all zero;
  * the lists of every level are S_l, the counts |S_l| below L0 = ceil(log2(M)) and 1 from there to the depth;
  * the refilled ranges are the nodes that lie wholly in [s, M)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from oracle_lib import arr_ints, ints_to_arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
u8p, u32p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
DEPTH, CAP = 12, 2048
STREAMS = ("random", "ascending", "descending", "sawtooth")
SIZES = (2, 3, 18, 300, 1024, 1025)


@pytest.fixture(scope="module")
def rw(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rewind") / "librewindlists.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "native", "rewind_lists.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.rewind_host.argtypes = [u8p, u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint, ctypes.c_uint,
                                u32p, u32p, u32p, u32p, u32p, u8p, u32p, u64p]
    lib.rewind_host.restype = ctypes.c_int
    lib.rewind_refill_range.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint, u64p, u64p]
    lib.rewind_refill_range.restype = None
    return lib


def stream(kind, n, seed):
    v = oracle_lib.synth_values(n, seed)
    if kind == "ascending":
        return sorted(v)
    if kind == "descending":
        return sorted(v, reverse=True)
    if kind == "sawtooth":
        s, ramps = sorted(v), max(2, int(n ** 0.5))
        return [x for r in range(ramps) for x in s[r::ramps]]
    return v


def cuts(M):
    out = {1, 2, M - 1, M}
    p = 2
    while p < M:
        out |= {p - 1, p + 1}
        p *= 2
    return sorted(c for c in out if 1 <= c <= M)


def ceil_log2(x):
    return max(0, (x - 1).bit_length())


def prefix_preimages(oracle, vals, base, at):
    """{s: [s, 3, 32] preimages of the tree that holds the first s - 1 values} for every s in `at`, from one run"""
    h = oracle.sparse_new(DEPTH, CAP)
    oracle.sparse_set_index_base(h, base)
    out = {}
    try:
        for i in range(len(vals) + 1):
            if i + 1 in at:
                out[i + 1] = np.stack([oracle.sparse_preimage(h, k) for k in range(i + 1)])
            if i < len(vals):
                assert oracle.sparse_insert(h, DEPTH, vals[i])["rc"] == 0
    finally:
        oracle.sparse_free(h)
    return out


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("kind", STREAMS)
def test_rewind_index_work(rw, oracle, kind, M):
    base = (5 << DEPTH) if kind == "random" else 0           # one stream on a placed tree: next_idx is global
    vals = stream(kind, M - 1, 0x52570000 + M)
    allv = [0] + vals
    sorted_idx = sorted(range(M), key=allv.__getitem__)
    val = ints_to_arr(allv)
    srt = np.array(sorted_idx, np.uint32)
    pre_at = prefix_preimages(oracle, vals, base, set(cuts(M)))
    full = pre_at[M]
    l0 = min(ceil_log2(M), DEPTH)
    for s in cuts(M):
        rows = min(M - s, s) + 1
        compact = np.full(s, 0xFFFFFFFF, np.uint32)
        node, time = np.full(rows, 0xFFFFFFFF, np.uint32), np.full(rows, 0xFFFFFFFF, np.uint32)
        rs, re = np.full(rows, 0xFFFFFFFF, np.uint32), np.full(rows, 0xFFFFFFFF, np.uint32)
        pre = np.full((rows, 3, 32), 0xEE, np.uint8)
        lists = np.full((max(l0, 1), rows), 0xFFFFFFFF, np.uint32)
        cnt = np.full(DEPTH + 1, 0xDEAD, np.uint64)
        R = rw.rewind_host(val.ctypes.data_as(u8p), srt.ctypes.data_as(u32p), M, s, base, l0, DEPTH,
                           compact.ctypes.data_as(u32p), node.ctypes.data_as(u32p), time.ctypes.data_as(u32p),
                           rs.ctypes.data_as(u32p), re.ctypes.data_as(u32p), pre.ctypes.data_as(u8p),
                           lists.ctypes.data_as(u32p), cnt.ctypes.data_as(u64p))
        tag = f"{kind} M={M} s={s}"
        # the index of the prefix
        assert compact.tolist() == sorted(range(s), key=allv.__getitem__), tag
        # the leaves whose preimage differs between the two oracle runs
        want = pre_at[s]
        diff = [i for i in range(s) if not (want[i] == full[i]).all()]
        assert R == len(diff), tag
        if s == M:
            assert R == 0
            continue
        S = sorted(set(diff) | {s})
        assert node[:R + 1].tolist() == S, tag
        assert sorted(time[:R + 1].tolist()) == list(range(R + 1)) and rs[:R + 1].tolist() == list(range(R + 1))
        assert re[:R + 1].tolist() == list(range(1, R + 2)), tag
        for x, leaf in enumerate(S):
            got = pre[time[x]]
            assert (got == (want[leaf] if leaf < s else 0)).all(), f"{tag} leaf {leaf}"
        assert (pre[R + 1:] == 0xEE).all() and (node[R + 1:] == 0xFFFFFFFF).all(), "rows beyond R + 1 are not written"
        # the lists and counts of every level: S_l below L0, the single chain above
        level = set(S)
        for l in range(l0):
            k = len(level)
            assert cnt[l] == k and lists[l, :k].tolist() == sorted(level), f"{tag} level {l}"
            assert (lists[l, k:] == 0xFFFFFFFF).all()
            level = {x >> 1 for x in level}
        assert cnt[l0:].tolist() == [1] * (DEPTH + 1 - l0), tag
        # the nodes that become the empty subtree again: wholly inside [s, M)
        for l in range(DEPTH + 1):
            lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
            rw.rewind_refill_range(s, M, l, ctypes.byref(lo), ctypes.byref(hi))
            emptied = {i >> l for i in range(s, M)} - {i >> l for i in range(s)}
            assert set(range(lo.value, hi.value)) == emptied, f"{tag} level {l}"
            # every other node with a removed leaf below it straddles the cut: an ancestor of slot s, which is hashed
            assert {i >> l for i in range(s, M)} - emptied <= {s >> l}


def test_refused_arguments(rw):
    z = np.zeros(96, np.uint8)
    p8, p32, p64 = z.ctypes.data_as(u8p), z.ctypes.data_as(u32p), z.ctypes.data_as(u64p)
    assert rw.rewind_host(p8, p32, 4, 0, 0, 2, 4, p32, p32, p32, p32, p32, p8, p32, p64) == -1
    assert rw.rewind_host(p8, p32, 4, 5, 0, 2, 4, p32, p32, p32, p32, p32, p8, p32, p64) == -1
