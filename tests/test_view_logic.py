"""CPU: the rule of a view of the indexed tree at an earlier size (csrc/imt_view.hpp, the code the kernels run).

Node x of level l as of size s is the empty subtree iff x >= ceil(s / 2^l), the side table's entry iff x is in S_l
(S_0 = relinked leaves + {s}, S_(l+1) = {x >> 1}), at its place in the level's ascending list, and the stored node
otherwise.  tests/native/view_lists.cpp builds the lists the way a view's build does (imt_rewind.hpp, imt_apply.hpp) and
classifies every node (l, x), x <= ceil(M / 2^l); every expectation here is set arithmetic over the sequential oracle's
preimages of the full and the prefix run: the relinked leaves are the kept leaves whose preimage differs.

Streams random / ascending / descending / sawtooth, tree sizes up to 1 025, cuts at 1, 2, every power of two +- 1 below M,
M - 1 and M; the small sizes again at depth 64, where the levels from 32 up exercise ceil(s / 2^l) beyond a 32-bit shift
and at a shift of 64.  The same harness is also built as a stand-alone program under the address and undefined-behaviour
sanitizers and run over streams of its own."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle_lib import ints_to_arr
from test_rewind_logic import DEPTH, SIZES, STREAMS, ceil_log2, cuts, prefix_preimages, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "view_lists.cpp")
u8p, u32p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
EMPTY, SIDE, STORED = 0, 1, 2
GXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]


@pytest.fixture(scope="module")
def vw(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("view") / "libviewlists.so")
    subprocess.run(GXX + ["-O2", "-fPIC", "-shared", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.view_host.argtypes = [u8p, u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint, ctypes.c_uint,
                              u8p, u32p, u64p]
    lib.view_host.restype = ctypes.c_int
    lib.view_nodes.argtypes = [ctypes.c_uint32, ctypes.c_uint]
    lib.view_nodes.restype = ctypes.c_uint64
    lib.view_filled.argtypes = [ctypes.c_uint64, ctypes.c_uint]
    lib.view_filled.restype = ctypes.c_uint64
    return lib


def ceil_div_pow2(s, l):
    return -(-s // (1 << l))


def expected(M, s, depth, l0, relinked):
    """(class, rank) of every node view_host classifies, in its order; None where s == M leaves the rule unused"""
    level = set(relinked) | {s} if s < M else set()
    out = []
    for l in range(depth + 1):
        asc = sorted(level)
        place = {x: r for r, x in enumerate(asc)}
        fill = ceil_div_pow2(s, l)
        for x in range(ceil_div_pow2(M, l) + 1):
            if s == M and l >= l0:
                out.append(None)
            elif x >= fill:
                out.append((EMPTY, 0))
            elif x in place:
                out.append((SIDE, place[x]))
            else:
                out.append((STORED, 0))
        level = {x >> 1 for x in level}
    return out


def run_grid(vw, oracle, kind, M, depth):
    vals = stream(kind, M - 1, 0x56570000 + M)
    allv = [0] + vals
    val = ints_to_arr(allv)
    srt = np.array(sorted(range(M), key=allv.__getitem__), np.uint32)
    pre_at = prefix_preimages(oracle, vals, 0, set(cuts(M)))       # preimages do not depend on the depth
    full = pre_at[M]
    l0 = min(ceil_log2(M), depth)
    n = vw.view_nodes(M, depth)
    assert n == sum(ceil_div_pow2(M, l) + 1 for l in range(depth + 1))
    for s in cuts(M):
        cls, rank = np.full(n, 0xEE, np.uint8), np.full(n, 0xEEEEEEEE, np.uint32)
        cnt = np.full(depth + 1, 0xDEAD, np.uint64)
        R = vw.view_host(val.ctypes.data_as(u8p), srt.ctypes.data_as(u32p), M, s, 0, l0, depth, cls.ctypes.data_as(u8p),
                         rank.ctypes.data_as(u32p), cnt.ctypes.data_as(u64p))
        tag = f"{kind} M={M} s={s} depth={depth}"
        relinked = [i for i in range(s) if not (pre_at[s][i] == full[i]).all()]
        assert R == len(relinked), tag
        want = expected(M, s, depth, l0, relinked)
        assert len(want) == n
        got = list(zip(cls.tolist(), rank.tolist()))
        bad = [k for k in range(n) if want[k] is not None and got[k] != want[k]]
        assert not bad, f"{tag}: node #{bad[0]} is {got[bad[0]]}, expected {want[bad[0]]}"


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("kind", STREAMS)
def test_view_rule(vw, oracle, kind, M):
    run_grid(vw, oracle, kind, M, DEPTH)


@pytest.mark.parametrize("M", (2, 3, 18))
@pytest.mark.parametrize("kind", STREAMS)
def test_view_rule_depth_64(vw, oracle, kind, M):
    run_grid(vw, oracle, kind, M, 64)


def test_filled_at_every_shift(vw):
    for s in (0, 1, 2, 3, (1 << 31), (1 << 32) - 1, (1 << 32) + 1, (1 << 63), (1 << 64) - 1):
        for l in list(range(66)) + [100]:
            assert vw.view_filled(s, l) == -(-s // (1 << l)), (s, l)


def test_refused_arguments(vw):
    z = np.zeros(96, np.uint8)
    p8, p32, p64 = z.ctypes.data_as(u8p), z.ctypes.data_as(u32p), z.ctypes.data_as(u64p)
    assert vw.view_host(p8, p32, 4, 0, 0, 2, 4, p8, p32, p64) == -1
    assert vw.view_host(p8, p32, 4, 5, 0, 2, 4, p8, p32, p64) == -1
    assert vw.view_host(p8, p32, 4, 2, 0, 32, 40, p8, p32, p64) == -1


def test_harness_under_sanitizers(tmp_path):
    """the same functions as a stand-alone program built with -fsanitize=address,undefined, on the CPU"""
    exe = str(tmp_path / "view_lists_san")
    subprocess.run(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DVIEW_LISTS_MAIN",
                          "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cuts ok" in r.stdout
