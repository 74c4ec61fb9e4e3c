"""CPU: pins tests/mirror_corpus.py -- the model tests/test_gpu_mirror_edges.py judges the kernels by -- to the oracle's
own dense tree and zero table and to the golden file, before it is used on anything."""
import json
import os

import numpy as np
import pytest

import mirror_corpus as mc
from oracle_lib import P, arr_ints, ints_to_arr

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "vectors.json")))


def test_formats_round_trip_and_edge_values():
    e = mc.edge_values()
    for v in (0, 1, 2, (1 << 128) - 1, 1 << 128, (1 << 128) + 1, P - 1, P - 2, 1 << 253, (1 << 29) - 1, (1 << 232) - 1):
        assert v in e
    top = max(x for x in e if x & ((1 << 232) - 1) == (1 << 232) - 1)       # low eight limbs all ones
    assert top >> 232 == (P >> 232) - 1 and top + (1 << 232) >= P            # ... and the top limb as large as p allows
    a = ints_to_arr(e)
    assert mc.R_OF == {0: 1, 1: (1 << 256) % P, 2: (1 << 261) % P}
    for fmt in mc.FMTS:
        b = mc.to_fmt(a, fmt)
        assert arr_ints(b) == [x * mc.R_OF[fmt] % P for x in e]
        assert (mc.from_fmt(b, fmt) == a).all()
    for n in (1, 2, 4, 64, 1024):
        v = mc.mixed_values(n, 5)
        assert len(v) == n and all(0 <= x < P for x in v) and v == mc.mixed_values(n, 5)
    assert set(e) <= set(mc.mixed_values(64, 5)) and mc.mixed_values(64, 5)[0] == 0


@pytest.mark.parametrize("n", [1, 2, 4, 64, 1024])
def test_dense_model_equals_the_oracles_tree(oracle, n):
    leaves = ints_to_arr(mc.mixed_values(n, 100 + n))
    m = mc.dense_model(leaves)
    rc, ot = oracle.tree_new(leaves)
    assert rc == 0 and m.depth + 1 == oracle.lib.orc_tree_num_levels(ot) and m.n == n
    for l in range(m.depth + 1):
        assert (m.levels[l] == oracle.tree_level(ot, l)).all(), l
    assert m.root == oracle.tree_root(ot)
    assert m.concatenated().shape == (2 * n - 1, 32)
    for i in (range(n) if n <= 64 else (0, 1, n // 2 - 1, n // 2, n - 1, 300)):
        op, oh = oracle.tree_proof(ot, i)
        assert (m.proof(i) == op).all() and m.helper(i) == arr_ints(oh), i
        assert oracle.path_root(arr_ints(leaves[i])[0], i, m.proof(i)) == m.root
    oracle.tree_free(ot)


def test_zero_chain_equals_the_oracles_table_and_the_golden_roots(oracle):
    z = mc.zero_chain(64)
    assert len(z) == 65 and z == arr_ints(oracle.zero_hashes(64))
    assert mc.zero_chain(0) == z[:1] == [oracle.hash([0, 0, 0])]
    seen = 0
    for e in GOLD["entries"]:
        if e["kind"] == "empty_root":
            assert z[int(e["in"][0])] == int(e["out"])
            seen += 1
    assert seen >= 2


@pytest.mark.parametrize("k", [0, 1, 6, 10])
def test_all_empty_dense_tree_is_the_zero_chain(oracle, k):
    """2^k leaves all Z[0]: every node of level l is Z[l] -- the dense build and the zero chain are one computation"""
    z = mc.zero_chain(k)
    m = mc.dense_model(ints_to_arr([z[0]] * (1 << k)))
    for l in range(k + 1):
        assert arr_ints(m.levels[l]) == [z[l]] * (1 << (k - l)), l
    assert m.root == z[k]


def test_combined_root_of_empty_subtrees_is_the_zero_chain(oracle):
    z = mc.zero_chain(64)
    assert mc.combined_root([z[3]] * 8, 3, 6) == z[6]
    assert mc.combined_root([z[3]], 3, 64) == z[64]
    assert mc.combined_root([z[0]] * 4, 0, 64) == z[64]


def test_combined_root_of_a_trees_own_level_is_its_root(oracle):
    m = mc.dense_model(ints_to_arr(mc.mixed_values(64, 7)))
    sub = arr_ints(m.levels[3])
    assert len(sub) == 8 and mc.combined_root(sub, 3, 6) == m.root
    for l in range(7):
        assert mc.combined_root(arr_ints(m.levels[l]), l, 6) == m.root, l
    # above the subtrees: one hash with the empty subtree of that height on the right per level
    z = mc.zero_chain(8)
    assert mc.combined_root(sub, 3, 8) == oracle.hash([oracle.hash([m.root, z[6]]), z[7]])
    assert mc.combined_root([5], 0, 0) == 5


def test_guarded_buffers_notice_a_write_on_either_side():
    g = mc.guarded((3, 32))
    assert g.body.shape == (3, 32) and g.untouched() and g.ptr % 16 == g.raw.ctypes.data % 16
    g.body[:] = 0
    assert (mc.check_guards(g) == 0).all() and not g.untouched()
    for pos in (mc.GUARD - 1, mc.GUARD + 96):
        h = mc.guarded((3, 32))
        h.raw[pos] = 0
        with pytest.raises(AssertionError):
            mc.check_guards(h)
    w = mc.guarded(5, np.uint64)
    assert w.body.dtype == np.uint64 and w.nbytes == 40
