"""Inputs and expectations for the calls that mirror the reference's own functions one to one: the dense tree
(IndexedMerkleTree::new / get_root / get_proof, src/utils.rs:20-85), the bare permutation, the 128-bit split, the
zero-hash chain and the subtree-root combiner.  Plain Python over the oracle's HASH (oracle.hash / oracle.hash2_batch);
nothing here calls oracle.tree_new or oracle.zero_hashes -- tests/test_mirror_corpus.py compares the two.

Formats: a field element x is written as x * R mod p with R = 1 (IMT_FMT_CANONICAL), 2^256 (IMT_FMT_MONT256) or
2^261 (IMT_FMT_DEVICE), 32 bytes little-endian.
"""
import functools
import random

import numpy as np

import fe_corpus
import fe_model
import oracle_lib
from oracle_lib import P, arr_ints, ints_to_arr

R_OF = {0: 1, 1: pow(2, 256, P), 2: pow(2, 261, P)}          # canonical, MONT256 (halo2curves), DEVICE (the library's)
FMTS = (0, 1, 2)
M128 = (1 << 128) - 1
GUARD, SENTINEL = 64, 0xA5


def to_fmt(a, fmt):
    if fmt == 0:
        return a
    return ints_to_arr([x * R_OF[fmt] % P for x in arr_ints(a)]).reshape(a.shape)


def from_fmt(a, fmt):
    if fmt == 0:
        return a
    inv = pow(R_OF[fmt], -1, P)
    return ints_to_arr([x * inv % P for x in arr_ints(a)]).reshape(a.shape)


def edge_values():
    """the values at which a limb carry, the 128-bit split or the reduction changes: small ones, both sides of 2^128,
    both sides of p, 2^253 (the largest power of two below p), and the values whose low k 29-bit limbs are all ones
    (k = 1..8: 2^(29k) - 1), the last of them with the top limb as large as p allows (fe_corpus.max_limbs)"""
    vals = [0, 1, 2, M128, 1 << 128, (1 << 128) + 1, P - 1, P - 2, 1 << 253]
    vals += [(1 << (fe_model.W * k)) - 1 for k in range(1, fe_model.NL)]
    vals.append(fe_model.from_limbs(fe_corpus.max_limbs(fe_model.W, P)))
    assert all(0 <= v < P for v in vals) and len(set(vals)) == len(vals)
    return vals


def mixed_values(n, seed):
    """n values < p: the edge values spread over random ones (all of them when n allows, the first and last positions
    included), seeded"""
    rng = random.Random(seed)
    vals = [rng.randrange(P) for _ in range(n)]
    edges = edge_values()
    if n >= 2 * len(edges):
        slots = [0, n - 1] + rng.sample(range(1, n - 1), len(edges) - 2)
    else:
        slots = list(range(0, n, 2))
    for s, e in zip(slots, edges):
        vals[s] = e
    return vals


class DenseModel:
    """every level of IndexedMerkleTree::new over `leaves` (uint8 [n, 32] canonical, n a power of two), bottom-up, each
    from the one below by oracle.hash2_batch"""

    def __init__(self, leaves):
        oracle = oracle_lib.load()
        leaves = np.ascontiguousarray(leaves, dtype=np.uint8).reshape(-1, 32)
        n = leaves.shape[0]
        assert n >= 1 and n & (n - 1) == 0
        self.n = n
        self.levels = [leaves.copy()]
        while self.levels[-1].shape[0] > 1:
            self.levels.append(oracle.hash2_batch(self.levels[-1].reshape(-1, 2, 32)))
        self.depth = len(self.levels) - 1
        self.root = arr_ints(self.levels[-1])[0]

    def proof(self, i):
        """siblings bottom-up, uint8 [depth, 32] (src/utils.rs:63-85)"""
        assert 0 <= i < self.n
        out = np.zeros((self.depth, 32), np.uint8)
        for l in range(self.depth):
            out[l] = self.levels[l][(i >> l) ^ 1]
        return out

    def helper(self, i):
        """1 where the node on the path is a left child (:79), as integers"""
        return [1 - ((i >> l) & 1) for l in range(self.depth)]

    def concatenated(self):
        """what imt_tree_build writes: [2n - 1][32], the levels one after the other"""
        return np.concatenate(self.levels)


def dense_model(leaves):
    return DenseModel(leaves)


@functools.lru_cache(maxsize=None)
def _zero_chain(depth):
    oracle = oracle_lib.load()
    z = [oracle.hash([0, 0, 0])]
    for _ in range(depth):
        z.append(oracle.hash([z[-1], z[-1]]))
    return tuple(z)


def zero_chain(depth):
    """Z[0] = H(0, 0, 0), Z[l + 1] = H(Z[l], Z[l]) as integers, Z[0..depth]"""
    return list(_zero_chain(depth))


@functools.lru_cache(maxsize=16)
def _top_over(sub_roots):
    return dense_model(ints_to_arr(sub_roots)).root


def combined_root(sub_roots, sub_height, depth):
    """root of the depth-`depth` tree whose leftmost 2^k subtrees of height sub_height have the given roots (integers)
    and whose other subtrees are empty: the levels over the roots, then one hash with Z[l] on the right per level"""
    oracle = oracle_lib.load()
    n = len(sub_roots)
    assert n >= 1 and n & (n - 1) == 0
    k = n.bit_length() - 1
    assert sub_height + k <= depth
    top = _top_over(tuple(int(x) for x in sub_roots))       # the same roots come back with other heights and depths
    z = zero_chain(depth)
    for l in range(sub_height + k, depth):
        top = oracle.hash([top, z[l]])
    return top


class Guarded:
    """an output buffer of `shape` with GUARD sentinel bytes on each side; the body starts out as sentinel bytes too, so
    a call that must write nothing can be shown to have written nothing"""

    def __init__(self, shape, dtype=np.uint8, alloc=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        total = GUARD + self.nbytes + GUARD
        self.raw = alloc(total) if alloc else np.empty(total, np.uint8)
        self.raw[:] = SENTINEL
        self.body = self.raw[GUARD:GUARD + self.nbytes].view(dtype).reshape(shape)
        self.ptr = self.raw.ctypes.data + GUARD

    def untouched(self):
        return bool((self.raw == SENTINEL).all())


def guarded(shape, dtype=np.uint8, alloc=None):
    return Guarded(shape, dtype, alloc)


def check_guards(buf):
    assert (buf.raw[:GUARD] == SENTINEL).all(), "wrote in front of the buffer"
    assert (buf.raw[GUARD + buf.nbytes:] == SENTINEL).all(), "wrote behind the buffer"
    return buf.body
