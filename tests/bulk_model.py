"""The bulk witness form of imt_itree_insert_bulk (include/imt.h) as a plain walk, and a sparse tree to hash it with.

bulk_walk is the definition: the batch in descending value order, each value's low leaf the stored leaf with the largest
value below it, the preimages as the rewrites before it left them.  It knows nothing of how the library finds them (the
neighbour above in the sorted batch, imt_prep_logic.hpp bulk_row).  SparseModel is a dict of nodes over the oracle's
hashes; bulk_witness plays the rewrites on it in that order and then the append.
"""
import bisect


P = 21888242871839275222246405745257275088548364400416034343698204186575808495617

REFUSED_ZERO, REFUSED_NONCANONICAL, REFUSED_DUPLICATE = "zero", "noncanonical", "duplicate"


class Refused(Exception):
    pass


def refusal(stored, vals):
    """why the library refuses the batch, or None; the order of the checks is insertion_verdict's"""
    if any(v >= P for v in vals):
        return REFUSED_NONCANONICAL
    if any(v == 0 for v in vals):
        return REFUSED_ZERO
    if len(set(vals)) != len(vals) or set(vals) & set(stored):
        return REFUSED_DUPLICATE
    return None


def bulk_walk(stored, vals):
    """stored: the values in leaf order, stored[0] == 0 the sentinel; vals: the batch in the caller's order.
    Returns (rows, new_leaves): rows[k] = dict(order, low_index, low_leaf=(val, next_val, next_idx), is_largest, rewritten),
    new_leaves[i] = the final preimage of leaf M + i."""
    why = refusal(stored, vals)
    if why:
        raise Refused(why)
    M = len(stored)
    by_val = sorted((v, i) for i, v in enumerate(stored))
    keys = [v for v, _ in by_val]
    nxt = {}                                                    # stored leaf -> (next_val, next_idx) as the walk goes on
    for r, (_, i) in enumerate(by_val):
        nxt[i] = by_val[r + 1] if r + 1 < M else (0, 0)
    rows, new_leaves = [], [None] * len(vals)
    for i in sorted(range(len(vals)), key=lambda i: -vals[i]):
        v = vals[i]
        low = by_val[bisect.bisect_left(keys, v) - 1][1]        # the stored predecessor: never a leaf of the batch
        before = (stored[low],) + tuple(nxt[low])
        new_leaves[i] = (v,) + tuple(nxt[low])                  # everything larger is in: that is v's final successor
        nxt[low] = (v, M + i)
        rows.append(dict(order=i, low_index=low, low_leaf=before, is_largest=int(before[1] == 0),
                         rewritten=(stored[low], v, M + i)))
    return rows, new_leaves


def final_preimages(stored, vals):
    """the leaves of the tree after insert_batch(vals): one sorted linked list over stored + vals"""
    allv = list(stored) + list(vals)
    by_val = sorted((v, i) for i, v in enumerate(allv))
    out = [None] * len(allv)
    for r, (v, i) in enumerate(by_val):
        out[i] = (v,) + (by_val[r + 1] if r + 1 < len(allv) else (0, 0))
    return out


class SparseModel:
    """nodes[(level, index)], anything absent the empty subtree of that height"""

    def __init__(self, orc, depth):
        from oracle_lib import arr_ints, ints_to_arr
        self.orc, self.depth = orc, depth
        self._ints, self._arr = arr_ints, ints_to_arr
        self.Z = arr_ints(orc.zero_hashes(depth))
        self.nodes = {}

    def get(self, l, i):
        return self.nodes.get((l, i), self.Z[l])

    def h3(self, triples):
        return self._ints(self.orc.hash3_batch(self._arr([x for t in triples for x in t]).reshape(-1, 3, 32)))

    def h2(self, pairs):
        return self._ints(self.orc.hash2_batch(self._arr([x for p in pairs for x in p]).reshape(-1, 2, 32)))

    def set_leaves(self, leaves):
        """leaves: {index: (val, next_val, next_idx)}; every node above them once"""
        idx = sorted(leaves)
        for i, h in zip(idx, self.h3([leaves[i] for i in idx])):
            self.nodes[(0, i)] = h
        for l in range(self.depth):
            idx = sorted({i >> 1 for i in idx})
            for i, h in zip(idx, self.h2([(self.get(l, 2 * i), self.get(l, 2 * i + 1)) for i in idx])):
                self.nodes[(l + 1, i)] = h

    def proof(self, i):
        return [self.get(l, (i >> l) ^ 1) for l in range(self.depth)]

    def root(self):
        return self.get(self.depth, 0)


def bulk_witness(orc, depth, stored, vals):
    """every output of imt_itree_insert_bulk as ints / lists of ints, from the walk and the sparse model"""
    rows, new_leaves = bulk_walk(stored, vals)
    M = len(stored)
    tree = SparseModel(orc, depth)
    tree.set_leaves(dict(enumerate(final_preimages(stored, []))))
    for r in rows:
        r["root_before"] = tree.root()
        r["low_sib"] = tree.proof(r["low_index"])
        tree.set_leaves({r["low_index"]: r["rewritten"]})
        r["root_after"] = tree.root()
    append_sib = tree.proof(M)
    assert all(append_sib[l] == tree.Z[l] for l in range(depth) if not (M >> l) & 1)
    tree.set_leaves({M + i: p for i, p in enumerate(new_leaves)})
    return dict(rows=rows, new_leaf=new_leaves, append_sib=append_sib, root=tree.root(), model=tree)


def frontier_append(orc, depth, sib, start, leaf_hashes):
    """(root_before, root_after) of imt_frontier_append_root: the sparse model seeded with the left-hand siblings"""
    tree = SparseModel(orc, depth)

    def climb(nodes):
        # nodes: {(level 0 index): hash}; returns the root with siblings from `sib` on the left, Z on the right
        level = dict(nodes)
        for l in range(depth):
            up = {}
            for i in sorted({j >> 1 for j in level}):
                a = level.get(2 * i, sib[l] if (start >> l) & 1 and 2 * i == (start >> l) ^ 1 else tree.Z[l])
                b = level.get(2 * i + 1, tree.Z[l])
                up[i] = tree.h2([(a, b)])[0]
            level = up
        return level[0]

    before = climb({start: tree.Z[0]})
    after = climb({start + j: h for j, h in enumerate(leaf_hashes)})
    return before, after
