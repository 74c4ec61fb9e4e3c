"""Operands and items for the gadget tests at every lookup width (TEST INFRASTRUCTURE ONLY), shared by
tests/test_gadget_widths_cpu.py and tests/test_gpu_gadget_widths.py.

  less_than_pairs(lb)     the operand pairs of one width: fixed edges, random pairs, pairs that share their high limb,
                          and for every limb boundary e = 0, lb, 2 lb, ... < 128 the pairs (2^e, 2^e - 1), (2^e - 1, 2^e)
                          in the low half and, shifted by 128 and kept below p, in the high half
  coverage(lb, pairs)     what those pairs exercise, read off the rows of the Python model alone
  insert_items(d, n, s)   real insertions into an oracle sparse tree (depth 64: forged, as witness_corpus does it)
  non_members(d, n, s)    real non-membership witnesses of such a tree
  reject(items)           every third item turned into a witness the circuit rejects
  chain_pairs(items)      the `pairs` array the C entries hand to the insert-gadget kernel, from the oracle's hash
"""
import functools
import random

import numpy as np

import oracle_lib
import witness_corpus as wc
from oracle_lib import P, arr_ints, ints_to_arr
from test_gadget_cpu import EDGE

WIDTHS = tuple(range(1, 29))
M128 = (1 << 128) - 1


def limbs_of(lb):
    """(k, padded, L) of range.is_less_than(., ., 128) at lookup_bits = lb"""
    k = -(-128 // lb)
    return k, k * lb, k + 1


def less_than_rows(lb):
    return 4 * limbs_of(lb)[2] + 27


@functools.lru_cache(maxsize=None)
def less_than_pairs(lb):
    rng = random.Random(0x494D5700 + lb)
    pairs = list(EDGE)
    pairs += [(rng.randrange(P), rng.randrange(P)) for _ in range(24)]
    pairs += [((q << 128) + rng.randrange(1 << 128), (q << 128) + rng.randrange(1 << 128))
              for q in (0, 1, rng.randrange(1 << 120), rng.randrange(1 << 125))]
    for e in range(0, 128, lb):
        pairs += [(1 << e, (1 << e) - 1), ((1 << e) - 1, 1 << e)]
        if (1 << (128 + e)) < P:
            pairs += [(1 << (128 + e), (1 << (128 + e)) - 1), ((1 << (128 + e)) - 1, 1 << (128 + e))]
    pairs += [(M128, 0), (0, M128), ((1 << 253) - 1, 0), (0, (1 << 253) - 1)]
    assert all(0 <= a < P and 0 <= b < P for a, b in pairs)
    return tuple(pairs)


def padded_pairs(lb, block=128):
    """the pairs of one width, filled up with random pairs to one past a multiple of the block"""
    pairs = list(less_than_pairs(lb))
    rng = random.Random(0x494D5780 + lb)
    n = -(-(len(pairs) - 1) // block) * block + 1
    return pairs + [(rng.randrange(P), rng.randrange(P)) for _ in range(n - len(pairs))]


def range_block(rows, start, lb):
    """(shifted difference, limbs, running sums, is_zero's z) of the range.is_less_than block that begins at `start`"""
    L = limbs_of(lb)[2]
    limbs = [rows[start + 2]] + [rows[start + 3 + 2 * (i - 1)] for i in range(1, L)]
    sums = [rows[start + 4 + 2 * (i - 1)] for i in range(1, L)]
    return rows[start], limbs, sums, rows[start + 2 * L + 3]


def coverage(lb, pairs):
    """What `pairs` exercise at width lb, computed from oracle_lib.less_than_rows_model's rows only (never from the
    code under test): the outcomes of the two range.is_less_than and the two is_equal calls, the top limbs seen in
    each half, whether an inner limb was all ones / zero, and whether a limb had bits on both sides of a 32-bit word
    boundary of the shifted difference."""
    L = limbs_of(lb)[2]
    R = 2 * L + 4                                            # rows of one range.is_less_than block; is_equal has 4
    seen = dict(msb_lt=set(), msb_eq=set(), lsb_lt=set(), lsb_eq=set(), top_zero=[set(), set()], inner_ones=False,
                inner_zero=False, straddle=False, out=set())
    for a, b in pairs:
        rows, out = oracle_lib.less_than_rows_model(a, b, lb)
        assert len(rows) == 2 * R + 8 + 11
        seen["out"].add(out)
        for name, r in (("msb_lt", R - 1), ("msb_eq", R + 3), ("lsb_lt", 2 * R + 3), ("lsb_eq", 2 * R + 7)):
            assert rows[r] in (0, 1)
            seen[name].add(rows[r])
        for half, start in enumerate((0, R + 4)):
            _, limbs, _, _ = range_block(rows, start, lb)
            seen["top_zero"][half].add(limbs[-1] == 0)
            for i in range(1, L - 1):
                seen["inner_ones"] |= limbs[i] == (1 << lb) - 1
                seen["inner_zero"] |= limbs[i] == 0
                lo, hi = i * lb, i * lb + lb - 1
                if lo // 32 != hi // 32:
                    cut = 32 * (hi // 32) - lo               # bits of the limb below the word boundary
                    seen["straddle"] |= bool(limbs[i] & ((1 << cut) - 1)) and bool(limbs[i] >> cut)
    return seen


# ---------------------------------------------------------------- insert_leaf / verify_non_inclusion items
@functools.lru_cache(maxsize=None)
def _tree(depth, n, seed):
    """n real insertions into an oracle sparse tree and the witnesses of n values the final tree does not hold"""
    orc = oracle_lib.load()
    cap = min(1 << depth, 1 << n.bit_length())               # a power of two that holds the sentinel too
    h = orc.sparse_new(depth, cap)
    stored, ins = {0: 0}, []
    try:
        for i, v in enumerate(oracle_lib.synth_values(n, seed)):
            o = orc.sparse_insert(h, depth, v)
            assert o["rc"] == 0, o["rc"]
            low = arr_ints(o["low_leaf"])
            ins.append(dict(depth=depth, low_leaf=low, low_index=o["low"], low_sib=arr_ints(o["low_proof"]),
                            new_leaf=[v, low[1], low[2]], new_index=1 + i, new_path_index=1 + i,
                            new_sib=arr_ints(o["new_proof"]), is_largest=o["largest"]))
            stored[v] = 1 + i
        order = sorted(stored)
        rng = random.Random(seed + 1)
        cands = [order[-1] + 1 + rng.randrange(1 << 20), 1]  # above the largest; just above the sentinel
        cands += [v + 1 for v in order[1:] if v + 1 not in stored]
        nm = []
        for c in cands[:n]:
            li = stored[max(v for v in order if v < c)]
            ll = arr_ints(orc.sparse_preimage(h, li))
            nm.append(dict(depth=depth, low_leaf=ll, low_index=li, low_sib=arr_ints(orc.sparse_proof(h, depth, li)),
                           new_val=c, is_largest=int(ll[1] == 0)))
    finally:
        orc.sparse_free(h)
    return ins, nm


def insert_items(depth, n, seed):
    """n insert_leaf witnesses: real insertions into the oracle's sparse tree; that tree stops at depth 63, so depth 64
    is forged the way witness_corpus does it"""
    if depth == 64:
        return wc._forged_honest(oracle_lib.load(), random.Random(seed), 64, n)
    return [dict(w) for w in _tree(depth, n, seed)[0]]


def non_members(depth, n, seed):
    return [dict(w) for w in _tree(depth, n, seed)[1]]


def reject(items):
    """every third item changed into a witness the circuit rejects, in turn: is_largest flipped, the new value swapped
    with low.val, new_path_index != new_index (an insert_leaf witness only; a bare candidate gets the flip instead)"""
    out = []
    for j, w in enumerate(items):
        w = dict(w, low_leaf=list(w["low_leaf"]))
        kind = (j // 3) % 3 if j % 3 == 2 else None
        if kind == 2 and "new_leaf" not in w:
            kind = 0
        if kind == 0:
            w["is_largest"] = 1 - w["is_largest"]
        elif kind == 1 and "new_leaf" in w:
            w["new_leaf"] = [w["low_leaf"][0]] + list(w["new_leaf"][1:])
            w["low_leaf"][0] = items[j]["new_leaf"][0]
        elif kind == 1:
            w["new_val"], w["low_leaf"][0] = w["low_leaf"][0], w["new_val"]
        elif kind == 2:
            w["new_path_index"] = w["new_index"] ^ 1
        out.append(w)
    return out


def with_rejected(items):
    """the items as they are, then one copy of each with every kind of rejection (for the small CPU corpora)"""
    out = [dict(w) for w in items]
    for w in items:
        out += [dict(w, is_largest=1 - w["is_largest"]),
                dict(w, low_leaf=[w["new_leaf"][0]] + list(w["low_leaf"][1:]), new_leaf=[w["low_leaf"][0]] + list(w["new_leaf"][1:])),
                dict(w, new_path_index=w["new_index"] ^ 1)]
    return out


def chain_pairs(items, whole=True):
    """uint8 [chains][depth][n][2][32], canonical: the (left, right) inputs of every path hash of the four chains of
    insert_leaf (whole) or of the low leaf's chain alone, built with the oracle's hash as
    oracle_lib.insert_gadget_rows_model's chain() walks them"""
    orc = oracle_lib.load()
    depth, n = items[0]["depth"], len(items)
    out = np.zeros((4 if whole else 1, depth, n, 2, 32), np.uint8)
    for i, w in enumerate(items):
        low = w["low_leaf"]
        chains = [(orc.hash(low), w["low_index"], w["low_sib"])]
        if whole:
            chains += [(orc.hash([low[0], w["new_leaf"][0], w["new_index"]]), w["low_index"], w["low_sib"]),
                       (orc.hash([0, 0, 0]), w["new_path_index"], w["new_sib"]),
                       (orc.hash(w["new_leaf"]), w["new_path_index"], w["new_sib"])]
        for c, (cur, index, sib) in enumerate(chains):
            for l in range(depth):
                pair = [sib[l], cur] if (index >> l) & 1 else [cur, sib[l]]
                out[c, l, i] = ints_to_arr(pair)
                cur = orc.hash(pair)
    return out


def stacked(items):
    """the items as the arrays the entry points take (siblings level-major [depth][n][32])"""
    n, depth = len(items), items[0]["depth"]
    a = dict(low_leaf=ints_to_arr([x for w in items for x in w["low_leaf"]]).reshape(n, 3, 32),
             low_index=np.array([w["low_index"] for w in items], np.uint64),
             low_sib=np.ascontiguousarray(ints_to_arr([x for w in items for x in w["low_sib"]]).reshape(n, depth, 32).transpose(1, 0, 2)),
             is_largest=np.array([w["is_largest"] for w in items], np.uint8))
    if "new_leaf" in items[0]:
        a.update(new_leaf=ints_to_arr([x for w in items for x in w["new_leaf"]]).reshape(n, 3, 32),
                 new_index=np.array([w["new_index"] for w in items], np.uint64),
                 new_path_index=np.array([w["new_path_index"] for w in items], np.uint64),
                 new_sib=np.ascontiguousarray(ints_to_arr([x for w in items for x in w["new_sib"]]).reshape(n, depth, 32).transpose(1, 0, 2)))
    else:
        a.update(new_val=ints_to_arr([w["new_val"] for w in items]))
    return a


def oracle_insert_rows(w, lb):
    rows, segs = oracle_lib.load().insert_gadget_trace(w["low_leaf"], w["low_index"], ints_to_arr(w["low_sib"]), w["new_leaf"],
                                                       w["new_index"], ints_to_arr(w["new_sib"]), w["is_largest"], w["depth"], lb,
                                                       new_path_index=w["new_path_index"])
    return rows, segs


def oracle_non_inclusion_rows(w, lb):
    new_val = w["new_val"] if "new_val" in w else w["new_leaf"][0]
    return oracle_lib.load().non_inclusion_gadget_trace(w["low_leaf"], w["low_index"], ints_to_arr(w["low_sib"]), new_val,
                                                        w["is_largest"], w["depth"], lb)


def model_insert_rows(w, lb):
    return oracle_lib.insert_gadget_rows_model(oracle_lib.load(), w["low_leaf"], w["low_index"], ints_to_arr(w["low_sib"]),
                                               w["new_leaf"], w["new_index"], ints_to_arr(w["new_sib"]), w["is_largest"],
                                               w["depth"], lb, new_path_index=w["new_path_index"])


def scaled(rows, factor):
    """uint8 [..., 32] canonical -> every value times `factor` mod p (the Montgomery forms), each distinct value once"""
    a = np.ascontiguousarray(rows, dtype=np.uint8)
    flat = a.reshape(-1, 32)
    uniq, inv = np.unique(flat.view("V32").ravel(), return_inverse=True)
    conv = ints_to_arr([int.from_bytes(u.tobytes(), "little") * factor % P for u in uniq])
    return conv[inv].reshape(a.shape)
