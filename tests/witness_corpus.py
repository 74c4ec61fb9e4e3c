"""Deterministic corpus of relation-checker witnesses that must pass or fail (TEST INFRASTRUCTURE ONLY).

Every record carries every input of one checker call and the CPU oracle's answers for it; nothing here is a
hand-written mask.  Three checkers are covered:

  insert    insert_leaf (src/indexed_merkle_tree.rs:231-314): fail mask + the 7-row trace of oracle.insert_leaf
  nonmem    verify_non_inclusion (:127-229): fail mask + the recomputed root of oracle.verify_non_inclusion
  path      verify_proof / compute_merkle_root (src/utils.rs:87-107, :78-96): root of oracle.path_root + ok bit

Witnesses start from real insertions into, and real non-members of, oracle sparse trees at depths 1, 3 and 32.  The
oracle's sparse tree stops at depth 63, so depth-64 witnesses (and witnesses with chosen values at every depth) come from
`forge_insert`, which builds a self-consistent witness from random siblings: the low leaf's path, the rewritten low
leaf's path and the zero leaf's path at the new slot meet where the two indices part.

Records (`group`):
  honest    a valid witness (mask 0)
  mutation  one field of an honest witness changed; `base_mask` is the honest mask, `noop` marks the documented no-ops
            (index bits at or above the depth, which no path reads)
  reseal    one field changed, then every root the witness itself supplies (old_root, new_root) recomputed from the
            oracle's trace, so that one constraint alone is left to catch it; `alone` names that bit
  edge      range-predicate edge values (new = low.val, low.val + 1, next_val - 1, next_val; pairs that straddle 2^128
            or share their high 128 bits; 0 and p - 1; next_val = 0 with is_largest 0 and 1), valid and invalid, in a
            witness whose paths all hold
"""
import functools
import random

import numpy as np

import oracle_lib
from oracle_lib import P, arr_ints, ints_to_arr

DEPTHS = (1, 3, 32, 64)
F_RANGE_PRED, F_LOW_IN_ROOT, F_LOW_LT_NEW, F_ZERO_SLOT, F_NEXT_VAL, F_NEXT_IDX, F_NEW_ROOT, F_BAD_BIT = (
    0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80)
M64 = (1 << 64) - 1
INSERT_FE = ("old_root", "low_leaf", "low_sib", "new_root", "new_leaf", "new_sib")   # field-element inputs
NONMEM_FE = ("root", "low_leaf", "low_sib", "new_val")


def helper_bits(index, depth):
    """the circuit's proof_helper column of a path: 1 = the current node is the left input (dual_mux :47-63)"""
    return ints_to_arr([1 - ((index >> l) & 1) for l in range(depth)])


def fold(orc, leaf, index, sib):
    """root of `leaf` at `index` over the siblings `sib` (bottom-up), by the oracle's hash2"""
    return orc.path_root(leaf, index, ints_to_arr(sib)) if sib else leaf


# ---------------------------------------------------------------- the oracle's answers
def insert_expect(orc, w):
    d = w["depth"]
    f, tr = orc.insert_leaf(w["old_root"], w["low_leaf"], ints_to_arr(w["low_sib"]), helper_bits(w["low_index"], d),
                            w["new_root"], w["new_leaf"], w["new_index"], ints_to_arr(w["new_sib"]),
                            helper_bits(w["new_path_index"], d), w["is_largest"])
    assert f >= 0, f
    return f, tr


def nonmem_expect(orc, w):
    d = w["depth"]
    f, r = orc.verify_non_inclusion(w["root"], w["low_leaf"], ints_to_arr(w["low_sib"]), helper_bits(w["low_index"], d),
                                    w["new_val"], w["is_largest"])
    assert f >= 0, f
    return f, r


def path_expect(orc, w):
    r = orc.path_root(w["leaf"], w["index"], ints_to_arr(w["sib"]))
    return r, int(r == w["root"])


def _insert_rec(orc, w, group, name, base_mask=None, noop=False, alone=None):
    f, tr = insert_expect(orc, w)
    return dict(kind="insert", group=group, name=name, depth=w["depth"], w=w, mask=f, trace=tr, base_mask=base_mask,
                noop=noop, alone=alone)


def _nonmem_rec(orc, w, group, name, base_mask=None, noop=False, alone=None):
    f, r = nonmem_expect(orc, w)
    return dict(kind="nonmem", group=group, name=name, depth=w["depth"], w=w, mask=f, root_out=r, base_mask=base_mask,
                noop=noop, alone=alone)


def _path_rec(orc, w, name):
    r, ok = path_expect(orc, w)
    return dict(kind="path", group="path", name=name, depth=w["depth"], w=w, root_out=r, ok=ok)


# ---------------------------------------------------------------- witnesses
def forge_insert(orc, rng, depth, low_leaf, low_index, new_leaf, new_index, new_path_index, is_largest):
    """A witness of insert_leaf whose four paths all agree, for any leaf values and indices (low_index and
    new_path_index must differ in their low `depth` bits): random siblings below level k, where the two indices part;
    at k each path's sibling is the other's node (the zero leaf's subtree for the low path, the rewritten low leaf's for
    the new path); above k both share random siblings."""
    mask = M64 if depth == 64 else (1 << depth) - 1
    diff = (low_index ^ new_path_index) & mask
    assert diff, "the new slot must not be the low leaf's"
    k = diff.bit_length() - 1
    rnd = lambda: rng.randrange(P)
    low_sib = [rnd() for _ in range(depth)]
    new_sib = [rnd() for _ in range(depth)]
    zero_leaf = orc.hash([0, 0, 0])
    low_sib[k] = fold(orc, zero_leaf, new_path_index, new_sib[:k])
    new_sib[k] = fold(orc, orc.hash([low_leaf[0], new_leaf[0], new_index]), low_index, low_sib[:k])
    new_sib[k + 1:] = low_sib[k + 1:]
    return dict(depth=depth, old_root=fold(orc, orc.hash(list(low_leaf)), low_index, low_sib), low_leaf=list(low_leaf),
                low_index=low_index, low_sib=low_sib, new_root=fold(orc, orc.hash(list(new_leaf)), new_path_index, new_sib),
                new_leaf=list(new_leaf), new_index=new_index, new_path_index=new_path_index, new_sib=new_sib,
                is_largest=is_largest)


def nonmem_of(w, new_val=None):
    """the verify_non_inclusion witness inside an insert_leaf witness (:253-257)"""
    return dict(depth=w["depth"], root=w["old_root"], low_leaf=list(w["low_leaf"]), low_index=w["low_index"],
                low_sib=list(w["low_sib"]), new_val=w["new_leaf"][0] if new_val is None else new_val,
                is_largest=w["is_largest"])


def _tree_witnesses(orc, depth, n_ins, seed):
    """n_ins real insertions into an oracle sparse tree of `depth` (insert_leaf witnesses) and real non-members of the
    final tree (verify_non_inclusion witnesses)"""
    rng = random.Random(seed)
    cap = min(1 << depth, 1 << n_ins.bit_length())      # a power of two that holds the sentinel too
    h = orc.sparse_new(depth, cap)
    stored = {0: 0}                      # value -> leaf index (the sentinel)
    ins = []
    try:
        vals = oracle_lib.synth_values(n_ins, seed)
        for i, v in enumerate(vals):
            old_root = orc.sparse_root(h)
            o = orc.sparse_insert(h, depth, v)
            assert o["rc"] == 0, o["rc"]
            low_leaf = arr_ints(o["low_leaf"])
            idx = len(stored)
            ins.append(dict(depth=depth, old_root=old_root, low_leaf=low_leaf, low_index=o["low"],
                            low_sib=arr_ints(o["low_proof"]), new_root=o["new_root"], new_leaf=[v, low_leaf[1], low_leaf[2]],
                            new_index=idx, new_path_index=idx, new_sib=arr_ints(o["new_proof"]),
                            is_largest=o["largest"]))
            stored[v] = idx
        root = orc.sparse_root(h)
        order = sorted(stored)
        cands = [order[-1] + 1 + rng.randrange(1 << 20), 1]       # above the largest; just above the sentinel
        while len(cands) < 6:
            c = rng.randrange(1, P)
            if c not in stored:
                cands.append(c)
        nm = []
        for c in cands:
            low_val = max(v for v in order if v < c)
            li = stored[low_val]
            ll = arr_ints(orc.sparse_preimage(h, li))
            nm.append(dict(depth=depth, root=root, low_leaf=ll, low_index=li, low_sib=arr_ints(orc.sparse_proof(h, depth, li)),
                           new_val=c, is_largest=int(ll[1] == 0)))
    finally:
        orc.sparse_free(h)
    return ins, nm


def _forged_honest(orc, rng, depth, n):
    """n valid insert_leaf witnesses with random values and indices; every other one is a largest insertion, and
    new_index (hashed into the rewritten low leaf) differs from new_path_index (the new slot) in every third"""
    out = []
    span = M64 if depth == 64 else (1 << depth) - 1
    for j in range(n):
        lv = rng.randrange(1, P // 2)
        largest = j % 2
        nx = 0 if largest else rng.randrange(lv + 2, P)
        nv = rng.randrange(lv + 1, P if largest else nx)
        nidx = rng.randrange(1 << 63) if largest else rng.randrange(M64)
        li = rng.randrange(span + 1)
        npi = li
        while npi == li:
            npi = rng.randrange(span + 1)
        ni = npi if j % 3 else (npi ^ (1 << rng.randrange(64))) & M64
        out.append(forge_insert(orc, rng, depth, [lv, nx, nidx], li, [nv, nx, nidx], ni, npi, largest))
    return out


def _bump(x):
    return (x + 1) % P


def _insert_mutations(orc, w, base_mask, tag):
    d = w["depth"]
    out = []

    def mut(name, noop=False, **change):
        m = dict(w, **change)
        out.append(_insert_rec(orc, m, "mutation", f"{tag}:{name}", base_mask=base_mask, noop=noop))

    mut("old_root", old_root=_bump(w["old_root"]))
    for j in range(3):
        mut(f"low_leaf[{j}]", low_leaf=[_bump(x) if k == j else x for k, x in enumerate(w["low_leaf"])])
        mut(f"new_leaf[{j}]", new_leaf=[_bump(x) if k == j else x for k, x in enumerate(w["new_leaf"])])
    for l in sorted({0, 1, d - 1, d, 63}):
        if l < 64:
            mut(f"low_index^bit{l}", noop=l >= d, low_index=w["low_index"] ^ (1 << l))
            mut(f"new_path_index^bit{l}", noop=l >= d, new_path_index=w["new_path_index"] ^ (1 << l))
    for l in sorted({0, d // 2, d - 1}):
        mut(f"low_sib[{l}]", low_sib=[_bump(x) if k == l else x for k, x in enumerate(w["low_sib"])])
        mut(f"new_sib[{l}]", new_sib=[_bump(x) if k == l else x for k, x in enumerate(w["new_sib"])])
    mut("new_root", new_root=_bump(w["new_root"]))
    mut("new_index!=new_path_index", new_index=w["new_index"] ^ 1)
    for s in (1 - w["is_largest"], 2, 255):
        mut(f"is_largest={s}", is_largest=s)
    return out


def _nonmem_mutations(orc, w, base_mask, tag):
    d = w["depth"]
    out = []

    def mut(name, noop=False, **change):
        out.append(_nonmem_rec(orc, dict(w, **change), "mutation", f"{tag}:{name}", base_mask=base_mask, noop=noop))

    mut("root", root=_bump(w["root"]))
    for j in range(3):
        mut(f"low_leaf[{j}]", low_leaf=[_bump(x) if k == j else x for k, x in enumerate(w["low_leaf"])])
    for l in sorted({0, 1, d - 1, d, 63}):
        if l < 64:
            mut(f"low_index^bit{l}", noop=l >= d, low_index=w["low_index"] ^ (1 << l))
    for l in sorted({0, d // 2, d - 1}):
        mut(f"low_sib[{l}]", low_sib=[_bump(x) if k == l else x for k, x in enumerate(w["low_sib"])])
    mut("new_val=low.val", new_val=w["low_leaf"][0])
    for s in (1 - w["is_largest"], 2, 255):
        mut(f"is_largest={s}", is_largest=s)
    return out


def _reseal(orc, w):
    """recompute the roots the witness supplies from the oracle's own trace of it"""
    _, tr = insert_expect(orc, w)
    return dict(w, old_root=tr[1], new_root=tr[6])


def _insert_reseals(orc, w, tag):
    """each insert_leaf bit caught alone (LOW_LT_NEW: see the nonmem reseals -- a smaller new value also moves the
    interim root)"""
    d = w["depth"]
    out = []

    def rs(name, alone, reseal=True, **change):
        m = dict(w, **change)
        out.append(_insert_rec(orc, _reseal(orc, m) if reseal else m, "reseal", f"{tag}:{name}", alone=alone))

    rs("old_root", F_LOW_IN_ROOT, reseal=False, old_root=_bump(w["old_root"]))
    rs("is_largest flipped", F_RANGE_PRED, is_largest=1 - w["is_largest"])
    rs(f"new_sib[{d // 2}]", F_ZERO_SLOT, new_sib=[_bump(x) if k == d // 2 else x for k, x in enumerate(w["new_sib"])])
    rs("new_index", F_ZERO_SLOT, new_index=(w["new_index"] + 1) & M64)
    rs("new_leaf.next_val", F_NEXT_VAL, new_leaf=[w["new_leaf"][0], _bump(w["new_leaf"][1]), w["new_leaf"][2]])
    rs("new_leaf.next_idx", F_NEXT_IDX, new_leaf=[w["new_leaf"][0], w["new_leaf"][1], _bump(w["new_leaf"][2])])
    rs("new_root", F_NEW_ROOT, reseal=False, new_root=_bump(w["new_root"]))
    if w["is_largest"] == 1:
        rs("is_largest=2", F_BAD_BIT, is_largest=2)
        rs("is_largest=255", F_BAD_BIT, is_largest=255)
    return out


def _nonmem_reseals(orc, w, tag):
    out = []
    lv = w["low_leaf"][0]
    if w["is_largest"] or w["low_leaf"][1] > lv:         # new = low.val keeps the range predicate
        out.append(_nonmem_rec(orc, dict(w, new_val=lv), "reseal", f"{tag}:new_val=low.val", alone=F_LOW_LT_NEW))
    out.append(_nonmem_rec(orc, dict(w, root=_bump(w["root"])), "reseal", f"{tag}:root", alone=F_LOW_IN_ROOT))
    out.append(_nonmem_rec(orc, dict(w, is_largest=1 - w["is_largest"]), "reseal", f"{tag}:is_largest flipped",
                           alone=F_RANGE_PRED))
    if w["is_largest"] == 1:
        out.append(_nonmem_rec(orc, dict(w, is_largest=2), "reseal", f"{tag}:is_largest=2", alone=F_BAD_BIT))
    return out


def _edge_pairs(rng):
    """(low.val, next_val, is_largest) pairs and the new values tried between them"""
    h = rng.randrange(1, (P >> 128) - 1) << 128
    pairs = [
        ((1 << 128) - 1, (1 << 128) + 1, 0),          # straddles 2^128
        ((1 << 128) - 2, (1 << 128), 0),              # next_val on 2^128 itself
        (h | 5, h | 9, 0),                            # same high 128 bits
        (h | ((1 << 128) - 3), h + (1 << 128) + 2, 0),  # high halves differ by one, low halves wrap
        (0, P - 1, 0),                                # the sentinel and p - 1
        (P - 3, 0, 1),                                # next_val = 0: largest, valid
        (P - 3, 0, 0),                                # next_val = 0 without the flag: the range predicate fails
        (rng.randrange(1, P // 2), 0, 1),
    ]
    out = []
    for lv, nx, s in pairs:
        news = sorted({x for x in (lv, lv + 1, (nx or P) - 1, nx or P - 1) if 0 <= x < P})
        out.append((lv, nx, s, news))
    return out


def _edges(orc, rng, depth, tag):
    span = M64 if depth == 64 else (1 << depth) - 1
    ins, nm = [], []
    for lv, nx, s, news in _edge_pairs(rng):
        nidx = 0 if nx == 0 else rng.randrange(1, span + 1)
        for nv in news:
            li = rng.randrange(span + 1)
            npi = (li ^ (1 << rng.randrange(depth))) & span
            w = forge_insert(orc, rng, depth, [lv, nx, nidx], li, [nv, nx, nidx], npi, npi, s)
            name = f"{tag}:low={lv:#x} next={nx:#x} new={nv:#x} largest={s}"
            ins.append(_insert_rec(orc, w, "edge", name))
            nm.append(_nonmem_rec(orc, nonmem_of(w), "edge", name))
    return ins, nm


def _paths(orc, insert_recs, depth, rng):
    """verify_proof witnesses out of insert_leaf records: the low leaf against old_root and the new leaf against
    new_root (ok exactly where the record's own chain holds), plus random roots"""
    out = []
    for r in insert_recs:
        w, tr = r["w"], r["trace"]
        out.append(_path_rec(orc, dict(depth=depth, leaf=tr[0], index=w["low_index"], sib=w["low_sib"],
                                       root=w["old_root"]), r["name"] + ":low path"))
        out.append(_path_rec(orc, dict(depth=depth, leaf=tr[5], index=w["new_path_index"], sib=w["new_sib"],
                                       root=w["new_root"] if rng.random() < 0.8 else rng.randrange(P)),
                             r["name"] + ":new path"))
    return out


@functools.lru_cache(maxsize=None)
def corpus(depth):
    """all records of one depth: dict(insert=[...], nonmem=[...], path=[...])"""
    orc = oracle_lib.load()
    rng = random.Random(0x57C0 + depth)
    if depth < 64:
        real_ins, real_nm = _tree_witnesses(orc, depth, {1: 1, 3: 6, 32: 10}.get(depth, 8), 0x494D5500 + depth)
    else:
        real_ins = _forged_honest(orc, rng, depth, 6)
        real_nm = [nonmem_of(w) for w in real_ins]
    forged = _forged_honest(orc, rng, depth, 3)
    ins = [_insert_rec(orc, w, "honest", f"d{depth}:honest{j}") for j, w in enumerate(real_ins + forged)]
    nm = [_nonmem_rec(orc, w, "honest", f"d{depth}:nm{j}") for j, w in enumerate(real_nm)]
    assert all(r["mask"] == 0 for r in ins + nm), [(r["name"], r["mask"]) for r in ins + nm if r["mask"]]
    largest = next(r for r in ins if r["w"]["is_largest"] == 1)
    inner = next((r for r in ins if r["w"]["is_largest"] == 0), None)
    bases = [largest] + ([inner] if inner else [])
    for b in bases:
        ins += _insert_mutations(orc, b["w"], b["mask"], b["name"])
        ins += _insert_reseals(orc, b["w"], b["name"])
    nm_largest = next((r for r in nm if r["w"]["is_largest"] == 1), None)
    nm_inner = next(r for r in nm if r["w"]["is_largest"] == 0)
    for b in [nm_inner] + ([nm_largest] if nm_largest else []):
        nm += _nonmem_mutations(orc, b["w"], b["mask"], b["name"])
        nm += _nonmem_reseals(orc, b["w"], b["name"])
    e_ins, e_nm = _edges(orc, rng, depth, f"d{depth}:edge")
    ins += e_ins
    nm += e_nm
    return dict(insert=ins, nonmem=nm, path=_paths(orc, ins, depth, rng))
