"""CPU: the relation-checker corpus (tests/witness_corpus.py) is what it says it is.  Every oracle mask equals an
independent restatement of the eight constraints (Python integers, the oracle's Poseidon only), every mutation moves
the mask except the documented no-ops, and every bit is caught alone at every depth."""
import pytest

import witness_corpus as wc
from oracle_lib import P


def _fold(orc, cur, index, sib):
    for l, s in enumerate(sib):
        cur = orc.hash([s, cur] if (index >> l) & 1 else [cur, s])
    return cur


def restate_non_inclusion(orc, root, low_leaf, low_index, low_sib, new_val, s):
    """verify_non_inclusion (src/indexed_merkle_tree.rs:127-229) on integers: (mask, recomputed root)"""
    lv, nx, _ = low_leaf
    fail = 0
    if s not in (0, 1):
        fail |= wc.F_BAD_BIT                                         # assert_bit in select :41
    if not ((nx == 0) if s else (new_val < nx)):
        fail |= wc.F_RANGE_PRED                                      # :182-191
    r = _fold(orc, orc.hash(list(low_leaf)), low_index, low_sib)
    if r != root:
        fail |= wc.F_LOW_IN_ROOT                                     # :196-204
    if not lv < new_val:
        fail |= wc.F_LOW_LT_NEW                                      # :206-228
    return fail, r


def restate_insert(orc, w):
    """insert_leaf (:231-314) on integers: (mask, [low_leaf_hash, root_from_low, new_low_leaf_hash, interim_root,
    zero_slot_root, new_leaf_hash, new_root])"""
    fail, r0 = restate_non_inclusion(orc, w["old_root"], w["low_leaf"], w["low_index"], w["low_sib"], w["new_leaf"][0],
                                     w["is_largest"])
    nlh = orc.hash([w["low_leaf"][0], w["new_leaf"][0], w["new_index"]])
    interim = _fold(orc, nlh, w["low_index"], w["low_sib"])
    zroot = _fold(orc, orc.hash([0, 0, 0]), w["new_path_index"], w["new_sib"])
    if zroot != interim:
        fail |= wc.F_ZERO_SLOT
    if w["new_leaf"][1] != w["low_leaf"][1]:
        fail |= wc.F_NEXT_VAL
    if w["new_leaf"][2] != w["low_leaf"][2]:
        fail |= wc.F_NEXT_IDX
    nh = orc.hash(list(w["new_leaf"]))
    nr = _fold(orc, nh, w["new_path_index"], w["new_sib"])
    if nr != w["new_root"]:
        fail |= wc.F_NEW_ROOT
    return fail, [orc.hash(list(w["low_leaf"])), r0, nlh, interim, zroot, nh, nr]


@pytest.mark.parametrize("depth", wc.DEPTHS)
def test_oracle_masks_equal_the_restated_constraints(oracle, depth):
    c = wc.corpus(depth)
    for r in c["insert"]:
        assert restate_insert(oracle, r["w"]) == (r["mask"], r["trace"]), r["name"]
    for r in c["nonmem"]:
        w = r["w"]
        assert restate_non_inclusion(oracle, w["root"], w["low_leaf"], w["low_index"], w["low_sib"], w["new_val"],
                                     w["is_largest"]) == (r["mask"], r["root_out"]), r["name"]
    for r in c["path"]:
        w = r["w"]
        root = _fold(oracle, w["leaf"], w["index"], w["sib"])
        assert (root, int(root == w["root"])) == (r["root_out"], r["ok"]), r["name"]


@pytest.mark.parametrize("depth", wc.DEPTHS)
def test_corpus_shape(depth):
    """every input is a canonical field element / 64-bit index of the right length, and the records cover what they
    claim: honest witnesses with new_index != new_path_index, largest and inner insertions, failing and passing paths"""
    c = wc.corpus(depth)
    for r in c["insert"] + c["nonmem"]:
        w = r["w"]
        fes = [w[k] for k in ("old_root", "new_root", "root", "new_val") if k in w] + w["low_leaf"] + w.get("new_leaf", [])
        fes += w["low_sib"] + w.get("new_sib", [])
        assert all(0 <= x < P for x in fes), r["name"]
        assert len(w["low_sib"]) == depth and len(w.get("new_sib", w["low_sib"])) == depth
        assert all(0 <= w[k] < 1 << 64 for k in ("low_index", "new_index", "new_path_index") if k in w)
    honest = [r for r in c["insert"] if r["group"] == "honest"]
    assert {r["w"]["is_largest"] for r in honest} == {0, 1}
    assert any(r["w"]["new_index"] != r["w"]["new_path_index"] for r in honest)
    assert {r["ok"] for r in c["path"]} == {0, 1}
    if depth == 64:
        assert any(r["w"]["low_index"] >> 63 for r in c["insert"])


@pytest.mark.parametrize("depth", wc.DEPTHS)
def test_every_mutation_moves_the_mask_except_the_documented_no_ops(depth):
    c = wc.corpus(depth)
    muts = [r for r in c["insert"] + c["nonmem"] if r["group"] == "mutation"]
    assert len(muts) > 40
    for r in muts:
        if r["noop"]:
            assert r["mask"] == r["base_mask"], r["name"]
        else:
            assert r["mask"] != r["base_mask"], r["name"]
    assert any(r["noop"] for r in muts) == (depth < 64)


@pytest.mark.parametrize("depth", wc.DEPTHS)
def test_each_bit_is_caught_alone(depth):
    """insert_leaf isolates each of its bits but LOW_LT_NEW (a smaller new value moves the interim root too, unless the
    whole witness is rebuilt, as the edge records do), verify_non_inclusion isolates LOW_LT_NEW"""
    c = wc.corpus(depth)
    ins_alone = {r["mask"] for r in c["insert"]}
    for bit in (wc.F_RANGE_PRED, wc.F_LOW_IN_ROOT, wc.F_ZERO_SLOT, wc.F_NEXT_VAL, wc.F_NEXT_IDX, wc.F_NEW_ROOT,
                wc.F_BAD_BIT):
        assert bit in ins_alone, hex(bit)
    assert wc.F_LOW_LT_NEW in {r["mask"] for r in c["nonmem"]}
    for r in c["insert"] + c["nonmem"]:
        if r["group"] == "reseal":
            assert r["mask"] == r["alone"], (r["name"], r["mask"])
    # at depth 32 a flipped new_sib level gives ZERO_SLOT | NEW_ROOT; the resealed one (above) ZERO_SLOT alone
    if depth == 32:
        flipped = [r for r in c["insert"] if r["group"] == "mutation" and ":new_sib[16]" in r["name"]]
        assert flipped and all(r["mask"] == wc.F_ZERO_SLOT | wc.F_NEW_ROOT for r in flipped)


@pytest.mark.parametrize("depth", wc.DEPTHS)
def test_edge_records_are_the_range_predicates(depth):
    """edge records hold every path, so their mask is exactly the two integer comparisons (and select)"""
    c = wc.corpus(depth)
    edges = [r for r in c["insert"] if r["group"] == "edge"]
    assert len(edges) >= 20
    seen = set()
    for r in edges:
        w = r["w"]
        lv, nx, _ = w["low_leaf"]
        nv, s = w["new_leaf"][0], w["is_largest"]
        want = (0 if ((nx == 0) if s else nv < nx) else wc.F_RANGE_PRED) | (0 if lv < nv else wc.F_LOW_LT_NEW)
        assert r["mask"] == want, r["name"]
        seen.add(want)
    assert seen == {0, wc.F_RANGE_PRED, wc.F_LOW_LT_NEW, wc.F_RANGE_PRED | wc.F_LOW_LT_NEW}
    # the named edge values are all there
    vals = {r["w"]["new_leaf"][0] for r in edges}
    assert {0, P - 1, 1 << 128, (1 << 128) - 1} <= vals
