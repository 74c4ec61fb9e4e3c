"""CPU: tests/tree_model.py -- the plain-Python list against the sequential oracle, and the coverage of the committed
step scripts that tests/test_gpu_tree_sequences.py plays on the GPU.

  test_model_replays_the_corpus    every scenario of tests/insert_corpus.py at depth <= 63 through TreeModel.insert: the
                                   oracle's low leaf, is_largest and low-leaf preimage of every insertion; the oracle
                                   loaded with the model's preimages has the corpus's root at every batch boundary (at the
                                   middle and the last one for the scenario of 16 000 values), also after rewind() to each (there: the
                                   middle one).
  test_model_filter_and_readers    classify / lookup / find_low / nm_witness against a brute-force statement.
  test_model_load_refusals         the breakages of test_oracle_golden's sparse_load cases, and a few more.
  test_model_mixed_against_the_walk TreeModel.mixed (written from include/imt.h) against test_mixed_logic.walk over that
                                   file's adversarial and random scripts: rows, refusals and bad_op.
  test_first_pass_scripts_are_unchanged  the digest of the nine scripts that ran before the mixed batch existed.
  test_script_coverage             the pair coverage of scripts(), asserted: the ten older kinds over the first pass, all
                                   twelve over everything, and what the second pass owes by itself (the triples with a
                                   mixed batch in them, its refusals with bad_op, pointer modes and layouts, READs on a
                                   full tree, more operations than room, reads at size 1, READs whose rows change
                                   inside one batch, where the READ values come from).
  test_second_pass_scripts_are_unchanged  the digest of the five scripts of the second pass.
  test_third_pass_coverage         what the third pass (kinds 14 to 20) owes by itself: every ordered pair of new kinds at
                                   both check levels, every pair of a new and an older kind at some level, every new kind
                                   right after a refused call, the new refusals, all five shapes, FULL - reserve - the same
                                   batch accepted on d3, every one of the 19 kinds entering behind two batches in flight
                                   of two pipelined kinds, two runs of five or more pipelined steps with no check between
                                   them and a refused step inside one, every variant of every new kind; at most 20 scripts
                                   of at most 40 steps.
  test_model_load_values_and_reserve  TreeModel.load_values of corpus prefixes against the oracle, its refusals and bad_pos;
                                   TreeModel.reserve changes nothing but the capacity.
  test_scripts_are_self_consistent every accepted step accepted by the model, every refused one refused with its code.
  test_view_schedule               view_schedule() and view_rounds(): the rules of the schedule and of the expected rebuilds.
  test_view_coverage               what tests/test_gpu_view_sequences.py sees with that schedule on the committed scripts:
                                   every writer kind makes a view stale, every transition of a view's state, histories
                                   that change beneath a view, replays of leaves of every origin, rounds that must not
                                   rebuild (behind a mixed batch of READs only and a refused one among them).  It fails for a schedule that keeps the view at size 1 alone.
"""
import os
import sys

import pytest

import insert_corpus as ic
import oracle_lib
import tree_model as tmod
from member_model import MemberModel
from oracle_lib import P, arr_ints, ints_to_arr
from tree_model import FULL, KINDS, LIGHT, Refused, TreeModel

CORPUS = [sc.name for sc in ic.SCENARIOS if sc.depth <= ic.ORACLE_MAX_DEPTH]


def loaded_root(oracle, sc, m):
    h = oracle.sparse_new(sc.depth, sc.cap)
    oracle.sparse_set_index_base(h, sc.index_base)
    try:
        if m.size > 1:
            assert oracle.sparse_load(h, tmod.pre_arr(m.preimages(range(m.size)))) == 0
        return oracle.sparse_root(h)
    finally:
        oracle.sparse_free(h)


@pytest.mark.parametrize("name", CORPUS)
def test_model_replays_the_corpus(oracle, name):
    sc, exp = ic.BY_NAME[name], ic.expected(name)
    vals, rec, bounds = exp["vals"], exp["rec"], ic.batch_bounds(sc)
    m = TreeModel(sc.depth, sc.cap, sc.index_base)
    checked = set(range(len(bounds))) if len(vals) <= 4096 else {len(bounds) // 2, len(bounds) - 1}
    assert loaded_root(oracle, sc, m) == exp["batch_roots"][0]
    for j, (a, b) in enumerate(bounds):
        rows = m.insert(vals[a:b])
        assert [r["low"] for r in rows] == rec["low_index"][a:b].tolist(), (name, j)
        assert [r["largest"] for r in rows] == rec["is_largest"][a:b].tolist(), (name, j)
        assert [x for r in rows for x in r["low_leaf"]] == arr_ints(rec["low_leaf"][a:b]), (name, j)
        if j in checked:
            assert loaded_root(oracle, sc, m) == exp["batch_roots"][j + 1], (name, j)
    fin = exp["final"]
    local = [int(i) - sc.index_base for i in fin["index"]]
    assert [x for p in m.preimages(local) for x in p] == arr_ints(fin["preimages"]), name
    if sc.full:
        with pytest.raises(Refused) as e:
            m.insert([exp["full_value"]])
        assert e.value.code == "FULL"
    back = checked if len(vals) <= 4096 else {len(bounds) // 2}
    for j in sorted(back, reverse=True):                          # back to the boundaries: the oracle's tree of the prefix
        m.rewind(bounds[j][0] + 1)
        assert m.vals[1:] == vals[:bounds[j][0]]
        assert loaded_root(oracle, sc, m) == exp["batch_roots"][j], (name, j)
    for bad in (0, m.size + 1):
        with pytest.raises(Refused) as e:
            m.rewind(bad)
        assert e.value.code == "RANGE"


@pytest.mark.parametrize("part", [(0, 0), (3, 1)])
def test_model_filter_and_readers(part):
    base = 5 << 8
    m = TreeModel(8, 64, base, *part)
    mine = [v for v in oracle_lib.synth_values(400, 0x544D0001) if m.mine(v)]
    m.insert(mine[:20])
    stored = {v: base + 1 + i for i, v in enumerate(mine[:20])}
    a, b, c = mine[20:23]
    foreign = next(v for v in range(2, 50) if not m.mine(v)) if part[0] else None
    batch = [a, 0, mine[3], a, b, mine[3], b, c] + ([foreign, foreign] if foreign else [])
    status, leaf, acc = m.classify(batch)
    N, Z, S, R, F = tmod.NEW, tmod.ZERO, tmod.PRESENT, tmod.REPEATED, tmod.FOREIGN
    assert status == [N, Z, S, R, N, S, R, N] + ([F, F] if foreign else [])
    assert leaf == [base + 21, base, stored[mine[3]], base + 21, base + 22, stored[mine[3]], base + 22, base + 23] + \
        ([tmod.NONE] * 2 if foreign else [])
    assert acc == [a, b, c] and m.size == 21
    with pytest.raises(Refused) as e:
        m.classify([a, P])
    assert e.value.code == "NONCANONICAL"
    for v in m.probes() + [a, b, c]:
        below = max(x for x in list(stored) + [0] if x < v)
        want = stored.get(below, base)
        above = [x for x in stored if x > v]
        assert m.find_low(v) == want and m.lookup(v) == (N, want)
        low, pre, largest = m.nm_witness(v)
        assert (low, largest) == (want, int(not above))
        assert pre == (below, min(above) if above else 0, stored[min(above)] if above else 0)
    assert m.lookup(0) == (Z, base) and m.lookup(mine[7]) == (S, stored[mine[7]])
    for v, code in ((0, "VALUE"), (mine[7], "VALUE"), (P, "NONCANONICAL")) + (((foreign, "VALUE"),) if foreign else ()):
        with pytest.raises(Refused) as e:
            m.find_low(v)
        assert e.value.code == code
    if foreign:
        assert m.lookup(foreign) == (F, tmod.NONE)
    assert m.preimages([0, 64, 21]) == [(0, min(stored), stored[min(stored)]), (0, 0, 0), (0, 0, 0)]
    m.filtered(batch)
    assert m.vals[21:] == [a, b, c]
    with pytest.raises(Refused) as e:                              # 24 leaves + 41 new values > 64
        m.filtered(mine[30:71])
    assert e.value.code == "FULL" and m.size == 24


def test_model_load_refusals(oracle):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_config4_digest import preimages_after
    vals = ints_to_arr(oracle_lib.synth_values(400, 0x494D5404))

    def triples(arr):
        x = arr_ints(arr)
        return [tuple(x[3 * i:3 * i + 3]) for i in range(len(x) // 3)]

    def both(pre):
        """the model's verdict, which must be the oracle's"""
        m = TreeModel(32, 1024)
        g = oracle.sparse_new(32, 1024)
        rc = oracle.sparse_load(g, pre)
        oracle.sparse_free(g)
        try:
            m.load(triples(pre))
        except Refused as e:
            assert rc == -10, "the oracle accepts what the model refuses"
            return e.code, m
        assert rc == 0, "the oracle refuses what the model accepts"
        return None, m

    for k in (0, 1, 2, 10, 333):
        code, m = both(preimages_after(vals, k))
        assert code is None and m.vals == [0] + arr_ints(vals[:k])
        assert m.preimages(range(k + 1)) == triples(preimages_after(vals, k))
    for breakage in ("pointer", "value", "sentinel", "duplicate", "last", "last_idx", "order"):
        pre = preimages_after(vals, 10).copy()
        if breakage == "pointer":
            pre[3, 2, 0] ^= 1
        elif breakage == "value":
            pre[4, 1, 5] ^= 1
        elif breakage == "sentinel":
            pre[0, 0, 0] = 1
        elif breakage == "duplicate":
            pre[7, 0] = pre[6, 0]
        elif breakage in ("last", "last_idx"):
            big = max(range(11), key=lambda i: arr_ints(pre[i, 0])[0])
            pre[big, 1 if breakage == "last" else 2, 0] = 1
        else:
            pre[[2, 5]] = pre[[5, 2]]                              # two leaves swapped: every next_idx is off
        code, m = both(pre)
        assert code == "VALUE" and m.vals == [0], breakage
    m = TreeModel(32, 8)
    for pre, code in (([], "ARG"), (triples(preimages_after(vals, 8)), "FULL"), ([(0, P, 1), (P, 0, 0)], "NONCANONICAL")):
        with pytest.raises(Refused) as e:
            m.load(pre)
        assert e.value.code == code and m.vals == [0]
    part = TreeModel(32, 8, 0, 3, 1)
    with pytest.raises(Refused) as e:
        part.load([(0, 5, 1), (5, 0, 0)])
    assert e.value.code == "VALUE"
    part.load([(0, 4, 1), (4, 0, 0)])
    assert part.vals == [0, 4]


# ---------------------------------------------------------------- TreeModel.mixed against the walk of test_mixed_logic
def test_model_mixed_against_the_walk():
    """Two independent statements of one definition: TreeModel.mixed (from include/imt.h) and test_mixed_logic.walk (the
    expectation of the rules the kernels run), over that file's adversarial and random scripts."""
    import test_mixed_logic as tml
    cases = tml.all_cases()
    assert len(cases) >= 900 and all(c in cases for c in tml.ADVERSARIAL.values())
    n_refused = 0
    beyond = [c for c in cases if max(v for _, v in c[1]) >= P]   # the walk knows no modulus: "limbs" reads 2^255
    assert len(beyond) == 1
    for ci, (stored, script) in enumerate(c for c in cases if c not in beyond):
        m = TreeModel(8, 256)
        m._reset(stored)
        vals, ops = [v for _, v in script], [op for op, _ in script]
        assert (tml.INSERT, tml.READ) == (tmod.OP_INSERT, tmod.OP_READ)
        rows, bad = tml.walk(stored, script)
        if bad >= 0:
            with pytest.raises(Refused) as e:
                m.mixed(vals, ops)
            assert (e.value.code, e.value.bad_op) == ("VALUE", bad) and m.vals == stored, (ci, stored, script)
            assert m.order == sorted(stored) and m.where == {v: i for i, v in enumerate(stored)}, ci
            n_refused += 1
            continue
        acc, reads = m.mixed(vals, ops)
        assert acc == [v for op, v in script if op == tml.INSERT] and m.vals == stored + acc, (ci, stored, script)
        assert [r[0] for r in reads] == [p for p, op in enumerate(ops) if op == tml.READ], ci
        for p, low, leaf, largest, n_before in reads:
            succ = rows[p][1]
            assert low == rows[p][0] and largest == int(succ < 0) and n_before == ops[:p].count(tml.INSERT), (ci, p, stored, script)
            assert leaf == (m.vals[low], 0 if succ < 0 else m.vals[succ], max(succ, 0)), (ci, p, stored, script)
    assert n_refused >= 50
    full = TreeModel(3, 8)
    full.insert([10, 20, 30, 40, 50, 60])
    with pytest.raises(Refused) as e:                              # FULL counts the INSERTs only
        full.mixed([70, 80, 15], [0, 0, 1])
    assert e.value.code == "FULL" and full.size == 7
    assert full.mixed([70, 5, 15, 70, 25], [1, 1, 1, 0, 1])[0] == [70] and full.size == 8
    assert len(full.mixed([5, 75], [1, 1])[1]) == 2                # READs only on a full tree
    with pytest.raises(Refused) as e:
        full.mixed([5, P], [1, 1])
    assert e.value.code == "NONCANONICAL"
    for m in (TreeModel(8, 64, 5 << 8), TreeModel(8, 64, 0, 3, 1)):
        with pytest.raises(Refused) as e:
            m.mixed([4], [1])
        assert e.value.code == "ARG"


# ---------------------------------------------------------------- the committed scripts
FIRST_PASS_DIGEST = "93cad3ee244feb5f5b33d7922700a6ac88035175a865acc3290861467724f726"


def test_first_pass_scripts_are_unchanged():
    """the nine scripts of the first pass are the record of what has passed on the GPU: byte for byte what they were"""
    import hashlib
    assert tmod.N_FIRST_PASS == 9
    assert hashlib.sha256(repr(tmod.scripts()[:9]).encode()).hexdigest() == FIRST_PASS_DIGEST


SECOND_PASS_DIGEST = "06ce560b0c4124a5f77226a85110764fb18a95c6e82c1cbcba78ab62ad1355b4"


def test_second_pass_scripts_are_unchanged():
    """the five scripts of the second pass as they were before kinds 14 to 20 were played: byte for byte"""
    import hashlib
    assert (tmod.N_FIRST_PASS, tmod.N_OLD_PASSES) == (9, 14)
    assert hashlib.sha256(repr(tmod.scripts()[9:14]).encode()).hexdigest() == SECOND_PASS_DIGEST


def survey(scripts):
    """what a set of scripts covers"""
    cov = dict(pairs=set(), after_refusal=set(), refusals=set(), refused_kinds=set(), rewinds=set(), loads=set(),
               shapes={s.shape for s in scripts}, d3_story=False)
    for s in scripts:
        assert s.steps[-1].check == FULL, s.name
        assert all(st.check in (LIGHT, FULL) for st in s.steps)
        tr = tmod.trace(s)
        for (st, before, after, res), nxt in zip(tr, list(tr[1:]) + [None]):
            assert len(after) <= tmod.SIZE_LIMIT and (st.vals is None or 1 <= len(st.vals) <= 16), s.name
            if nxt is not None and not nxt[0].refusal:
                if st.refusal:
                    cov["after_refusal"].add(nxt[0].kind)
                else:
                    cov["pairs"].add((st.kind, nxt[0].kind, st.check))
            if st.refusal:
                cov["refusals"].add(st.refusal)
                cov["refused_kinds"].add(st.kind)
            elif st.kind == 9:
                M = len(before)
                cov["rewinds"].add("noop" if st.arg == M else "one" if st.arg == 1 else "size-1" if st.arg == M - 1 else "interior")
            elif st.kind == 10:
                n = len(st.arg["pre"])
                cov["loads"] |= {("fmt", st.arg["fmt"]), ("device", st.arg["device"]), st.arg["source"],
                                 "shorter" if n < len(before) else "longer" if n > len(before) else "same"}
        if s.shape.cap == 8:                     # the tree fills, FULL is reached, and a rewind makes room again
            sizes = [(st, len(before), len(after)) for st, before, after, _ in tr]
            for i, (st, M, _) in enumerate(sizes):
                if st.refusal in ("full", "mixed_full") and M == 8:
                    back = [j for j in range(i + 1, len(sizes)) if sizes[j][0].kind == 9 and sizes[j][2] < sizes[j][1]]
                    if back and any(b > a for _, a, b in sizes[back[0] + 1:]):
                        cov["d3_story"] = True
    return cov


def test_script_coverage():
    scripts = tmod.scripts()
    assert scripts is tmod.scripts() and len({s.name for s in scripts}) == len(scripts)
    scripts = scripts[:tmod.N_OLD_PASSES]                          # the third pass: test_third_pass_coverage
    first, second = scripts[:tmod.N_FIRST_PASS], scripts[tmod.N_FIRST_PASS:]
    # ---- the first pass: the ten older kinds, as before the mixed batch existed
    cov = survey(first)
    pairs, shapes = cov["pairs"], cov["shapes"]
    missing = [(a, b, lv) for lv in (LIGHT, FULL) for a in KINDS for b in KINDS if (a, b, lv) not in pairs]
    assert not missing, f"pairs of writer kinds never adjacent: {missing}"
    assert cov["after_refusal"] == set(KINDS), f"never right after a refused call: {sorted(set(KINDS) - cov['after_refusal'])}"
    assert cov["refusals"] == set(tmod.REFUSALS)
    assert cov["rewinds"] == set(tmod.REWIND_VARIANTS)
    assert cov["loads"] >= {("fmt", 0), ("fmt", 1), ("fmt", 2), ("device", False), ("device", True), "earlier", "unrelated",
                            "shorter", "longer"}
    assert shapes == set(tmod.SHAPES) and cov["d3_story"]
    g5 = ic.BY_NAME["placed_g5"]
    assert any(sh.placement == tuple(g5.placement) and (sh.depth, sh.cap) == (g5.depth, g5.cap) for sh in shapes)
    assert any(sh.partition == (3, 1) for sh in shapes)
    assert {(sh.depth, sh.cap) for sh in shapes} >= {(3, 8), (8, 64), (32, 256)}
    # the values: 1, p - 1, neighbours of stored values, groups that share their top 64 bits
    stored = [v for s in first for st in s.steps if st.vals and not st.refusal for v in st.vals]
    assert 1 in stored and P - 1 in stored
    every = set(stored)
    assert sum(v + 1 in every or v - 1 in every for v in every) >= 20
    tops = [v >> 192 for v in every]
    assert max(tops.count(t) for t in tmod.TOPS) >= 20
    print(f"{len(first)} scripts, {sum(len(s.steps) for s in first)} steps, refused base kinds {sorted(cov['refused_kinds'])}")
    # ---- everything: all twelve kinds in every adjacent order at both check levels, each right after a refused call
    A = tmod.ALL_KINDS
    cov = survey(scripts)
    missing = [(a, b, lv) for lv in (LIGHT, FULL) for a in A for b in A if (a, b, lv) not in cov["pairs"]]
    assert not missing, f"pairs of writer kinds never adjacent: {missing}"
    assert cov["after_refusal"] == set(A), f"never right after a refused call: {sorted(set(A) - cov['after_refusal'])}"
    assert cov["refusals"] == set(tmod.REFUSALS) | set(tmod.MIXED_REFUSALS)
    assert cov["shapes"] == set(tmod.SHAPES) and cov["d3_story"]
    # ---- the second pass by itself: whatever a mixed batch takes part in
    new = (tmod.MIXED, tmod.MIXED_READS)
    cov = survey(second)
    missing = [(a, b, lv) for lv in (LIGHT, FULL) for a in A for b in A if (a in new or b in new) and (a, b, lv) not in cov["pairs"]]
    assert not missing, f"the second pass: pairs never adjacent: {missing}"
    assert cov["after_refusal"] >= set(new) and cov["refusals"] >= set(tmod.MIXED_REFUSALS)
    assert cov["shapes"] == set(tmod.MIXED_SHAPES) and cov["d3_story"] and len(second) <= 6
    seen, modes, sources = set(), set(), dict.fromkeys(("neighbour", "top 64 bits", "read twice", "1 or p - 1", "other"), 0)
    for s in second:
        tr = tmod.trace(s)
        for i, (st, before, after, res) in enumerate(tr):
            if st.kind not in new:
                continue
            vals, ops, room = st.vals, st.arg["ops"], s.shape.cap - len(before)
            assert len(vals) == len(ops) and set(ops) <= {0, 1} and set(st.arg) == {"ops", "device", "item_major"}, s.name
            assert (st.kind == tmod.MIXED) == (0 in ops), f"{s.name} step {i}: kind 12 has an INSERT, kind 13 has none"
            if st.refusal:
                assert st.refusal in tmod.MIXED_REFUSALS and isinstance(res, Refused), s.name
                modes.add(("refused", st.arg["device"]))
                b = res.bad_op
                if st.refusal == "mixed_read_stored":
                    assert ops[b] == 1 and vals[b] in before[1:] and vals[b] not in vals[:b], (s.name, i)
                elif st.refusal == "mixed_read_inserted_earlier":
                    assert ops[b] == 1 and any(o == 0 and v == vals[b] for o, v in zip(ops[:b], vals[:b])), (s.name, i)
                elif st.refusal == "mixed_insert_repeat":
                    assert ops[b] == 0 and any(o == 0 and v == vals[b] for o, v in zip(ops[:b], vals[:b])), (s.name, i)
                    assert ops.count(0) <= room, (s.name, i)
                elif st.refusal == "mixed_full":
                    assert b is None and ops.count(0) == room + 1 and all(0 < v < P for v in vals), (s.name, i)
                else:
                    assert b is None and any(o == 1 and v >= P for o, v in zip(ops, vals)) and ops.count(0) <= room, (s.name, i)
                continue
            assert 1 in ops, f"{s.name} step {i}: a mixed batch of the scripts has a READ"
            modes.add((st.kind, st.arg["device"], st.arg["item_major"]))
            reads, n_ins = res["reads"], ops.count(0)
            assert res["acc"] == [v for v, o in zip(vals, ops) if o == 0] and after == before + tuple(res["acc"]), (s.name, i)
            if st.kind == tmod.MIXED_READS and s.shape.cap == 8 and len(before) == 8:
                seen.add("READs only on a full tree")
            if st.kind == tmod.MIXED and len(ops) > room >= n_ins:
                seen.add("more operations than room")
            if i == 0:
                seen.add("reads at size 1")
                assert reads[0][1:4] == (0, (0, 0, 0), 1) or ops[0] == 0, s.name
            stored_now = set(before)
            for q, (p, low, leaf, largest, n_before) in enumerate(reads):
                v = vals[p]
                if v in [x for x, o in zip(vals[p + 1:], ops[p + 1:]) if o == 0]:
                    seen.add("a READ of a value a later INSERT inserts")
                for p2, low2, leaf2, largest2, n2 in reads[q + 1:]:
                    if vals[p2] == v and n2 > n_before and (low2, leaf2, largest2) != (low, leaf, largest):
                        seen.add("two READs of one value, rows differ")
                        if low2 != low:
                            seen.add("two READs of one value, another low leaf")
                    if largest == 1 and largest2 == 0:
                        seen.add("is_largest 1, later 0")
                known = stored_now | set(res["acc"][:n_before])
                src = "read twice" if v in [vals[r[0]] for r in reads[:q]] else "1 or p - 1" if v in (1, P - 1) else \
                    "neighbour" if v - 1 in known or v + 1 in known else \
                    "top 64 bits" if any(v >> 192 == x >> 192 for x in known if x) else "other"
                sources[src] += 1
    want = {"READs only on a full tree", "more operations than room", "reads at size 1", "a READ of a value a later INSERT inserts",
            "two READs of one value, rows differ", "two READs of one value, another low leaf", "is_largest 1, later 0"}
    assert seen == want, f"the second pass never has: {sorted(want - seen)}"
    want = {(tmod.MIXED, d, im) for d in (False, True) for im in (False, True)} | {("refused", False), ("refused", True)}
    assert modes >= want | {(tmod.MIXED_READS, d, im) for d in (False, True) for im in (False, True)}, \
        f"pointer modes and layouts never played: {sorted(map(str, want - modes))}"
    assert all(n >= 5 for n in sources.values()), f"where the values of the READs come from: {sources}"
    print(f"{len(second)} scripts of the second pass, {sum(len(s.steps) for s in second)} steps, READ values {sources}")


def test_third_pass_coverage():
    """What the third pass owes by itself: kinds 14 to 20 among themselves and against the twelve older kinds, their
    refusals, and what only a step without a check behind it brings about -- several pipelined batches in flight."""
    from collections import Counter
    NEW, ALL, NO = tmod.NEW_KINDS, tmod.KINDS19, tmod.NO_CHECK
    assert NEW == tuple(range(14, 21)) and len(ALL) == 19
    old, third = tmod.scripts()[:tmod.N_OLD_PASSES], tmod.scripts()[tmod.N_OLD_PASSES:]
    assert all(st.check in (LIGHT, FULL) and st.kind <= 13 for s in old for st in s.steps), "NO_CHECK and the new kinds: third pass only"
    assert len(third) <= 20 and all(len(s.steps) <= 40 for s in third)
    pairs, after_refusal, followed, refusals, variants = set(), set(), Counter(), {}, set()
    entered, runs, run_with_refusal, d3_story, ran = set(), 0, 0, False, set()
    for s in third:
        assert s.shape in tmod.THIRD_SHAPES and s.steps[-1].check == FULL, s.name
        plain = not (s.shape.placement or s.shape.partition[0])
        tr, fl, cp = tmod.trace(s), tmod.flights(s), tmod.caps(s)
        assert isinstance(tmod.new_model(s.shape), MemberModel), "the third pass is played on MemberModel, not a bare TreeModel"
        for i, (st, before, after, res) in enumerate(tr):
            tag = f"{s.name} step {i} kind {tmod.writer_kind(st)}"
            n_ops = len(st.vals) if st.vals is not None else 0
            assert len(after) <= tmod.SIZE_LIMIT and n_ops <= 16 and cp[i] <= 1 << s.shape.depth, tag
            if st.kind == tmod.LOAD_VALUES:                        # a value log is a whole tree, not a batch: like the snapshot of
                n_log = len(st.arg["vals"])                        # kind 10 it is bounded by the size of a tree, not by 16
                assert 1 <= n_log < tmod.SIZE_LIMIT and (not st.refusal or n_log <= 32), f"{tag}: a log of {n_log} values"
            if st.check == NO:
                assert st.kind in tmod.PIPELINED and i + 1 < len(tr), f"{tag}: no check only behind a pipelined call, never last"
            if st.kind in tmod.PLAIN_ONLY and not plain:
                assert st.refusal and res.code == "ARG", f"{tag}: refused on a placed or partitioned tree"
            nxt = tr[i + 1][0] if i + 1 < len(tr) else None
            if st.refusal:
                refusals.setdefault(st.refusal, []).append((s, i, st, res))
                if nxt is not None and not nxt.refusal:
                    after_refusal.add(nxt.kind)
            else:
                followed[st.kind, st.check] += 1
                ran.add((s.shape.name, st.kind))
                if nxt is not None and not nxt.refusal:
                    pairs.add((st.kind, nxt.kind, st.check))
                if len(fl[i]) >= 2 and len(set(fl[i])) >= 2:
                    entered.add(st.kind)
                if st.kind == tmod.BULK:
                    variants |= {("bulk", st.arg["device"], st.arg["item_major"])}
                elif st.kind == tmod.APPLY_PIPE:
                    variants |= {("apply_pipelined", st.arg["host_prep"], st.arg["inputs_ready"])}
                elif st.kind == tmod.MIXED_FILT:
                    variants |= {("mixed_filtered", "device", st.arg["device"]), ("mixed_filtered", "item_major", st.arg["item_major"]),
                                 ("mixed_filtered", "members", tmod.OP_MEMBER in st.arg["ops"])}
                elif st.kind == tmod.APPLY_MIXED:
                    variants |= {("apply_mixed", st.arg["filtered"], tmod.OP_MEMBER in st.arg["ops"])}
                elif st.kind == tmod.MIXED_PIPE:
                    variants |= {("mixed_pipelined", st.arg["apply"], tmod.OP_MEMBER in st.arg["ops"])}
                elif st.kind == tmod.LOAD_VALUES:
                    n = len(st.arg["vals"]) + 1
                    variants |= {("load_values", "device", st.arg["device"]), ("load_values", "fmt", st.arg["fmt"]),
                                 ("load_values", st.arg["source"]),
                                 ("load_values", "shorter" if n < len(before) else "longer" if n > len(before) else "same")}
                elif st.kind == tmod.RESERVE:
                    variants |= {("reserve", "grow" if st.arg > cp[i] else "shrink" if st.arg < cp[i] else "same")}
                    if st.arg < cp[i]:
                        assert st.arg == max(2, 1 << (len(before) - 1).bit_length()), f"{tag}: shrinks to the smallest legal capacity"
            # FULL, then reserve, then the same batch accepted
            if s.shape.depth == 3 and st.refusal and res.code == "FULL" and i + 2 < len(tr):
                (r, _, _, rres), (again, _, _, ares) = tr[i + 1][:4], tr[i + 2][:4]
                if r.kind == tmod.RESERVE and not r.refusal and r.arg > cp[i + 1] and not again.refusal and \
                        (again.kind, again.vals) == (st.kind, st.vals):
                    d3_story = True
        # runs of pipelined steps with nothing between them
        i = 0
        while i < len(tr):
            j, n_acc, n_ref = i, 0, 0
            while j < len(tr) and tr[j][0].kind in tmod.PIPELINED and (j == i or tr[j - 1][0].check == NO):
                n_acc, n_ref = n_acc + (not tr[j][0].refusal), n_ref + bool(tr[j][0].refusal)
                j += 1
            if n_acc >= 5:
                runs += 1
                run_with_refusal += bool(n_ref)
            i = max(j, i + 1)
    lv = (LIGHT, FULL)
    missing = [(a, b, l) for l in lv for a in NEW for b in NEW if (a, b, l) not in pairs]
    assert not missing, f"pairs of new kinds never adjacent: {missing}"
    some = {(a, b) for a, b, _ in pairs}
    missing = [(a, b) for a in ALL for b in ALL if (a in NEW) != (b in NEW) and (a, b) not in some]
    assert not missing, f"a new and an older kind never adjacent: {missing}"
    assert after_refusal >= set(NEW), f"never right after a refused call: {sorted(set(NEW) - after_refusal)}"
    assert all(followed[k, l] >= 5 for k in NEW for l in lv), followed
    assert set(refusals) >= set(tmod.NEW_REFUSALS), f"refusals that never occur: {sorted(set(tmod.NEW_REFUSALS) - set(refusals))}"
    assert {s.shape for s in third} == set(tmod.THIRD_SHAPES) and [sh.name for sh in tmod.THIRD_SHAPES] == [sh.name for sh in tmod.SHAPES]
    missing = [(sh.name, k) for sh in tmod.THIRD_SHAPES for k in NEW
               if (k not in tmod.PLAIN_ONLY or not (sh.placement or sh.partition[0])) and (sh.name, k) not in ran]
    assert not missing, f"new kinds never accepted on a shape they run on: {missing}"
    assert d3_story, "FULL, then reserve, then the same batch accepted: never on d3"
    assert entered >= set(ALL), f"kinds that never enter behind two batches in flight of two kinds: {sorted(set(ALL) - entered)}"
    assert runs >= 2 and run_with_refusal >= 1, (runs, run_with_refusal)
    # the refusals are what their names say
    for name, found in refusals.items():
        for s, i, st, res in found:
            tag = f"{s.name} step {i}: {name}"
            before = tmod.trace(s)[i][1]
            if name in ("lv_zero", "lv_repeat", "lv_ge_p"):
                vals, b = st.arg["vals"], res.bad_pos
                off = [p for p, v in enumerate(vals) if v >= P or v == 0 or v in vals[:p]]
                assert b == off[0] and (name != "lv_ge_p" or any(v >= P for v in vals)), tag
            elif name == "lv_full":
                assert len(st.arg["vals"]) + 1 > tmod.caps(s)[i] and res.bad_pos is None, tag
            elif name == "member_absent":
                b = res.bad_op
                assert st.arg["members"] and st.arg["ops"][b] == tmod.OP_MEMBER and st.vals[b] not in before, tag
                assert not any(o == tmod.OP_INSERT and v == st.vals[b] for o, v in zip(st.arg["ops"][:b], st.vals[:b])), tag
            elif name == "op2_no_flag":
                assert not st.arg["members"] and tmod.OP_MEMBER in st.arg["ops"], tag
            elif name.startswith("reserve"):
                size, depth = len(before), s.shape.depth
                pow2 = st.arg & (st.arg - 1) == 0
                assert dict(reserve_below=pow2 and 2 <= st.arg < size, reserve_npot=not pow2 and size <= st.arg <= 1 << depth,
                            reserve_above=pow2 and st.arg > 1 << depth)[name], tag
    want = {("bulk", d, im) for d in (False, True) for im in (False, True)} | \
        {("apply_pipelined", h, r) for h in (False, True) for r in (False, True)} | \
        {("mixed_filtered", what, x) for what in ("device", "item_major", "members") for x in (False, True)} | \
        {(call, x, mem) for call in ("apply_mixed", "mixed_pipelined") for x in (False, True) for mem in (False, True)} | \
        {("load_values", "device", False), ("load_values", "device", True), ("load_values", "fmt", 0), ("load_values", "fmt", 1),
         ("load_values", "fmt", 2), ("load_values", "earlier"), ("load_values", "unrelated"), ("load_values", "shorter"),
         ("load_values", "longer"), ("load_values", "same"), ("reserve", "grow"), ("reserve", "shrink"), ("reserve", "same")}
    assert variants >= want, f"variants never played: {sorted(map(str, want - variants))}"
    d32 = tmod.third_pass_d32()
    assert d32.shape.depth == 32 and {st.kind for st in d32.steps if not st.refusal} >= set(NEW)
    print(f"{len(third)} scripts of the third pass, {sum(len(s.steps) for s in third)} steps, {runs} runs of five or more pipelined steps")


def test_model_load_values_and_reserve(oracle):
    """load_values of a corpus prefix gives the corpus's root and preimages; reserve leaves every answer as it was; the
    refusals of both with their codes and bad_pos."""
    sc = next(s for s in ic.SCENARIOS if s.depth <= ic.ORACLE_MAX_DEPTH and len(ic.expected(s.name)["vals"]) <= 4096 and
              len(ic.batch_bounds(s)) >= 2)
    exp, bounds = ic.expected(sc.name), ic.batch_bounds(sc)
    for j, (a, b) in enumerate(bounds):
        m, ref = TreeModel(sc.depth, sc.cap, sc.index_base), TreeModel(sc.depth, sc.cap, sc.index_base)
        m.insert(exp["vals"][:3])                                  # whatever it held before is gone
        m.load_values(exp["vals"][:b])
        ref.insert(exp["vals"][:b])
        assert m.vals == ref.vals and m.order == ref.order and m.where == ref.where, (sc.name, j)
        assert m.preimages(range(m.size)) == ref.preimages(range(ref.size)), (sc.name, j)
        assert loaded_root(oracle, sc, m) == exp["batch_roots"][j + 1], (sc.name, j)
    fin = exp["final"]
    assert [x for p in m.preimages([int(i) - sc.index_base for i in fin["index"]]) for x in p] == arr_ints(fin["preimages"])
    # reserve: nothing but the capacity
    m = TreeModel(8, 64, 0, 3, 1)
    mine = [v for v in oracle_lib.synth_values(200, 0x544D0002) if m.mine(v)]
    m.insert(mine[:20])
    probes = m.probes()
    answers = lambda: (m.preimages(range(64)), [m.find_low(v) for v in probes], [m.lookup(v) for v in probes + mine[:25] + [0, 5]],
                       [m.nm_witness(v) for v in probes], m.vals[:], m.size)
    was = answers()
    for cap in (32, 256, 128, 32, 32):
        m.reserve(cap)
        assert m.cap == cap and answers() == was, cap
    for bad in (16, 8, 0, 1, 3, 48, 33, 512, 1 << 32):             # below the size (21), no power of two, above 2^depth
        with pytest.raises(Refused) as e:
            m.reserve(bad)
        assert e.value.code == "RANGE" and m.cap == 32 and answers() == was, bad
    with pytest.raises(Refused) as e:                              # 21 leaves + 12 > 32: FULL until the tree is reserved larger
        m.insert(mine[30:42])
    assert e.value.code == "FULL"
    m.reserve(64)
    m.insert(mine[30:42])
    assert TreeModel(3, 8).reserve(8) is None and TreeModel(32, 8).reserve(1 << 31) is None
    for bad in (16, 1 << 32):
        with pytest.raises(Refused):
            TreeModel(3, 8).reserve(bad)
    # load_values: the refusals
    m = TreeModel(8, 8, 0, 3, 1)
    a, b, c, d = mine[50:54]
    foreign = a + 1
    for vals, code, pos in (([], "ARG", None), ([a, b, c, d] + mine[60:64], "FULL", None), ([a, 0, b, P], "NONCANONICAL", 1),
                            ([a, P + 1, 0], "NONCANONICAL", 1), ([a, b, 0, a], "VALUE", 2), ([a, b, a, 0], "VALUE", 2),
                            ([a, foreign, b], "VALUE", 1), ([0], "VALUE", 0), ([a, b, c, b, a], "VALUE", 3)):
        with pytest.raises(Refused) as e:
            m.load_values(vals)
        assert (e.value.code, e.value.bad_pos) == (code, pos) and m.vals == [0], vals
    m.load_values([a, b, c, d, mine[60], mine[61], mine[62]])       # n + 1 == capacity
    assert m.size == 8


@pytest.mark.parametrize("script", tmod.scripts(), ids=lambda s: s.name)
def test_scripts_are_self_consistent(script):
    for i, (st, before, after, res) in enumerate(tmod.trace(script)):
        tag = f"{script.name} step {i} kind {tmod.writer_kind(st)}"
        if st.refusal:
            assert isinstance(res, Refused) and res.code == tmod.REFUSAL_CODE[st.refusal] and after == before, tag
        else:
            assert not isinstance(res, Exception), f"{tag}: refused with {res}"
            if st.kind in (1, 2, 3, 6, 7):
                assert after == before + tuple(st.vals), tag
            elif st.kind in (4, 5, 8):
                assert after == before + tuple(res["acc"]) and len(res["status"]) == len(st.vals), tag
            elif st.kind == 9:
                assert after == before[:st.arg], tag
            elif st.kind in (tmod.MIXED, tmod.MIXED_READS):
                ops = st.arg["ops"]
                assert after == before + tuple(v for v, o in zip(st.vals, ops) if o == tmod.OP_INSERT), tag
                assert len(res["reads"]) == ops.count(tmod.OP_READ) and (after == before) == (st.kind == tmod.MIXED_READS), tag
            elif st.kind in (tmod.BULK, tmod.APPLY_PIPE):
                assert after == before + tuple(st.vals), tag
            elif st.kind in (tmod.MIXED_FILT, tmod.APPLY_MIXED, tmod.MIXED_PIPE):
                ops, carried = st.arg["ops"], res["carried"]
                assert len(ops) == len(st.vals) and max(ops) <= (2 if st.arg["members"] else 1), tag
                assert after == before + tuple(st.vals[p] for p in carried if ops[p] == tmod.OP_INSERT) == before + tuple(res["acc"]), tag
                assert len(res["reads"]) == sum(ops[p] != tmod.OP_INSERT for p in carried), tag
                if "status" not in res:
                    assert carried == list(range(len(ops))), tag
            elif st.kind == tmod.LOAD_VALUES:
                assert after == (0, ) + st.arg["vals"], tag
            elif st.kind == tmod.RESERVE:
                assert after == before, tag
            else:
                assert after == tuple(p[0] for p in st.arg["pre"]), tag


def test_scripts_reach_the_states_of_the_two_copies():
    """The scripts are about the two lazily synchronised copies of the list, so the combinations of the flags (DESIGN.md
    section 5: mirror_valid, dev_index_valid) must occur where they matter.  Followed here with the rules of DESIGN.md: a
    GPU-prepared call needs the device index and a batch of it invalidates the mirror, a host-prepared call the other
    way round, a rewind and a load leave the device index alone valid, a full check calls device-pointer readers."""
    seen = set()
    for s in tmod.scripts():
        mirror = dev = True
        tr = tmod.trace(s)
        for i, (st, before, after, res) in enumerate(tr):
            k = st.kind
            host_prep = k in (2, 5, 7) or (k == 8 and bool(st.arg))
            changed = after != before
            if k in (1, 2, 3, 4, 5, 6, 7, 8, tmod.MIXED, tmod.MIXED_READS):
                if k >= tmod.MIXED and not dev:                  # a mixed batch is GPU-prepared: it needs the device index
                    behind = tr[i - 1][0]
                    seen.add(("mixed batch, device index stale", k, "refused" if st.refusal else "accepted"))
                    if behind.refusal and behind.kind in (2, 5, 7):
                        seen.add(("mixed batch right behind a refused host-prepared call, device index stale", k))
                if k == tmod.MIXED_READS and not st.refusal and mirror:
                    seen.add(("READs only with the mirror valid: it stays valid", ))
                seen.add(("host-prepared call, mirror dropped", ) if host_prep and not mirror else
                         ("GPU-prepared call, device index stale", ) if not host_prep and not dev else ("batch", ))
                if host_prep:
                    mirror, dev = True, dev and not changed
                else:
                    mirror, dev = mirror and not changed, True
            elif k == 9 and not st.refusal and st.arg != len(before):
                later = [x[0] for x in tr[i + 1:] if not x[0].refusal]
                nxt = later[0] if later else None
                if mirror and (st.check == FULL or (nxt is not None and (nxt.kind in (2, 5, 7) or (nxt.kind == 8 and nxt.arg)))):
                    seen.add(("rewind with the mirror valid, then a reader of the mirror", ))
                if not dev:
                    seen.add(("rewind, device index stale", ))
                mirror, dev = False, True
            elif k == 10:
                if not dev:
                    seen.add(("load, device index stale", "refused" if st.refusal else "accepted"))
                if not st.refusal:
                    mirror, dev = False, True
            # the kinds of the third pass: bulk and the mixed calls are GPU-prepared, apply_pipelined either way,
            # load_values commits into the device index and drops the mirror, reserve keeps whatever it finds
            elif k in (tmod.BULK, tmod.MIXED_FILT, tmod.APPLY_MIXED, tmod.MIXED_PIPE) and st.refusal != "plain_only":
                behind = tr[i - 1][0] if i else None
                if k == tmod.BULK and not dev:
                    seen.add(("bulk, device index stale", "refused" if st.refusal else "accepted"))
                if k != tmod.BULK and not st.refusal and tmod.OP_MEMBER in st.arg["ops"] and behind is not None and behind.refusal \
                        and (behind.kind in (2, 5, 7) or (behind.kind == tmod.APPLY_PIPE and behind.arg["host_prep"])):
                    seen.add(("MEMBERs right behind a refused host-prepared call", ))
                mirror, dev = mirror and not changed, True
            elif k == tmod.APPLY_PIPE:
                behind = tr[i - 1][0] if i else None
                if st.arg["host_prep"]:
                    if not st.refusal and behind is not None and not behind.refusal and behind.check == tmod.NO_CHECK and \
                            (behind.kind in (3, tmod.MIXED_PIPE) or (behind.kind == tmod.APPLY_PIPE and not behind.arg["host_prep"])):
                        seen.add(("host-prepared apply_pipelined right behind a GPU-prepared pipelined block", ))
                    mirror, dev = True, dev and not changed
                else:
                    mirror, dev = mirror and not changed, True
            elif k == tmod.LOAD_VALUES:
                if not dev and not st.refusal:
                    seen.add(("load_values, device index stale", ))
                if not st.refusal:
                    mirror, dev = False, True
            elif k == tmod.RESERVE and not st.refusal:
                seen.add(("reserve", mirror, dev))
            if st.check == FULL or (st.refusal and st.check != tmod.NO_CHECK):
                if st.check == FULL:
                    seen.add(("full check", mirror, dev))
                if st.refusal:
                    seen.add(("refused call, then a reader", mirror, dev))
                dev = dev or st.check == FULL or not mirror          # device-pointer readers; snapshot() without a mirror
    want = {("host-prepared call, mirror dropped", ), ("GPU-prepared call, device index stale", ),
            ("rewind with the mirror valid, then a reader of the mirror", ), ("rewind, device index stale", ),
            ("load, device index stale", "accepted"), ("full check", True, False), ("full check", False, True),
            ("full check", True, True), ("refused call, then a reader", True, False),
            ("refused call, then a reader", False, True),
            ("mixed batch, device index stale", tmod.MIXED, "accepted"), ("mixed batch, device index stale", tmod.MIXED_READS, "accepted"),
            ("mixed batch right behind a refused host-prepared call, device index stale", tmod.MIXED),
            ("mixed batch right behind a refused host-prepared call, device index stale", tmod.MIXED_READS),
            ("READs only with the mirror valid: it stays valid", ),
            ("bulk, device index stale", "accepted"), ("bulk, device index stale", "refused"),
            ("load_values, device index stale", ), ("reserve", True, False), ("reserve", False, True), ("reserve", True, True),
            ("host-prepared apply_pipelined right behind a GPU-prepared pipelined block", ),
            ("MEMBERs right behind a refused host-prepared call", )}
    assert want <= seen, f"states the scripts never reach: {sorted(map(str, want - seen))}"


# ---------------------------------------------------------------- the views kept alive beside the scripts
def test_view_schedule():
    """the schedule is a pure function of the script, and view_rounds() restates imt.h's rules of a view's cache"""
    for s in tmod.scripts():
        sched, rounds, tr = tmod.view_schedule(s), tmod.view_rounds(s), tmod.trace(s)
        assert sched == tmod.view_schedule(s) and len(sched) == len(rounds) == len(s.steps)
        live, builds_due = [1], {1: True}
        for i, ((st, before, after, res), (closed, created), rnd) in enumerate(zip(tr, sched, rounds)):
            tag = f"{s.name} step {i}"
            assert not (closed or created) or (i % tmod.VIEW_EVERY == 0 and not isinstance(res, Refused)), tag
            assert 1 not in closed and all(c in live for c in closed), tag
            live = [x for x in live if x not in closed]
            for c in created:
                assert c not in live and 1 <= c <= len(after), f"{tag}: a view is created at a size the tree has reached"
                live.append(c)
            if st.check == tmod.NO_CHECK:                          # not one call between this step and the next: no round,
                assert not rnd and not closed and not created, tag      # no view made; what it changed is due in the next round
            assert len(live) <= tmod.MAX_VIEWS and [r.size for r in rnd] == (live if st.check != tmod.NO_CHECK else []), tag
            if tmod.changes_content(st, before, after, res):
                assert after != before or st.kind in (10, tmod.LOAD_VALUES), tag
                builds_due = dict.fromkeys(builds_due, True)
            else:
                assert after == before, tag
            builds_due = {x: builds_due.get(x, True) for x in live}
            for r in rnd:
                M = len(after)
                assert r.state == (tmod.SMALLER if M < r.size else tmod.HEAD if M == r.size else tmod.BEHIND), tag
                if r.state == tmod.SMALLER:
                    assert (r.prefix, r.build, r.n_replay) == (None, False, 0), tag
                else:
                    assert r.prefix == after[:r.size] and r.build == builds_due[r.size], tag
                    assert r.n_replay == min(M - r.size, tmod.REPLAY_MAX), tag
                    builds_due[r.size] = False


def view_coverage(scripts, rounds_of):
    """what the rounds of `rounds_of(script)` cover, as a dict of counters and sets"""
    from collections import Counter, defaultdict
    cov = dict(stale_by=defaultdict(Counter), transitions=Counter(), history=Counter(), origins=Counter(), crossings=0,
               quiet=Counter(), whole_mixed=0, exactly=Counter())
    for s in scripts:
        origin, state, answered = [0], {}, {}                     # who wrote leaf i; per view its last state and prefix
        just_answered = set()                                     # the views that answered in the round before
        for (st, before, after, res), rnd in zip(tmod.trace(s), rounds_of(s)):
            k = tmod.writer_kind(st)
            if not isinstance(res, Refused) and st.kind != tmod.RESERVE:
                origin = origin + [st.kind] * len(res["acc"]) if st.kind <= 8 or tmod.MIXED <= st.kind <= tmod.MIXED_PIPE else \
                    origin[:st.arg] if st.kind == 9 else [0] + [st.kind] * (len(after) - 1)
            assert len(origin) == len(after)
            live = {r.size for r in rnd}
            state = {x: v for x, v in state.items() if x in live}
            answered = {x: v for x, v in answered.items() if x in live}
            for r in rnd:
                if r.build and r.since == (k, ):                  # the view was answering, this step made it stale
                    cov["stale_by"][s.shape.name][k] += 1
                if state.get(r.size, r.state) != r.state:
                    cov["transitions"][state[r.size], r.state] += 1
                state[r.size] = r.state
                if r.prefix is None:
                    continue
                if answered.get(r.size, r.prefix) != r.prefix:
                    cov["history"][s.shape.name] += 1
                answered[r.size] = r.prefix
                cov["origins"].update(origin[r.size:r.size + r.n_replay])
                if r.size > 2 and (r.size - 1).bit_length() != (r.size + r.n_replay - 1).bit_length():
                    cov["crossings"] += 1                         # ceil_log2 of the size changes inside the replayed range
                if not r.build and not tmod.changes_content(st, before, after, res) and st.kind != 9:
                    cov["quiet"]["refused" if st.refusal else "reserve" if st.kind == tmod.RESERVE else "accepted nothing"] += 1
                    if st.kind in (tmod.MIXED, tmod.MIXED_READS) and r.size in just_answered:      # fresh one round ago, and fresh still
                        cov["quiet"]["refused mixed batch" if st.refusal else "READs only"] += 1
                if k == tmod.MIXED and r.size <= len(before) and r.size + r.n_replay >= len(after):
                    cov["whole_mixed"] += 1                       # the replay covers every INSERT of the mixed batch
                if r.size == len(before) < len(after):            # the replayed range is exactly what this step put in
                    if k == tmod.BULK:
                        cov["exactly"]["bulk"] += 1
                    elif k == tmod.MIXED_FILT or (k == tmod.MIXED_PIPE and not st.arg["apply"]):
                        cov["exactly"]["members" if tmod.OP_MEMBER in st.arg["ops"] else "block"] += 1
            just_answered = {r.size for r in rnd if r.prefix is not None}
    return cov


def test_view_coverage():
    scripts = tmod.scripts()
    cov = view_coverage(scripts, tmod.view_rounds)
    shapes = {s.shape.name for s in scripts}
    # (a) every writer kind makes a live answering view stale and is followed by a round, within each shape
    for name in shapes:
        missing = [k for k in KINDS if not cov["stale_by"][name][k]]
        assert not missing, f"{name}: writer kinds that never make a view stale: {missing}"
    # (b) the six transitions between the three states of a view
    states = (tmod.HEAD, tmod.BEHIND, tmod.SMALLER)
    missing = [(a, b) for a in states for b in states if a != b and not cov["transitions"][a, b]]
    assert not missing, f"transitions of a view's state that never occur: {missing}"
    # (c) per shape the history changes beneath a view: it answers for another prefix than at its last answered round
    assert all(cov["history"][name] for name in shapes), cov["history"]
    # (d) replayed ranges hold leaves written by every inserting kind and by a load
    assert all(cov["origins"][k] for k in (1, 2, 3, 4, 5, 6, 7, 8, 10)), cov["origins"]
    # (e) a replayed range crosses a power of two in size
    assert cov["crossings"]
    # (f) a refused step and a filtered batch that accepted nothing are followed by a round that must not rebuild
    assert cov["quiet"]["refused"] and cov["quiet"]["accepted nothing"], cov["quiet"]
    # (g) the mixed batch: with an INSERT it makes views stale on every plain shape; READs only and a refused one right
    # behind an answered round are followed by a round that must not rebuild; replays cover leaves a mixed batch wrote,
    # and the whole of one (the replayed rows are then that step's INSERT rows: both are the oracle's)
    for name in ("d3", "d8", "d32"):
        assert cov["stale_by"][name][tmod.MIXED], f"{name}: a mixed batch never makes a view stale"
        assert not cov["stale_by"][name][tmod.MIXED_READS], f"{name}: READs only make nothing stale"
    assert cov["quiet"]["READs only"] >= 10 and cov["quiet"]["refused mixed batch"], cov["quiet"]
    assert cov["origins"][tmod.MIXED] >= 20 and cov["whole_mixed"] >= 10, (cov["origins"], cov["whole_mixed"])
    total = sum((c for c in cov["stale_by"].values()), start=type(cov["transitions"])())
    print(f"stale by kind {dict(sorted(total.items()))}, transitions {dict(cov['transitions'])}, history changes "
          f"{dict(cov['history'])}, replayed origins {dict(sorted(cov['origins'].items()))}, crossings {cov['crossings']}, "
          f"quiet rounds {dict(cov['quiet'])}")
    # the scripts replayed on the other two forms of the hash kernels, a round after every second step: every writer kind
    # is still among what a rebuilt view is stale by, every state of a view occurs, and no expectation is lost -- what a
    # skipped round would have rebuilt for, the next one does
    for name in ("d32", "part3"):
        s = next(x for x in scripts if x.shape.name == name)
        thin, full = tmod.view_rounds(s, tmod.VIEW_ROUNDS_OTHER_FORMS), tmod.view_rounds(s)
        assert all(not rnd for rnd in thin[1::2]) and all(len(a) == len(b) for a, b in zip(thin[::2], full[::2])), s.name
        assert all((a.size, a.state, a.prefix, a.n_replay) == (b.size, b.state, b.prefix, b.n_replay)
                   for x, y in zip(thin[::2], full[::2]) for a, b in zip(x, y)), s.name
        by = {k for rnd in thin for r in rnd if r.build for k in r.since}
        assert by == set(KINDS), f"{s.name}: writer kinds no rebuilt view is stale by: {sorted(set(KINDS) - by)}"
        assert {r.state for rnd in thin for r in rnd} == set(states), s.name
    # (h) the third pass by itself: every content-changing new kind makes a live answering view stale on every shape it
    # runs on, reserve is followed by an answered round that must not rebuild, replays hold leaves of kinds 14 to 19
    third = scripts[tmod.N_OLD_PASSES:]
    cov3 = view_coverage(third, tmod.view_rounds)
    for sh in tmod.THIRD_SHAPES:
        plain = not (sh.placement or sh.partition[0])
        runs = [k for k in tmod.NEW_KINDS if k != tmod.RESERVE and (plain or k not in tmod.PLAIN_ONLY)]
        missing = [k for k in runs if not cov3["stale_by"][sh.name][k]]
        assert not missing, f"{sh.name}: new kinds that never make a view stale: {missing}"
        assert not cov3["stale_by"][sh.name][tmod.RESERVE], f"{sh.name}: reserve makes nothing stale"
    assert cov3["quiet"]["reserve"] >= 5, cov3["quiet"]
    # views whose replayed range is exactly one bulk batch / one witness block that has just run (with and without MEMBERs):
    # there imt_itree_view_bulk_witness / _view_mixed_witness must give that step's own rows
    assert all(cov3["exactly"][x] for x in ("bulk", "block", "members")), cov3["exactly"]
    assert all(cov3["origins"][k] for k in tmod.NEW_KINDS if k != tmod.RESERVE), cov3["origins"]
    s = tmod.third_pass_d32()
    thin = tmod.view_rounds(s, tmod.VIEW_ROUNDS_OTHER_FORMS)
    assert all(not rnd for rnd in thin[1::2]) and any(r.build for rnd in thin for r in rnd), s.name
    # the view at size 1 alone is not enough: the tree is never smaller than it, and it never sees another history
    alone = view_coverage(scripts, lambda s: [[r for r in rnd if r.size == 1] for rnd in tmod.view_rounds(s)])
    assert not any(tmod.SMALLER in pair for pair in alone["transitions"]) and not alone["history"]
