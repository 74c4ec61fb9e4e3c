"""CPU: a mixed list replayed against the rows the tree stores (imt_itree_view_mixed_witness), through the functions the
device runs -- replay_op_class, read_neighbours, insert_is_duplicate (csrc/imt_prep_logic.hpp), sweep::merge_element and
replay::sibling_source (csrc/imt_replay.hpp, what k_sweep_view_mixed asks) -- in the stand-alone program
tests/native/replay_mixed_rules.cpp.

Every case is "stored prefix, the list, a tail of later insertions": the tree holds the prefix, then the INSERTs of the list
as it applied them, then the tail; the view is at the prefix.  The expectation is the definition:

  * walk the list over a sorted list of the prefix.  The first position at which the walk refuses the operation (0, in the
    list by then) OR the operation is an INSERT of rank r whose value is not the tree's row S + r is the offending position;
    a list with more INSERTs than the tree holds rows beyond the prefix is out of range before anything else;
  * an accepted list is compared operation by operation (low leaf, successor) and event by event: the sibling
    y = (pos >> l) ^ 1 of event e at level l < L0 comes from
        BATCH   an earlier event of the list under y, if there is one (a READ's event counts: it rewrites its low leaf);
        EMPTY   iff y >= ceil(S / 2^l);
        SIDE    iff y is in S_l (S_0 = the kept leaves whose successor in the tree as it is now is not kept, and S itself;
                S_(l+1) = {x >> 1});
        STORED  otherwise
    -- tests/test_replay_logic.py's rule for events that are READs as well.

Cases: the adversarial scripts of test_mixed_logic (refused ones included) and 900 random scripts, each with a tail; from
accepted ones the mismatches: one INSERT altered, two altered, an altered INSERT behind a READ the walk refuses and in front
of one, the tree's rows in another order, one INSERT too many.  The program runs once more built with
-fsanitize=address,undefined, as a program of its own."""
import bisect
import os
import random
import subprocess

from test_mixed_logic import ADVERSARIAL, GXX, INSERT, READ, random_case, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "replay_mixed_rules.cpp")
EMPTY, SIDE, STORED, BATCH = 0, 1, 2, 3
DEPTH = 12


def ceil_log2(x):
    return (x - 1).bit_length()


def expect(prefix, rows, script):
    """("range",) | ("bad", p) | ("ok", [(low, succ)], {(l, e): class}) for the list against the tree prefix + rows"""
    S, M = len(prefix), len(prefix) + len(rows)
    n_ins = sum(op == INSERT for op, _ in script)
    if n_ins > len(rows):
        return ("range",)
    order = sorted((v, i) for i, v in enumerate(prefix))
    out, pos, r = [], [], 0
    for p, (op, v) in enumerate(script):
        if op == INSERT and rows[r] != v:
            return ("bad", p)
        k = bisect.bisect_left(order, (v, -1))
        if v == 0 or (k < len(order) and order[k][0] == v):
            return ("bad", p)
        out.append((order[k - 1][1], order[k][1] if k < len(order) else -1))
        pos.append(order[k - 1][1])
        if op == INSERT:
            pos.append(S + r)
            order.insert(k, (v, S + r))
            r += 1
    cls = {}
    if S < M:
        full = list(prefix) + list(rows)
        by_val = sorted(range(M), key=full.__getitem__)
        level = {S} | {by_val[j] for j in range(M - 1) if by_val[j] < S <= by_val[j + 1]}
        for l in range(min(ceil_log2(S + n_ins), DEPTH)):
            fill, seen = -(-S // (1 << l)), set()
            for e, x in enumerate(pos):
                y = (x >> l) ^ 1
                cls[l, e] = BATCH if y in seen else EMPTY if y >= fill else SIDE if y in level else STORED
                seen.add(x >> l)
            level = {x >> 1 for x in level}
    return ("ok", out, cls)


def render(prefix, rows, script):
    lines = [f"C {len(prefix)} {len(prefix) + len(rows)} {len(script)} {DEPTH}"]
    lines += [format(v, "064x") for v in list(prefix) + list(rows)]
    return "\n".join(lines + [f"{op} {v:064x}" for op, v in script]) + "\n"


def run(exe, cases):
    r = subprocess.run([exe], input="".join(render(*c) for c in cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.split("\n")
    assert out[-2] == f"cases {len(cases)} ok"
    at, kinds, sources = 0, {"range": 0, "bad": 0, "ok": 0}, set()
    for ci, (prefix, rows, script) in enumerate(cases):
        want = expect(prefix, rows, script)
        head = out[at].split()
        at += 1
        tag = (ci, prefix, rows, script, head, want[:2])
        assert head[0] == want[0], tag
        kinds[want[0]] += 1
        if want[0] == "bad":
            assert int(head[1]) == want[1], tag
        if want[0] != "ok":
            continue
        n_ins = sum(op == INSERT for op, _ in script)
        L0, E = int(head[1]), int(head[2])
        assert E == len(script) + n_ins, tag
        assert L0 == (min(ceil_log2(len(prefix) + n_ins), DEPTH) if rows else 0), tag
        for p, (op, _) in enumerate(script):
            g = out[at + p].split()
            assert g[0] == "IR"[op] and (int(g[1]), int(g[2])) == want[1][p], (tag, p, g)
        at += len(script)
        assert len(want[2]) == L0 * E
        for l in range(L0):
            line = out[at + l]
            assert len(line) == E, tag
            for e in range(E):
                assert int(line[e]) == want[2][l, e], (tag, f"level {l} event {e}: {line[e]}, expected {want[2][l, e]}")
                sources.add((want[2][l, e], script_kind(script, e)))
        at += L0
    return kinds, sources


def script_kind(script, e):
    """READ if event e of the list is a READ's"""
    at = 0
    for op, _ in script:
        if e == at:
            return op
        at += 2 if op == INSERT else 1
        if e < at:
            return INSERT
    raise AssertionError(e)


def tail_for(rng, prefix, script, k):
    """k later values: fresh ones, and values the list only READs"""
    present = set(prefix) | {v for op, v in script if op == INSERT}
    reads = [v for op, v in script if op == READ and v not in present and v != 0]
    out = []
    while len(out) < k:
        v = rng.choice(reads) if reads and rng.random() < 0.3 else rng.randrange(1, 1 << 20) * 2 + (1 << 30)
        if v not in present:
            present.add(v)
            out.append(v)
    return out


def played(rng, stored, script):
    """(prefix, rows, script): the tree applied the INSERTs of the list up to the walk's first refusal, then whatever of the
    rest it could, then a tail long enough for every INSERT of the list to have a row"""
    bad = walk(stored, script)[1]
    upto = len(script) if bad < 0 else bad
    rows = [v for op, v in script[:upto] if op == INSERT]
    present = set(stored) | set(rows)
    for op, v in script[upto:]:
        if op == INSERT and v != 0 and v not in present:
            present.add(v)
            rows.append(v)
    need = sum(op == INSERT for op, _ in script) - len(rows)
    return list(stored), rows + tail_for(rng, stored + rows, script, need + rng.randrange(0, 7)), script


def mismatches(rng, prefix, rows, script):
    """variants of an accepted case in which the list is not the block the tree applied"""
    ins = [p for p, (op, _) in enumerate(script) if op == INSERT]
    rds = [p for p, (op, _) in enumerate(script) if op == READ]
    fresh = lambda: rng.randrange(1, 1 << 20) * 2 + 1 + (1 << 40)           # odd: in no tree, no list and no tail
    out = []
    if ins:
        p = rng.choice(ins)
        out.append((prefix, rows, script[:p] + [(INSERT, fresh())] + script[p + 1:]))
        out.append((prefix, rows[:len(ins) - 1], script))                           # one INSERT too many for the tree
    if len(ins) >= 2:
        p, q = sorted(rng.sample(ins, 2))
        alt = list(script)
        alt[p], alt[q] = (INSERT, fresh()), (INSERT, fresh())
        out.append((prefix, rows, alt))
        swapped = list(rows)
        swapped[0], swapped[1] = swapped[1], swapped[0]
        out.append((prefix, swapped, script))                                       # the same values in another order
    if ins and rds and len(prefix) > 1:
        for p in (min(ins), max(ins)):                                              # an altered INSERT and a refused READ
            q = rng.choice(rds)
            alt = list(script)
            alt[p] = (INSERT, fresh())
            alt[q] = (READ, rng.choice(prefix[1:]))
            out.append((prefix, rows, alt))
    return out


def all_cases():
    rng = random.Random(0x564D4C47)
    scripts = list(ADVERSARIAL.values())
    scripts += [random_case(rng, wide=False) for _ in range(600)]
    scripts += [random_case(rng, wide=True) for _ in range(300)]
    cases = [played(rng, st, sc) for st, sc in scripts]
    extra = []
    for prefix, rows, script in cases[::3]:
        if expect(prefix, rows, script)[0] == "ok":
            extra += mismatches(rng, prefix, rows, script)
    # by hand: the minimum over both kinds of offence, in both orders
    tree = ([0, 10, 20, 30], [5, 50, 40, 25, 60, 15])
    for script in ([(INSERT, 5), (READ, 6), (INSERT, 51), (INSERT, 40)], [(INSERT, 6), (READ, 7), (INSERT, 50), (INSERT, 41)],
                   [(INSERT, 5), (READ, 20), (INSERT, 51)], [(INSERT, 5), (INSERT, 51), (READ, 20)],
                   [(INSERT, 5), (READ, 5), (INSERT, 50), (INSERT, 41)], [(INSERT, 50), (INSERT, 5)],
                   [(INSERT, 5), (INSERT, 50), (INSERT, 40), (INSERT, 25), (INSERT, 61)],
                   [(INSERT, 5), (READ, 60), (INSERT, 50), (READ, 15), (READ, 15)],
                   [(INSERT, x) for x in tree[1]] + [(READ, 9), (INSERT, 70)], [(READ, 9), (READ, 35)]):
        extra.append(tree + (script,))
    extra.append(([0, 10, 20, 30], [], [(READ, 9), (READ, 35), (READ, 9)]))       # the view at the tree's size
    extra.append(([0, 10, 20, 30], [], [(READ, 9), (INSERT, 35)]))
    return cases + extra


def test_the_expectation_itself():
    """by hand: the minimum of the two offences, the range, the sources of a small list"""
    tree = ([0, 10, 20, 30], [5, 50, 40, 25, 60, 15])
    assert expect(*tree, [(INSERT, 5), (READ, 20), (INSERT, 51)]) == ("bad", 1)
    assert expect(*tree, [(INSERT, 5), (INSERT, 51), (READ, 20)]) == ("bad", 1)
    assert expect(*tree, [(INSERT, 6), (READ, 20)]) == ("bad", 0)
    assert expect(*tree, [(INSERT, x) for x in tree[1]] + [(INSERT, 70)]) == ("range",)
    kind, rows, cls = expect(*tree, [(READ, 60), (INSERT, 5), (READ, 7)])
    assert kind == "ok" and rows == [(3, -1), (0, 1), (4, 1)]
    # S = 4 and every kept leaf got a new successor (5, 15, 25, 40): S_0 = {0, 1, 2, 3, 4}.  The events sit at leaves 3, 0, 4, 4.
    assert [cls[0, e] for e in range(4)] == [SIDE, SIDE, EMPTY, EMPTY]
    assert [cls[1, e] for e in range(4)] == [SIDE, BATCH, EMPTY, EMPTY]
    assert [cls[2, e] for e in range(4)] == [EMPTY, EMPTY, BATCH, BATCH]


def test_replay_mixed_rules(tmp_path):
    exe = str(tmp_path / "replay_mixed_rules")
    subprocess.run(GXX + ["-I", os.path.dirname(SRC), "-O2", "-o", exe, SRC], check=True)
    kinds, sources = run(exe, all_cases())
    assert kinds["ok"] >= 400 and kinds["bad"] >= 300 and kinds["range"] >= 100, kinds
    assert sources == {(c, k) for c in (EMPTY, SIDE, STORED, BATCH) for k in (INSERT, READ)}, "every source, for both kinds of event"


def test_replay_mixed_rules_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, over the same cases, on the CPU"""
    exe = str(tmp_path / "replay_mixed_rules_san")
    subprocess.run(GXX + ["-I", os.path.dirname(SRC), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-o", exe, SRC], check=True)
    run(exe, all_cases())
