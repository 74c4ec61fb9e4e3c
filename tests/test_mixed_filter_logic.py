"""CPU: the per-operation rule of imt_itree_mixed_filtered (csrc/imt_filter_logic.hpp: filter_class, mixed_pos_less,
mixed_filter_rank -- the code the kernels of prep::mixed_filter run), through the stand-alone program
tests/native/mixed_filter_rules.cpp.

The expectation is the definition: walk the operations in order over the set of stored values.  An operation whose value
is 0 is ZERO, one whose value was stored before the call is PRESENT, one whose value an earlier accepted INSERT of the
block put in is REPEATED, every other one is NEW and carried out; first[v] is recorded at an accepted INSERT only.  Two
more things are asserted of the accepted sub-script: test_mixed_logic.walk never refuses it, and its rows are the rows of
the full walk with the refusals skipped.

Scripts: every adversarial script of test_mixed_logic (refused or not: here all of them are legal input), 900 random ones
and the handwritten ones below.  The program runs once more built with -fsanitize=address,undefined."""
import bisect
import os
import random
import subprocess

import test_mixed_logic as ml
from test_mixed_logic import ADVERSARIAL, INSERT, READ, random_case, render, walk

SRC = os.path.join(ml.ROOT, "tests", "native", "mixed_filter_rules.cpp")
NEW, ZERO, PRESENT, REPEATED = 0, 1, 2, 3


def filtered_walk(stored, script):
    """(status, aux, leaf, rows, accepted): status / aux / leaf per position (aux: stored leaf of a PRESENT value, f(v) of
    a REPEATED one, else -1); rows = (low leaf, successor leaf or -1) of the accepted operations; accepted = their
    positions"""
    have = {v: i for i, v in enumerate(stored)}
    order = sorted((v, i) for i, v in enumerate(stored))
    first, first_leaf = {}, {}
    status, aux, leaf, rows, accepted = [], [], [], [], []
    n_ins = 0
    for p, (op, v) in enumerate(script):
        if v == 0:
            status.append(ZERO), aux.append(-1), leaf.append(0)
        elif v in have:
            status.append(PRESENT), aux.append(have[v]), leaf.append(have[v])
        elif v in first:
            status.append(REPEATED), aux.append(first[v]), leaf.append(first_leaf[v])
        else:
            k = bisect.bisect_left(order, (v, -1))
            low = order[k - 1][1]
            rows.append((low, order[k][1] if k < len(order) else -1))
            accepted.append(p)
            status.append(NEW), aux.append(-1)
            if op == INSERT:
                first[v], first_leaf[v] = p, len(stored) + n_ins
                leaf.append(first_leaf[v])
                order.insert(k, (v, first_leaf[v]))
                n_ins += 1
            else:
                leaf.append(low)
    return status, aux, leaf, rows, accepted


TOP = 1 << 192
HANDWRITTEN = {
    "nothing accepted": ([0, 10, 20], [(INSERT, 0), (READ, 10), (INSERT, 20), (READ, 0), (INSERT, 10), (READ, 20)]),
    "one value 64 times": ([0, 10], [(READ, 7), (INSERT, 7)] + [(p & 1, 7) for p in range(62)]),
    "reads around the inserts of one value": ([0, 10], [(READ, 5), (READ, 5), (INSERT, 5), (READ, 5), (INSERT, 5)]),
    "stored value inserted, then read": ([0, 10, 20], [(INSERT, 20), (READ, 20), (INSERT, 15)]),
    "top limb only": ([0, 5 + TOP], [(READ, 5), (INSERT, 5 + 2 * TOP), (READ, 5 + TOP), (INSERT, 5), (READ, 5 + 2 * TOP),
                                      (INSERT, 5 + 3 * TOP), (READ, 5), (INSERT, 5 + 2 * TOP), (READ, 5 + 3 * TOP),
                                      (READ, 5 + 4 * TOP)]),
}


def all_cases():
    rng = random.Random(0x4D46494C)
    cases = list(ADVERSARIAL.values()) + list(HANDWRITTEN.values())
    cases += [random_case(rng, wide=False) for _ in range(600)]
    cases += [random_case(rng, wide=True) for _ in range(300)]
    return cases


def run(exe, cases):
    r = subprocess.run([exe], input="".join(render(s, sc) for s, sc in cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.split("\n")
    assert out[-2] == f"scripts {len(cases)} ok"
    at = 0
    for ci, (stored, script) in enumerate(cases):
        got = [ln.split() for ln in out[at:at + len(script)]]
        assert out[at + len(script)] == "end"
        at += len(script) + 1
        status, aux, _, rows, accepted = filtered_walk(stored, script)
        for p, ((op, v), g) in enumerate(zip(script, got)):
            assert g[0] == "IR"[op] and (int(g[1]), int(g[2])) == (status[p], aux[p]), (ci, p, stored, script, g, status[p], aux[p])
        # the accepted sub-script is a block imt_itree_mixed_batch takes, and its rows are the walk's with refusals skipped
        sub_rows, bad = walk(stored, [script[p] for p in accepted])
        assert bad == -1 and sub_rows == rows, (ci, stored, script)


def test_the_walk_by_hand():
    """the expectation's own edge cases"""
    st, aux, leaf, rows, acc = filtered_walk(*HANDWRITTEN["one value 64 times"])
    assert st == [NEW, NEW] + [REPEATED] * 62 and aux[2:] == [1] * 62 and leaf == [0] + [2] * 63 and acc == [0, 1]
    st, aux, leaf, rows, acc = filtered_walk(*HANDWRITTEN["reads around the inserts of one value"])
    assert st == [NEW, NEW, NEW, REPEATED, REPEATED] and aux == [-1, -1, -1, 2, 2] and leaf == [0, 0, 2, 2, 2]
    st, aux, leaf, rows, acc = filtered_walk(*HANDWRITTEN["stored value inserted, then read"])
    assert st == [PRESENT, PRESENT, NEW] and aux == [2, 2, -1] and leaf == [2, 2, 3]
    st, _, _, _, acc = filtered_walk(*HANDWRITTEN["nothing accepted"])
    assert acc == [] and set(st) == {ZERO, PRESENT}
    st, aux, leaf, rows, acc = filtered_walk(*HANDWRITTEN["top limb only"])
    assert st == [NEW, NEW, PRESENT, NEW, REPEATED, NEW, REPEATED, REPEATED, REPEATED, NEW]
    assert aux == [-1, -1, 1, -1, 1, -1, 3, 1, 5, -1]
    # a script nothing is refused in is the walk of test_mixed_logic
    stored, script = ADVERSARIAL["reads between value neighbours"]
    st, _, _, rows, acc = filtered_walk(stored, script)
    assert set(st) == {NEW} and acc == list(range(len(script))) and (rows, -1) == walk(stored, script)


def test_the_scripts_cover_every_kind():
    pairs = {(op, s): 0 for op in (INSERT, READ) for s in (NEW, ZERO, PRESENT, REPEATED)}
    read_before_insert = 0
    for stored, script in all_cases():
        status = filtered_walk(stored, script)[0]
        for key in {(op, s) for (op, _), s in zip(script, status)}:
            pairs[key] += 1
        ins_at = {}
        for p, (op, v) in enumerate(script):
            if op == INSERT:
                ins_at[v] = max(ins_at.get(v, -1), p)
        read_before_insert += any(op == READ and s == NEW and ins_at.get(v, -1) > p for p, ((op, v), s) in enumerate(zip(script, status)))
    assert min(pairs.values()) >= 30, pairs
    assert read_before_insert >= 300, read_before_insert


def test_mixed_filter_rules(tmp_path):
    exe = str(tmp_path / "mixed_filter_rules")
    subprocess.run(ml.GXX + ["-O2", "-o", exe, SRC], check=True)
    run(exe, all_cases())


def test_mixed_filter_rules_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, over the same scripts, on the CPU"""
    exe = str(tmp_path / "mixed_filter_rules_san")
    subprocess.run(ml.GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    run(exe, all_cases())
