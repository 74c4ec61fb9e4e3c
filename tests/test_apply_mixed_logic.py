"""CPU: the event rule of a witness-free mixed block (csrc/imt_prep_logic.hpp: insert_event, insert_event_preimages -- the
code the kernel of prep::mixed_insert_events runs for imt_itree_apply_mixed), through the stand-alone program
tests/native/apply_mixed_rules.cpp, which runs it over the low / succ rows the mixed checks leave.

The expectation is the definition: a READ changes nothing, so the events of a block are those of its INSERTs alone.
Remove the READs and walk what is left over a sorted list (test_mixed_logic.walk): the INSERT of rank r has low leaf and
successor as that walk finds them, event 2r rewrites the low leaf to {low.val, v, M + r} under key (low << 32) | 2r, and
event 2r + 1 writes leaf M + r as {v, succ.val, succ} ({v, 0, 0} above everything) under key ((M + r) << 32) | (2r + 1).

Scripts: the adversarial scripts of test_mixed_logic, the handwritten ones of test_mixed_filter_logic and 900 random ones.
A script the walk refuses is played as imt_itree_apply_mixed_filtered plays it -- its accepted operations
(filtered_walk) -- and once as it is, where the program must name the refused position and run no event.  The program
runs once more built with -fsanitize=address,undefined."""
import os
import random
import subprocess

import test_mixed_logic as ml
from test_mixed_filter_logic import HANDWRITTEN, filtered_walk
from test_mixed_logic import ADVERSARIAL, INSERT, random_case, render, walk

SRC = os.path.join(ml.ROOT, "tests", "native", "apply_mixed_rules.cpp")


def le(v):
    return v.to_bytes(32, "little").hex()


def expected_events(stored, script):
    """one tuple per INSERT: (low, succ, key_low, key_new, preimage of event 2r, preimage of event 2r + 1)"""
    inserts = [(op, v) for op, v in script if op == INSERT]
    rows, bad = walk(stored, inserts)
    assert bad == -1
    vals, m = list(stored) + [v for _, v in inserts], len(stored)
    out = []
    for r, ((_, v), (low, succ)) in enumerate(zip(inserts, rows)):
        nxt = le(vals[succ]) + le(succ) if succ >= 0 else le(0) + le(0)
        out.append((low, succ, (low << 32) | (2 * r), ((m + r) << 32) | (2 * r + 1), le(vals[low]) + le(v) + le(m + r), le(v) + nxt))
    return out


def all_cases():
    """(stored, script): every script once as the filter leaves it, the refused ones also as they are"""
    rng = random.Random(0x41504D58)
    raw = list(ADVERSARIAL.values()) + list(HANDWRITTEN.values())
    raw += [random_case(rng, wide=False) for _ in range(600)]
    raw += [random_case(rng, wide=True) for _ in range(300)]
    cases = []
    for stored, script in raw:
        accepted = filtered_walk(stored, script)[4]
        cases.append((stored, [script[p] for p in accepted]))
        if len(accepted) < len(script):
            cases.append((stored, script))
    return [c for c in cases if c[1]]


def run(exe, cases):
    r = subprocess.run([exe], input="".join(render(s, sc) for s, sc in cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.split("\n")
    assert out[-2] == f"scripts {len(cases)} ok"
    at = events = 0
    for ci, (stored, script) in enumerate(cases):
        want_bad = walk(stored, script)[1]
        if want_bad >= 0:
            assert out[at] == f"bad {want_bad}", (ci, stored, script, out[at])
            at += 1
            continue
        want = expected_events(stored, script)
        for r_, w in enumerate(want):
            g = out[at + r_].split()
            assert g[0] == "E" and (int(g[1]), int(g[2]), int(g[3]), int(g[4]), g[5], g[6]) == w, (ci, r_, stored, script, g, w)
        assert out[at + len(want)] == "bad -1", (ci, stored, script)
        at += len(want) + 1
        events += len(want)
    return events


def test_the_expectation_by_hand():
    """[0, 10] + READ 5, INSERT 20, READ 25, INSERT 5: the READs leave no trace, 5 lands between the sentinel and 10"""
    ev = expected_events([0, 10], [(1, 5), (0, 20), (1, 25), (0, 5)])
    assert [e[:4] for e in ev] == [(1, -1, (1 << 32) | 0, (2 << 32) | 1), (0, 1, 2, (3 << 32) | 3)]
    assert ev[0][4] == le(10) + le(20) + le(2) and ev[0][5] == le(20) + le(0) + le(0)
    assert ev[1][4] == le(0) + le(5) + le(3) and ev[1][5] == le(5) + le(10) + le(1)


def test_the_scripts_cover_the_ground():
    cases = all_cases()
    accepted = [(s, sc) for s, sc in cases if walk(s, sc)[1] < 0]
    assert len(accepted) >= 900 and len(cases) - len(accepted) >= 50
    with_reads = sum(any(op != INSERT for op, _ in sc) and any(op == INSERT for op, _ in sc) for _, sc in accepted)
    largest = sum(any(e[1] < 0 for e in expected_events(s, sc)) for s, sc in accepted)
    chained = sum(any(e[0] >= len(s) for e in expected_events(s, sc)) for s, sc in accepted)       # low leaf from this block
    assert with_reads >= 600 and largest >= 200 and chained >= 400, (with_reads, largest, chained)


def test_apply_mixed_rules(tmp_path):
    exe = str(tmp_path / "apply_mixed_rules")
    subprocess.run(ml.GXX + ["-O2", "-o", exe, SRC], check=True)
    assert run(exe, all_cases()) >= 5000


def test_apply_mixed_rules_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, over the same scripts, on the CPU"""
    exe = str(tmp_path / "apply_mixed_rules_san")
    subprocess.run(ml.GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    run(exe, all_cases())
