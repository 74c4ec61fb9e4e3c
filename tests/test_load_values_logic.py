"""CPU: the check of imt_itree_load_values through the functions the device runs -- load_values_rank and lv_pos_less
(csrc/imt_prep_logic.hpp) -- in the stand-alone program tests/native/load_values_rules.cpp, which orders the positions the
way the device does (by the top 64 bits first, by the full comparator after a reported tie).

The expectation is a plain walk: insert the values one at a time into a set and stop at the first one that is >= p, 0, of
a foreign residue or in the set already.  Where the walk stops is the offending position; a list it gets through is
accepted and its order must be the positions sorted by (value, position).  The error bits are checked against their
definition over the whole list (they decide the return code: NONCANONICAL wins wherever the value >= p stands).

Cases: random lists; lists equal in the top 64 bits and in the top 192 bits; one value repeated 64 times between two
others; a zero at the first, middle and last position; a value >= p before and after a repeat; a foreign residue.  The
program runs once more built with -fsanitize=address,undefined, as a program of its own."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "load_values_rules.cpp")
GXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
P = 0x30644e72e131a029b85045b68181585d2833e84879b97091_43e1f593f0000001
NONCANONICAL, ZERO, DUPLICATE, FOREIGN, TIE = 1, 2, 4, 8, 128


def foreign(v, mod, res):
    return mod > 1 and v % mod != res


def walk(vals, mod=0, res=0):
    """the position one-by-one insertion stops at, -1 if it gets through"""
    seen = set()
    for q, v in enumerate(vals):
        if v >= P or v == 0 or foreign(v, mod, res) or v in seen:
            return q
        seen.add(v)
    return -1


def bits_of(vals, mod=0, res=0):
    """the error bits by their definition: every position judged, equal values against the one before in (value, position)"""
    order = sorted(range(len(vals)), key=lambda q: (vals[q], q))
    bits = 0
    for r, q in enumerate(order):
        v = vals[q]
        bits |= NONCANONICAL * (v >= P) | ZERO * (v == 0) | FOREIGN * foreign(v, mod, res)
        bits |= DUPLICATE * (r > 0 and vals[order[r - 1]] == v)
    return bits


def render(vals, mod=0, res=0):
    return "\n".join([f"C {len(vals)} {mod} {res}"] + [format(v, "064x") for v in vals]) + "\n"


def run(exe, cases):
    r = subprocess.run([exe], input="".join(render(*c) for c in cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.split("\n")
    assert out[-2] == f"cases {len(cases)} ok"
    at, stats = 0, dict(ok=0, bad=0, fallback=0)
    for ci, case in enumerate(cases):
        vals = case[0]
        bits, bad, attempts = map(int, out[at].split())
        at += 1
        tag = (ci, [hex(v) for v in vals[:8]], len(vals), case[1:], bits, bad, attempts)
        assert bad == walk(*case), tag
        assert bits == bits_of(*case), tag
        stats["fallback"] += attempts == 2
        if bits:
            stats["bad"] += 1
            continue
        stats["ok"] += 1
        order = list(map(int, out[at].split()))
        at += 1
        assert order == sorted(range(len(vals)), key=lambda q: (vals[q], q)), tag
    return stats


def distinct(rng, n, bits=254, top=0):
    s = set()
    while len(s) < n:
        v = top | rng.getrandbits(bits)
        if 0 < v < P:
            s.add(v)
    out = list(s)
    rng.shuffle(out)
    return out


def all_cases():
    rng = random.Random(0x4C56414C)
    cases = []
    for n in (1, 2, 3, 17, 64, 257, 1000):
        cases.append((distinct(rng, n),))
    top64 = 0x1234_5678_9ABC_DEF0 << 192
    top192 = (0x0FED_CBA9_8765_4321 << 128 | 0x1111_2222_3333_4444 << 64 | 0x5555_6666_7777_8888) << 64
    for n in (2, 33, 300):
        cases.append((distinct(rng, n, 192, top64),))
        cases.append((distinct(rng, n, 64, top192),))
        cases.append((distinct(rng, n, 192, top64) + distinct(rng, n),))      # a tied group among others
    # one value repeated 64 times between two others; the same with equal top limbs around it (repeats behind the fallback)
    a, b, c = sorted(distinct(rng, 3))
    cases.append(([a] + [b] * 64 + [c],))
    cases.append(([c] + [b] * 64 + [a],))
    t = sorted(distinct(rng, 3, 192, top64))
    cases.append(([t[2]] + [t[1]] * 64 + [t[0]],))
    cases.append(([t[2], t[0], t[1], t[0]],))
    # a zero at the first, middle and last position (a repeat of the sentinel), and two of them
    base = distinct(rng, 40)
    for at in (0, 20, 40):
        cases.append((base[:at] + [0] + base[at:],))
    cases.append((base[:7] + [0] + base[7:30] + [0] + base[30:],))
    cases.append(([0],))
    # a value >= p before and after a repeat: the code (NONCANONICAL wherever it stands) and the position apart
    for big in (P, P + 1, (1 << 256) - 1):
        cases.append((base[:5] + [big] + base[5:20] + [base[10]] + base[20:],))
        cases.append((base[:5] + [base[2]] + base[5:20] + [big] + base[20:],))
        cases.append(([big] + base,))
        cases.append((base + [big],))
        cases.append((base[:9] + [big, big] + base[9:],))                     # >= p AND a repeat of one another
    cases.append((base + [P - 1],))                                           # the largest canonical value is fine
    # a repeat at the first possible and at the last position
    cases.append(([base[0], base[0]] + base[1:],))
    cases.append((base + [base[0]],))
    cases.append((base + [base[-1]],))
    # a value partition: every value of residue 3 mod 7, then one foreign value at the front, the middle, the end
    res = [v for v in distinct(rng, 400) if v % 7 == 3][:30]
    odd = next(v for v in distinct(rng, 50) if v % 7 != 3)
    cases.append((res, 7, 3))
    for at in (0, 15, len(res)):
        cases.append((res[:at] + [odd] + res[at:], 7, 3))
    cases.append((res[:4] + [odd] + res[4:] + [res[0]], 7, 3))
    cases.append((res[:4] + [res[0]] + res[4:] + [odd], 7, 3))
    # random lists with random defects
    for _ in range(300):
        n = rng.randrange(1, 80)
        top = rng.choice([0, 0, top64, top192])
        vals = distinct(rng, n, {0: 254, top64: 192, top192: 64}[top], top)
        for _ in range(rng.choice([0, 0, 1, 1, 2, 3])):
            vals.insert(rng.randrange(len(vals) + 1), rng.choice([0, P, P + rng.getrandbits(60), rng.choice(vals), rng.choice(vals)]))
        cases.append((vals,))
    return cases


def test_the_expectation_itself():
    assert walk([5, 9, 7]) == -1 and bits_of([5, 9, 7]) == 0
    assert walk([5, 9, 5, 0]) == 2 and bits_of([5, 9, 5, 0]) == DUPLICATE | ZERO
    assert walk([5, 0, 0]) == 1 and bits_of([5, 0, 0]) == ZERO | DUPLICATE
    assert walk([5, P, 5]) == 1 and walk([5, 5, P]) == 1 and bits_of([5, 5, P]) == NONCANONICAL | DUPLICATE
    assert walk([3, 10, 4], 7, 3) == 2 and bits_of([3, 10, 4], 7, 3) == FOREIGN


def test_load_values_rules(tmp_path):
    exe = str(tmp_path / "load_values_rules")
    subprocess.run(GXX + ["-O2", "-o", exe, SRC], check=True)
    stats = run(exe, all_cases())
    assert stats["ok"] >= 100 and stats["bad"] >= 100 and stats["fallback"] >= 50, stats


def test_load_values_rules_under_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, over the same cases, on the CPU"""
    exe = str(tmp_path / "load_values_rules_san")
    subprocess.run(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    run(exe, all_cases())
