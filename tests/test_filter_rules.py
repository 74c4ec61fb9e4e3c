"""CPU: the classification rule of imt_itree_insert_filtered and imt_itree_lookup_batch (csrc/imt_filter_logic.hpp, the
code the kernels run) against a plain sequential model: the reference's insert_leaf loop with the rejected values
skipped.  The header is compiled here with g++ into a small driver (tests/native/filter_rules.cpp) that composes it the
way prep::filter does on the device.  10^5 random batches over a small value pool, so that repeats, stored values and
zeros are frequent, plus the edge cases by name."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
NEW, ZERO, PRESENT, REPEATED, FOREIGN = 0, 1, 2, 3, 4
NONE = (1 << 64) - 1
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter") / "filter_rules")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "native", "filter_rules.cpp")], check=True)
    return exe


def model(stored, batch, pm, pr, base):
    """stored: values by leaf index (leaf 0 = the sentinel 0).  The reference's loop, one value at a time."""
    M = len(stored)
    where = {v: i for i, v in enumerate(stored)}
    first = {}
    acc, status, leaf = [], [], []
    for v in batch:
        if v == 0:
            s, l = ZERO, base
        elif pm > 1 and v % pm != pr:
            s, l = FOREIGN, NONE
        elif v in where:
            s, l = PRESENT, base + where[v]
        elif v in first:
            s, l = REPEATED, base + M + first[v]
        else:
            first[v] = len(acc)
            acc.append(v)
            s, l = NEW, base + M + first[v]
        status.append(s)
        leaf.append(l)
    return status, leaf, acc


def lookup_model(stored, batch, pm, pr, base):
    where = {v: i for i, v in enumerate(stored)}
    status, leaf = [], []
    for v in batch:
        if v == 0:
            status.append(ZERO), leaf.append(base)
        elif pm > 1 and v % pm != pr:
            status.append(FOREIGN), leaf.append(NONE)
        elif v in where:
            status.append(PRESENT), leaf.append(base + where[v])
        else:
            low = max(x for x in stored if x < v)
            status.append(NEW), leaf.append(base + where[low])
    return status, leaf


def run(driver, tmp_path, cases):
    """cases: (stored, batch, pm, pr, base) -> per case (status, leaf, acc, lookup status, lookup leaf)"""
    parts = [struct.pack("<I", len(cases))]
    for stored, batch, pm, pr, base in cases:
        parts.append(struct.pack("<IIIIQ", len(stored), len(batch), pm, pr, base))
        parts.extend(v.to_bytes(32, "little") for v in stored)
        parts.extend(v.to_bytes(32, "little") for v in batch)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(b"".join(parts))
    subprocess.run([driver, str(fin), str(fout)], check=True)
    data, off, res = fout.read_bytes(), 0, []
    for stored, batch, pm, pr, base in cases:
        n = len(batch)
        st = list(data[off:off + n]); off += n
        leaf = list(np.frombuffer(data, np.uint64, n, off).tolist()); off += 8 * n
        (cnt,) = struct.unpack_from("<I", data, off); off += 4
        acc = [int.from_bytes(data[off + 32 * k:off + 32 * k + 32], "little") for k in range(cnt)]; off += 32 * cnt
        lst = list(data[off:off + n]); off += n
        lleaf = list(np.frombuffer(data, np.uint64, n, off).tolist()); off += 8 * n
        res.append((st, leaf, acc, lst, lleaf))
    assert off == len(data)
    return res


def check(driver, tmp_path, cases):
    for case, (st, leaf, acc, lst, lleaf) in zip(cases, run(driver, tmp_path, cases)):
        want = model(*case)
        assert (st, leaf, acc) == want, case
        assert (lst, lleaf) == lookup_model(*case), case
    return [model(*c)[0] for c in cases]


def pool_for(rng):
    """a small value range: plain integers, or integers that differ only in a low limb under equal high limbs, or only
    in the top limb -- the 256-bit comparison sees every limb"""
    kind = rng.randrange(4)
    if kind == 0:
        return list(range(1, 13))
    if kind == 1:
        hi = rng.randrange(1, 1 << 60)
        return [(hi << 192) | (k << 3) for k in range(1, 13)]
    if kind == 2:
        return [(k << 192) | 5 for k in range(1, 13)]
    return sorted({rng.randrange(1, P) for _ in range(12)})


def random_case(rng):
    pool = pool_for(rng)
    pm, pr = (0, 0) if rng.random() < 0.7 else (rng.choice([2, 3, 7]), None)
    if pm:
        pr = rng.randrange(pm)
    ok = [v for v in pool if not pm or v % pm == pr]
    stored = [0] + rng.sample(ok, rng.randint(0, len(ok)))
    n = rng.randint(1, 16)
    batch = [0 if rng.random() < 0.08 else rng.choice(pool) for _ in range(n)]
    base = 0 if rng.random() < 0.6 else rng.randrange(1, 1 << 20) << 12
    return stored, batch, pm, pr, base


def test_random_batches_against_the_sequential_model(driver, tmp_path):
    rng = random.Random(0x46494C54)
    cases = [random_case(rng) for _ in range(100_000)]
    statuses = check(driver, tmp_path, cases)
    seen = {s for st in statuses for s in st}
    assert seen == {NEW, ZERO, PRESENT, REPEATED, FOREIGN}


def test_edge_cases(driver, tmp_path):
    S = [0, 10, 20, 30]
    cases = [
        (S, [0, 5, 6], 0, 0, 0),                 # zero first
        (S, [5, 6, 0], 0, 0, 0),                 # zero last
        (S, [10, 5, 6], 0, 0, 0),                # stored first
        (S, [5, 6, 30], 0, 0, 0),                # stored last
        (S, [5, 6, 5], 0, 0, 0),                 # repeat last
        (S, [5, 5, 6], 0, 0, 0),                 # repeat right after the first occurrence
        (S, [0, 10, 20, 30, 0, 10], 0, 0, 0),    # everything rejected
        ([0], [7] * 64, 0, 0, 0),                # all repeats of one value: one accepted
        (S, [20] * 9, 0, 0, 0),                  # all repeats of one stored value: PRESENT at every occurrence
        (S, [20, 15, 15, 20], 0, 0, 1 << 32),    # stored and repeated: PRESENT wins; placed tree
        ([0, 4, 7], [4, 5, 1, 10, 0, 13, 13, 3], 3, 1, 0),   # residues: 5, 3 foreign, 0 is ZERO though 0 % 3 != 1
        ([0, 6], [0, 6, 9, 3, 3, 12, 2], 3, 0, 8),           # residue 0: 0 would pass the partition, still ZERO
        ([0], [P - 1, 1, P - 1], 0, 0, 0),       # the largest canonical value
    ]
    statuses = check(driver, tmp_path, cases)
    assert statuses[0][0] == ZERO and statuses[1][-1] == ZERO
    assert statuses[2][0] == PRESENT and statuses[3][-1] == PRESENT
    assert statuses[4] == [NEW, NEW, REPEATED] and statuses[5] == [NEW, REPEATED, NEW]
    assert NEW not in statuses[6]
    assert statuses[7] == [NEW] + [REPEATED] * 63
    assert statuses[8] == [PRESENT] * 9
    assert statuses[9] == [PRESENT, NEW, REPEATED, PRESENT]
    assert statuses[10] == [PRESENT, FOREIGN, NEW, NEW, ZERO, NEW, REPEATED, FOREIGN]
    assert statuses[11] == [ZERO, PRESENT, NEW, NEW, REPEATED, NEW, FOREIGN]
