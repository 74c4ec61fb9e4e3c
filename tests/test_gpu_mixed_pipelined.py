"""GPU (MI355X): consecutive mixed blocks that overlap -- imt_itree_mixed_pipelined and imt_itree_apply_mixed_pipelined.

The claim under test (include/imt.h): play the same blocks on a twin tree through imt_itree_mixed_batch or
imt_itree_apply_mixed, one at a time with a synchronisation after each; the pipelined call gives the same return code,
*n_inserted, *bad_op and size at return, and after imt_ctx_sync() the same rows in every array of both output structs, the
same root_out and the same tree, byte for byte -- although up to four blocks hash at once on the pipeline streams.

Every test builds its expectation the same way: the blocks through the un-pipelined call on the twin, that result pinned
by the Python walk (test_mixed_logic.walk: low leaves, the first refused position) and by the walk on the sequential oracle
(test_gpu_mixed.oracle_walk: every field of every row, the root); then the blocks on the tree under test with ALL blocks
enqueued before one imt_ctx_sync().  Every buffer a call may write is pre-filled with a sentinel byte; the blocks' values
and op bytes go through one staging buffer that is overwritten the moment each pipelined call returns, which is when the
header says the caller may reuse them.  Every comparison is bit-exact.

  test_chain_across_powers_of_two   eight blocks of 1..5 operations from size 6 past 8 and 16, depths 4 and 32.  Depth 4 has
                                    room for 16 leaves (a capacity cannot exceed 2^depth), so there the eighth block, which
                                    would make it 17, is refused with IMT_ERR_FULL behind seven blocks in flight -- by the
                                    twin as well; at depth 32 the capacity is 64 and all eight are carried out.
  test_single_operations_depth32    twenty blocks of one operation, INSERT and READ alternating
  test_reads_of_an_empty_tree       blocks of READs against the sentinel alone (occupied height 0), an INSERT behind them
  test_random_blocks                six blocks of <= 64 operations from the colliding pool of test_mixed_logic.random_case,
                                    both kernel forms
  test_refused_in_flight            every refusal as block 3 of 5, blocks 1 and 2 in flight
  test_kinds_in_one_sequence        all four pipelined kinds and two un-pipelined ones, no synchronisation inside
  test_behind_flight                view + replay, rewind, proofs, lookup, root_lagged, apply_stats, load_values
  test_counts                       apply_stats, READ-only blocks, a view's builds
  test_arguments                    the refusals that never reach the GPU
  test_python_wrappers, test_follow_mixed_pipelined_example
"""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib
from oracle_lib import P, arr_ints, ints_to_arr
from test_gpu_mixed import INS_FIELDS, RD_FIELDS, SENTINEL, check_rows, cut, oracle_walk
from test_gpu_rewind import forms  # noqa: F401  (the fixture: one context per hash form)
from test_mixed_logic import ADVERSARIAL, INSERT, READ, random_case, walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("mixed", "apply_mixed")
UNSET = 0xDEAD


def sync(c):
    import torch
    c.sync()
    torch.cuda.synchronize()


class Bufs:
    """Everything one block's call may write, in device memory, every byte the sentinel: the nine arrays of
    imt_insert_out and the five of imt_read_out for n operations (level stride n), and 32 bytes for root_out."""

    def __init__(self, depth, n):
        import torch
        self.n, self.depth = n, depth
        rows = max(n, 1)
        shapes = dict(low_index=(rows, 8), low_leaf=(rows, 3, 32), new_leaf=(rows, 3, 32), is_largest=(rows,), old_root=(rows, 32),
                      interim_root=(rows, 32), new_root=(rows, 32), root=(rows, 32), low_sib=(depth, rows, 32),
                      new_sib=(depth, rows, 32))
        mk = lambda shape: torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda")
        self.ins = {k: mk(shapes[k]) for k in INS_FIELDS}
        self.rd = {k: mk(shapes[k]) for k in RD_FIELDS}
        self.root = mk((32,))

    def structs(self, f):
        return (f.InsertOut(**{k: x.data_ptr() for k, x in self.ins.items()}),
                f.ReadOut(**{k: x.data_ptr() for k, x in self.rd.items()}))

    def host(self):
        get = lambda d: {k: (x.cpu().numpy().view(np.uint64).reshape(-1) if k == "low_index" else x.cpu().numpy()) for k, x in d.items()}
        return dict(ins=get(self.ins), rd=get(self.rd), root=self.root.cpu().numpy())


class Stage:
    """The one place the values and op bytes of every block pass through on their way to the GPU"""

    def __init__(self, n_max):
        import torch
        self.v = torch.zeros((n_max, 32), dtype=torch.uint8, device="cuda")
        self.o = torch.zeros((n_max,), dtype=torch.uint8, device="cuda")

    def put(self, script):
        import torch
        n = len(script)
        if n:
            self.v[:n] = torch.from_numpy(ints_to_arr([v for _, v in script]).reshape(n, 32))
            self.o[:n] = torch.from_numpy(np.array([op for op, _ in script], np.uint8))
        return n

    def clobber(self):
        self.v.fill_(0xFF)          # a value >= p in every row,
        self.o.fill_(7)             # an op byte that is neither INSERT nor READ


def issue(imt, t, kind, pipelined, stage, n, bufs, flags=0):
    """One call of `kind` over the n operations staged: (rc, *n_inserted, *bad_op).  kind: mixed / apply_mixed -- the
    calls under test and their un-pipelined twins -- or apply / witness, the insertion-only calls (every op an INSERT)."""
    f, lib = imt._ffi, imt.lib
    n_ins, bad = ctypes.c_uint64(UNSET), ctypes.c_uint64(UNSET)
    pv, po = ctypes.c_void_p(stage.v.data_ptr()), ctypes.c_void_p(stage.o.data_ptr())
    root = ctypes.c_void_p(bufs.root.data_ptr())
    flags |= f.DEVICE_PTRS
    ins, rd = bufs.structs(f)
    if kind == "mixed":
        fn = lib.imt_itree_mixed_pipelined if pipelined else lib.imt_itree_mixed_batch
        rc = fn(t.h, pv, po, n, ctypes.byref(ins), ctypes.byref(rd), ctypes.byref(n_ins), ctypes.byref(bad), flags)
    elif kind == "apply_mixed":
        fn = lib.imt_itree_apply_mixed_pipelined if pipelined else lib.imt_itree_apply_mixed
        rc = fn(t.h, pv, po, n, root, ctypes.byref(n_ins), ctypes.byref(bad), flags)
    elif kind == "apply":
        fn = lib.imt_itree_apply_pipelined if pipelined else lib.imt_itree_apply_batch
        rc = fn(t.h, pv, n, root, flags)
        n_ins.value = n
    else:
        rc = lib.imt_itree_insert_batch(t.h, pv, n, ctypes.byref(ins), flags | (f.PIPELINE if pipelined else 0))
        n_ins.value = n
    return rc, n_ins.value, bad.value


def play(imt, c, t, kinds, pipelined, blocks, depth, stage=None):
    """The blocks on tree t, block j through kinds[j] (or the one kind) -- un-pipelined with a synchronisation after each,
    pipelined with none and the staging buffer overwritten as soon as each call returns.  One record per block: what the
    call returned at return (rc, n_ins, bad, size) and its buffers; the caller synchronises and reads them."""
    sync_each = pipelined is False
    if isinstance(kinds, str):
        kinds = [kinds] * len(blocks)
    if isinstance(pipelined, bool):
        pipelined = [pipelined] * len(blocks)
    stage = stage or Stage(max(len(b) for b in blocks) + 1)
    out = []
    for script, kind, pipe in zip(blocks, kinds, pipelined):
        bufs = Bufs(depth, len(script))
        n = stage.put(script)
        rc, n_ins, bad = issue(imt, t, kind, pipe, stage, n, bufs)
        if pipe:
            stage.clobber()
        if sync_each:
            sync(c)
        out.append(dict(kind=kind, rc=rc, n_ins=n_ins, bad=bad, size=t.size, bufs=bufs))
    return out


def settle(c, results):
    sync(c)
    for r in results:
        r["host"] = r["bufs"].host()
    return results


def untouched(h):
    return all((a.view(np.uint8) == SENTINEL).all() for a in list(h["ins"].values()) + list(h["rd"].values()) + [h["root"]])


def same_results(imt, got, want, tag=""):
    """the pipelined blocks against the twin's, block by block: at return, and every byte of every buffer"""
    E = imt._ffi.ERR
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        t = f"{tag} block {j} ({g['kind']})"
        assert g["rc"] == w["rc"] and g["size"] == w["size"], (t, g["rc"], w["rc"], g["size"], w["size"])
        assert g["n_ins"] == w["n_ins"] and g["bad"] == w["bad"], t
        assert (g["n_ins"] == UNSET) == (g["rc"] != 0) and (g["bad"] == UNSET) == (g["rc"] != E["VALUE"]), t
        if g["rc"]:
            assert untouched(g["host"]), f"{t}: a refused call wrote to the caller's buffers"
        for part in ("ins", "rd"):
            for k, a in g["host"][part].items():
                assert (a == w["host"][part][k]).all(), f"{t}: {part}.{k}"
        assert (g["host"]["root"] == w["host"]["root"]).all(), f"{t}: root_out"


def pin(imt, orc, depth, cap, stored, blocks, results, tag=""):
    """The twin's results against the two walks, block by block: a refused block by its code and position, a carried-out
    one by every field of every row (nothing beyond row n_ins / n - n_ins written) or by its root.  Returns the values
    stored afterwards."""
    E = imt._ffi.ERR
    stored = list(stored)
    for j, (script, r) in enumerate(zip(blocks, results)):
        t = f"{tag} twin block {j} ({r['kind']})"
        n, h = len(script), r["host"]
        rows, bad = walk([0] + stored, script)
        k = sum(op == INSERT for op, _ in script)
        if r["rc"]:
            assert untouched(h), t
            if r["rc"] == E["VALUE"]:
                assert bad == r["bad"] >= 0, (t, bad, r["bad"])
            elif r["rc"] == E["FULL"]:
                assert bad < 0 and 1 + len(stored) + k > cap, t
            else:
                assert r["rc"] in (E["ARG"], E["NONCANONICAL"]), (t, r["rc"])
            assert r["size"] == 1 + len(stored), t
            continue
        assert bad < 0 and r["n_ins"] == k and r["size"] == 1 + len(stored) + k, t
        want_ins, want_rd, (root, _) = oracle_walk(orc, depth, cap, stored, script)
        if r["kind"] in ("mixed", "witness"):
            ins, rd = cut(h["ins"], k, max(n, 1), False), cut(h["rd"], n - k, max(n, 1), False)
            check_rows(ins, rd, want_ins, want_rd, False, t)
            lows = {INSERT: iter(ins["low_index"]), READ: iter(rd["low_index"])}
            for p, (op, _) in enumerate(script):
                assert int(next(lows[op])) == rows[p][0], f"{t}: low leaf of operation {p}"
            assert (h["root"] == SENTINEL).all(), t
        else:
            assert arr_ints(h["root"]) == [root], t
            assert untouched(dict(h, root=np.full(32, SENTINEL, np.uint8))), t
        stored += [v for op, v in script if op == INSERT]
    return stored


def same_tree(a, b, tag=""):
    """index, leaf preimages, every stored node on a path, root"""
    assert a.size == b.size and a.root() == b.root(), tag
    assert (a.snapshot() == b.snapshot()).all(), tag
    idx = np.arange(a.size, dtype=np.uint64)
    assert (a.get_proof_batch(idx) == b.get_proof_batch(idx)).all(), tag
    probe = ints_to_arr([1, 2, 3, P - 1] + arr_ints(a.snapshot()[:, 0])[1:9])
    for x, y in zip(a.lookup(probe), b.lookup(probe)):
        assert (x == y).all(), tag
    for x, y in zip(a.non_membership_witness(probe[:4]), b.non_membership_witness(probe[:4])):
        assert (x == y).all(), tag


def lagged(imt, t, lag):
    buf = np.zeros(32, np.uint8)
    rc = imt.lib.imt_itree_root_lagged(t.h, lag, buf.ctypes.data_as(ctypes.c_void_p), 0)
    return rc, arr_ints(buf)[0]


def twins(imt, c, depth, cap, stored):
    a, b = imt.IndexedTree(c, depth, cap), imt.IndexedTree(c, depth, cap)
    if stored:
        for t in (a, b):
            t.apply_batch(stored)
    sync(c)
    return a, b


def run_and_compare(imt, c, orc, depth, cap, stored, blocks, call, tag=""):
    """the common body: twin, pins, every block enqueued before one synchronisation, comparison of results and trees"""
    t, twin = twins(imt, c, depth, cap, stored)
    try:
        want = settle(c, play(imt, c, twin, call, False, blocks, depth))
        pin(imt, orc, depth, cap, stored, blocks, want, tag)
        got = settle(c, play(imt, c, t, call, True, blocks, depth))
        same_results(imt, got, want, tag)
        same_tree(t, twin, tag)
        for lag in (0, 1):
            assert lagged(imt, t, lag) == lagged(imt, twin, lag), f"{tag}: root_lagged({lag})"
        return got
    finally:
        sync(c)
        t.close()
        twin.close()


# ---------------------------------------------------------------- 1. eight small blocks past two powers of two
CHAIN_SEED = [10, 20, 30, 40, 50]                         # size 6
CHAIN = [
    [(READ, 100), (INSERT, 100)],                                               # a READ of a value its own block inserts later
    [(READ, 150), (INSERT, 200)],                                               # a READ whose low leaf the block before put in
    [(INSERT, 300)],                                                            # INSERTs only; size 9: past 8
    [(READ, 350), (READ, 250), (READ, 350)],                                    # READs only, between two inserting blocks
    [(INSERT, 400), (READ, 450), (INSERT, 500), (READ, 600), (INSERT, 600)],
    [(INSERT, 700), (READ, 650), (INSERT, 800)],
    [(READ, 850), (INSERT, 900), (INSERT, 1000), (READ, 950)],                  # size 16
    [(INSERT, 1100), (READ, 1050)],                                             # size 17: past 16
]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("depth", [4, 32])
def test_chain_across_powers_of_two(imt, forms, oracle, depth, call):
    assert [sum(op == INSERT for op, _ in b) for b in CHAIN] == [1, 1, 1, 0, 3, 2, 2, 1]
    assert all(1 <= len(b) <= 5 for b in CHAIN) and len(CHAIN) > 4
    flat = [v for b in CHAIN for _, v in b if _ == INSERT]
    assert flat == sorted(flat) and flat[0] > max(CHAIN_SEED)       # ascending: the low leaf is the block before's last leaf
    cap = min(64, 1 << depth)
    got = run_and_compare(imt, forms["default"], oracle, depth, cap, CHAIN_SEED, CHAIN, call, f"chain depth {depth} {call}")
    sizes = [r["size"] for r in got]
    if depth == 4:
        assert sizes == [7, 8, 9, 9, 12, 14, 16, 16] and got[-1]["rc"] == imt._ffi.ERR["FULL"]
    else:
        assert sizes == [7, 8, 9, 9, 12, 14, 16, 17] and all(r["rc"] == 0 for r in got)


# ---------------------------------------------------------------- 2. one operation per block
@pytest.mark.parametrize("call", CALLS)
def test_single_operations_depth32(imt, forms, oracle, call):
    vals = [v for v in oracle_lib.synth_values(40, 0x4D505001) if 0 < v < P]
    blocks = [[(INSERT if j % 2 == 0 else READ, vals[j])] for j in range(20)]
    got = run_and_compare(imt, forms["default"], oracle, 32, 64, [], blocks, call, f"single {call}")
    assert [r["size"] for r in got] == [2 + j // 2 for j in range(20)]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("depth", [4, 32])
def test_reads_of_an_empty_tree(imt, forms, oracle, depth, call):
    blocks = [[(READ, 5)], [(READ, 7), (READ, 5)], [(INSERT, 5)], [(READ, 7)], [(READ, 3), (INSERT, 7)]]
    got = run_and_compare(imt, forms["default"], oracle, depth, 16, [], blocks, call, f"empty tree depth {depth} {call}")
    assert [r["size"] for r in got] == [1, 1, 2, 2, 3]


# ---------------------------------------------------------------- 3. random blocks, both kernel forms
def random_chain(seed):
    """(stored, six clean blocks): each block a clean script of random_case over its own small colliding pool, block k's
    value v mapped to 8 v + k -- the blocks stay clean against each other, and their values interleave in value order,
    so the neighbours of a block's operations are mostly leaves of the blocks still in flight"""
    rng = random.Random(seed)
    stored, blocks = None, []
    while len(blocks) < 6:
        st, script = random_case(rng, wide=False)
        if walk(st, script)[1] >= 0:
            continue
        k = len(blocks) + 1
        if stored is None:
            stored = [8 * v + k for v in st[1:]]
        blocks.append([(op, 8 * v + k) for op, v in script])
    return stored, blocks


_RANDOM = {}


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("form", ["thread", "quad"])
@pytest.mark.parametrize("seed", [0x4D50A1, 0x4D50A2, 0x4D50A3])
def test_random_blocks(imt, forms, oracle, seed, form, call):
    c, depth, cap = forms[form], 32, 512
    stored, blocks = random_chain(seed)
    assert len(stored) <= 32 and all(1 <= len(b) <= 64 for b in blocks)
    t = imt.IndexedTree(c, depth, cap)
    try:
        if stored:
            t.apply_batch(stored)
        if (seed, call) not in _RANDOM:                         # the expectation once per script, whichever form comes first
            twin = imt.IndexedTree(c, depth, cap)
            try:
                if stored:
                    twin.apply_batch(stored)
                want = settle(c, play(imt, c, twin, call, False, blocks, depth))
                pin(imt, oracle, depth, cap, stored, blocks, want, f"random {seed:#x} {call}")
                idx = np.arange(twin.size, dtype=np.uint64)
                for r in want:
                    del r["bufs"]
                _RANDOM[seed, call] = (want, twin.size, twin.root(), twin.snapshot().tobytes(), twin.get_proof_batch(idx).tobytes())
            finally:
                twin.close()
        want, size, root, snap, proofs = _RANDOM[seed, call]
        got = settle(c, play(imt, c, t, call, True, blocks, depth))
        same_results(imt, got, want, f"random {seed:#x} {form} {call}")
        assert (t.size, t.root(), t.snapshot().tobytes()) == (size, root, snap)
        assert t.get_proof_batch(np.arange(size, dtype=np.uint64)).tobytes() == proofs
    finally:
        sync(c)
        t.close()


# ---------------------------------------------------------------- 4. a refused block with blocks in flight
FAR = [(3 << 100) + 7 * k for k in range(1, 40)]            # values none of the adversarial scripts uses
AROUND = [
    [(INSERT, FAR[0]), (READ, FAR[1]), (INSERT, FAR[2]), (INSERT, FAR[3])],     # block 1
    [(READ, FAR[4]), (INSERT, FAR[1]), (INSERT, FAR[5]), (READ, FAR[6])],       # block 2
    None,                                                                      # block 3: the refused one
    [(INSERT, FAR[7]), (READ, FAR[4]), (INSERT, FAR[8])],                       # block 4
    [(READ, FAR[9]), (READ, FAR[4])],                                           # block 5
]
REFUSING = {k: v for k, v in ADVERSARIAL.items() if walk(*v)[1] >= 0}
REFUSED_CASES = list(REFUSING) + ["overflows the capacity", "a bad op byte", "a value >= p"]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("name", REFUSED_CASES)
def test_refused_in_flight(imt, forms, oracle, name, call):
    E = imt._ffi.ERR
    assert len(REFUSING) >= 6
    depth, cap, stored = 32, 64, [10, 20]
    if name in REFUSING:
        stored, bad_block = REFUSING[name][0][1:], REFUSING[name][1]
        code = E["VALUE"]
    elif name == "overflows the capacity":
        cap, bad_block, code = 16, [(INSERT if k % 5 else READ, FAR[20 + k]) for k in range(12)], E["FULL"]     # 3 + 5 + 9 > 16
    elif name == "a bad op byte":
        bad_block, code = [(INSERT, FAR[20]), (2, FAR[21]), (READ, FAR[22])], E["ARG"]
    else:
        bad_block, code = [(INSERT, FAR[20]), (READ, P), (INSERT, P + 5)], E["NONCANONICAL"]
    blocks = [b if b is not None else bad_block for b in AROUND]
    got = run_and_compare(imt, forms["default"], oracle, depth, cap, stored, blocks, call, f"refused: {name} {call}")
    assert [r["rc"] for r in got] == [0, 0, code, 0, 0]
    assert got[2]["size"] == got[1]["size"] and untouched(got[2]["host"])
    if code == E["VALUE"]:
        assert got[2]["bad"] == walk(*REFUSING[name])[1]


# ---------------------------------------------------------------- 5. every kind behind every other
def test_kinds_in_one_sequence(imt, forms, oracle):
    c, depth, cap = forms["default"], 32, 512
    vals = [v for v in oracle_lib.synth_values(400, 0x4D505005) if 0 < v < P]
    stored, pool = vals[:21], iter(vals[21:])
    mixed_block = lambda n: [(READ if i % 4 == 3 else INSERT, next(pool)) for i in range(n)]
    plain_block = lambda n: [(INSERT, next(pool)) for _ in range(n)]
    seq = [("mixed", True, mixed_block(70)), ("apply", True, plain_block(33)), ("apply_mixed", True, mixed_block(41)),
           ("witness", True, plain_block(17)), ("mixed", False, mixed_block(35)), ("apply", False, plain_block(9)),
           ("mixed", True, mixed_block(66))]
    kinds, pipes, blocks = [k for k, _, _ in seq], [p for _, p, _ in seq], [b for _, _, b in seq]
    t, twin = twins(imt, c, depth, cap, stored)
    try:
        want = settle(c, play(imt, c, twin, kinds, False, blocks, depth))
        pin(imt, oracle, depth, cap, stored, blocks, want, "kinds")
        got = settle(c, play(imt, c, t, kinds, pipes, blocks, depth))       # no synchronisation inside
        same_results(imt, got, want, "kinds")
        same_tree(t, twin, "kinds")
        assert t.apply_stats().tolist() == twin.apply_stats().tolist()
        for lag in (0, 1):
            assert lagged(imt, t, lag) == lagged(imt, twin, lag)
    finally:
        sync(c)
        t.close()
        twin.close()


# ---------------------------------------------------------------- 6. other calls right behind blocks in flight
def flight_blocks():
    vals = [v for v in oracle_lib.synth_values(200, 0x4D505006) if 0 < v < P]
    stored, pool = vals[:20], iter(vals[20:])
    block = lambda n: [(READ if i % 4 == 1 else INSERT, next(pool)) for i in range(n)]
    reads = lambda n: [(READ, next(pool)) for _ in range(n)]
    return stored, [block(24), block(9), reads(5), block(31), reads(3)]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("what", ["view", "rewind", "proofs", "lookup", "root_lagged", "apply_stats", "load_values"])
def test_behind_flight(imt, forms, oracle, what, call):
    c, depth, cap = forms["default"], 32, 256
    stored, blocks = flight_blocks()
    t, twin = twins(imt, c, depth, cap, stored)
    rows_twin = imt.IndexedTree(c, depth, cap)          # the witness rows of every block, whichever call is under test
    try:
        rows_twin.apply_batch(stored)
        want = settle(c, play(imt, c, twin, call, False, blocks, depth))
        after = pin(imt, oracle, depth, cap, stored, blocks, want, f"behind {what} {call}")
        rows = settle(c, play(imt, c, rows_twin, "mixed", False, blocks, depth))
        if call == "apply_mixed":
            pin(imt, oracle, depth, cap, stored, blocks, rows, f"behind {what} rows")
        roots, r = [], imt.IndexedTree(c, depth, cap)    # the root after every block
        try:
            r.apply_batch(stored)
            for b in blocks:
                ins = [v for op, v in b if op == INSERT]
                roots.append(r.apply_batch(ins) if ins else r.root())
        finally:
            r.close()
        sync(c)
        # ---- all five blocks in flight, then the call in question with nothing waited for ----
        got = play(imt, c, t, call, True, blocks, depth)
        size3 = want[2]["size"]                          # before block 3 (blocks count from 0)
        if what == "view":
            v = t.view(size3)
            try:
                ins, rd = v.mixed_witness([x for _, x in blocks[3]], [op for op, _ in blocks[3]])
                h, n, k = rows[3]["host"], len(blocks[3]), rows[3]["n_ins"]
                for key, a in cut(h["ins"], k, n, False).items():
                    assert (ins[key] == a).all(), f"replayed ins.{key}"
                for key, a in cut(h["rd"], n - k, n, False).items():
                    assert (rd[key] == a).all(), f"replayed rd.{key}"
                assert v.root() == roots[2]
            finally:
                v.close()
        elif what == "rewind":
            assert t.rewind(size3) == roots[2] and t.size == size3
            again = play(imt, c, t, call, True, blocks[3:], depth)
            settle(c, again)
            same_results(imt, again, want[3:], "after the rewind")
            assert t.root() == roots[-1]
        elif what == "proofs":
            idx = np.arange(twin.size, dtype=np.uint64)
            assert (t.get_proof_batch(idx) == twin.get_proof_batch(idx)).all()
            assert (t.get_leaves(idx) == twin.get_leaves(idx)).all()
        elif what == "lookup":
            probe = ints_to_arr(after[5:25] + [x for _, x in blocks[4]] + [0])
            for x, y in zip(t.lookup(probe), twin.lookup(probe)):
                assert (x == y).all()
        elif what == "root_lagged":
            assert lagged(imt, twin, 0) == (0, roots[3]) and lagged(imt, twin, 1) == (0, roots[1])     # READs only: not counted
            for lag in (0, 1):
                assert lagged(imt, t, lag) == lagged(imt, twin, lag), f"root_lagged({lag})"
        elif what == "apply_stats":
            assert t.apply_stats().tolist() == twin.apply_stats().tolist()
        else:
            for x in (t, twin):
                x.load_values(ints_to_arr(after[:30]))
            assert t.size == 31 and t.root() == twin.root()
        settle(c, got)
        same_results(imt, got, want, f"behind {what} {call}")
        same_tree(t, twin, f"behind {what} {call}")
    finally:
        sync(c)
        for x in (t, twin, rows_twin):
            x.close()


# ---------------------------------------------------------------- 7. counts
def test_counts(imt, forms):
    c, depth, cap = forms["default"], 32, 512
    vals = [v for v in oracle_lib.synth_values(300, 0x4D505007) if 0 < v < P]
    stored, pool = vals[:40], iter(vals[40:])
    blocks = [[(READ if i % 3 == 1 else INSERT, next(pool)) for i in range(n)] for n in (50, 7, 64)]
    reads = [(READ, next(pool)) for _ in range(6)]
    t, twin = twins(imt, c, depth, cap, stored)
    stage = Stage(65)
    view = t.view(11)
    try:
        view_root, builds = view.root(), view.stats()[1]
        for b in blocks:
            n = stage.put(b)
            rc, n_ins, _ = issue(imt, t, "apply_mixed", True, stage, n, Bufs(depth, n))
            ins = [v for op, v in b if op == INSERT]
            assert rc == 0 and n_ins == len(ins)
            twin.apply_batch(ins)
            assert t.apply_stats().tolist() == twin.apply_stats().tolist()      # that call's own counts, the call alone waited for
        assert view.root() == view_root and view.stats()[1] == builds + 1       # the tree has changed: rebuilt once
        stats, size, root, builds = t.apply_stats().tolist(), t.size, t.root(), view.stats()[1]
        for kind in CALLS:                                                       # a block of READs adds nothing
            n = stage.put(reads)
            bufs = Bufs(depth, n)
            rc, n_ins, _ = issue(imt, t, kind, True, stage, n, bufs)
            assert rc == 0 and n_ins == 0 and t.size == size
            assert t.apply_stats().tolist() == stats
            assert view.root() == view_root and view.stats()[1] == builds       # no change of the tree: the view stays fresh
            sync(c)
            h = bufs.host()
            if kind == "mixed":
                assert arr_ints(h["rd"]["root"]) == [root] * n and untouched(dict(h, rd={}))
            else:
                assert arr_ints(h["root"]) == [root]
        same_tree(t, twin)
    finally:
        sync(c)
        view.close()
        t.close()
        twin.close()


# ---------------------------------------------------------------- 8. arguments
@pytest.mark.parametrize("call", CALLS)
def test_arguments(imt, forms, call):
    import torch
    c, f, lib, E = forms["default"], imt._ffi, imt.lib, imt._ffi.ERR
    depth, cap = 8, 64
    t = imt.IndexedTree(c, depth, cap)
    stage = Stage(8)
    script = [(INSERT, 5), (READ, 7), (INSERT, 9)]
    try:
        t.apply_batch([100, 200])
        before = (t.size, t.root(), t.snapshot().tobytes())

        def refused(fl, tree=t, code=E["ARG"], vals=True, ops=True, shift=None, look=True):
            n, bufs = stage.put(script), Bufs(depth, 3)
            ins, rd = bufs.structs(f)
            if isinstance(shift, tuple):
                which = ins if shift[0] == "ins" else rd
                setattr(which, shift[1], getattr(which, shift[1]) + shift[2])
            n_ins, bad = ctypes.c_uint64(UNSET), ctypes.c_uint64(UNSET)
            pv = ctypes.c_void_p(stage.v.data_ptr() + (8 if vals == "misaligned" else 0)) if vals else None
            po = ctypes.c_void_p(stage.o.data_ptr()) if ops else None
            root = bufs.root.data_ptr() + (4 if shift == "root" else 0)
            if call == "mixed":
                rc = lib.imt_itree_mixed_pipelined(tree.h if tree else None, pv, po, n, ctypes.byref(ins), ctypes.byref(rd),
                                                   ctypes.byref(n_ins), ctypes.byref(bad), fl)
            else:
                rc = lib.imt_itree_apply_mixed_pipelined(tree.h if tree else None, pv, po, n, ctypes.c_void_p(root),
                                                         ctypes.byref(n_ins), ctypes.byref(bad), fl)
            sync(c)
            assert rc == code, (rc, lib.imt_last_error(c.h))
            assert untouched(bufs.host()) and n_ins.value == bad.value == UNSET
            if tree is t and look:
                assert (t.size, t.root(), t.snapshot().tobytes()) == before

        D = f.DEVICE_PTRS
        refused(0)                                              # IMT_DEVICE_PTRS is required
        refused(f.PIPELINE)
        refused(D | f.HOST_PREP)
        refused(D | f.INPUTS_READY)
        refused(D | 3)                                          # unknown format
        refused(D, tree=None)
        refused(D, vals=False)
        refused(D, ops=False)
        refused(D, vals="misaligned")
        if call == "mixed":
            refused(D, shift=("ins", "low_index", 4))
            refused(D, shift=("rd", "root", 8))
            refused(D, shift=("ins", "new_sib", 8))
        else:
            refused(D, shift="root")
        placed = imt.IndexedTree(c, 8, 64)
        placed.set_placement(10, 1)
        refused(D, tree=placed)
        placed.close()
        part = imt.IndexedTree(c, depth, cap)
        c._check(lib.imt_itree_set_value_partition(part.h, 3, 1))
        refused(D, tree=part)
        part.close()
        # between imt_itree_batch_begin and _end; an open slice
        ev, l0 = ctypes.c_uint32(), ctypes.c_uint32()
        more = ints_to_arr([71, 72, 73, 74])
        assert lib.imt_itree_batch_begin(t.h, more.ctypes.data_as(ctypes.c_void_p), 4, 0, ctypes.byref(ev), ctypes.byref(l0)) == 0
        refused(D)
        assert lib.imt_itree_batch_abort(t.h) == 0
        dv8 = torch.from_numpy(ints_to_arr([81, 82, 83, 84, 85, 86, 87, 88])).cuda()
        pay = torch.zeros(int(lib.imt_itree_slice_payload_bytes(8)) + 64, dtype=torch.uint8, device="cuda")
        sl = ctypes.c_int(-1)
        assert lib.imt_itree_slice_prepare(t.h, ctypes.c_void_p(dv8.data_ptr()), 0, 8, 0, None, D, ctypes.byref(sl), None) == 0
        refused(D, look=False)                                  # the slice owns the tree until its last unit
        for q in range(depth + 1):
            assert lib.imt_itree_slice_unit(t.h, sl.value, q, ctypes.c_void_p(pay.data_ptr()), None) == 0
        sync(c)
        assert t.size == before[0] + 8
        # n == 0: IMT_OK, *n_inserted = 0, the current root behind everything in flight; IMT_PIPELINE means nothing more
        n, bufs = stage.put(script), Bufs(depth, 3)
        rc, n_ins, _ = issue(imt, t, call, True, stage, n, bufs, f.PIPELINE)
        assert rc == 0 and n_ins == 2 and t.size == before[0] + 10
        empty = Bufs(depth, 0)
        rc, n_ins, bad = issue(imt, t, call, True, stage, 0, empty)
        assert rc == 0 and n_ins == 0 and bad == UNSET
        sync(c)
        h = empty.host()
        if call == "apply_mixed":
            assert arr_ints(h["root"]) == [t.root()] == arr_ints(bufs.host()["root"])
            assert untouched(dict(h, root=np.full(32, SENTINEL, np.uint8)))
        else:
            assert untouched(h)
        # the un-pipelined calls still refuse the flag
        n = stage.put([(INSERT, 11), (READ, 12)])
        un = Bufs(depth, n)
        assert issue(imt, t, call, False, stage, n, un, f.PIPELINE)[0] == E["ARG"] and t.size == before[0] + 10
        sync(c)
        assert untouched(un.host())
    finally:
        sync(c)
        t.close()


# ---------------------------------------------------------------- 9. the wrappers and the example
def test_python_wrappers(imt, forms, oracle):
    import torch
    c, depth, cap = forms["default"], 32, 64
    stored = [10, 20]
    blocks = [[(INSERT, 5), (READ, 15), (INSERT, 15)], [(READ, 7), (READ, 30)], [(INSERT, 30), (READ, 7)]]
    t, twin = twins(imt, c, depth, cap, stored)
    a = imt.IndexedTree(c, depth, cap)
    stage = Stage(4)
    try:
        a.apply_batch(stored)
        bufs, roots, counts = [], torch.full((3, 32), SENTINEL, dtype=torch.uint8, device="cuda"), []
        for j, b in enumerate(blocks):
            n = stage.put(b)
            bufs.append(Bufs(depth, n))
            k = t.mixed_pipelined(stage.v.data_ptr(), stage.o.data_ptr(), n, ins={k: x.data_ptr() for k, x in bufs[j].ins.items()},
                                  rd={k: x.data_ptr() for k, x in bufs[j].rd.items()})
            assert k == a.apply_mixed_pipelined(stage.v.data_ptr(), stage.o.data_ptr(), n, roots[j].data_ptr())
            counts.append(k)
            stage.clobber()
        sync(c)
        assert counts == [2, 0, 1] and t.size == a.size == 6
        want_roots = []
        for j, b in enumerate(blocks):
            ins, rd = twin.mixed_batch([v for _, v in b], [op for op, _ in b])
            h, n = bufs[j].host(), len(b)
            for key, x in cut(h["ins"], counts[j], n, False).items():
                assert (x == ins[key]).all(), (j, key)
            for key, x in cut(h["rd"], n - counts[j], n, False).items():
                assert (x == rd[key]).all(), (j, key)
            want_roots.append(twin.root())
        assert arr_ints(roots.cpu().numpy()) == want_roots
        same_tree(t, twin)
        same_tree(a, twin)
        # a refused value raises with the position; only ins / rd given, or neither
        n = stage.put([(INSERT, 40), (READ, 5)])
        for call in (lambda: t.mixed_pipelined(stage.v.data_ptr(), stage.o.data_ptr(), n),
                     lambda: a.apply_mixed_pipelined(stage.v.data_ptr(), stage.o.data_ptr(), n)):
            with pytest.raises(ValueError) as e:
                call()
            assert e.value.bad_op == 1
        assert t.size == a.size == 6
        n = stage.put([(INSERT, 40), (READ, 41)])
        only = Bufs(depth, n)
        assert t.mixed_pipelined(stage.v.data_ptr(), stage.o.data_ptr(), n, rd=dict(root=only.rd["root"].data_ptr())) == 1
        assert a.apply_mixed_pipelined(stage.v.data_ptr(), stage.o.data_ptr(), n) == 1
        sync(c)
        assert a.root() == t.root() and arr_ints(only.host()["rd"]["root"][:1]) == [t.root()]
    finally:
        sync(c)
        for x in (t, twin, a):
            x.close()


def test_follow_mixed_pipelined_example(imt, oracle):
    """examples/follow_mixed_pipelined.c enqueues ten blocks of INSERTs and READs, then prints each block's root beside
    the one its second tree announced; given the oracle's last root as its argument it compares and fails on a difference."""
    exe = os.path.join(ROOT, "examples", "follow_mixed_pipelined")
    csrc = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "follow_mixed_pipelined.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the example's INSERTs: transaction i of block j, i % 4 != 1, block 6 none -> 1 + 7919023757 (64 j + i + 1) mod (2^61 - 1)
    depth, h = 32, oracle.sparse_new(32, 1024)
    roots, total = [], 0
    for j in range(10):
        for i in range(64):
            if j != 6 and i % 4 != 1:
                assert oracle.sparse_insert(h, depth, 1 + 7919023757 * (64 * j + i + 1) % ((1 << 61) - 1))["rc"] == 0
                total += 1
        roots.append(oracle.sparse_root(h))
    oracle.sparse_free(h)
    assert roots[6] == roots[5]
    r = subprocess.run([exe, f"{roots[-1]:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{total} insertions in 10 blocks" in r.stdout
    for j, want in enumerate(roots):
        assert f"block {j}: root {want:064x} as announced" in r.stdout, r.stdout
    assert "final root equals the expected one" in r.stdout
    r = subprocess.run([exe, f"{roots[-2]:064x}"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "DIFFERS" in r.stdout
