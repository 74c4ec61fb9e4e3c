"""CPU: the per-item code of the gadget kernels (csrc/imt_gadget_device.hpp, host build: tests/native/emul_gadget.cpp) at
EVERY lookup width 1..28, bit for bit against oracle/gadget.c and the Python model (oracle_lib.less_than_rows_model,
insert_gadget_rows_model).

The width decides everything the limb code does: k = ceil(128 / lb) limbs + 1, padded = k lb between 128 and 140, which
limbs straddle a 32-bit word, how far above bit 128 the top limb sits.  Per width: the operand pairs of
gadget_corpus.less_than_pairs (edges, random, shared high limb, every limb boundary of both halves), whose coverage is
asserted from the model's rows; is_equal differences that make the binary Euclid of inv_mod run long; real insertions
and their rejected variants at depths 1, 3, 32 and 64; the column rebuilt from the product's layout with every vertical
gate holding; the lookup rows; and the same comparisons as a program under AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gadget_corpus as gc
import oracle_lib
from oracle_lib import P, arr_ints, ints_to_arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "emul_gadget.cpp")
DEPS = [SRC, os.path.join(CSRC, "imt_gadget_device.hpp")]
FLAGS = ["-std=c++17", "-I", CSRC]
DEEP_WIDTHS = (1, 2, 7, 17, 18, 27, 28)
M128 = gc.M128


def _run(cmd):
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stdout}\n{r.stderr}"
    return r.stdout


@pytest.fixture(scope="module")
def emul_g():
    """Host build of the kernels' per-item code (tests/native/emul_gadget.cpp), a shared object of its own."""
    so = os.path.join(NATIVE, "libemul_gadget.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
        _run(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", so, SRC])
    return ctypes.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_less_than(lib, pairs, lb, item_major=False):
    """(rows uint8 [rows, n, 32], lt uint8 [n]) of the host build, in a buffer with sentinel rows on both sides"""
    n, rows = len(pairs), gc.less_than_rows(lb)
    a, b = ints_to_arr([p[0] for p in pairs]), ints_to_arr([p[1] for p in pairs])
    buf = np.full((2 + rows * n + 2, 32), 0xA5, np.uint8)
    lt = np.full(n + 2, 0xA5, np.uint8)
    rs, its = (32, rows * 32) if item_major else (n * 32, 32)
    assert lib.emul_gadget_less_than(_ptr(a), _ptr(b), ctypes.c_size_t(n), lb, ctypes.c_void_p(buf.ctypes.data + 64),
                                     ctypes.c_uint64(rs), ctypes.c_uint64(its), _ptr(lt)) == 0
    assert (buf[:2] == 0xA5).all() and (buf[-2:] == 0xA5).all() and (lt[n:] == 0xA5).all(), "wrote outside [rows][n]"
    body = buf[2:-2]
    return (body.reshape(n, rows, 32).transpose(1, 0, 2) if item_major else body.reshape(rows, n, 32)), lt[:n]


def host_insert(lib, items, lb, whole=True, item_major=False):
    """glue rows uint8 [rows, n, 32] of the host build for insert_leaf (whole) or verify_non_inclusion alone"""
    orc = oracle_lib.load()
    n, depth = len(items), items[0]["depth"]
    orc.lib.orc_insert_gadget_rows.restype = orc.lib.orc_non_inclusion_gadget_rows.restype = ctypes.c_size_t
    rows = (orc.lib.orc_insert_gadget_rows if whole else orc.lib.orc_non_inclusion_gadget_rows)(ctypes.c_size_t(depth), ctypes.c_uint(lb))
    s = gc.stacked(items)
    new = s["new_leaf"] if whole else np.ascontiguousarray(s["new_leaf"][:, 0]) if "new_leaf" in s else s["new_val"]
    pairs = gc.chain_pairs(items, whole)
    buf = np.full((2 + rows * n + 2, 32), 0xA5, np.uint8)
    rs, its = (32, rows * 32) if item_major else (n * 32, 32)
    assert lib.emul_gadget_insert(_ptr(s["low_leaf"]), _ptr(s["low_index"]), _ptr(new), _ptr(s["new_path_index"]) if whole else None,
                                  _ptr(s["is_largest"]), _ptr(pairs), depth, lb, ctypes.c_size_t(n), 1 if whole else 0,
                                  ctypes.c_void_p(buf.ctypes.data + 64), ctypes.c_uint64(rs), ctypes.c_uint64(its)) == 0
    assert (buf[:2] == 0xA5).all() and (buf[-2:] == 0xA5).all(), "wrote outside [rows][n]"
    body = buf[2:-2]
    return body.reshape(n, rows, 32).transpose(1, 0, 2) if item_major else body.reshape(rows, n, 32)


# ---------------------------------------------------------------- is_less_than
@pytest.mark.parametrize("lb", gc.WIDTHS)
def test_less_than_rows_host_build_oracle_and_model_agree(emul_g, oracle, lb):
    pairs = gc.less_than_pairs(lb)
    got, lt = host_less_than(emul_g, pairs, lb)
    got_im, lt_im = host_less_than(emul_g, pairs, lb, item_major=True)
    assert (got == got_im).all() and (lt == lt_im).all()
    k, padded, L = gc.limbs_of(lb)
    assert got.shape[0] == 4 * (-(-128 // lb) + 1) + 27 and 128 <= padded < 128 + lb and L == k + 1
    for i, (a, b) in enumerate(pairs):
        t = oracle.less_than_trace(a, b, lb)
        model, out = oracle_lib.less_than_rows_model(a, b, lb)
        host = arr_ints(got[:, i])
        assert len(host) == len(model) == len(t["witness"]) == got.shape[0]
        assert host == model, (lb, a, b, [r for r in range(len(host)) if host[r] != model[r]][:4])
        assert (got[:, i] == t["witness"]).all(), (lb, a, b)
        assert int(lt[i]) == out == host[t["out_row"]] == (1 if a < b else 0)


@pytest.mark.parametrize("lb", gc.WIDTHS)
def test_the_operand_pairs_cover_every_outcome_limb_value_and_word_boundary(lb):
    """from the model's rows alone: a later edit of the corpus cannot thin it out silently"""
    seen = gc.coverage(lb, gc.less_than_pairs(lb))
    for call in ("msb_lt", "msb_eq", "lsb_lt", "lsb_eq"):
        assert seen[call] == {0, 1}, (lb, call)
    assert seen["out"] == {0, 1}
    assert seen["top_zero"] == [{False, True}, {False, True}]
    assert seen["inner_ones"] and seen["inner_zero"]
    if 32 % lb:
        assert seen["straddle"], lb
    else:
        assert not any((i * lb) // 32 != (i * lb + lb - 1) // 32 for i in range(gc.limbs_of(lb)[2]))


# ---------------------------------------------------------------- is_equal: the inverse
def test_is_equal_inverses_at_the_differences_that_stress_the_euclid_loop(emul_g):
    """inv_mod is a binary extended Euclid with a guard of 1100 rounds: powers of two (the longest halving runs), their
    negatives, the ends of the field and (p - 1) / 2.  Each inverse is pow(d, p - 2, p)."""
    ds = [1, 2, P - 1, P - 2, (P - 1) // 2] + [1 << k for k in range(254)] + [P - (1 << k) for k in range(254)]
    assert all(0 < d < P for d in ds)
    rng_b = [0, 1, P - 1, 12345678901234567890]
    for b in rng_b:
        a = ints_to_arr([(d + b) % P for d in ds])
        bb = ints_to_arr([b] * len(ds))
        rows = np.full((len(ds) * 4 + 1, 32), 0xA5, np.uint8)
        emul_g.emul_gadget_is_equal(_ptr(a), _ptr(bb), ctypes.c_size_t(len(ds)), _ptr(rows))
        assert (rows[-1] == 0xA5).all()
        got = arr_ints(rows[:-1])
        for j, d in enumerate(ds):
            assert got[4 * j:4 * j + 4] == [d, 0, pow(d, P - 2, P), 0], (b, d)
            assert got[4 * j + 2] * d % P == 1
    z = ints_to_arr([0, 7, P - 1])
    rows = np.zeros((12, 32), np.uint8)
    emul_g.emul_gadget_is_equal(_ptr(z), _ptr(z), ctypes.c_size_t(3), _ptr(rows))
    assert arr_ints(rows) == [0, 1, 1, 1] * 3                                # equal: z = 1 and the "inverse" is 1


# ---------------------------------------------------------------- insert_leaf, verify_non_inclusion
def _items(depth):
    n = {1: 1, 3: 6, 32: 4, 64: 4}[depth]
    return gc.with_rejected(gc.insert_items(depth, n, 0x494D5800 + depth))


@pytest.mark.parametrize("depth,lb", [(3, lb) for lb in gc.WIDTHS] + [(d, lb) for d in (1, 32, 64) for lb in DEEP_WIDTHS])
def test_insert_and_non_inclusion_rows_host_build_oracle_and_model_agree(emul_g, oracle, depth, lb):
    items = _items(depth)
    K = gc.less_than_rows(lb)
    got = host_insert(emul_g, items, lb)
    head = host_insert(emul_g, items, lb, whole=False, item_major=True)
    assert got.shape[0] == 20 + 2 * K + 16 * depth and head.shape[0] == 17 + 2 * K + 4 * depth
    assert (head == got[:head.shape[0]]).all()                                # verify_non_inclusion is the head of insert_leaf
    select, lts = set(), set()
    for i, w in enumerate(items):
        want, _ = gc.oracle_insert_rows(w, lb)
        assert (got[:, i] == want).all(), (depth, lb, i)
        want_head, _ = gc.oracle_non_inclusion_rows(w, lb)
        assert (head[:, i] == want_head).all(), (depth, lb, i)
        model = gc.model_insert_rows(w, lb)
        assert arr_ints(got[:, i]) == model, (depth, lb, i)
        select.add(model[10 + K + 2])
        lts.add(model[10 + K - 1])
    # the rejected variants reach the 0 branches (depth 1 holds one insertion, the largest: new < next_val never holds)
    assert select == {0, 1} and lts == ({0, 1} if depth > 1 else {0})


# ---------------------------------------------------------------- the column and the lookup rows
@pytest.mark.parametrize("lb", gc.WIDTHS)
def test_layout_rebuilds_a_satisfied_column_from_the_host_builds_rows(emul_g, emul, imt, lb):
    """the product's layout (csrc/imt_gadget_layout.cpp) + its constants + the four limb inputs + the rows of the host
    build of the kernel code: every vertical gate holds, and there are as many as the gadget has"""
    emul.emul_less_than_layout.restype = ctypes.c_int

    def check(rc):
        assert rc == 0, rc
    cells, consts, out_row = imt.trace_layout(lambda *a: emul.emul_less_than_layout(*a), lb, 0, check)
    L = gc.limbs_of(lb)[2]
    n_gates = 2 * (2 + (L - 1) + 2) + 2 * 3 + 4 + 4 + 2     # range.is_less_than x2, is_equal x2, not x4, and x4, or
    assert int(cells["gate"].sum()) == n_gates
    pairs = gc.less_than_pairs(lb)
    pairs = pairs[:20] + pairs[-8:]
    got, lt = host_less_than(emul_g, pairs, lb)
    for i, (a, b) in enumerate(pairs):
        col = imt.rebuild_advice_column(cells, consts, [a >> 128, a & M128, b >> 128, b & M128], got[:, i])
        assert imt.check_vertical_gates(cells, col) == n_gates, (lb, a, b)
        assert arr_ints(got[out_row, i])[0] == int(lt[i]) == (1 if a < b else 0)


def _recomposes(rows, lookup, lb, operands):
    """the lookup rows, L per range check, hold limbs below 2^lb that add up to the shifted differences"""
    _, padded, L = gc.limbs_of(lb)
    assert len(lookup) == L * len(operands) and len(set(lookup)) == len(lookup)
    for g, (x, y) in enumerate(operands):
        limbs = [rows[r] for r in lookup[L * g:L * g + L]]
        assert all(v < (1 << lb) for v in limbs)
        assert sum(v << (lb * i) for i, v in enumerate(limbs)) == (1 << padded) + x - y


@pytest.mark.parametrize("lb", gc.WIDTHS)
def test_lookup_rows_name_limbs_that_recompose_the_shifted_differences(emul_g, imt, lb):
    lk = imt.Context.less_than_lookup_rows(lb).tolist()
    pairs = gc.less_than_pairs(lb)
    pairs = pairs[:16] + pairs[-6:]
    got, _ = host_less_than(emul_g, pairs, lb)
    for i, (a, b) in enumerate(pairs):
        _recomposes(arr_ints(got[:, i]), lk, lb, [(a >> 128, b >> 128), (a & M128, b & M128)])
    depth = 3
    items = _items(depth)
    lk = imt.Context.insert_gadget_lookup_rows(depth, lb).tolist()
    got = host_insert(emul_g, items, lb)
    assert max(lk) < got.shape[0]
    for i, w in enumerate(items):
        v, low, nxt = w["new_leaf"][0], w["low_leaf"][0], w["low_leaf"][1]
        _recomposes(arr_ints(got[:, i]), lk, lb, [(v >> 128, nxt >> 128), (v & M128, nxt & M128), (low >> 128, v >> 128),
                                                  (low & M128, v & M128)])


def test_entry_points_refuse_widths_outside_1_to_28(emul_g):
    one = ints_to_arr([1])
    out = np.zeros((4, 32), np.uint8)
    for lb in (0, 29):
        assert emul_g.emul_gadget_less_than(_ptr(one), _ptr(one), ctypes.c_size_t(1), lb, _ptr(out), ctypes.c_uint64(32),
                                            ctypes.c_uint64(32), None) == -3
    assert not out.any()


# ---------------------------------------------------------------- the same under sanitizers
def test_the_same_checks_as_a_program_under_address_and_undefined_sanitizers(oracle, tmp_path):
    """tests/native/emul_gadget.cpp with its own main (every width: less_than rows in both layouts, insert and
    non-inclusion rows of real and rejected insertions at depth 3, depth 32 at three widths, against liboracle.so, in
    buffers of exactly the documented size), compiled with -fsanitize=address,undefined and run as a child process.
    Nothing is loaded into this interpreter under a sanitizer."""
    exe = str(tmp_path / "gadget_check")
    _run(["g++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEMUL_GADGET_MAIN"] + FLAGS +
         ["-o", exe, SRC, "-L", oracle_lib.ODIR, "-loracle", "-Wl,-rpath," + oracle_lib.ODIR])
    out = _run([exe])
    assert "gadget host checks ok: lookup widths 1..28" in out
