"""GPU: the fixed-length Poseidon hash of 1 to 16 inputs (imt_hash_n_batch, imt_hash_n_trace_batch,
imt_hash_n_trace_layout; kernels k_hash_n, k_hash_n_coop, k_hash_n_trace of csrc/imt_hash_n.hip) against the CPU oracle's
sponge and its advice column (oracle/poseidon.c orc_hash_var, oracle/trace.c orc_hash_trace), bit for bit.

  test_values                 every length, n = 1 / 64 / 65 / 257 (a lone lane, a full wave, one past it, one past a
                              block), one thread per hash and a quad per hash, formats 0 / 1 / 2
  test_values_equal_fixed     len 2, 3 byte-equal to imt_hash2_batch / imt_hash3_batch
  test_traces                 len 1, 2, 3, 4, 5, 15, 16 x n = 1 / 65 x row- / item-major x formats, device pointers into a
                              sentinel-filled buffer: every row of every item, the output row, nothing written outside
  test_traces_equal_fixed     len 2, 3 byte-equal to imt_hash_trace_batch
  test_host_pointer_traces    the Python wrapper (host pointers) gives the same rows
  test_edges                  len 0 / 17, n = 0, an input >= p in the last chunk (host pointers: at return; device
                              pointers: at imt_ctx_sync), in both value kernels and the trace kernel
  test_layout_and_golden      the cell map through the library; golden digests on the GPU's rows
  test_nullifier_example      examples/nullifier_demo.c against the oracle
"""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import hash_n_model as hn
import oracle_lib
from oracle_lib import P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 257
TRACE_LENS = [1, 2, 3, 4, 5, 15, 16]
TRACE_N = 65
SENTINEL = 0xA5
PAD_ROWS = 64                 # sentinel rows kept on either side of a trace buffer


@pytest.fixture(scope="module")
def ref(oracle):
    """per length: N_MAX input vectors (the first two [0] * len and [p - 1] * len) and their hashes, computed once"""
    out = {}
    for length in hn.LENS:
        flat = oracle_lib.synth_values((N_MAX - 2) * length, 0x484E1000 + length)
        items = [[0] * length, [P - 1] * length] + [flat[i * length:(i + 1) * length] for i in range(N_MAX - 2)]
        want = oracle_lib.ints_to_arr([oracle.hash(xs) for xs in items])
        out[length] = (np.stack([hn.to_arr(xs) for xs in items]), want)
    return out


_scaled = {}


def _in_fmt(ref, length, fmt):
    """(inputs [N_MAX, len, 32], hashes [N_MAX, 32]) of `ref` in format fmt"""
    key = ("v", length, fmt)
    if key not in _scaled:
        _scaled[key] = (hn.scaled(ref[length][0], fmt), hn.scaled(ref[length][1], fmt))
    return _scaled[key]


@pytest.fixture(scope="module")
def ref_rows(oracle, ref):
    """per trace length: the oracle's rows of the first TRACE_N items, uint8 [rows, TRACE_N, 32], computed once"""
    return {length: np.stack([hn.oracle_rows(oracle, hn.ints(ref[length][0][i])) for i in range(TRACE_N)], axis=1)
            for length in TRACE_LENS}


def _rows_fmt(ref_rows, length, fmt):
    key = ("r", length, fmt)
    if key not in _scaled:
        _scaled[key] = hn.scaled(ref_rows[length], fmt)
    return _scaled[key]


@pytest.fixture()
def coop(imt, ctx):
    """sets IMT_OPT_COOP_MAX_EVENTS for one test and puts the default back"""
    def set_to(value):
        ctx.set_option(imt._ffi.OPT_COOP_MAX_EVENTS, value)
    yield set_to
    ctx.set_option(imt._ffi.OPT_COOP_MAX_EVENTS, 16384)


# ------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("length", hn.LENS)
def test_values(imt, ctx, ref, coop, length):
    for fmt in (0, 1, 2):
        inp, want = _in_fmt(ref, length, fmt)
        for form in (0, 4 * N_MAX + 4):           # never the quad kernel / the quad kernel at every n used here
            coop(form)
            for n in (1, 64, 65, 257):
                got = ctx.hash_n(inp[:n], fmt)
                assert got.shape == (n, 32)
                bad = np.nonzero((got != want[:n]).any(axis=1))[0]
                assert bad.size == 0, (length, fmt, form, n, bad[:8])


@pytest.mark.parametrize("form", [0, 1 << 20])
def test_values_equal_fixed(imt, ctx, ref, coop, form):
    coop(form)
    for fmt in (0, 1, 2):
        for length, fixed in ((2, ctx.hash2), (3, ctx.hash3)):
            inp, _ = _in_fmt(ref, length, fmt)
            assert ctx.hash_n(inp, fmt).tobytes() == fixed(inp, fmt).tobytes()


# ------------------------------------------------------------------------------------ traces
def _device_trace(imt, c, inp, fmt, item_major, fixed_arity=False):
    """the trace call with device pointers (page-locked, device-addressable host memory: imt_host_alloc) into a
    sentinel-filled buffer; returns the rows as [rows, n, 32]"""
    n, length = inp.shape[0], inp.shape[1]
    rows = hn.rows(length)
    d_in = c.host_alloc(inp.shape)
    buf = c.host_alloc((PAD_ROWS + rows * n + PAD_ROWS, 32))
    try:
        d_in[:] = inp
        buf[:] = SENTINEL
        flags = fmt | imt._ffi.DEVICE_PTRS | (imt._ffi.TRACE_ITEM_MAJOR if item_major else 0)
        call = imt.lib.imt_hash_trace_batch if fixed_arity else imt.lib.imt_hash_n_trace_batch
        assert call(c.h, ctypes.c_void_p(d_in.ctypes.data), length, n, ctypes.c_void_p(buf.ctypes.data + PAD_ROWS * 32), flags) == 0
        c.sync()
        host = buf.copy()
    finally:
        c.host_free(d_in)
        c.host_free(buf)
    assert (host[:PAD_ROWS] == SENTINEL).all() and (host[PAD_ROWS + rows * n:] == SENTINEL).all(), "wrote outside [rows][n]"
    body = host[PAD_ROWS:PAD_ROWS + rows * n]
    return body.reshape(n, rows, 32).transpose(1, 0, 2) if item_major else body.reshape(rows, n, 32)


@pytest.mark.parametrize("item_major", [False, True])
@pytest.mark.parametrize("n", [1, TRACE_N])
@pytest.mark.parametrize("length", TRACE_LENS)
def test_traces(imt, ctx, ref, ref_rows, length, n, item_major):
    for fmt in (0, 1, 2):
        inp, hashes = _in_fmt(ref, length, fmt)
        got = _device_trace(imt, ctx, inp[:n], fmt, item_major)
        want = _rows_fmt(ref_rows, length, fmt)[:, :n]
        assert got.shape == want.shape == (hn.rows(length), n, 32)
        bad = np.argwhere((got != want).any(axis=2))
        assert bad.size == 0, (length, n, item_major, fmt, bad[:8])
        assert (got[hn.rows(length) - 4] == ctx.hash_n(inp[:n], fmt)).all() and (got[-4] == hashes[:n]).all()


@pytest.mark.parametrize("item_major", [False, True])
def test_traces_equal_fixed(imt, ctx, ref, item_major):
    for fmt in (0, 1, 2):
        for length in (2, 3):
            inp = _in_fmt(ref, length, fmt)[0][:TRACE_N]
            a = _device_trace(imt, ctx, inp, fmt, item_major)
            b = _device_trace(imt, ctx, inp, fmt, item_major, fixed_arity=True)
            assert a.tobytes() == b.tobytes()


def test_host_pointer_traces(imt, ctx, ref, ref_rows):
    inp = ref[5][0][:3]
    a = ctx.hash_n_trace(inp)
    b = ctx.hash_n_trace(inp, item_major=True)
    assert a.shape == (hn.rows(5), 3, 32) and b.shape == (3, hn.rows(5), 32)
    assert (a == ref_rows[5][:, :3]).all() and (b.transpose(1, 0, 2) == a).all()
    assert ctx.hash_n_trace(np.zeros((0, 4, 32), np.uint8)).shape == (hn.rows(4), 0, 32)


# ------------------------------------------------------------------------------------ edges
def test_edges(imt, ctx, ref, coop):
    lib, ERR = imt.lib, imt._ffi.ERR
    inp, out = ref[16][0][:1].copy(), np.zeros((hn.rows(16), 32), np.uint8)
    pi, po = inp.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    for length in (0, 17):
        assert lib.imt_hash_n_trace_rows(length) == 0
        assert lib.imt_hash_n_batch(ctx.h, pi, length, po, 1, 0) == ERR["ARG"]
        assert lib.imt_hash_n_trace_batch(ctx.h, pi, length, 1, po, 0) == ERR["ARG"]
        assert lib.imt_hash_n_trace_layout(ctx.h, length, None, 0, None, None, 0, None, None, 0) == ERR["ARG"]
    assert [lib.imt_hash_n_trace_rows(n) for n in (1, 2, 3, 4, 16)] == [604, 1208, 1209, 1813, 5443]
    assert lib.imt_hash_n_batch(ctx.h, None, 4, None, 0, 0) == 0                       # n == 0
    assert lib.imt_hash_n_trace_batch(ctx.h, None, 4, 0, None, 0) == 0
    assert ctx.hash_n(np.zeros((0, 7, 32), np.uint8)).shape == (0, 32)
    with pytest.raises(ValueError):
        ctx.hash_n(np.zeros((1, 17, 32), np.uint8))
    # an input >= p in the last chunk of a 5-input item, among good items
    bad = ref[5][0][:3].copy()
    bad[1, 4] = np.frombuffer(oracle_lib.b32(P), np.uint8)
    pb = bad.ctypes.data_as(ctypes.c_void_p)
    for form in (0, 1 << 20):
        coop(form)
        assert lib.imt_hash_n_batch(ctx.h, pb, 5, po, 3, 0) == ERR["NONCANONICAL"]
        assert (ctx.hash_n(ref[5][0][:3]) == ref[5][1][:3]).all()                      # the context goes on working
    tr = np.zeros((hn.rows(5), 3, 32), np.uint8)
    assert lib.imt_hash_n_trace_batch(ctx.h, pb, 5, 3, tr.ctypes.data_as(ctypes.c_void_p), 0) == ERR["NONCANONICAL"]
    # device pointers (imt_host_alloc memory): accepted at the call, reported at imt_ctx_sync
    c2 = imt.Context(0)
    d_bad, d_out, d_tr = c2.host_alloc(bad.shape), c2.host_alloc((3, 32)), c2.host_alloc((hn.rows(5), 3, 32))
    try:
        d_bad[:] = bad
        pd, pdo = ctypes.c_void_p(d_bad.ctypes.data), ctypes.c_void_p(d_out.ctypes.data)
        for form in (0, 1 << 20):
            c2.set_option(imt._ffi.OPT_COOP_MAX_EVENTS, form)
            assert lib.imt_hash_n_batch(c2.h, pd, 5, pdo, 3, imt._ffi.DEVICE_PTRS) == 0
            with pytest.raises(imt.ImtError) as e:
                c2.sync()
            assert e.value.code == ERR["NONCANONICAL"]
        assert lib.imt_hash_n_trace_batch(c2.h, pd, 5, 3, ctypes.c_void_p(d_tr.ctypes.data), imt._ffi.DEVICE_PTRS) == 0
        with pytest.raises(imt.ImtError) as e:
            c2.sync()
        assert e.value.code == ERR["NONCANONICAL"]
        # a misaligned device pointer is an argument error, as for the fixed-length calls
        assert lib.imt_hash_n_batch(c2.h, ctypes.c_void_p(d_bad.ctypes.data + 8), 1, pdo, 1, imt._ffi.DEVICE_PTRS) == ERR["ARG"]
        # ... and a good batch through the same pointers is the oracle's
        d_bad[:] = ref[5][0][:3]
        assert lib.imt_hash_n_batch(c2.h, pd, 5, pdo, 3, imt._ffi.DEVICE_PTRS) == 0
        c2.sync()
        assert (d_out == ref[5][1][:3]).all()
    finally:
        for a in (d_bad, d_out, d_tr):
            c2.host_free(a)
        c2.close()


# ------------------------------------------------------------------------------------ cell map, golden digests
def test_layout_and_golden(imt, ctx, oracle):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "hash_n_digest.json")))
    assert [g["len"] for g in gold["hashes"]] == hn.LENS
    for g in gold["hashes"]:
        xs = [int(x) for x in g["in"]]
        inp = hn.to_arr(xs)[None]
        assert hn.ints(ctx.hash_n(inp)) == [int(g["hash"])]
        rows = ctx.hash_n_trace(inp)[:, 0]
        assert hashlib.sha256(rows.tobytes()).hexdigest() == g["sha256_rows"]
        cells, consts, out_row = ctx.hash_n_trace_layout(g["len"])
        assert len(cells) == g["cells"] and out_row == g["rows"] - 4
        col = imt.rebuild_advice_column(cells, consts, xs, rows)
        assert hashlib.sha256(oracle_lib.ints_to_arr(col).tobytes()).hexdigest() == g["sha256_cells"]
    for arity in (2, 3):
        a, b = ctx.hash_n_trace_layout(arity, 1), ctx.hash_trace_layout(arity, 1)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ------------------------------------------------------------------------------------ the C example
def test_nullifier_example(imt, oracle):
    """examples/nullifier_demo.c derives six nullifiers as hashes of four fields on the GPU and inserts them; the fifth
    repeats the second and is skipped: its nullifiers and its root against the oracle's"""
    exe, csrc = os.path.join(ROOT, "examples", "nullifier_demo"), os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "nullifier_demo.c"), "-L", csrc, "-limt_hip", "-Wl,-rpath," + csrc,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    notes = [[101, 7, 0, 1], [102, 7, 1, 1], [103, 9, 2, 1], [104, 9, 3, 1], [102, 7, 1, 1], [105, 11, 4, 1]]
    nul = [oracle.hash(x) for x in notes]
    h = oracle.sparse_new(8, 64)
    leaf = {}
    for v in nul:
        if v not in leaf:
            assert oracle.sparse_insert(h, 8, v)["rc"] == 0
            leaf[v] = len(leaf) + 1
    root = oracle.sparse_root(h)
    oracle.sparse_free(h)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for i, v in enumerate(nul):
        word = "double spend, first seen at leaf" if i == 4 else "inserted at leaf"
        assert f"tx {i}: nullifier {v:064x}: {word} {leaf[v]}" in r.stdout, r.stdout
    assert f"6 transactions: 5 nullifiers inserted, 1 skipped; root {root:064x}" in r.stdout, r.stdout
