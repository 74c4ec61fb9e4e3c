"""GPU (MI355X): the gadget trace kernels (csrc/imt_gadget.hip: k_less_than_trace, k_insert_gadget) at EVERY lookup
width 1..28, bit for bit against oracle/gadget.c, with the Python model on a sample of items per width.

What the compiler makes of the limb code at the unusual widths -- 543 rows per comparison at width 1, a top limb that
starts at bit 135 or 140 at widths 27 and 28, limbs that straddle a 32-bit word -- is seen nowhere else.  Per width:
 * imt_less_than_trace_batch on the operand pairs of gadget_corpus (the CPU tests assert what they cover), filled up to
   one past a 128-thread block, and on the 1, 128 and 129 item prefixes, row-major and item-major; lt_out, the layout's
   output cell and the integer comparison agree; at widths 1, 18 and 28 also both Montgomery formats, and device
   pointers into a sentinel-filled buffer with guard rows on both sides;
 * imt_insert_gadget_trace_batch / imt_non_inclusion_gadget_trace_batch on 129 real insertions into a depth-8 tree of
   256 slots and on non-members of it, every third item turned into a witness the circuit rejects, new_path_index
   explicit, with the default context and with IMT_OPT_COOP_MAX_EVENTS = 0 (both forms of k_path_pairs); every row of
   every item; at widths 1, 18, 28 item-major with item-major siblings in halo2curves' form; depths 32 and 64 at
   widths 1 and 28;
 * the lookup rows hold limbs below 2^lb that recompose the four shifted differences; the segment tables equal the
   oracle's and their glue rows add up to the trace's row count;
 * widths 0 and 29 are refused."""
import ctypes
import functools

import numpy as np
import pytest

import gadget_corpus as gc
import oracle_lib
from oracle_lib import P, arr_ints, ints_to_arr
from test_gadget_cpu import EDGE

pytestmark = pytest.mark.gpu

R_OF = {0: 1, 1: pow(2, 256, P), 2: pow(2, 261, P)}          # canonical, MONT256 (halo2curves), DEVICE (the library's)
FULL = (1, 18, 28)              # the widths that also run the other formats, item-major Montgomery and the guarded buffer
DEPTH, N = 8, 129
PAD_ROWS, SENTINEL = 8, 0xA5
M128 = gc.M128


@pytest.fixture(scope="module")
def ctx_thread(imt):
    """a context with the quad-per-item kernels switched off (IMT_OPT_COOP_MAX_EVENTS = 0): one thread per path"""
    c = imt.Context(0)
    c.set_option(imt._ffi.OPT_COOP_MAX_EVENTS, 0)
    yield c
    c.close()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------- is_less_than
@functools.lru_cache(maxsize=None)
def less_than_expect(lb):
    """(pairs, oracle rows uint8 [rows, n, 32]) of one width"""
    orc = oracle_lib.load()
    pairs = gc.padded_pairs(lb)
    assert len(pairs) % 128 == 1 and len(pairs) >= N
    want = np.stack([orc.less_than_trace(a, b, lb)["witness"] for a, b in pairs], axis=1)
    want.setflags(write=False)
    return pairs, want


def _guarded_less_than(imt, c, a, b, lb, fmt, item_major):
    """the call with device pointers into page-locked host memory filled with a sentinel, guard rows on both sides of
    the trace and guard bytes behind lt_out; returns (rows [rows, n, 32], lt)"""
    n, rows = a.shape[0], gc.less_than_rows(lb)
    d_a, d_b = c.host_alloc(a.shape), c.host_alloc(b.shape)
    buf = c.host_alloc((PAD_ROWS + rows * n + PAD_ROWS, 32))
    d_lt = c.host_alloc(n + 64)
    try:
        d_a[:], d_b[:] = a, b
        buf[:] = SENTINEL
        d_lt[:] = SENTINEL
        flags = fmt | imt._ffi.DEVICE_PTRS | (imt._ffi.TRACE_ITEM_MAJOR if item_major else 0)
        assert imt.lib.imt_less_than_trace_batch(c.h, _p(d_a), _p(d_b), n, lb, ctypes.c_void_p(buf.ctypes.data + PAD_ROWS * 32),
                                                 _p(d_lt), flags) == 0
        c.sync()
        host, lt = buf.copy(), d_lt.copy()
    finally:
        for x in (d_a, d_b, buf, d_lt):
            c.host_free(x)
    assert (host[:PAD_ROWS] == SENTINEL).all() and (host[PAD_ROWS + rows * n:] == SENTINEL).all(), "wrote outside [rows][n]"
    assert (lt[n:] == SENTINEL).all(), "wrote behind lt_out[n]"
    body = host[PAD_ROWS:PAD_ROWS + rows * n]
    return (body.reshape(n, rows, 32).transpose(1, 0, 2) if item_major else body.reshape(rows, n, 32)), lt[:n]


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, (what, "first (row, item) that differ:", bad[:6].tolist())


@pytest.mark.parametrize("lb", gc.WIDTHS)
def test_less_than_trace_at_every_width(imt, ctx, lb):
    pairs, want = less_than_expect(lb)
    n, rows = len(pairs), gc.less_than_rows(lb)
    assert want.shape == (rows, n, 32) and rows == 4 * (-(-128 // lb) + 1) + 27
    a, b = ints_to_arr([p[0] for p in pairs]), ints_to_arr([p[1] for p in pairs])
    want_lt = np.array([1 if x < y else 0 for x, y in pairs], np.uint8)
    for j in (0, 3, len(EDGE) + 5, 128, n - 1):                          # the model, on a sample
        assert arr_ints(want[:, j]) == oracle_lib.less_than_rows_model(pairs[j][0], pairs[j][1], lb)[0]
    _, _, out_row = ctx.less_than_layout(lb)
    for m in sorted({1, 128, N, n}):
        for item_major in (False, True):
            got, lt = ctx.less_than_trace(a[:m], b[:m], lb, item_major=item_major)
            _same(got.transpose(1, 0, 2) if item_major else got, want[:, :m], f"lb {lb} n {m} item_major {item_major}")
            assert (lt == want_lt[:m]).all()
    got, lt = ctx.less_than_trace(a, b, lb)
    assert (got[out_row, :, 0] == lt).all() and not got[out_row, :, 1:].any()
    # the rows the RangeChip sends to its lookup table: limbs below 2^lb that recompose both shifted differences
    _, padded, L = gc.limbs_of(lb)
    lk = ctx.less_than_lookup_rows(lb)
    limbs = got[lk]                                                      # [2 L, n, 32]
    assert len(lk) == 2 * L and not limbs[:, :, 4:].any()
    v = limbs[:, :, :4].copy().view("<u4")[..., 0]                       # [2 L, n]
    assert (v < (1 << lb)).all()
    for j, (x, y) in enumerate(pairs):
        for h, (p, q) in enumerate(((x >> 128, y >> 128), (x & M128, y & M128))):
            assert sum(int(t) << (lb * i) for i, t in enumerate(v[h * L:(h + 1) * L, j])) == (1 << padded) + p - q, (lb, j, h)
    if lb in FULL:
        for fmt in (1, 2):
            af, bf = gc.scaled(a, R_OF[fmt]), gc.scaled(b, R_OF[fmt])
            got_f, lt_f = ctx.less_than_trace(af, bf, lb, fmt=fmt)
            _same(got_f, gc.scaled(want, R_OF[fmt]), f"lb {lb} fmt {fmt}")
            assert (lt_f == want_lt).all()
        for fmt, item_major in ((0, False), (0, True), (1, False), (2, True)):
            af, bf = gc.scaled(a[:N], R_OF[fmt]), gc.scaled(b[:N], R_OF[fmt])
            got_d, lt_d = _guarded_less_than(imt, ctx, af, bf, lb, fmt, item_major)
            _same(got_d, gc.scaled(want[:, :N], R_OF[fmt]), f"lb {lb} device pointers fmt {fmt} item_major {item_major}")
            assert (lt_d == want_lt[:N]).all()


# ---------------------------------------------------------------- insert_leaf, verify_non_inclusion
@functools.lru_cache(maxsize=None)
def insert_corpus(depth, n):
    """(insert_leaf items, their arrays, verify_non_inclusion items, their arrays): real insertions into a tree of
    min(2^depth, 256) slots and non-members of it, every third one rejected"""
    items = gc.reject(gc.insert_items(depth, n, 0x494D5900 + depth))
    if depth == 64:                                                      # forged witnesses: their own non-inclusion part
        nm = [dict(depth=depth, low_leaf=w["low_leaf"], low_index=w["low_index"], low_sib=w["low_sib"],
                   new_val=w["new_leaf"][0], is_largest=w["is_largest"]) for w in items]
    else:
        nm = gc.reject(gc.non_members(depth, n, 0x494D5900 + depth))
    assert len(items) == len(nm) == n
    return items, gc.stacked(items), nm, gc.stacked(nm)


@functools.lru_cache(maxsize=None)
def insert_expect(depth, n, lb):
    items, _, nm, _ = insert_corpus(depth, n)
    ins = [gc.oracle_insert_rows(w, lb) for w in items]
    non = [gc.oracle_non_inclusion_rows(w, lb) for w in nm]
    return np.stack([r for r, _ in ins], axis=1), ins[0][1], np.stack([r for r, _ in non], axis=1), non[0][1]


def _insert(c, s, depth, lb, **kw):
    return c.insert_gadget_trace(s["low_leaf"], s["low_index"], s["low_sib"], s["new_leaf"], s["new_index"], s["new_sib"],
                                 s["is_largest"], depth, lb, new_path_index=s["new_path_index"], **kw)


def _non_inclusion(c, s, depth, lb, **kw):
    return c.non_inclusion_gadget_trace(s["low_leaf"], s["low_index"], s["low_sib"], s["new_val"], s["is_largest"], depth, lb, **kw)


def _item_major_mont(s):
    """the arrays in halo2curves' in-memory form, siblings item-major [n][depth][32]"""
    out = dict(s)
    for k, v in s.items():
        if v.dtype == np.uint8 and v.ndim >= 2:
            out[k] = gc.scaled(np.ascontiguousarray(v.transpose(1, 0, 2)) if k.endswith("_sib") else v, R_OF[1])
    return out


@pytest.mark.parametrize("lb", gc.WIDTHS)
def test_insert_and_non_inclusion_gadget_traces_at_every_width(imt, ctx, ctx_thread, lb):
    items, s, nm, s_nm = insert_corpus(DEPTH, N)
    want, want_segs, want_nm, want_nm_segs = insert_expect(DEPTH, N, lb)
    K = gc.less_than_rows(lb)
    rows, head = 20 + 2 * K + 16 * DEPTH, 17 + 2 * K + 4 * DEPTH
    assert want.shape == (rows, N, 32) and want_nm.shape == (head, N, 32)
    assert imt.lib.imt_insert_gadget_rows(DEPTH, lb) == rows and imt.lib.imt_non_inclusion_gadget_rows(DEPTH, lb) == head
    for j in (0, 2, 5, 8, N - 1):                                        # the model: honest, the three rejections, the last
        assert arr_ints(want[:, j]) == gc.model_insert_rows(items[j], lb)
    assert {int(x) for x in want[10 + K + 2, :, 0]} == {0, 1} and {int(x) for x in want[10 + K - 1, :, 0]} == {0, 1}
    for name, c in (("default", ctx), ("thread per path", ctx_thread)):
        got = _insert(c, s, DEPTH, lb)
        _same(got, want, f"insert gadget, lb {lb}, {name}")
        got_nm = _non_inclusion(c, s_nm, DEPTH, lb)
        _same(got_nm, want_nm, f"non-inclusion gadget, lb {lb}, {name}")
    # verify_non_inclusion of the inserted values is the head of insert_leaf
    got_head = ctx.non_inclusion_gadget_trace(s["low_leaf"], s["low_index"], s["low_sib"], np.ascontiguousarray(s["new_leaf"][:, 0]),
                                              s["is_largest"], DEPTH, lb)
    _same(got_head, want[:head], f"head of insert_leaf, lb {lb}")
    # segments: the oracle's, and their glue rows are the trace's rows
    segs, segs_nm = imt.insert_column_segments(DEPTH, lb), imt.non_inclusion_column_segments(DEPTH, lb)
    assert segs == want_segs and segs_nm == want_nm_segs and segs_nm == segs[:len(segs_nm)]
    assert sum(x[3] for x in segs if x[0] == 0) == rows and sum(x[3] for x in segs_nm if x[0] == 0) == head
    # lookup rows: the limbs of the four shifted differences of the two comparisons (:180, :226)
    _, padded, L = gc.limbs_of(lb)
    lk = ctx.insert_gadget_lookup_rows(DEPTH, lb)
    assert len(lk) == 4 * L and len(set(lk.tolist())) == 4 * L and lk.max() < head
    limbs = got[lk]
    assert not limbs[:, :, 4:].any()
    v = limbs[:, :, :4].copy().view("<u4")[..., 0]
    assert (v < (1 << lb)).all() and (got_nm[lk][:, :, :4].copy().view("<u4")[..., 0] < (1 << lb)).all()
    for j, w in enumerate(items):
        nv, low, nxt = w["new_leaf"][0], w["low_leaf"][0], w["low_leaf"][1]
        for g, (x, y) in enumerate(((nv >> 128, nxt >> 128), (nv & M128, nxt & M128), (low >> 128, nv >> 128), (low & M128, nv & M128))):
            assert sum(int(t) << (lb * i) for i, t in enumerate(v[g * L:(g + 1) * L, j])) == (1 << padded) + x - y, (lb, j, g)
    if lb in FULL:
        F = imt._ffi
        m, m_nm = _item_major_mont(s), _item_major_mont(s_nm)
        for name, c in (("default", ctx), ("thread per path", ctx_thread)):
            got_m = _insert(c, m, DEPTH, lb, fmt=F.FMT_MONT256, item_major=True)
            _same(got_m.transpose(1, 0, 2), gc.scaled(want, R_OF[1]), f"insert gadget, item-major Montgomery, lb {lb}, {name}")
            got_m = _non_inclusion(c, m_nm, DEPTH, lb, fmt=F.FMT_MONT256, item_major=True)
            _same(got_m.transpose(1, 0, 2), gc.scaled(want_nm, R_OF[1]), f"non-inclusion gadget, item-major Montgomery, lb {lb}, {name}")


@pytest.mark.parametrize("lb", (1, 28))
@pytest.mark.parametrize("depth", (32, 64))
def test_deep_trees_at_the_narrowest_and_widest_lookup(imt, ctx, ctx_thread, depth, lb):
    n = 5
    items, s, nm, s_nm = insert_corpus(depth, n)
    want, want_segs, want_nm, want_nm_segs = insert_expect(depth, n, lb)
    assert want.shape[0] == 20 + 2 * gc.less_than_rows(lb) + 16 * depth
    for j in (0, 2):
        assert arr_ints(want[:, j]) == gc.model_insert_rows(items[j], lb)
    for name, c in (("default", ctx), ("thread per path", ctx_thread)):
        _same(_insert(c, s, depth, lb), want, f"insert gadget, depth {depth}, lb {lb}, {name}")
        _same(_non_inclusion(c, s_nm, depth, lb), want_nm, f"non-inclusion gadget, depth {depth}, lb {lb}, {name}")
    got_m = _insert(ctx, _item_major_mont(s), depth, lb, fmt=imt._ffi.FMT_MONT256, item_major=True)
    _same(got_m.transpose(1, 0, 2), gc.scaled(want, R_OF[1]), f"insert gadget, item-major Montgomery, depth {depth}, lb {lb}")
    assert imt.insert_column_segments(depth, lb) == want_segs and imt.non_inclusion_column_segments(depth, lb) == want_nm_segs


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("lb", (0, 29))
def test_widths_outside_1_to_28_are_refused(imt, ctx, lb):
    F, lib = imt._ffi, imt.lib
    _, s, _, s_nm = insert_corpus(DEPTH, N)
    one = ints_to_arr([1])
    out = np.full((2000, 32), SENTINEL, np.uint8)
    lt = np.full(4, SENTINEL, np.uint8)
    assert lib.imt_less_than_trace_batch(ctx.h, _p(one), _p(one), 1, lb, _p(out), _p(lt), 0) == F.ERR["RANGE"]
    sib = np.ascontiguousarray(s["low_sib"][:, :1])
    nsib = np.ascontiguousarray(s["new_sib"][:, :1])
    assert lib.imt_insert_gadget_trace_batch(ctx.h, _p(s["low_leaf"]), _p(s["low_index"]), _p(sib), _p(s["new_leaf"]),
                                             _p(s["new_index"]), _p(s["new_path_index"]), _p(nsib), _p(s["is_largest"]), DEPTH, lb,
                                             1, _p(out), 0) == F.ERR["RANGE"]
    assert lib.imt_non_inclusion_gadget_trace_batch(ctx.h, _p(s_nm["low_leaf"]), _p(s_nm["low_index"]),
                                                    _p(np.ascontiguousarray(s_nm["low_sib"][:, :1])), _p(s_nm["new_val"]),
                                                    _p(s_nm["is_largest"]), DEPTH, lb, 1, _p(out), 0) == F.ERR["RANGE"]
    assert (out == SENTINEL).all() and (lt == SENTINEL).all()
    # the five row and segment functions: 0 rows, or an error
    assert lib.imt_less_than_trace_rows(lb) == 0
    assert lib.imt_insert_gadget_rows(DEPTH, lb) == 0 and lib.imt_non_inclusion_gadget_rows(DEPTH, lb) == 0
    n_segs = ctypes.c_size_t()
    assert lib.imt_insert_column_segments(DEPTH, lb, None, 0, ctypes.byref(n_segs)) == F.ERR["RANGE"]
    assert lib.imt_non_inclusion_column_segments(DEPTH, lb, None, 0, ctypes.byref(n_segs)) == F.ERR["RANGE"]
    # and the context still works
    got, lt = ctx.less_than_trace(one, ints_to_arr([2]), 18)
    assert lt.tolist() == [1] and got.shape == (63, 1, 32)
