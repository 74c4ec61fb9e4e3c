"""GPU (MI355X): the three relation checkers against the witness corpus (tests/witness_corpus.py), bit-exactly.

imt_insert_witness_batch (insert_leaf), imt_non_membership_batch (verify_non_inclusion) and imt_path_root_batch /
imt_compute_merkle_root_batch / imt_verify_proof_batch (compute_merkle_root, verify_proof) judge witnesses, most of
which here must fail.  Every per-item result is compared with the oracle's: the fail mask itself, every trace row, the
recomputed root, the ok bit.  Both forms of each kernel run (thread per item, quad of lanes per item) at batch sizes
ragged against 256-thread blocks and 64-item quad blocks and across the n*16 / n*4 switches of the default context, in
both sibling layouts, with shared and per-item roots, in all three field-element formats; every field-element input
refuses p and 2^256 - 1; the gadget traces of failing witnesses are compared row for row; and bench.py's verdict
rejects each single corruption of a real batch."""
import functools
import types

import numpy as np
import pytest

import witness_corpus as wc
from mirror_corpus import R_OF, from_fmt, to_fmt     # the three boundary formats, shared with test_gpu_mirror_edges.py
from oracle_lib import P, arr_ints, ints_to_arr

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 1024, 1025, 4096, 4097)
FORMS = ("default", "thread", "quad")


@pytest.fixture(scope="module")
def forms(imt, ctx):
    """the default context (the size switches apply), thread per item (IMT_OPT_COOP_MAX_EVENTS = 0) and quad per item
    for every size (1 << 30)"""
    thread, quad = imt.Context(0), imt.Context(0)
    thread.set_option(imt._ffi.OPT_COOP_MAX_EVENTS, 0)
    quad.set_option(imt._ffi.OPT_COOP_MAX_EVENTS, 1 << 30)
    yield dict(default=ctx, thread=thread, quad=quad)
    thread.close()
    quad.close()


def _fe(xs, shape):
    return ints_to_arr(xs).reshape(shape)


@functools.lru_cache(maxsize=None)
def arrays(kind, depth):
    """the records of one checker and depth as stacked arrays (siblings item-major [R, depth, 32]) + their expectations"""
    recs = wc.corpus(depth)[kind]
    W = [r["w"] for r in recs]
    R = len(recs)
    u64 = lambda k: np.array([w[k] for w in W], dtype=np.uint64)
    if kind == "insert":
        a = dict(old_root=_fe([w["old_root"] for w in W], (R, 32)), low_leaf=_fe([x for w in W for x in w["low_leaf"]], (R, 3, 32)),
                 low_index=u64("low_index"), low_sib=_fe([x for w in W for x in w["low_sib"]], (R, depth, 32)),
                 new_root=_fe([w["new_root"] for w in W], (R, 32)), new_leaf=_fe([x for w in W for x in w["new_leaf"]], (R, 3, 32)),
                 new_index=u64("new_index"), new_path_index=u64("new_path_index"),
                 new_sib=_fe([x for w in W for x in w["new_sib"]], (R, depth, 32)),
                 is_largest=np.array([w["is_largest"] for w in W], np.uint8),
                 mask=np.array([r["mask"] for r in recs], np.uint8), trace=_fe([x for r in recs for x in r["trace"]], (R, 7, 32)))
    elif kind == "nonmem":
        a = dict(root=_fe([w["root"] for w in W], (R, 32)), low_leaf=_fe([x for w in W for x in w["low_leaf"]], (R, 3, 32)),
                 low_index=u64("low_index"), low_sib=_fe([x for w in W for x in w["low_sib"]], (R, depth, 32)),
                 new_val=_fe([w["new_val"] for w in W], (R, 32)), is_largest=np.array([w["is_largest"] for w in W], np.uint8),
                 mask=np.array([r["mask"] for r in recs], np.uint8), root_out=_fe([r["root_out"] for r in recs], (R, 32)))
    else:
        a = dict(leaf=_fe([w["leaf"] for w in W], (R, 32)), index=u64("index"),
                 sib=_fe([x for w in W for x in w["sib"]], (R, depth, 32)), root=_fe([w["root"] for w in W], (R, 32)),
                 root_out=_fe([r["root_out"] for r in recs], (R, 32)), ok=np.array([r["ok"] for r in recs], np.uint8))
    a["honest"] = np.array([j for j, r in enumerate(recs) if r["group"] in ("honest", "path") and r.get("ok", 1)
                            and not r.get("mask", 0)])
    a["names"] = [r["name"] for r in recs]
    return a


def tile(a, n, salt, pool=None):
    """n record indices: the corpus (or `pool`) cycled through the even slots, honest witnesses in the odd ones, so that
    a result smeared onto a neighbouring item or lane changes an honest item's answer"""
    pool = np.arange(len(a["names"])) if pool is None else np.asarray(pool)
    j = np.arange(n)
    return np.where(j % 2 == 0, pool[(j // 2 + salt) % len(pool)], a["honest"][(j // 2) % len(a["honest"])])


def take(a, sel, item_major, fmt=0):
    """the batch `sel` of stacked arrays: field elements in format `fmt`, siblings in the layout asked for"""
    out = {}
    for k, v in a.items():
        if k in ("honest", "names") or k in ("mask", "trace", "root_out", "ok"):
            continue
        b = v[sel]
        if k.endswith("sib") and not item_major:
            b = b.transpose(1, 0, 2)
        b = np.ascontiguousarray(b)
        out[k] = to_fmt(b, fmt) if b.dtype == np.uint8 and b.ndim >= 2 else b
    return out


def same(got, want, sel, a, what):
    g = np.asarray(got).reshape(len(sel), -1)
    w = np.asarray(want).reshape(len(sel), -1)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert not bad.size, (f"{what}: {bad.size} of {len(sel)} items differ; first item {bad[0]} "
                          f"({a['names'][sel[bad[0]]]}): got {g[bad[0]][:8]} want {w[bad[0]][:8]}")


# ---------------------------------------------------------------- insert_leaf
def run_insert(c, a, sel, depth, item_major=False, fmt=0, explicit_npi=True):
    b = take(a, sel, item_major, fmt)
    fail, tr = c.insert_witness(b["old_root"], b["low_leaf"], b["low_index"], b["low_sib"], b["new_root"], b["new_leaf"],
                                b["new_index"], b["new_sib"], b["is_largest"], depth, item_major=item_major, fmt=fmt,
                                want_trace=True, new_path_index=b["new_path_index"] if explicit_npi else None)
    what = f"insert depth {depth} n {len(sel)} item_major {item_major} fmt {fmt} npi {explicit_npi}"
    same(fail, a["mask"][sel], sel, a, what + " fail_out")
    same(from_fmt(tr, fmt).transpose(1, 0, 2), a["trace"][sel], sel, a, what + " trace_out")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_insert_witness_every_record(forms, form, n):
    """fail_out equal to the oracle's mask and every trace row, level-major with explicit new_path_index; at a ragged
    subset of sizes also item-major and with new_path_index NULL (on the records where the two indices agree)"""
    c = forms[form]
    for depth in wc.DEPTHS:
        a = arrays("insert", depth)
        sel = tile(a, n, n)
        run_insert(c, a, sel, depth)
        if n in (63, 65, 1025, 4097):
            run_insert(c, a, sel, depth, item_major=True)
            same_idx = np.nonzero(a["new_index"] == a["new_path_index"])[0]
            sub = dict(a, honest=np.intersect1d(a["honest"], same_idx))
            run_insert(c, sub, tile(sub, n, n + 1, pool=same_idx), depth, explicit_npi=False)


# ---------------------------------------------------------------- verify_non_inclusion
def run_nonmem(c, a, sel, depth, item_major=False, fmt=0, shared_root=None):
    b = take(a, sel, item_major, fmt)
    root = b["root"] if shared_root is None else to_fmt(shared_root, fmt)
    fail, rout = c.non_membership(root, b["low_leaf"], b["low_index"], b["low_sib"], depth, b["new_val"], b["is_largest"],
                                  item_major=item_major, fmt=fmt, want_root=True)
    what = f"non_membership depth {depth} n {len(sel)} item_major {item_major} fmt {fmt} shared {shared_root is not None}"
    same(fail, a["mask"][sel], sel, a, what + " fail_out")
    same(from_fmt(rout, fmt), a["root_out"][sel], sel, a, what + " root_out")


def _common_root(a):
    """the most frequent root of the records and those that carry it (the shared-root batches)"""
    keys = [bytes(r) for r in a["root"]]
    best = max(set(keys), key=keys.count)
    return a["root"][keys.index(best)].copy(), np.array([j for j, k in enumerate(keys) if k == best])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_non_membership_every_record(forms, form, n):
    c = forms[form]
    for depth in wc.DEPTHS:
        a = arrays("nonmem", depth)
        sel = tile(a, n, n)
        run_nonmem(c, a, sel, depth)
        if n in (63, 65, 1025, 4097):
            run_nonmem(c, a, sel, depth, item_major=True)
            root, carriers = _common_root(a)
            sub = dict(a, honest=np.intersect1d(a["honest"], carriers))
            assert sub["honest"].size
            run_nonmem(c, sub, tile(sub, n, n, pool=carriers), depth, shared_root=root)


# ---------------------------------------------------------------- verify_proof / compute_merkle_root
def run_paths(c, a, sel, depth, item_major=False, fmt=0, shared_root=None):
    b = take(a, sel, item_major, fmt)
    what = f"paths depth {depth} n {len(sel)} item_major {item_major} fmt {fmt} shared {shared_root is not None}"
    r1 = c.path_root(b["leaf"], b["index"], b["sib"], depth, item_major=item_major, fmt=fmt)
    same(from_fmt(r1, fmt), a["root_out"][sel], sel, a, what + " path_root")
    helper = ~b["index"]                            # helper bit 1 = the current node is the left input
    r2 = c.compute_merkle_root(b["leaf"], helper, b["sib"], depth, item_major=item_major, fmt=fmt)
    same(from_fmt(r2, fmt), a["root_out"][sel], sel, a, what + " compute_merkle_root")
    root = b["root"] if shared_root is None else to_fmt(shared_root, fmt)
    ok = c.verify_proof_batch(b["leaf"], b["index"], root, b["sib"], depth, item_major=item_major, fmt=fmt)
    same(ok.astype(np.uint8), a["ok"][sel], sel, a, what + " ok_out")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_path_checkers_every_record(forms, form, n):
    c = forms[form]
    for depth in wc.DEPTHS:
        a = arrays("path", depth)
        sel = tile(a, n, n)
        run_paths(c, a, sel, depth)
        if n in (63, 65, 1025, 4097):
            run_paths(c, a, sel, depth, item_major=True)
            root, carriers = _common_root(a)
            sub = dict(a, ok=(a["root_out"] == root).all(axis=1).astype(np.uint8),
                       honest=np.array([j for j in a["honest"] if (a["root_out"][j] == root).all()]))
            if not sub["honest"].size:
                sub["honest"] = carriers
            run_paths(c, sub, tile(sub, n, n), depth, shared_root=root)


# ---------------------------------------------------------------- formats
@pytest.mark.parametrize("fmt", (1, 2))
@pytest.mark.parametrize("form", FORMS)
def test_checkers_in_every_format(imt, forms, form, fmt):
    """MONT256 (R = 2^256) and DEVICE (R = 2^261): the same masks, and traces and roots in the call's format"""
    c = forms[form]
    for depth in wc.DEPTHS:
        for n, item_major in ((65, False), (257, True)):
            a = arrays("insert", depth)
            run_insert(c, a, tile(a, n, 3), depth, item_major=item_major, fmt=fmt)
            a = arrays("nonmem", depth)
            run_nonmem(c, a, tile(a, n, 5), depth, item_major=item_major, fmt=fmt)
            root, carriers = _common_root(a)
            sub = dict(a, honest=np.intersect1d(a["honest"], carriers))
            run_nonmem(c, sub, tile(sub, n, 7, pool=carriers), depth, fmt=fmt, shared_root=root)
            a = arrays("path", depth)
            run_paths(c, a, tile(a, n, 11), depth, item_major=item_major, fmt=fmt)


# ---------------------------------------------------------------- non-canonical inputs
BAD = (P, (1 << 256) - 1)


def _poison(b, key, bad_raw, item, field, depth, item_major):
    """b with the field element `key` (`field`: a leaf slot or a sibling level) of one item replaced by raw bytes"""
    b = {k: v.copy() for k, v in b.items()}
    raw = np.frombuffer(bad_raw.to_bytes(32, "little"), np.uint8)
    if b[key].ndim == 3 and not key.endswith("sib"):      # a leaf preimage: field = its slot
        b[key][item, field] = raw
    elif key.endswith("sib"):
        if item_major:
            b[key][item, field] = raw
        else:
            b[key][field, item] = raw
    elif b[key].ndim == 2:
        b[key][item] = raw
    else:
        b[key][:] = raw
    return b


@pytest.mark.parametrize("fmt", (0, 1, 2))
@pytest.mark.parametrize("form", FORMS)
def test_noncanonical_inputs_are_refused(imt, forms, form, fmt):
    """p and 2^256 - 1 in each field-element input of each checker, on one item of a batch: IMT_ERR_NONCANONICAL in
    every form and format, and the context answers the clean batch correctly afterwards"""
    c = forms[form]
    code = imt._ffi.ERR["NONCANONICAL"]
    depth, n, item = 32, 6, 3
    levels = (0, depth - 1)
    checks = []
    a = arrays("insert", depth)
    sel = tile(a, n, 1)
    for item_major in (False, True):
        b = take(a, sel, item_major, fmt)
        call = lambda b, im=item_major: c.insert_witness(
            b["old_root"], b["low_leaf"], b["low_index"], b["low_sib"], b["new_root"], b["new_leaf"], b["new_index"],
            b["new_sib"], b["is_largest"], depth, item_major=im, fmt=fmt, new_path_index=b["new_path_index"])
        for key in ("old_root", "new_root", "low_leaf", "new_leaf", "low_sib", "new_sib"):
            for field in ((0, 1, 2) if key.endswith("leaf") else levels if key.endswith("sib") else (0,)):
                checks.append((f"insert {key}[{field}] item_major {item_major}", call, b, key, field, item_major))
    clean_insert = (call, b, a["mask"][sel])
    a = arrays("nonmem", depth)
    sel = tile(a, n, 1)
    b = take(a, sel, False, fmt)
    call = lambda b: c.non_membership(b["root"], b["low_leaf"], b["low_index"], b["low_sib"], depth, b["new_val"],
                                      b["is_largest"], fmt=fmt)
    for key in ("root", "new_val", "low_leaf", "low_sib"):
        for field in ((0, 1, 2) if key.endswith("leaf") else levels if key.endswith("sib") else (0,)):
            checks.append((f"non_membership {key}[{field}]", call, b, key, field, False))
    root, _ = _common_root(a)
    bs = dict(b, root=to_fmt(root, fmt))
    checks.append(("non_membership shared root", lambda b: c.non_membership(
        b["root"], b["low_leaf"], b["low_index"], b["low_sib"], depth, b["new_val"], b["is_largest"], fmt=fmt), bs, "root",
        0, False))
    a = arrays("path", depth)
    sel = tile(a, n, 1)
    b = take(a, sel, False, fmt)
    calls = dict(path_root=lambda b: c.path_root(b["leaf"], b["index"], b["sib"], depth, fmt=fmt),
                 compute_merkle_root=lambda b: c.compute_merkle_root(b["leaf"], ~b["index"], b["sib"], depth, fmt=fmt),
                 verify_proof=lambda b: c.verify_proof_batch(b["leaf"], b["index"], b["root"], b["sib"], depth, fmt=fmt))
    for name, call in calls.items():
        for key in ("leaf", "sib") + (("root",) if name == "verify_proof" else ()):
            for field in (levels if key == "sib" else (0,)):
                checks.append((f"{name} {key}[{field}]", call, b, key, field, False))
    for what, call, b, key, field, item_major in checks:
        for bad in BAD:
            with pytest.raises(imt.ImtError) as ei:
                call(_poison(b, key, bad, item, field, depth, item_major))
            assert ei.value.code == code, (what, hex(bad), ei.value.code)
    call, b, mask = clean_insert
    assert (call(b) == mask).all()


# ---------------------------------------------------------------- gadget traces of failing witnesses
@functools.lru_cache(maxsize=None)
def gadget_expect(kind, depth, lookup_bits):
    """(record indices, oracle rows [k, rows, 32]) of the reseal and edge records"""
    from oracle_lib import load
    orc = load()
    recs = wc.corpus(depth)[kind]
    idx = [j for j, r in enumerate(recs) if r["group"] in ("reseal", "edge")]
    rows = []
    for j in idx:
        w = recs[j]["w"]
        if kind == "insert":
            g, _ = orc.insert_gadget_trace(w["low_leaf"], w["low_index"], ints_to_arr(w["low_sib"]), w["new_leaf"],
                                           w["new_index"], ints_to_arr(w["new_sib"]), w["is_largest"], depth, lookup_bits,
                                           new_path_index=w["new_path_index"])
        else:
            g, _ = orc.non_inclusion_gadget_trace(w["low_leaf"], w["low_index"], ints_to_arr(w["low_sib"]), w["new_val"],
                                                  w["is_largest"], depth, lookup_bits)
        rows.append(g)
    return np.array(idx), np.stack(rows)


@pytest.mark.parametrize("item_major", (False, True))
@pytest.mark.parametrize("lookup_bits", (18, 8))
def test_gadget_traces_of_failing_witnesses(forms, lookup_bits, item_major):
    """imt_insert_gadget_trace_batch / imt_non_inclusion_gadget_trace_batch on the resealed and edge records: the
    column a prover assigns for a witness the circuit then rejects, row for row against oracle/gadget.c"""
    for form in ("thread", "quad"):
        c = forms[form]
        for depth in wc.DEPTHS:
            a = arrays("insert", depth)
            sel, want = gadget_expect("insert", depth, lookup_bits)
            b = take(a, sel, item_major)
            got = c.insert_gadget_trace(b["low_leaf"], b["low_index"], b["low_sib"], b["new_leaf"], b["new_index"],
                                        b["new_sib"], b["is_largest"], depth, lookup_bits,
                                        new_path_index=b["new_path_index"], item_major=item_major)
            same(got if item_major else got.transpose(1, 0, 2), want, sel, a,
                 f"insert gadget {form} depth {depth} lookup_bits {lookup_bits} item_major {item_major}")
            a = arrays("nonmem", depth)
            sel, want = gadget_expect("nonmem", depth, lookup_bits)
            b = take(a, sel, item_major)
            got = c.non_inclusion_gadget_trace(b["low_leaf"], b["low_index"], b["low_sib"], b["new_val"], b["is_largest"],
                                               depth, lookup_bits, item_major=item_major)
            same(got if item_major else got.transpose(1, 0, 2), want, sel, a,
                 f"non-inclusion gadget {form} depth {depth} lookup_bits {lookup_bits} item_major {item_major}")


# ---------------------------------------------------------------- bench.py's verdict
def test_bench_witness_check_rejects_every_single_corruption(imt, ctx):
    """bench.witness_check on device tensors of one 2^12-insertion depth-32 batch in the bench's layout: True untouched,
    False after each single corruption"""
    import torch
    import bench
    import oracle_lib

    n, depth = 1 << 12, 32
    assert bench.DEPTH == depth
    t = imt.IndexedTree(ctx, depth, 2 * n)
    r = t.insert_batch(oracle_lib.synth_values(n, 0x494D5510))
    t.close()
    dev = torch.device("cuda", 0)
    env = types.SimpleNamespace(lib=imt.lib, F=imt._ffi, dev=dev)
    r["low_index"] = r["low_index"].astype(np.int64)
    base = {k: torch.from_numpy(np.ascontiguousarray(r[k])).to(dev)
            for k in ("old_root", "low_leaf", "low_index", "low_sib", "new_root", "new_leaf", "new_sib", "is_largest")}
    first = int(r["new_index"][0])
    assert bench.witness_check(env, ctx, base, first, n)

    def bump(x):     # +1 mod p on one field element: canonical, different
        v = (int.from_bytes(bytes(x.cpu().numpy()), "little") + 1) % P
        x.copy_(torch.from_numpy(np.frombuffer(v.to_bytes(32, "little"), np.uint8).copy()).to(dev))

    i, j = 0, 1234
    largest = int(np.nonzero(r["is_largest"])[0][0])
    corruptions = {
        "old_root[first]": lambda o: bump(o["old_root"][i]),
        "old_root[later]": lambda o: bump(o["old_root"][j]),
        "low_leaf.val": lambda o: bump(o["low_leaf"][j, 0]),
        "low_leaf.next_val": lambda o: bump(o["low_leaf"][j, 1]),
        "low_leaf.next_idx": lambda o: bump(o["low_leaf"][j, 2]),
        "low_index": lambda o: o["low_index"][j].bitwise_xor_(1),
        "low_sib[17]": lambda o: bump(o["low_sib"][17, j]),
        "new_root": lambda o: bump(o["new_root"][n - 1]),
        "new_leaf.val": lambda o: bump(o["new_leaf"][j, 0]),
        "new_leaf.next_val": lambda o: bump(o["new_leaf"][j, 1]),
        "new_leaf.next_idx": lambda o: bump(o["new_leaf"][j, 2]),
        "new_sib[5]": lambda o: bump(o["new_sib"][5, j]),
        "is_largest": lambda o: o["is_largest"][j].bitwise_xor_(1),
        "is_largest=2": lambda o: o["is_largest"][largest].fill_(2),
    }
    for name, corrupt in corruptions.items():
        o = {k: v.clone() for k, v in base.items()}
        corrupt(o)
        assert not bench.witness_check(env, ctx, o, first, n), name
    assert bench.witness_check(env, ctx, base, first, n)
